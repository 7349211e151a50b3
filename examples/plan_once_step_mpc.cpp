// plan_once_step_mpc.cpp -- planOnce() of CCC::StepMpc through the drop-in header (host C++ -> header shim -> C-ABI -> HIP
// kernel) on the reference data FootstepManager::makeStepMpcRefData gives for the scenario of
// /root/reference/tests/src/TestStepMpc.cpp:27-42 at t = 0 (standing before the first step) and at t = 2.5 (in the first
// swing, four steps ahead).  Prints the planned ZMP, the planned foothold and whether there is one.
#include <CCC/StepMpc.h>

#include <cstdio>

namespace
{
CCC::StepMpc::RefData::Element element(bool is_single_support, double zmp_x, double zmp_y, double end_time)
{
  CCC::StepMpc::RefData::Element e;
  e.is_single_support = is_single_support;
  e.zmp = CCC::Vector2d(zmp_x, zmp_y);
  e.end_time = end_time;
  return e;
}

void plan_and_print(CCC::StepMpc & mpc, const CCC::StepMpc::RefData & ref_data, double pos_x, double t)
{
  CCC::StepMpc::InitialParam initial_param;
  initial_param.pos = CCC::Vector2d(pos_x, 0.01);
  initial_param.vel = CCC::Vector2d(0.05, -0.02);
  const auto planned = mpc.planOnce(ref_data, initial_param, t);
  const bool has = planned.next_foot_zmp.has_value();
  const CCC::Vector2d foot = has ? planned.next_foot_zmp.value() : CCC::Vector2d(0.0, 0.0);
  std::printf("t=%.1f current_zmp= %.17g %.17g next_foot_zmp= %.17g %.17g has_next_foot=%d\n", t, planned.current_zmp[0],
              planned.current_zmp[1], foot[0], foot[1], has ? 1 : 0);
}
} // namespace

int main()
{
  try
  {
    CCC::StepMpc mpc(1.0);
    CCC::StepMpc::RefData at0, at25;
    // t = 0: double support until the first swing starts, the swing of the left foot, the transit that follows
    at0.element_list = {element(false, 0.0, 0.0, 2.1), element(true, 0.0, -0.1, 2.9), element(false, 0.1, 0.0, 3.1)};
    // t = 2.5: on the right foot, then the steps to (0.2, 0.1), (0.4, -0.1), (0.6, 0.1), (0.8, -0.1) in turn
    at25.element_list = {element(true, 0.0, -0.1, 2.9),  element(false, 0.1, 0.0, 3.1), element(true, 0.2, 0.1, 3.9),
                         element(false, 0.3, 0.0, 4.1),  element(true, 0.4, -0.1, 4.9), element(false, 0.5, 0.0, 5.1),
                         element(true, 0.6, 0.1, 5.9),   element(false, 0.7, 0.0, 6.1)};
    plan_and_print(mpc, at0, 0.0, 0.0);
    plan_and_print(mpc, at25, 0.02, 2.5);
    return 0;
  }
  catch(const std::exception & e)
  {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
