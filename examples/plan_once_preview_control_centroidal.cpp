// plan_once_preview_control_centroidal.cpp -- planOnce() / planOnceBatch() of CCC::PreviewControlCentroidal through the
// drop-in header (host C++ -> header shim -> C-ABI -> HIP kernel) with the parameters, contact and reference of the first
// phase of /root/reference/tests/src/TestPreviewControlCentroidal.cpp:17-74.  Prints the projected wrenches.
#include <CCC/PreviewControlCentroidal.h>

#include <cstdio>

int main()
{
  try
  {
    using PCC = CCC::PreviewControlCentroidal;
    PCC pc(100.0, CCC::Vector3d(40.0, 20.0, 10.0), 2.0, 0.01);
    PCC::MotionParam motion_param;
    motion_param.contact_list.push_back(CCC::makeContactFromRect({CCC::Vector2d(-0.1, -0.1), CCC::Vector2d(0.1, 0.1)}));
    std::function<PCC::RefData(double)> ref_data_func = [](double t) {
      PCC::RefData ref_data;
      ref_data.pos.linear() = t + 1e-6 < 1.4 ? CCC::Vector3d(0.0, 0.0, 1.0) : CCC::Vector3d(0.25, 0.0, 1.2);
      return ref_data;
    };
    std::vector<PCC::InitialParam> ips(3);
    for(size_t k = 0; k < ips.size(); k++) ips[k].pos.linear() = CCC::Vector3d(0.01 * static_cast<double>(k), 0.0, 1.0);
    const auto one = pc.planOnce(motion_param, ref_data_func, ips[0], 0.0, 0.005).vector();
    std::printf("planOnce wrench= %.17g %.17g %.17g %.17g %.17g %.17g\n", one[0], one[1], one[2], one[3], one[4], one[5]);
    const auto all = pc.planOnceBatch({motion_param, motion_param, motion_param}, {ref_data_func, ref_data_func, ref_data_func},
                                      ips, {0.0, 0.5, 1.0}, 0.005);
    for(size_t k = 0; k < all.size(); k++)
    {
      const auto w = all[k].vector();
      std::printf("batch[%zu] wrench= %.17g %.17g %.17g %.17g %.17g %.17g status=%d\n", k, w[0], w[1], w[2], w[3], w[4], w[5],
                  CCC_STATUS_CODE(pc.lastStatuses()[k]));
    }
    return 0;
  }
  catch(const std::exception & e)
  {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
