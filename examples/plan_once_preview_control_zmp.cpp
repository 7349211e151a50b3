// plan_once_preview_control_zmp.cpp -- planOnce() and planOnceBatchKnots() of CCC::PreviewControlZmp and
// CCC::SingularPreviewControlZmp through the drop-in headers (host C++ -> header shim -> C-ABI -> HIP kernel) with the
// parameters of /root/reference/tests/src/TestPreviewControlZmp.cpp:17-26 and the reference ZMP of its first step: at the
// middle of the feet until 2.0 s, over the right foot from 2.1 s to 2.9 s, at the new middle from 3.1 s.  The same plan
// comes back from the sampled std::function and from the four knots.
#include <CCC/PreviewControlZmp.h>
#include <CCC/SingularPreviewControlZmp.h>

#include <cstdio>

int main()
{
  try
  {
    const CCC::shim::RefZmpKnots knots = {{0.0, CCC::Vector2d(0.0, 0.0)},
                                          {2.0, CCC::Vector2d(0.0, 0.0)},
                                          {2.1, CCC::Vector2d(0.0, -0.1)},
                                          {2.9, CCC::Vector2d(0.0, -0.1)},
                                          {3.1, CCC::Vector2d(0.1, 0.0)},
                                          {10.0, CCC::Vector2d(0.1, 0.0)}};
    const auto ref_zmp_func = [&](double t) {
      auto hi = knots.upper_bound(t), lo = std::prev(hi);
      const double ratio = (t - lo->first) / (hi->first - lo->first);
      return CCC::Vector2d((1 - ratio) * lo->second[0] + ratio * hi->second[0],
                           (1 - ratio) * lo->second[1] + ratio * hi->second[1]);
    };
    const double t = 1.0, sim_dt = 0.005;

    CCC::PreviewControlZmp pc(1.0, 2.0, 0.01);
    CCC::PreviewControlZmp::InitialParam ip;
    ip.pos = CCC::Vector2d(0.01, -0.005);
    ip.vel = CCC::Vector2d(0.05, -0.02);
    ip.acc = CCC::Vector2d(0.1, 0.0);
    const CCC::Vector2d a = pc.planOnce(ref_zmp_func, ip, t, sim_dt), b = pc.planOnceBatchKnots({knots}, {ip}, {t}, sim_dt)[0];
    std::printf("PreviewControlZmp sampled= %.17g %.17g knots= %.17g %.17g status=%d\n", a[0], a[1], b[0], b[1],
                CCC_STATUS_CODE(pc.lastStatuses()[0]));

    CCC::SingularPreviewControlZmp spc(1.0, 2.0, 0.01);
    CCC::SingularPreviewControlZmp::InitialParam sip;
    sip.pos = ip.pos;
    sip.vel = ip.vel;
    sip.planned_zmp = CCC::Vector2d(0.0, 0.001);
    const CCC::Vector2d c = spc.planOnce(ref_zmp_func, sip, t, sim_dt), d = spc.planOnceBatchKnots({knots}, {sip}, {t}, sim_dt)[0];
    std::printf("SingularPreviewControlZmp sampled= %.17g %.17g knots= %.17g %.17g status=%d\n", c[0], c[1], d[0], d[1],
                CCC_STATUS_CODE(spc.lastStatuses()[0]));
    return 0;
  }
  catch(const std::exception & e)
  {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
