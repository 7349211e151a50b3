/* PreviewZmpShimBase.h -- what the header shims PreviewControlZmp.h and SingularPreviewControlZmp.h share: the ccc_pvz_t
 * handle of include/ccc_amd.h, the sampling of a ref_zmp_func on the host and the two batched calls.
 */
#pragma once

#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ccc_amd.h"

#include "EigenLite.h"
#include "ShimCommon.h"

namespace CCC
{
namespace shim
{
/** The knots of a piecewise-linear reference ZMP, time -> ZMP, as FootstepManager keeps them in ref_zmp_list_. */
using RefZmpKnots = std::map<double, Vector2d>;

/** One ccc_pvz_t handle.  State triples are per axis in the order of the controller's x (ccc_amd.h). */
class PreviewZmpHandle
{
public:
  PreviewZmpHandle(const char * cls,
                   int kind,
                   double com_height,
                   double horizon_duration,
                   double horizon_dt,
                   double weight_zmp,
                   double weight_com_jerk,
                   int device)
  : cls_(cls), horizon_dt_(horizon_dt), off_(kind == CCC_PVZ_PREVIEW ? 1 : 0)
  {
    ccc_pvz_t * h = nullptr;
    if(ccc_pvz_create(kind, com_height, horizon_duration, horizon_dt, weight_zmp, weight_com_jerk, device, &h) != CCC_OK)
    {
      throw std::runtime_error("[" + cls_ + "] " + ccc_last_error_string());
    }
    handle_.reset(h, ccc_pvz_destroy);
    horizon_steps_ = ccc_pvz_horizon_steps(h);
  }

  /** ref_zmp_func sampled as planOnce() of the reference does: out[axis * N + i] = f(current_time + (i + off) dt)[axis]. */
  void sample(const std::function<Vector2d(double)> & ref_zmp_func, double current_time, double * out) const
  {
    for(int i = 0; i < horizon_steps_; i++)
    {
      const Vector2d z = ref_zmp_func(current_time + (i + off_) * horizon_dt_);
      out[i] = z[0];
      out[horizon_steps_ + i] = z[1];
    }
  }

  /** x0 [n][2][3], ref [n][2][N] -> planned ZMPs. */
  std::vector<Vector2d> plan(const std::vector<double> & x0, const std::vector<double> & ref, double control_dt) const
  {
    const size_t n = x0.size() / 6;
    std::vector<double> zmp(2 * n);
    check(ccc_pvz_plan_batch(handle_.get(), static_cast<int64_t>(n), x0.data(), ref.data(), control_dt, zmp.data(), nullptr));
    return pairs(zmp);
  }

  /** x0 [n][2][3] and one knot list and current time per instance -> planned ZMPs; statuses: CCC_STATUS_* per instance. */
  std::vector<Vector2d> planKnots(const std::vector<double> & x0,
                                  const std::vector<RefZmpKnots> & knots,
                                  const std::vector<double> & current_times,
                                  double control_dt,
                                  std::vector<int32_t> & statuses) const
  {
    const size_t n = knots.size();
    if(x0.size() != 6 * n || current_times.size() != n)
    {
      throw std::runtime_error("[" + cls_ + "::planOnceBatchKnots] argument sizes differ");
    }
    std::vector<int32_t> num(n);
    std::vector<double> time(CCC_PVZ_MAX_KNOTS * n, 0.0), z(2 * CCC_PVZ_MAX_KNOTS * n, 0.0), zmp(2 * n);
    for(size_t k = 0; k < n; k++)
    {
      num[k] = static_cast<int32_t>(knots[k].size()); // (more than 32: the kernel flags the instance)
      size_t i = 0;
      for(auto it = knots[k].begin(); it != knots[k].end() && i < CCC_PVZ_MAX_KNOTS; ++it, ++i)
      {
        time[CCC_PVZ_MAX_KNOTS * k + i] = it->first;
        z[2 * (CCC_PVZ_MAX_KNOTS * k + i)] = it->second[0];
        z[2 * (CCC_PVZ_MAX_KNOTS * k + i) + 1] = it->second[1];
      }
    }
    statuses.assign(n, 0);
    check(ccc_pvz_plan_knots_batch(handle_.get(), static_cast<int64_t>(n), num.data(), time.data(), z.data(), x0.data(),
                                   current_times.data(), control_dt, zmp.data(), nullptr, statuses.data()));
    reportStatus(cls_.c_str(), statuses);
    return pairs(zmp);
  }

  ccc_pvz_t * get() const
  {
    return handle_.get();
  }

  std::string cls_;
  double horizon_dt_ = 0;
  int horizon_steps_ = -1, off_ = 0;

protected:
  void check(int rc) const
  {
    if(rc != CCC_OK) throw std::runtime_error("[" + cls_ + "] " + ccc_last_error_string());
  }
  static std::vector<Vector2d> pairs(const std::vector<double> & zmp)
  {
    std::vector<Vector2d> out(zmp.size() / 2);
    for(size_t k = 0; k < out.size(); k++) out[k] = Vector2d(zmp[2 * k], zmp[2 * k + 1]);
    return out;
  }
  std::shared_ptr<ccc_pvz_t> handle_;
};
} // namespace shim
} // namespace CCC
