/* PreviewControlZmp.h -- drop-in header shim: the class surface of /root/reference/include/CCC/PreviewControlZmp.h:16-140
 * over the MI355X C-ABI (include/ccc_amd.h).  Same namespace, classes (PreviewControlZmp1d, PreviewControlZmp), nested
 * InitialParam / WeightParam, constructors and planOnce() signatures; planOnce() samples ref_zmp_func on the host and plans
 * one instance.  planOnceBatch() (sampled) and planOnceBatchKnots() (piecewise-linear references by their knots) are new:
 * n independent planOnce() problems in one launch.
 */
#pragma once

#include "PreviewZmpShimBase.h"

namespace CCC
{
/** \brief Preview control for one-dimensional CoM-ZMP model, run as the two-dimensional kernel with a zero second axis. */
class PreviewControlZmp1d
{
  friend class PreviewControlZmp;

public:
  /** \brief Initial parameter: CoM position, velocity and acceleration (PreviewControlZmp.h:25). */
  using InitialParam = Vector3d;

  /** \brief Weight parameter (PreviewControlZmp.h:28-44, same defaults). */
  struct WeightParam
  {
    double zmp;      //!< ZMP weight
    double com_jerk; //!< CoM jerk weight
    WeightParam(double _zmp = 1.0, double _com_jerk = 1e-8) : zmp(_zmp), com_jerk(_com_jerk) {}
  };

public:
  /** \brief Constructor (PreviewControlZmp.h:55-64).  \param device HIP device ordinal (new) */
  PreviewControlZmp1d(double com_height,
                      double horizon_duration,
                      double horizon_dt,
                      const WeightParam & weight_param = WeightParam(),
                      int device = 0)
  : handle_("PreviewControlZmp", CCC_PVZ_PREVIEW, com_height, horizon_duration, horizon_dt, weight_param.zmp,
            weight_param.com_jerk, device),
    horizon_dt_(handle_.horizon_dt_), horizon_steps_(handle_.horizon_steps_)
  {
  }

  /** \brief Plan one step (PreviewControlZmp.h:73-76). */
  double planOnce(const std::function<double(double)> & ref_zmp_func,
                  const InitialParam & initial_param,
                  double current_time,
                  double control_dt = -1) const
  {
    std::vector<double> x0 = {initial_param[0], initial_param[1], initial_param[2], 0.0, 0.0, 0.0};
    std::vector<double> ref(2 * static_cast<size_t>(horizon_steps_), 0.0);
    handle_.sample([&](double t) { return Vector2d(ref_zmp_func(t), 0.0); }, current_time, ref.data());
    return handle_.plan(x0, ref, control_dt)[0][0];
  }

protected:
  shim::PreviewZmpHandle handle_;

public:
  double horizon_dt_ = 0;  //!< Discretization timestep in horizon [sec]
  int horizon_steps_ = -1; //!< Number of steps in horizon
};

/** \brief Preview control for CoM-ZMP model, batched on MI355X.  Mirrors CCC::PreviewControlZmp,
    /root/reference/include/CCC/PreviewControlZmp.h:92-140. */
class PreviewControlZmp
{
public:
  /** \brief Initial parameter (PreviewControlZmp.h:96-108). */
  struct InitialParam
  {
    Vector2d pos = Vector2d::Zero(); //!< CoM position [m]
    Vector2d vel = Vector2d::Zero(); //!< CoM velocity [m/s]
    Vector2d acc = Vector2d::Zero(); //!< CoM acceleration [m/s^2]
  };

  using RefZmpKnots = shim::RefZmpKnots;

public:
  /** \brief Constructor (PreviewControlZmp.h:117-123).  \param device HIP device ordinal (new) */
  PreviewControlZmp(double com_height,
                    double horizon_duration,
                    double horizon_dt,
                    const PreviewControlZmp1d::WeightParam & weight_param = PreviewControlZmp1d::WeightParam(),
                    int device = 0)
  : preview_control_1d_(std::make_shared<PreviewControlZmp1d>(com_height, horizon_duration, horizon_dt, weight_param, device))
  {
  }

  /** \brief Plan one step (PreviewControlZmp.h:132-135, src/PreviewControlZmp.cpp:51-76). */
  Vector2d planOnce(const std::function<Vector2d(double)> & ref_zmp_func,
                    const InitialParam & initial_param,
                    double current_time,
                    double control_dt = -1) const
  {
    return planOnceBatch({ref_zmp_func}, {initial_param}, {current_time}, control_dt)[0];
  }

  /** \brief Plan n independent instances in one launch, each ref_zmp_func sampled on the host (new). */
  std::vector<Vector2d> planOnceBatch(const std::vector<std::function<Vector2d(double)>> & ref_zmp_funcs,
                                      const std::vector<InitialParam> & initial_params,
                                      const std::vector<double> & current_times,
                                      double control_dt = -1) const
  {
    const size_t n = ref_zmp_funcs.size(), N = static_cast<size_t>(preview_control_1d_->horizon_steps_);
    if(initial_params.size() != n || current_times.size() != n)
    {
      throw std::runtime_error("[PreviewControlZmp::planOnceBatch] argument sizes differ");
    }
    std::vector<double> ref(2 * N * n);
    for(size_t k = 0; k < n; k++) preview_control_1d_->handle_.sample(ref_zmp_funcs[k], current_times[k], &ref[2 * N * k]);
    return preview_control_1d_->handle_.plan(flatten(initial_params), ref, control_dt);
  }

  /** \brief Plan n independent instances whose reference ZMP is the linear interpolation of knots (new): no sampling, the
      cost is per knot.  An instance whose knots do not cover every sample time comes back NaN, CCC_STATUS_INFEASIBLE. */
  std::vector<Vector2d> planOnceBatchKnots(const std::vector<RefZmpKnots> & knots,
                                           const std::vector<InitialParam> & initial_params,
                                           const std::vector<double> & current_times,
                                           double control_dt = -1)
  {
    return preview_control_1d_->handle_.planKnots(flatten(initial_params), knots, current_times, control_dt, last_status_);
  }

  /** \brief Status of the last planOnceBatchKnots(), one per instance (new). */
  const std::vector<int32_t> & lastStatuses() const
  {
    return last_status_;
  }

public:
  std::shared_ptr<PreviewControlZmp1d> preview_control_1d_; //!< One-dimensional preview control (owns the handle)

protected:
  static std::vector<double> flatten(const std::vector<InitialParam> & ips)
  {
    std::vector<double> x0(6 * ips.size());
    for(size_t k = 0; k < ips.size(); k++)
      for(int a = 0; a < 2; a++)
      {
        x0[6 * k + 3 * a] = ips[k].pos[a];
        x0[6 * k + 3 * a + 1] = ips[k].vel[a];
        x0[6 * k + 3 * a + 2] = ips[k].acc[a];
      }
    return x0;
  }
  std::vector<int32_t> last_status_;
};
} // namespace CCC
