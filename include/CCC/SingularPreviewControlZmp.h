/* SingularPreviewControlZmp.h -- drop-in header shim: the class surface of
 * /root/reference/include/CCC/SingularPreviewControlZmp.h:19-130 over the MI355X C-ABI (include/ccc_amd.h).  Same namespace,
 * classes (SingularPreviewControlZmp1d, SingularPreviewControlZmp), nested InitialParam, constructors and planOnce()
 * signatures; planOnceBatch() and planOnceBatchKnots() are new.  As in the reference's procOnce
 * (src/SingularPreviewControlZmp.cpp:54) control_dt is used AS PASSED: the default of -1 is not replaced by horizon_dt,
 * whatever the reference's header comment says -- pass it.
 */
#pragma once

#include "PreviewZmpShimBase.h"

namespace CCC
{
/** \brief Singular preview control for one-dimensional CoM-ZMP model, run as the two-dimensional kernel with a zero second
    axis. */
class SingularPreviewControlZmp1d
{
  friend class SingularPreviewControlZmp;

public:
  /** \brief Initial parameter (SingularPreviewControlZmp.h:25-35). */
  struct InitialParam
  {
    double pos = 0;         //!< CoM position [m]
    double vel = 0;         //!< CoM velocity [m/s]
    double planned_zmp = 0; //!< Current ZMP planned in previous step [m]
  };

public:
  /** \brief Constructor (SingularPreviewControlZmp.h:43-47).  \param device HIP device ordinal (new) */
  SingularPreviewControlZmp1d(double com_height, double horizon_duration, double horizon_dt, int device = 0)
  : handle_("SingularPreviewControlZmp", CCC_PVZ_SINGULAR, com_height, horizon_duration, horizon_dt, 0.0, 0.0, device),
    horizon_dt_(handle_.horizon_dt_), horizon_steps_(handle_.horizon_steps_)
  {
  }

  /** \brief Plan one step (SingularPreviewControlZmp.h:56-59). */
  double planOnce(const std::function<double(double)> & ref_zmp_func,
                  const InitialParam & initial_param,
                  double current_time,
                  double control_dt = -1) const
  {
    std::vector<double> x0 = {initial_param.planned_zmp, initial_param.pos, initial_param.vel, 0.0, 0.0, 0.0};
    std::vector<double> ref(2 * static_cast<size_t>(horizon_steps_), 0.0);
    handle_.sample([&](double t) { return Vector2d(ref_zmp_func(t), 0.0); }, current_time, ref.data());
    return handle_.plan(x0, ref, control_dt)[0][0];
  }

protected:
  shim::PreviewZmpHandle handle_;
  double horizon_dt_ = 0;  //!< Discretization timestep in horizon [sec]
  int horizon_steps_ = -1; //!< Number of steps in horizon
};

/** \brief Singular preview control for CoM-ZMP model, batched on MI355X.  Mirrors CCC::SingularPreviewControlZmp,
    /root/reference/include/CCC/SingularPreviewControlZmp.h:86-130. */
class SingularPreviewControlZmp
{
public:
  /** \brief Initial parameter (SingularPreviewControlZmp.h:90-102). */
  struct InitialParam
  {
    Vector2d pos = Vector2d::Zero();         //!< CoM position [m]
    Vector2d vel = Vector2d::Zero();         //!< CoM velocity [m/s]
    Vector2d planned_zmp = Vector2d::Zero(); //!< Current ZMP planned in previous step [m]
  };

  using RefZmpKnots = shim::RefZmpKnots;

public:
  /** \brief Constructor (SingularPreviewControlZmp.h:110-113).  \param device HIP device ordinal (new) */
  SingularPreviewControlZmp(double com_height, double horizon_duration, double horizon_dt, int device = 0)
  : spc_1d_(std::make_shared<SingularPreviewControlZmp1d>(com_height, horizon_duration, horizon_dt, device))
  {
  }

  /** \brief Plan one step (SingularPreviewControlZmp.h:122-125, src/SingularPreviewControlZmp.cpp:59-88). */
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
    const size_t n = ref_zmp_funcs.size(), N = static_cast<size_t>(spc_1d_->horizon_steps_);
    if(initial_params.size() != n || current_times.size() != n)
    {
      throw std::runtime_error("[SingularPreviewControlZmp::planOnceBatch] argument sizes differ");
    }
    std::vector<double> ref(2 * N * n);
    for(size_t k = 0; k < n; k++) spc_1d_->handle_.sample(ref_zmp_funcs[k], current_times[k], &ref[2 * N * k]);
    return spc_1d_->handle_.plan(flatten(initial_params), ref, control_dt);
  }

  /** \brief Plan n independent instances whose reference ZMP is the linear interpolation of knots (new): no sampling, the
      cost is per knot.  An instance whose knots do not cover every sample time comes back NaN, CCC_STATUS_INFEASIBLE. */
  std::vector<Vector2d> planOnceBatchKnots(const std::vector<RefZmpKnots> & knots,
                                           const std::vector<InitialParam> & initial_params,
                                           const std::vector<double> & current_times,
                                           double control_dt = -1)
  {
    return spc_1d_->handle_.planKnots(flatten(initial_params), knots, current_times, control_dt, last_status_);
  }

  /** \brief Status of the last planOnceBatchKnots(), one per instance (new). */
  const std::vector<int32_t> & lastStatuses() const
  {
    return last_status_;
  }

public:
  std::shared_ptr<SingularPreviewControlZmp1d> spc_1d_; //!< One-dimensional preview control (owns the handle)

protected:
  static std::vector<double> flatten(const std::vector<InitialParam> & ips)
  {
    std::vector<double> x0(6 * ips.size());
    for(size_t k = 0; k < ips.size(); k++)
      for(int a = 0; a < 2; a++)
      {
        x0[6 * k + 3 * a] = ips[k].planned_zmp[a];
        x0[6 * k + 3 * a + 1] = ips[k].pos[a];
        x0[6 * k + 3 * a + 2] = ips[k].vel[a];
      }
    return x0;
  }
  std::vector<int32_t> last_status_;
};
} // namespace CCC
