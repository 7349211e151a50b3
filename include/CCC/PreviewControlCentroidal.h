/* PreviewControlCentroidal.h -- drop-in header shim: the class surface of
 * /root/reference/include/CCC/PreviewControlCentroidal.h:137-262 over the MI355X C-ABI (include/ccc_amd.h).  Same
 * namespace, class, nested MotionParam / RefData / InitialParam / WeightParam, constructor and planOnce() signature.
 * sva::MotionVecd / sva::ForceVecd are stood in for by sva::MotionVecd / sva::ForceVecd below when SpaceVecAlg is not
 * installed (angular() / linear(), moment() / force(), vector() order [angular; linear]), ForceColl::Contact by
 * CCC::Contact (EigenLite.h), and mc_rtc::Configuration by the plain struct ccc_wrench_dist_config_t.
 * planOnceBatch() is new: n independent planOnce() problems in one launch.
 */
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ccc_amd.h"

#include "EigenLite.h"
#include "ShimCommon.h"

#if __has_include(<SpaceVecAlg/SpaceVecAlg>)
#  include <SpaceVecAlg/SpaceVecAlg>
#else
namespace sva
{
/** Stand-in for sva::MotionVecd: vector() = [angular; linear]. */
struct MotionVecd
{
  CCC::Vector3d angular_, linear_;
  MotionVecd() = default;
  MotionVecd(const CCC::Vector3d & a, const CCC::Vector3d & l) : angular_(a), linear_(l) {}
  static MotionVecd Zero()
  {
    return MotionVecd();
  }
  CCC::Vector3d & angular()
  {
    return angular_;
  }
  CCC::Vector3d & linear()
  {
    return linear_;
  }
  const CCC::Vector3d & angular() const
  {
    return angular_;
  }
  const CCC::Vector3d & linear() const
  {
    return linear_;
  }
  std::array<double, 6> vector() const
  {
    return {angular_[0], angular_[1], angular_[2], linear_[0], linear_[1], linear_[2]};
  }
};
/** Stand-in for sva::ForceVecd: vector() = [moment; force]. */
struct ForceVecd
{
  CCC::Vector3d moment_, force_;
  ForceVecd() = default;
  ForceVecd(const CCC::Vector3d & m, const CCC::Vector3d & f) : moment_(m), force_(f) {}
  static ForceVecd Zero()
  {
    return ForceVecd();
  }
  CCC::Vector3d & moment()
  {
    return moment_;
  }
  CCC::Vector3d & couple()
  {
    return moment_;
  }
  CCC::Vector3d & force()
  {
    return force_;
  }
  const CCC::Vector3d & moment() const
  {
    return moment_;
  }
  const CCC::Vector3d & force() const
  {
    return force_;
  }
  std::array<double, 6> vector() const
  {
    return {moment_[0], moment_[1], moment_[2], force_[0], force_[1], force_[2]};
  }
};
} // namespace sva
#endif

namespace CCC
{
/** \brief Preview control for the centroidal model with the wrench distribution on the device, batched on MI355X.
    Mirrors CCC::PreviewControlCentroidal, /root/reference/include/CCC/PreviewControlCentroidal.h:137-262. */
class PreviewControlCentroidal
{
public:
  /** \brief Motion parameter (PreviewControlCentroidal.h:141-147). */
  struct MotionParam
  {
    std::vector<std::shared_ptr<Contact>> contact_list; //!< Contact list
  };

  /** \brief Reference data (PreviewControlCentroidal.h:150-159). */
  struct RefData
  {
    sva::MotionVecd pos = sva::MotionVecd::Zero();   //!< CoM position [m] and base link orientation [rad]
    sva::ForceVecd wrench = sva::ForceVecd::Zero();  //!< Force [N] and moment [Nm]
  };

  /** \brief Initial parameter (PreviewControlCentroidal.h:162-179). */
  struct InitialParam
  {
    sva::MotionVecd pos = sva::MotionVecd::Zero(); //!< CoM position [m] and base link orientation [rad]
    sva::MotionVecd vel = sva::MotionVecd::Zero(); //!< CoM velocity [m/s] and base link angular velocity [rad/s]
    sva::MotionVecd acc = sva::MotionVecd::Zero(); //!< CoM acceleration and base link angular acceleration
  };

  /** \brief Weight parameter (PreviewControlCentroidal.h:182-218, same defaults). */
  struct WeightParam
  {
    sva::MotionVecd pos;    //!< Position weight
    sva::ForceVecd wrench;  //!< Wrench weight
    sva::MotionVecd jerk;   //!< Jerk weight
    ccc_wrench_dist_config_t wrench_dist_config; //!< Configuration of wrench distribution (plain struct)

    WeightParam(const sva::MotionVecd & _pos = sva::MotionVecd(Vector3d(1e2, 1e2, 1e2), Vector3d(2e2, 2e2, 2e2)),
                const sva::ForceVecd & _wrench = sva::ForceVecd(Vector3d(5e-3, 5e-3, 5e-3), Vector3d(5e-4, 5e-4, 5e-4)),
                const sva::MotionVecd & _jerk = sva::MotionVecd(Vector3d::Constant(1e-8), Vector3d::Constant(1e-8)),
                const ccc_wrench_dist_config_t * _wrench_dist_config = nullptr)
    : pos(_pos), wrench(_wrench), jerk(_jerk)
    {
      ccc_wrench_dist_default_config(&wrench_dist_config);
      if(_wrench_dist_config) wrench_dist_config = *_wrench_dist_config;
    }
  };

public:
  /** \brief Constructor (PreviewControlCentroidal.h:228-232, src/PreviewControlCentroidal.cpp:74-89).
      \param max_ridges ridge slots per contact list: 16, 32 or 64 (new)
      \param device HIP device ordinal (new) */
  PreviewControlCentroidal(double mass,
                           const Vector3d & moment_of_inertia,
                           double horizon_duration,
                           double horizon_dt,
                           const WeightParam & weight_param = WeightParam(),
                           int max_ridges = 16,
                           int device = 0)
  : mass_(mass), max_ridges_(max_ridges)
  {
    const auto wp = weight_param.pos.vector(), ww = weight_param.wrench.vector(), wj = weight_param.jerk.vector();
    ccc_pcc_t * h = nullptr;
    check(ccc_pcc_create(mass, moment_of_inertia.v, horizon_duration, horizon_dt, wp.data(), ww.data(), wj.data(),
                         &weight_param.wrench_dist_config, max_ridges, device, &h));
    handle_.reset(h, ccc_pcc_destroy);
    horizon_steps_ = ccc_pcc_horizon_steps(h);
    horizon_dt_ = horizon_dt;
  }

  /** \brief Plan one step (PreviewControlCentroidal.h:243-247, src/PreviewControlCentroidal.cpp:91-130).
      \returns planned wrench, projected onto the contact list */
  sva::ForceVecd planOnce(const MotionParam & motion_param,
                          const std::function<RefData(double)> & ref_data_func,
                          const InitialParam & initial_param,
                          double current_time,
                          double control_dt = -1)
  {
    return planOnceBatch({motion_param}, {ref_data_func}, {initial_param}, {current_time}, control_dt)[0];
  }

  /** \brief Plan n independent instances in one launch (new). */
  std::vector<sva::ForceVecd> planOnceBatch(const std::vector<MotionParam> & motion_params,
                                            const std::vector<std::function<RefData(double)>> & ref_data_funcs,
                                            const std::vector<InitialParam> & initial_params,
                                            const std::vector<double> & current_times,
                                            double control_dt = -1)
  {
    const size_t n = motion_params.size(), N = static_cast<size_t>(horizon_steps_), M = static_cast<size_t>(max_ridges_);
    if(ref_data_funcs.size() != n || initial_params.size() != n || current_times.size() != n)
    {
      throw std::runtime_error("[PreviewControlCentroidal::planOnceBatch] argument sizes differ");
    }
    std::vector<double> x0(18 * n), ref(12 * N * n), vertex(3 * M * n, 0.0), ridge(3 * M * n, 0.0), wrench(6 * n);
    std::vector<int32_t> dim(n, 0);
    for(size_t k = 0; k < n; k++)
    {
      const auto p = initial_params[k].pos.vector(), v = initial_params[k].vel.vector(), a = initial_params[k].acc.vector();
      for(size_t i = 0; i < 6; i++)
      {
        x0[18 * k + i] = p[i];
        x0[18 * k + 6 + i] = v[i];
        x0[18 * k + 12 + i] = a[i];
      }
      for(size_t i = 0; i < N; i++) // src/PreviewControlCentroidal.cpp:102-108
      {
        const RefData rd = ref_data_funcs[k](current_times[k] + static_cast<double>(i + 1) * horizon_dt_);
        const auto rp = rd.pos.vector(), rw = rd.wrench.vector();
        for(size_t j = 0; j < 6; j++)
        {
          ref[(k * N + i) * 12 + j] = rp[j];
          ref[(k * N + i) * 12 + 6 + j] = rw[j];
        }
      }
      size_t r = 0;
      for(const auto & contact : motion_params[k].contact_list)
        for(const auto & vr : contact->vertexWithRidgeList_)
          for(const auto & rd : vr.ridgeList)
          {
            if(r >= M) throw std::runtime_error("[PreviewControlCentroidal] the contact list has more ridges than max_ridges");
            for(size_t j = 0; j < 3; j++)
            {
              vertex[(k * M + r) * 3 + j] = vr.vertex[static_cast<int>(j)];
              ridge[(k * M + r) * 3 + j] = rd[static_cast<int>(j)];
            }
            r++;
          }
      dim[k] = static_cast<int32_t>(r);
    }
    last_status_.assign(n, 0);
    check(ccc_pcc_plan_batch(handle_.get(), static_cast<int64_t>(n), x0.data(), ref.data(), dim.data(), vertex.data(),
                             ridge.data(), control_dt, wrench.data(), nullptr, nullptr, last_status_.data()));
    shim::reportStatus("PreviewControlCentroidal", last_status_);
    std::vector<sva::ForceVecd> out(n);
    for(size_t k = 0; k < n; k++)
      out[k] = sva::ForceVecd(Vector3d(wrench[6 * k], wrench[6 * k + 1], wrench[6 * k + 2]),
                              Vector3d(wrench[6 * k + 3], wrench[6 * k + 4], wrench[6 * k + 5]));
    return out;
  }

  /** \brief The C-ABI handle, for the flat-array entry points of ccc_amd.h. */
  ccc_pcc_t * handle() const
  {
    return handle_.get();
  }

  /** \brief Solver status of the last call, one per instance: (iterations << 8) | CCC_STATUS_* (new). */
  const std::vector<int32_t> & lastStatuses() const
  {
    return last_status_;
  }

public:
  double mass_ = 0;        //!< Robot mass [kg]
  double horizon_dt_ = 0;  //!< Discretization timestep in horizon [sec]
  int horizon_steps_ = 0;  //!< Number of steps in horizon
  int max_ridges_ = 16;    //!< Ridge slots per contact list

protected:
  static void check(int rc)
  {
    if(rc != CCC_OK)
    {
      throw std::runtime_error(std::string("[PreviewControlCentroidal] ") + ccc_last_error_string());
    }
  }

protected:
  std::shared_ptr<ccc_pcc_t> handle_;
  std::vector<int32_t> last_status_;
};
} // namespace CCC
