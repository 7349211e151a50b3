/* StepMpc.h -- drop-in header shim: the class surface of /root/reference/include/CCC/StepMpc.h:17-240 over the MI355X
 * C-ABI (include/ccc_amd.h).  Same namespace, classes (StepMpc1d, StepMpc), nested RefData::Element / PlannedData /
 * InitialParam / WeightParam, constructors and planOnce() signatures.  planOnceBatch() is new: n independent planOnce()
 * problems in one launch.  The reference solves the normal equations of the least-squares problem; the kernel factors
 * the stacked rows themselves (csrc/step_mpc.h), so the plans agree to what the normal equations leave of them.
 */
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ccc_amd.h"

#include "EigenLite.h"
#include "ShimCommon.h"

namespace CCC
{
/** \brief One-dimensional footstep-adapting MPC (StepMpc.h:17-152), run as the two-dimensional kernel with a zero second
    axis. */
class StepMpc1d
{
  friend class StepMpc;

public:
  /** \brief Reference data (StepMpc.h:37-58). */
  struct RefData
  {
    struct Element
    {
      bool is_single_support = true; //!< Whether it is in single support phase
      double zmp = 0;                //!< ZMP [m]
      double end_time = 0;           //!< End time [sec]
    };
    /** At least one and at most CCC_STEP_MAX_ELEMENTS elements; no two consecutive double support phases. */
    std::vector<Element> element_list;
  };

  /** \brief Planned data (StepMpc.h:61-71). */
  struct PlannedData
  {
    double current_zmp = 0;              //!< Current ZMP [m]
    std::optional<double> next_foot_zmp; //!< ZMP of next foot [m]; null if no future single support is in the horizon
  };

  /** \brief Initial parameter: CoM position, CoM velocity (StepMpc.h:77). */
  using InitialParam = Vector2d;

  /** \brief Weight parameter (StepMpc.h:80-123, same defaults). */
  struct WeightParam
  {
    double free_zmp, fixed_zmp, double_support, pos, vel, capture_point_abs, capture_point_rel;
    WeightParam(double _free_zmp = 1e-2,
                double _fixed_zmp = 1e0,
                double _double_support = 1e0,
                double _pos = 0.0,
                double _vel = 0.0,
                double _capture_point_abs = 1e1,
                double _capture_point_rel = 1e1)
    : free_zmp(_free_zmp), fixed_zmp(_fixed_zmp), double_support(_double_support), pos(_pos), vel(_vel),
      capture_point_abs(_capture_point_abs), capture_point_rel(_capture_point_rel)
    {
    }
  };

public:
  /** \brief Constructor (StepMpc.h:130-133).  \param device HIP device ordinal (new) */
  StepMpc1d(double com_height, const WeightParam & weight_param = WeightParam(), int device = 0)
  : com_height_(com_height), weight_param_(weight_param)
  {
    const ccc_step_weights_t w = {weight_param.free_zmp, weight_param.fixed_zmp, weight_param.double_support,
                                  weight_param.pos,      weight_param.vel,       weight_param.capture_point_abs,
                                  weight_param.capture_point_rel};
    ccc_step_t * h = nullptr;
    if(ccc_step_create(com_height, &w, device, &h) != CCC_OK)
    {
      throw std::runtime_error(std::string("[StepMpc] ") + ccc_last_error_string());
    }
    handle_.reset(h, ccc_step_destroy);
  }

  /** \brief Plan one step (StepMpc.h:141). */
  PlannedData planOnce(const RefData & ref_data, const InitialParam & initial_param, double current_time)
  {
    Batch b(1);
    b.set(0, ref_data.element_list, current_time, [](const RefData::Element & e, int axis) { return axis == 0 ? e.zmp : 0.0; });
    b.x0[0] = initial_param[0];
    b.x0[2] = initial_param[1];
    b.run(handle_.get());
    PlannedData planned_data;
    planned_data.current_zmp = b.current[0];
    if(b.status[0] & CCC_STEP_HAS_NEXT_FOOT) planned_data.next_foot_zmp = b.foot[0];
    return planned_data;
  }

  /** \brief The C-ABI handle, for the flat-array entry points of ccc_amd.h. */
  ccc_step_t * handle() const
  {
    return handle_.get();
  }

protected:
  /** The flat arrays of ccc_step_plan_batch for n instances. */
  struct Batch
  {
    std::vector<int32_t> num, flags, status;
    std::vector<double> end_time, zmp, x0, time, current, foot;
    explicit Batch(size_t n)
    : num(n, 0), flags(16 * n, 0), status(n, 0), end_time(16 * n, 0.0), zmp(32 * n, 0.0), x0(4 * n, 0.0), time(n, 0.0),
      current(2 * n, 0.0), foot(2 * n, 0.0)
    {
    }
    template<class ElementList, class ZmpOf>
    void set(size_t k, const ElementList & list, double current_time, ZmpOf zmp_of)
    {
      if(list.empty() || list.size() > CCC_STEP_MAX_ELEMENTS)
      {
        throw std::runtime_error("[StepMpc] element_list must hold 1 .. 16 elements");
      }
      num[k] = static_cast<int32_t>(list.size());
      time[k] = current_time;
      for(size_t i = 0; i < list.size(); i++)
      {
        flags[16 * k + i] = list[i].is_single_support ? 1 : 0;
        end_time[16 * k + i] = list[i].end_time;
        zmp[32 * k + 2 * i] = zmp_of(list[i], 0);
        zmp[32 * k + 2 * i + 1] = zmp_of(list[i], 1);
      }
    }
    void run(ccc_step_t * h)
    {
      if(ccc_step_plan_batch(h, static_cast<int64_t>(num.size()), num.data(), flags.data(), end_time.data(), zmp.data(),
                             x0.data(), time.data(), current.data(), foot.data(), status.data())
         != CCC_OK)
      {
        throw std::runtime_error(std::string("[StepMpc] ") + ccc_last_error_string());
      }
      shim::reportStatus("StepMpc", status);
    }
  };

protected:
  double com_height_ = 0;    //!< Height of robot CoM [m]
  WeightParam weight_param_; //!< Weight parameter
  std::shared_ptr<ccc_step_t> handle_;
};

/** \brief Footstep-adapting MPC on the step-to-step dynamics, batched on MI355X.  Mirrors CCC::StepMpc,
    /root/reference/include/CCC/StepMpc.h:163-240. */
class StepMpc
{
public:
  /** \brief Reference data (StepMpc.h:167-190). */
  struct RefData
  {
    struct Element
    {
      bool is_single_support = true;   //!< Whether it is in single support phase
      Vector2d zmp = Vector2d::Zero(); //!< ZMP [m]
      double end_time = 0;             //!< End time [sec]
    };
    /** At least one and at most CCC_STEP_MAX_ELEMENTS elements; no two consecutive double support phases. */
    std::vector<Element> element_list;
  };

  /** \brief Planned data (StepMpc.h:193-205). */
  struct PlannedData
  {
    Vector2d current_zmp = Vector2d::Zero(); //!< Current ZMP [m]
    std::optional<Vector2d> next_foot_zmp;   //!< ZMP of next foot [m]; null if no future single support is in the horizon
  };

  /** \brief Initial parameter (StepMpc.h:208-217). */
  struct InitialParam
  {
    Vector2d pos = Vector2d::Zero(); //!< CoM position [m]
    Vector2d vel = Vector2d::Zero(); //!< CoM velocity [m/s]
  };

public:
  /** \brief Constructor (StepMpc.h:224-227).  \param device HIP device ordinal (new) */
  StepMpc(double com_height, const StepMpc1d::WeightParam & weight_param = StepMpc1d::WeightParam(), int device = 0)
  : mpc_1d_(std::make_shared<StepMpc1d>(com_height, weight_param, device))
  {
  }

  /** \brief Plan one step (StepMpc.h:235, src/StepMpc.cpp:202-247). */
  PlannedData planOnce(const RefData & ref_data, const InitialParam & initial_param, double current_time)
  {
    return planOnceBatch({ref_data}, {initial_param}, {current_time})[0];
  }

  /** \brief Plan n independent instances in one launch (new). */
  std::vector<PlannedData> planOnceBatch(const std::vector<RefData> & ref_data_list,
                                         const std::vector<InitialParam> & initial_params,
                                         const std::vector<double> & current_times)
  {
    const size_t n = ref_data_list.size();
    if(initial_params.size() != n || current_times.size() != n)
    {
      throw std::runtime_error("[StepMpc::planOnceBatch] argument sizes differ");
    }
    StepMpc1d::Batch b(n);
    for(size_t k = 0; k < n; k++)
    {
      b.set(k, ref_data_list[k].element_list, current_times[k],
            [](const RefData::Element & e, int axis) { return e.zmp[axis]; });
      b.x0[4 * k] = initial_params[k].pos[0];
      b.x0[4 * k + 1] = initial_params[k].pos[1];
      b.x0[4 * k + 2] = initial_params[k].vel[0];
      b.x0[4 * k + 3] = initial_params[k].vel[1];
    }
    b.run(mpc_1d_->handle());
    last_status_ = b.status;
    std::vector<PlannedData> out(n);
    for(size_t k = 0; k < n; k++)
    {
      out[k].current_zmp = Vector2d(b.current[2 * k], b.current[2 * k + 1]);
      if(b.status[k] & CCC_STEP_HAS_NEXT_FOOT) out[k].next_foot_zmp = Vector2d(b.foot[2 * k], b.foot[2 * k + 1]);
    }
    return out;
  }

  /** \brief The control loop of tests/src/TestStepMpc.cpp:55-116 for n instances in one launch (new): a thin forward to
      ccc_step_closed_loop_device (ccc_amd.h), whose argument list and layouts it shares.  All pointers are device pointers
      but disturb_times and params; asynchronous on `stream`. */
  void closedLoopBatch(int64_t n, int K, const double * foot0, double * foot_pos, const int32_t * foot_id,
                       const double * swing_start, const double * swing_end, const double * transit_end,
                       double * com_state, double t0, double sim_dt, int cycles,
                       const std::vector<double> & disturb_times = {}, double disturb_impulse = 0.0,
                       const ccc_step_loop_params_t * params = nullptr, int32_t * status = nullptr,
                       int32_t * updates = nullptr, double * traj_com = nullptr, double * traj_zmp = nullptr,
                       double * traj_next_foot = nullptr, void * stream = nullptr)
  {
    if(ccc_step_closed_loop_device(mpc_1d_->handle(), n, K, foot0, foot_pos, foot_id, swing_start, swing_end, transit_end,
                                   com_state, t0, sim_dt, cycles, static_cast<int>(disturb_times.size()),
                                   disturb_times.data(), disturb_impulse, params, status, updates, traj_com, traj_zmp,
                                   traj_next_foot, stream)
       != CCC_OK)
    {
      throw std::runtime_error(std::string("[StepMpc] ") + ccc_last_error_string());
    }
  }

  /** \brief Status of the last call, one per instance: CCC_STATUS_* | CCC_STEP_HAS_NEXT_FOOT (new). */
  const std::vector<int32_t> & lastStatuses() const
  {
    return last_status_;
  }

protected:
  std::shared_ptr<StepMpc1d> mpc_1d_; //!< One-dimensional linear MPC (owns the handle)
  std::vector<int32_t> last_status_;
};
} // namespace CCC
