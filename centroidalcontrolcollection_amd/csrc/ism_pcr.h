// ism_pcr.h -- what csrc/ism.hip (one plan) and csrc/ism_loop.hip (the closed loop) share: the handle, the constants of
// the tridiagonal path.  Its solver body, which both kernels include, is ism_pcr_body.inc.
#pragma once

#include "common.h"
#include "wave_group.h"

struct ccc_ism
{
  int device = 0;
  int N = 0;
  double com_height = 0, horizon_duration = 0, horizon_dt = 0, w_zmp = 1.0, w_zmp_vel = 1e-3;
  double *dG = nullptr, *dWc = nullptr;
  double * dAt = nullptr; // [N] stability row in ZMP-position variables (ism_plan_pcr_kernel, ism_closed_loop_kernel)
  double a0_dt = 0;
  int * redo = nullptr;   // [1 + 2 n]: count, list of QPs handed to the tableau kernel
  int64_t redo_cap = 0;
  int num_cu = 0;
  // staging for the host-pointer entry point
  int64_t cap = 0;
  double *d_in = nullptr, *d_out = nullptr;
  int32_t * d_status = nullptr;
  hipStream_t stream = nullptr;
  // development switches, read ONCE in ccc_ism_create (never per launch)
  bool env_tableau = false;
  int env_pcr_outer = -1; // CCC_ISM_PCR_OUTER: the outer budget (small values exercise the list); < 0: the default
};

namespace ccc_amd
{
constexpr double kIsmInf = __builtin_huge_val();
constexpr int kPcrNP = 128;
constexpr int kPcrOuter = 40, kPcrInner = 30;

struct IsmPcrDev
{
  int N;
  const double * at; // [N]  (a_i - a_{i+1}) / dt, a_N = 0: the stability row in y
  double a0_dt;      // a_0 / dt
  double w_zmp, w_vel, dt;
};

__device__ __forceinline__ double ism_lane_value(double v, int k) // k uniform: two v_readlane_b32
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

} // namespace ccc_amd
