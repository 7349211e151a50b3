// ism_loop.hip -- the closed loop of IntrinsicallyStableMpc in ONE launch: plan -> ComZmpSim2d::update -> disturbance,
// `cycles` times, for n instances, the QP of every cycle warm-started from the one before.
//
// Path replaced (reference file:line under /root/reference):
//   tests/src/TestIntrinsicallyStableMpc.cpp:55-100   the control loop (capture point :67, planOnce, the limit check
//                                                     :84-85, t += sim_dt, update, addDisturb :92-99)
//   tests/src/FootstepManager.h:179-196,242-254        zmpLimits, as csrc/zmp_loop.hip restates it
//   tests/src/FootstepManager.h:228-237,370-380        refZmp (linear interpolation) / makeIntrinsicallyStableMpcRefData
//   tests/src/SimModels.h:11-41,125-129                ComZmpSimModel1d (exact ZOH), addDisturb (x impulse on both axes)
//   src/IntrinsicallyStableMpc.cpp:63-104              procOnce, in the ZMP-position variables of csrc/ism.hip
//
// Work split: the two axes of an instance never interact (two 1-d models; limits, reference and disturbance per axis),
// so ONE WAVEFRONT OWNS ONE AXIS OF ONE INSTANCE FOR ALL CYCLES; four wavefronts per workgroup, no workgroup barrier
// and no wait between wavefronts; a wavefront whose axis stops exits.
// On chip across the cycles: CoM position / velocity, planned ZMP, t (uniform over the wavefront); y, the clamped flags
// and the constants (at, diagonal) of the lane's two rows (row `lane` and row `lane + 64`: N <= 127); nu.
// LDS per wavefront (IsmLoopSlice): the six exchange arrays of the cyclic reduction [6][128] f64 = 6144 B, the knots of
// the axis [32] + [32] f64 = 512 B, the footstep timeline of the axis (swing start, swing end, position [16] f64, foot id
// [16] i32, the two first positions) = 464 B: 7120 B, 28480 B per workgroup.  It is filled once; after that nothing is
// read from HBM, and a cycle writes only its trajectory record (lane 0).
#include "common.h"
#include "ism_pcr.h"
#include "wave_group.h"

#include <cmath>

namespace ccc_amd
{
constexpr int kLoopMaxSteps = 16;   // footsteps per instance the LDS slice is sized for
constexpr int kLoopMaxKnots = CCC_PVZ_MAX_KNOTS;
constexpr int kLoopMaxDisturb = 8;

struct IsmLoopSlice
{
  double pcr[6][kPcrNP];
  double kt[kLoopMaxKnots], kz[kLoopMaxKnots];                           // knot times, reference ZMP of the axis
  double ss[kLoopMaxSteps], se[kLoopMaxSteps], fp[kLoopMaxSteps], f0[2]; // swing start / end, landing position; first
  int fid[kLoopMaxSteps];                                                // positions (L, R); foot of the step
};

struct IsmLoopArgs
{
  IsmPcrDev P;
  long n;
  int K;
  const double *foot0, *foot_pos;
  const int * foot_id;
  const double *swing_start, *swing_end;
  double half[2]; // half the foot size per axis
  const int * num_knots;
  const double *knot_time, *knot_zmp;
  double *com, *zmp;
  double t0, sim_dt;
  int cycles, n_disturb;
  double dist[kLoopMaxDisturb], imp;
  int warm;
  int *status, *viol;
  double *traj_com, *traj_zmp;
  double a00, a01, a10, a11, b0, b1; // exact ZOH of x'' = w^2 (x - zmp) over sim_dt (SimModels.h:11-41)
  double cp_gain;                    // sqrt(h / g)  (TestIntrinsicallyStableMpc.cpp:67)
};

// The samplers, the capture point and the simulator round every product and sum separately, as the host code they
// restate does (csrc/zmp_loop.hip does the same for the limits); the QP data and the solver keep the contraction of
// ism_plan_pcr_kernel, so that a cycle plans what that kernel plans from the same samples.
__device__ __forceinline__ double loop_sample_time(double t, double dt, int i, double eps)
{
#pragma clang fp contract(off)
  return (t + dt * (double)i) + eps;
}

// limits of the axis at time t (epsilons included): FootstepManager.h:179-196,242-254
__device__ __forceinline__ void loop_limits(const IsmLoopSlice & S, int K, double half, double t, double & lo, double & hi)
{
#pragma clang fp contract(off)
  double p0 = S.f0[0], p1 = S.f0[1];
  bool g0 = true, g1 = true;
  for(int j = 0; j < K; j++)
  {
    const bool right = S.fid[j] != 0;
    const bool landed = t >= S.se[j];
    const bool swinging = t >= S.ss[j] && !landed;
    const double p = S.fp[j];
    p0 = (landed && !right) ? p : p0;
    p1 = (landed && right) ? p : p1;
    g0 = g0 && !(swinging && !right);
    g1 = g1 && !(swinging && right);
  }
  const double big = 1e30;
  lo = fmin(g0 ? p0 : big, g1 ? p1 : big) - half;
  hi = fmax(g0 ? p0 : -big, g1 ? p1 : -big) + half;
}

// reference ZMP of the axis at time t: FootstepManager.h:228-237 on the instance's knots, constant outside them
__device__ __forceinline__ double loop_ref_zmp(const IsmLoopSlice & S, int nk, double t)
{
#pragma clang fp contract(off)
  int k = 0;
  for(int j = 0; j < nk; j++) k += (S.kt[j] <= t) ? 1 : 0;
  if(k == 0) return S.kz[0];
  if(k >= nk) return S.kz[nk - 1];
  const double t0 = S.kt[k - 1], t1 = S.kt[k];
  const double ratio = (t - t0) / (t1 - t0);
  return (1.0 - ratio) * S.kz[k - 1] + ratio * S.kz[k];
}

__device__ __forceinline__ double loop_capture_point(double pos, double vel, double gain)
{
#pragma clang fp contract(off)
  return pos + gain * vel;
}

__device__ __forceinline__ void loop_sim_update(const IsmLoopArgs & A, double zmp, double & pos, double & vel)
{
#pragma clang fp contract(off)
  const double np = (A.a00 * pos + A.a01 * vel) + A.b0 * zmp, nv = (A.a10 * pos + A.a11 * vel) + A.b1 * zmp;
  pos = np;
  vel = nv;
}

__global__ __launch_bounds__(256) void ism_closed_loop_kernel(IsmLoopArgs A)
{
  __shared__ IsmLoopSlice slices[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long qp = (long)blockIdx.x * 4 + wave;
  if(qp >= 2 * A.n) return; // (whole wavefront; the kernel uses no workgroup barrier)
  const long inst = qp >> 1;
  const int ax = (int)(qp & 1);
  IsmLoopSlice & S = slices[wave];
  const IsmPcrDev & P = A.P;
  const int N = P.N, K = A.K;
  // ---- the only reads from HBM: timeline and knots of the axis -> LDS, state and row constants -> registers
  if(lane < K)
  {
    S.ss[lane] = A.swing_start[inst * K + lane];
    S.se[lane] = A.swing_end[inst * K + lane];
    S.fp[lane] = A.foot_pos[(inst * K + lane) * 2 + ax];
    S.fid[lane] = A.foot_id[inst * K + lane];
  }
  if(lane < 2) S.f0[lane] = A.foot0[inst * 4 + lane * 2 + ax];
  const int nk_in = A.num_knots[inst];
  const bool knots_ok = nk_in >= 1 && nk_in <= kLoopMaxKnots;
  const int nk = knots_ok ? nk_in : 0;
  if(lane < nk)
  {
    S.kt[lane] = A.knot_time[inst * kLoopMaxKnots + lane];
    S.kz[lane] = A.knot_zmp[(inst * kLoopMaxKnots + lane) * 2 + ax];
  }
  double pos = A.com[inst * 4 + ax * 2 + 0], vel = A.com[inst * 4 + ax * 2 + 1], z0 = A.zmp[inst * 2 + ax], t = A.t0;
  double * Sy = S.pcr[0];
  double * Sa = S.pcr[1];
  double * Sr = S.pcr[2];
  double * Sc = S.pcr[3];
  double * Sd = S.pcr[4];
  double * Se = S.pcr[5];
  const double kk = P.w_vel / (P.dt * P.dt), e = -kk;
  const int idx[2] = {lane, lane + 64};
  bool in[2];
  double at[2], dgn[2];
#pragma unroll
  for(int u = 0; u < 2; u++)
  {
    const int i = idx[u];
    in[u] = i < N;
    at[u] = in[u] ? P.at[i] : 0.0;
    dgn[u] = P.w_zmp + (i == N - 1 ? kk : 2.0 * kk);
  }
  __builtin_amdgcn_wave_barrier();
  const double half = A.half[ax];
  const int max_outer = kPcrOuter;
  double y[2] = {0.0, 0.0}, nu = 0.0;
  bool cl[2] = {false, false};
  int solves = 0, nviol = 0;
  int stop = knots_ok ? CCC_STATUS_SOLVED : CCC_STATUS_INFEASIBLE; // (a knot count the slice cannot hold: cycle 0)
  int c = 0;
  for(; c < A.cycles && stop == CCC_STATUS_SOLVED; c++)
  {
    // ---- 1. the references of the lane's rows (src/IntrinsicallyStableMpc.cpp:112-124; FootstepManager.h:370-380 adds
    //         1e-6, zmpLimits and refZmp another 1e-6 each)
    double lo[2], hi[2], q[2];
    bool bad = false;
#pragma unroll
    for(int u = 0; u < 2; u++)
    {
      const int i = idx[u];
      const double ts = loop_sample_time(t, P.dt, i, 2e-6);
      double l, h;
      loop_limits(S, K, half, ts, l, h);
      const double zr = in[u] ? loop_ref_zmp(S, nk, ts) : 0.0;
      lo[u] = in[u] ? l : 0.0;
      hi[u] = in[u] ? h : 0.0;
      q[u] = -P.w_zmp * zr - (i == 0 ? kk * z0 : 0.0);
      bad = bad || (in[u] && lo[u] > hi[u]);
    }
    // ---- 2. the QP data
    const double cp = loop_capture_point(pos, vel, A.cp_gain);
    const double c_eq = cp - z0 + P.a0_dt * z0;
    // ---- 3. feasibility in closed form: every at_i > 0, so at'y over the box spans [at'lo, at'hi]
    const double span_lo = WaveGroup<64>::sum(at[0] * lo[0] + at[1] * lo[1]);
    const double span_hi = WaveGroup<64>::sum(at[0] * hi[0] + at[1] * hi[1]);
    if(__any(bad) || !(span_lo <= c_eq && c_eq <= span_hi))
    {
      stop = CCC_STATUS_INFEASIBLE;
      break;
    }
    // ---- 4. solve (cold: as ism_plan_pcr_kernel starts; warm: from the y, cl and nu of the cycle before)
    {
      const bool pcr_warm = A.warm != 0 && c > 0;
#include "ism_pcr_body.inc"
      if(st != CCC_STATUS_SOLVED)
      {
        stop = CCC_STATUS_MAX_ITER; // (feasible, but a budget ran out; inside a loop there is no tableau hand-over)
        break;
      }
    }
    // ---- 5. the cycle's outputs: zmp = clamp(z0 + sim_dt u_0, zmin_0, zmax_0)  (src/IntrinsicallyStableMpc.cpp:93-101)
    const double y0 = ism_lane_value(y[0], 0), lo0 = ism_lane_value(lo[0], 0), hi0 = ism_lane_value(hi[0], 0);
    const double u0 = (y0 - z0) / P.dt;
    const double cdt = A.sim_dt;
    double zv = z0 + cdt * u0;
    zv = zv < lo0 ? lo0 : (hi0 < zv ? hi0 : zv);
    {
      double vl, vh;
      loop_limits(S, K, half, loop_sample_time(t, 0.0, 0, 1e-6), vl, vh); // zmpLimits(t) of the check (:84-85)
      if(!(zv - vl >= 0 && vh - zv >= 0)) nviol++;
    }
    if(lane == 0)
    {
      if(A.traj_com) A.traj_com[((size_t)c * A.n + inst) * 2 + ax] = pos;
      if(A.traj_zmp) A.traj_zmp[((size_t)c * A.n + inst) * 2 + ax] = zv;
    }
    loop_sim_update(A, zv, pos, vel);
    z0 = zv;
    t += A.sim_dt;
#pragma unroll
    for(int d = 0; d < kLoopMaxDisturb; d++) // the first match only (:92-99); the x impulse goes to both axes
      if(d < A.n_disturb && A.dist[d] <= t && t < A.dist[d] + A.sim_dt)
      {
        vel += A.imp;
        break;
      }
  }
  // ---- a stopped axis: the records from its cycle on are NaN, its state is the one it entered that cycle with
  if(stop != CCC_STATUS_SOLVED)
  {
    const double qnan = __builtin_nan("");
    for(int r = c + lane; r < A.cycles; r += 64)
    {
      if(A.traj_com) A.traj_com[((size_t)r * A.n + inst) * 2 + ax] = qnan;
      if(A.traj_zmp) A.traj_zmp[((size_t)r * A.n + inst) * 2 + ax] = qnan;
    }
  }
  if(lane == 0)
  {
    A.com[inst * 4 + ax * 2 + 0] = pos;
    A.com[inst * 4 + ax * 2 + 1] = vel;
    A.zmp[inst * 2 + ax] = z0;
    if(A.status) A.status[qp] = ((stop == CCC_STATUS_SOLVED ? solves : c) << 8) | stop;
    if(A.viol && nviol) atomicAdd(A.viol + inst, nviol);
  }
}
} // namespace ccc_amd

using namespace ccc_amd;

extern "C" int ccc_ism_closed_loop_device(ccc_ism_t * h, int64_t n, int K, const double * foot0, const double * foot_pos,
                                          const int32_t * foot_id, const double * swing_start, const double * swing_end,
                                          const double * foot_size, const int32_t * num_knots, const double * knot_time,
                                          const double * knot_zmp, double * com_state, double * planned_zmp, double t0,
                                          double sim_dt, int cycles, int n_disturb, const double * disturb_times,
                                          double disturb_impulse, int warm_start, int32_t * status, int32_t * violations,
                                          double * traj_com, double * traj_zmp, void * stream)
{
  const char * who = "ccc_ism_closed_loop_device";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0 || K < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n or K < 0", who);
  if(cycles < 0 || !(sim_dt > 0)) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: cycles < 0 or sim_dt <= 0", who);
  if(n_disturb < 0 || n_disturb > kLoopMaxDisturb || (n_disturb > 0 && !disturb_times))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n_disturb outside 0 .. %d, or NULL disturb_times", who, kLoopMaxDisturb);
  if(n == 0) return CCC_OK;
  if(!foot0 || (K > 0 && (!foot_pos || !foot_id || !swing_start || !swing_end)))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL footstep timeline array", who);
  if(!num_knots || !knot_time || !knot_zmp) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL knot array", who);
  if(!com_state || !planned_zmp) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL com_state / planned_zmp", who);
  if(h->N >= kPcrNP)
    return fail(CCC_ERR_UNSUPPORTED, "%s: horizon_steps %d > %d, the limit of the tridiagonal kernel", who, h->N, kPcrNP - 1);
  if(K > kLoopMaxSteps)
    return fail(CCC_ERR_UNSUPPORTED, "%s: %d footsteps per instance > %d, what the LDS slice of a wavefront holds", who, K,
                kLoopMaxSteps);
  if(n > ((int64_t)1 << 30)) return fail(CCC_ERR_UNSUPPORTED, "%s: n = %lld > 2^30", who, (long long)n);
  if(cycles == 0) return CCC_OK;
  CCC_DEVICE_GUARD(h->device);
  IsmLoopArgs A{};
  A.P = IsmPcrDev{h->N, h->dAt, h->a0_dt, h->w_zmp, h->w_zmp_vel, h->horizon_dt};
  A.n = (long)n;
  A.K = K;
  A.foot0 = foot0;
  A.foot_pos = foot_pos;
  A.foot_id = foot_id;
  A.swing_start = swing_start;
  A.swing_end = swing_end;
  A.half[0] = 0.5 * (foot_size ? foot_size[0] : 0.1); // FootstepManager.h:464
  A.half[1] = 0.5 * (foot_size ? foot_size[1] : 0.05);
  A.num_knots = num_knots;
  A.knot_time = knot_time;
  A.knot_zmp = knot_zmp;
  A.com = com_state;
  A.zmp = planned_zmp;
  A.t0 = t0;
  A.sim_dt = sim_dt;
  A.cycles = cycles;
  A.n_disturb = n_disturb;
  for(int d = 0; d < n_disturb; d++) A.dist[d] = disturb_times[d];
  A.imp = disturb_impulse;
  A.warm = warm_start;
  A.status = status;
  A.viol = violations;
  A.traj_com = traj_com;
  A.traj_zmp = traj_zmp;
  const double kG = 9.80665; // include/CCC/Constants.h:10
  const double w = std::sqrt(kG / h->com_height), ch = std::cosh(w * sim_dt), sh = std::sinh(w * sim_dt);
  A.a00 = ch;
  A.a01 = sh / w;
  A.a10 = w * sh;
  A.a11 = ch;
  A.b0 = 1 - ch;
  A.b1 = -w * sh;
  A.cp_gain = std::sqrt(h->com_height / kG);
  hipLaunchKernelGGL(ism_closed_loop_kernel, dim3((unsigned)((2 * n + 3) / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), A);
  CCC_HIP_CHECK(hipGetLastError());
  return CCC_OK;
}
