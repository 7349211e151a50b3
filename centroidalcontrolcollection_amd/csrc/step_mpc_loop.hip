// step_mpc_loop.hip -- the closed loop of CCC::StepMpc in ONE launch: FootstepManager::update -> makeStepMpcRefData ->
// planOnce -> ComZmpSim2d::update -> disturbance -> footstep update, `cycles` times, for n instances.
//
// Path replaced (reference file:line under /root/reference):
//   tests/src/TestStepMpc.cpp:55-116            the control loop, with the footstep update of :99-115
//   tests/src/FootstepManager.h:147-160         update: the front footstep lands, old footsteps are popped
//   tests/src/FootstepManager.h:385-448         makeStepMpcRefData: the element list planOnce is given
//   tests/src/SimModels.h:11-41,125-129         ComZmpSimModel1d (exact ZOH), addDisturb (x impulse on both axes)
//   src/StepMpc.cpp:26-247                      planOnce: the row-append QR of csrc/step_mpc.h, shared
//
// Work split: one instance per 16-lane DPP row for all cycles, as in the planner; four instances per wavefront, no LDS, no
// barrier.  A lane plays two parts.  As FOOTSTEP lane k it keeps footstep k of the timeline for the whole launch: landing
// position (the one thing the loop rewrites), swing start / end, transit end and the end of the double support that
// follows it (the next swing start; the transit end for the last one).  As ELEMENT lane i it builds element i of this
// cycle's list: it works out which footstep j and which half (single / double support) element i is from the front
// index and two flags, finds the latest earlier footstep of the other foot in a bit mask of the foot ids, and fetches
// the end time and the two positions from the footstep lanes j and src by ds_bpermute (register exchange through the
// LDS crossbar; no LDS is allocated).  Uniform over the row, replicated in its lanes: the front index, the front
// footstep's data (re-fetched when a footstep is popped), the footstance (two feet x 2), the CoM state.  t is uniform
// over the grid.  After the first loads nothing is read from HBM; a cycle writes its trajectory records only.
#include "common.h"
#include "step_mpc.h"

#include <cmath>

namespace ccc_amd
{
namespace
{
constexpr int kStepLoopMaxDisturb = 8;

struct StepLoopArgs
{
  StepParams P;
  long n;
  int K;
  const double * foot0;
  double * foot_pos;
  const int * foot_id;
  const double *swing_start, *swing_end, *transit_end;
  double * com;
  double t0, sim_dt;
  int cycles, n_disturb;
  double dist[kStepLoopMaxDisturb], imp;
  double horizon, const_zmp, pre;
  int enable_update;
  int *status, *updates;
  double *traj_com, *traj_zmp, *traj_foot;
  double a00, a01, a10, a11, b0, b1; // exact ZOH of x'' = w^2 (x - zmp) over sim_dt (SimModels.h:11-41)
};

// rounds every product and sum separately, as the host simulator it restates does
__device__ __forceinline__ void step_loop_sim(const StepLoopArgs & A, double zmp, double & pos, double & vel)
{
#pragma clang fp contract(off)
  const double np = (A.a00 * pos + A.a01 * vel) + A.b0 * zmp, nv = (A.a10 * pos + A.a11 * vel) + A.b1 * zmp;
  pos = np;
  vel = nv;
}

// The arguments as the loop body sees them: read again from the kernel-argument segment through a pointer the compiler
// cannot see through, once per cycle.  With the by-value copy everything that does not change between cycles (the
// weights and their products, the ZOH constants, the disturbance times) is hoisted out of the loop and stays in
// registers across the 136 rotation bodies: 106 SGPRs + 138 spilled, 255 VGPRs.  Scalar loads per cycle cost nothing
// beside the factorisation.  (The struct is the kernel's only argument: offset 0 of the segment.)
__device__ __forceinline__ const StepLoopArgs & step_loop_args(const StepLoopArgs & by_value)
{
#if defined(__HIP_DEVICE_COMPILE__)
  auto p = (const __attribute__((address_space(4))) StepLoopArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *p;
#else
  return by_value;
#endif
}

// value of lane `src` (0 .. 15) of the caller's row
__device__ __forceinline__ double row_fetch(double v, int src)
{
  return __shfl(v, src, 16);
}

// 256 threads = four wavefronts = sixteen instances per workgroup.  Every lane stays active to the end: the planner's
// DPP broadcasts and ballots need the whole wavefront; an absent or stopped instance plans nothing (S.n = 0).
__global__ __launch_bounds__(256) void step_closed_loop_kernel(StepLoopArgs A0)
{
  const StepLoopArgs & A = A0;
  const int tid = (int)threadIdx.x;
  const int lane0 = tid & 15;
  const int lane = lane0;
  const long inst = (long)blockIdx.x * 16 + (tid >> 4);
  const bool present = inst < A.n;
  const unsigned rshift = (unsigned)(tid & 48); // this row's sixteen bits of a wavefront ballot
  const int K = A.K;
  const unsigned maskK = (1u << K) - 1u; // (K <= 16)

  // ---- the only reads from HBM: footstep `lane`, the footstance, the CoM state
  int fid = 0;
  double fpx = 0.0, fpy = 0.0, fss = 0.0, fse = 0.0, fte = 0.0, dse = 0.0;
  double sLx = 0.0, sLy = 0.0, sRx = 0.0, sRy = 0.0, px = 0.0, vx = 0.0, py = 0.0, vy = 0.0;
  if(present)
  {
    if(lane < K)
    {
      const long k = inst * K + lane;
      fid = A.foot_id[k] != 0 ? 1 : 0;
      fpx = A.foot_pos[k * 2];
      fpy = A.foot_pos[k * 2 + 1];
      fss = A.swing_start[k];
      fse = A.swing_end[k];
      fte = A.transit_end[k];
      dse = lane + 1 < K ? A.swing_start[k + 1] : fte; // end of the double support after this footstep (:430-437)
    }
    sLx = A.foot0[inst * 4];
    sLy = A.foot0[inst * 4 + 1];
    sRx = A.foot0[inst * 4 + 2];
    sRy = A.foot0[inst * 4 + 3];
    px = A.com[inst * 4];
    vx = A.com[inst * 4 + 1];
    py = A.com[inst * 4 + 2];
    vy = A.com[inst * 4 + 3];
  }
  const unsigned right = (unsigned)(__ballot(fid != 0) >> rshift) & 0xffffu; // bit k: footstep k is of the right foot

  // front footstep of the list (uniform over the row)
  int fr = 0, f_id = 0;
  double f_ss, f_se, f_te, f_px, f_py;
  auto fetch_front = [&](bool take) {
    const int src = fr < 15 ? fr : 15;
    const double a = row_fetch(fss, src), b = row_fetch(fse, src), c = row_fetch(fte, src);
    const double d = row_fetch(fpx, src), e = row_fetch(fpy, src);
    if(take)
    {
      f_id = (int)((right >> src) & 1u);
      f_ss = a;
      f_se = b;
      f_te = c;
      f_px = d;
      f_py = e;
    }
  };
  f_ss = f_se = f_te = f_px = f_py = 0.0;
  fetch_front(true);

  bool alive = present;
  int stop_cycle = 0, nupd = 0;
  double t = A.t0;
  const double qnan = __builtin_nan("");
  int c = 0;
  for(; c < A.cycles; c++)
  {
    if(__ballot(alive) == 0ull) break;
    const StepLoopArgs & A = step_loop_args(A0);
    const StepParams & P = A.P;
    // (the same for the lane index: the sixty-odd masks `lane == k`, `lane < k` of the rotations are compared per cycle,
    // as the planner kernel compares them, instead of living in SGPR pairs through the launch)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    // ---- 1. FootstepManager::update (:147-160): the front footstep lands, then old footsteps are popped
    if(alive && fr < K && f_se <= t)
    {
      sLx = f_id ? sLx : f_px;
      sLy = f_id ? sLy : f_py;
      sRx = f_id ? f_px : sRx;
      sRy = f_id ? f_py : sRy;
    }
    for(;;)
    {
      const bool pop = alive && fr < K && f_te < t;
      if(__ballot(pop) == 0ull) break;
      fr += pop ? 1 : 0;
      fetch_front(pop);
    }
    // ---- 2. makeStepMpcRefData (:385-448): element `lane` of the list at tc = t - 1e-6
    const double tc = t - 1e-6;
    const bool empty = fr >= K;
    const bool lead = !empty && tc < f_ss;    // the double support before the front's swing
    const bool skip = !empty && !(tc < f_se); // the front has landed: its single-support element is gone
    const unsigned in_list = maskK & ~((1u << fr) - 1u);
    const unsigned cut = (unsigned)(__ballot(((in_list >> lane) & 1u) != 0u && dse > tc + A.horizon) >> rshift) & 0xffffu;
    const int last = cut ? __ffs((int)cut) - 1 : K - 1;
    const int n = empty ? 1 : (lead ? 1 : 0) + 2 * (last - fr + 1) - (skip ? 1 : 0);
    bool is_ds;
    double zx, zy, te;
    {
      const int e2 = lane - (lead ? 1 : 0) + (skip ? 1 : 0);
      const int j = (fr + (e2 >> 1)) & 15; // the footstep element `lane` belongs to (lanes at and beyond n: unused)
      is_ds = (e2 & 1) != 0;
      const unsigned jright = (right >> j) & 1u;
      // the other foot: where its latest earlier footstep of the list put it, else the footstance.  A front footstep
      // whose single-support element is skipped has not been written into tmp_footstance either (:416-425)
      const unsigned moved = in_list & ~(skip ? 1u << fr : 0u) & ((1u << j) - 1u) & (jright ? ~right : right);
      const int src = moved ? 31 - __clz((int)moved) : 0;
      const double ox = row_fetch(fpx, src), oy = row_fetch(fpy, src);
      const double jx = row_fetch(fpx, j), jy = row_fetch(fpy, j);
      const double jse = row_fetch(fse, j), jde = row_fetch(dse, j);
      const double otx = moved ? ox : (jright ? sLx : sRx), oty = moved ? oy : (jright ? sLy : sRy);
      const bool own_stance = skip && j == fr;
      const double mx = own_stance ? (jright ? sRx : sLx) : jx, my = own_stance ? (jright ? sRy : sLy) : jy;
      zx = is_ds ? 0.5 * (mx + otx) : otx;
      zy = is_ds ? 0.5 * (my + oty) : oty;
      te = is_ds ? jde : jse;
      if(empty || (lead && lane == 0))
      {
        is_ds = true;
        zx = 0.5 * (sLx + sRx);
        zy = 0.5 * (sLy + sRy);
        te = empty ? tc + A.const_zmp : f_ss;
      }
    }
    // ---- 3. plannable?  planOnce gets t itself, so the first duration may lie in (-1e-6, 0]
    const bool n_ok = n <= 16;
    const bool mine = alive && n_ok && lane < n;
    const double tprev = dpp_f64<0x111>(te); // DPP row_shr:1 (lane 0 of a row: bound_ctrl zero, not used)
    const double T = te - (lane == 0 ? t : tprev);
    const unsigned ss = (unsigned)(__ballot(mine && !is_ds) >> rshift) & 0xffffu;
    const unsigned have = (unsigned)(__ballot(mine) >> rshift) & 0xffffu;
    const unsigned bad_t = (unsigned)(__ballot(mine && !(T > (lane == 0 ? -2e-6 : 0.0))) >> rshift) & 0xffffu;
    const unsigned ds = have & ~ss;
    const bool valid = alive && n_ok && bad_t == 0u && (ds & (ds >> 1)) == 0u; // no two double supports in a row
    if(alive && !valid)
    {
      alive = false;
      stop_cycle = c;
    }
    // ---- 4. planOnce: csrc/step_mpc.h on the list in registers (set up as step_mpc_kernel sets it up)
    StepRow S;
    S.lane = lane;
    S.n = valid ? n : 0;
    S.ss = valid ? ss : 0u;
    S.future_ss = (S.ss & ~1u) != 0u;
    const bool el = valid && mine;
    {
      const double wt = el ? P.omega * T : 0.0;
      const double em = expm1(wt), en = expm1(-wt);
      S.e = 1.0 + em;
      S.einv = 1.0 + en;
      S.ce = -em;
      S.cinv = -en;
    }
    S.zx = el ? zx : 0.0;
    S.zy = el ? zy : 0.0;
    S.a = 0.0;
    S.b = 0.0;
    {
      const double ox = valid ? vx / P.omega : 0.0, oy = valid ? vy / P.omega : 0.0;
      const double qx = valid ? px : 0.0, qy = valid ? py : 0.0;
      S.xix = qx + ox;
      S.xiy = qy + oy;
      S.zex = qx - ox;
      S.zey = qy - oy;
    }
    double Rc[16];
    const bool fixed = lane == 0 || (lane == 1 && S.n > 1 && !(S.ss & 1u));
    const double sz = fixed ? P.s_fixed : P.s_free;
#pragma unroll
    for(int k = 0; k < 16; ++k) Rc[k] = lane == k ? sz : 0.0;
    double dx = sz * S.zx, dy = sz * S.zy;
    step_all_stages<15>(P, S, Rc, dx, dy);
    double ux = 0.0, uy = 0.0;
    step_backsub<15>(Rc, dx, dy, ux, uy, lane);
    // ---- 5. the cycle's records, the simulator step, the disturbance (TestStepMpc.cpp:70-97)
    const int foot = S.future_ss ? __ffs((int)(S.ss & ~1u)) - 1 : -1; // element of the next foot, if any (:188-197)
    const double u0x = step_bcast<0>(ux), u0y = step_bcast<0>(uy);
    if(valid)
    {
      const size_t rec = ((size_t)c * (size_t)A.n + (size_t)inst) * 2;
      if(lane == 0)
      {
        if(A.traj_com)
        {
          A.traj_com[rec] = px;
          A.traj_com[rec + 1] = py;
        }
        if(A.traj_zmp)
        {
          A.traj_zmp[rec] = ux;
          A.traj_zmp[rec + 1] = uy;
        }
      }
      if(A.traj_foot && lane == (foot < 0 ? 0 : foot))
      {
        A.traj_foot[rec] = foot < 0 ? qnan : ux;
        A.traj_foot[rec + 1] = foot < 0 ? qnan : uy;
      }
      step_loop_sim(A, u0x, px, vx);
      step_loop_sim(A, u0y, py, vy);
    }
    t += A.sim_dt;
#pragma unroll
    for(int d = 0; d < kStepLoopMaxDisturb; d++) // the first match only (:90-97); the x impulse goes to both axes
      if(d < A.n_disturb && A.dist[d] <= t && t < A.dist[d] + A.sim_dt)
      {
        vx = valid ? vx + A.imp : vx;
        vy = valid ? vy + A.imp : vy;
        break;
      }
    // ---- 6. footstep update (:99-115): 0.1 s before the front's swing ends it lands where the plan puts the next foot
    const double pre_t = f_se - A.pre;
    const bool adapt = valid && A.enable_update != 0 && !empty && pre_t <= t && t < pre_t + A.sim_dt && foot >= 0;
    if(__ballot(adapt) != 0ull)
    {
      const double nx = row_fetch(ux, foot & 15), ny = row_fetch(uy, foot & 15);
      if(adapt)
      {
        fpx = lane == fr ? nx : fpx;
        fpy = lane == fr ? ny : fpy;
        f_px = nx;
        f_py = ny;
        nupd++;
      }
    }
  }
  // ---- an instance that stopped: its records from that cycle on are NaN, its state is the one it entered the cycle with
  if(!present) return;
  const bool stopped = !alive;
  if(stopped)
    for(int r = stop_cycle + lane; r < A.cycles; r += 16)
    {
      const size_t rec = ((size_t)r * (size_t)A.n + (size_t)inst) * 2;
      if(A.traj_com) A.traj_com[rec] = A.traj_com[rec + 1] = qnan;
      if(A.traj_zmp) A.traj_zmp[rec] = A.traj_zmp[rec + 1] = qnan;
      if(A.traj_foot) A.traj_foot[rec] = A.traj_foot[rec + 1] = qnan;
    }
  if(lane < K)
  {
    A.foot_pos[(inst * K + lane) * 2] = fpx;
    A.foot_pos[(inst * K + lane) * 2 + 1] = fpy;
  }
  if(lane == 0)
  {
    A.com[inst * 4] = px;
    A.com[inst * 4 + 1] = vx;
    A.com[inst * 4 + 2] = py;
    A.com[inst * 4 + 3] = vy;
    if(A.status) A.status[inst] = stopped ? ((stop_cycle << 8) | CCC_STATUS_INFEASIBLE) : CCC_STATUS_SOLVED;
    if(A.updates) A.updates[inst] += nupd;
  }
}
} // namespace
} // namespace ccc_amd

using namespace ccc_amd;

extern "C" int ccc_step_closed_loop_device(ccc_step_t * h, int64_t n, int K, const double * foot0, double * foot_pos,
                                           const int32_t * foot_id, const double * swing_start, const double * swing_end,
                                           const double * transit_end, double * com_state, double t0, double sim_dt,
                                           int cycles, int n_disturb, const double * disturb_times, double disturb_impulse,
                                           const ccc_step_loop_params_t * params, int32_t * status, int32_t * updates,
                                           double * traj_com, double * traj_zmp, double * traj_next_foot, void * stream)
{
  const char * who = "ccc_step_closed_loop_device";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0 || K < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n or K < 0", who);
  if(cycles < 0 || !(sim_dt > 0)) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: cycles < 0 or sim_dt <= 0", who);
  if(n_disturb < 0 || n_disturb > kStepLoopMaxDisturb || (n_disturb > 0 && !disturb_times))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n_disturb outside 0 .. %d, or NULL disturb_times", who, kStepLoopMaxDisturb);
  const ccc_step_loop_params_t prm = params ? *params : ccc_step_loop_params_t{3.0, 0.2, 0.1, 1}; // FootstepManager.h:392-393
  if(!(prm.horizon_duration > 0) || !(prm.constant_zmp_duration > 0) || !(prm.pre_duration > 0))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: horizon_duration, constant_zmp_duration and pre_duration must be > 0", who);
  if(n == 0) return CCC_OK;
  if(!foot0 || !com_state) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL foot0 / com_state", who);
  if(K > 0 && (!foot_pos || !foot_id || !swing_start || !swing_end || !transit_end))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL footstep timeline array", who);
  if(K > CCC_STEP_MAX_ELEMENTS)
    return fail(CCC_ERR_UNSUPPORTED, "%s: %d footsteps per instance > %d, one per lane of a 16-lane row", who, K,
                CCC_STEP_MAX_ELEMENTS);
  if(n > ((int64_t)1 << 30)) return fail(CCC_ERR_UNSUPPORTED, "%s: n = %lld > 2^30", who, (long long)n);
  if(cycles == 0) return CCC_OK;
  CCC_DEVICE_GUARD(h->device);
  StepLoopArgs A{};
  A.P = h->P;
  A.n = (long)n;
  A.K = K;
  A.foot0 = foot0;
  A.foot_pos = foot_pos;
  A.foot_id = foot_id;
  A.swing_start = swing_start;
  A.swing_end = swing_end;
  A.transit_end = transit_end;
  A.com = com_state;
  A.t0 = t0;
  A.sim_dt = sim_dt;
  A.cycles = cycles;
  A.n_disturb = n_disturb;
  for(int d = 0; d < n_disturb; d++) A.dist[d] = disturb_times[d];
  A.imp = disturb_impulse;
  A.horizon = prm.horizon_duration;
  A.const_zmp = prm.constant_zmp_duration;
  A.pre = prm.pre_duration;
  A.enable_update = prm.enable_footstep_update;
  A.status = status;
  A.updates = updates;
  A.traj_com = traj_com;
  A.traj_zmp = traj_zmp;
  A.traj_foot = traj_next_foot;
  const double w = h->P.omega, ch = std::cosh(w * sim_dt), sh = std::sinh(w * sim_dt);
  A.a00 = ch;
  A.a01 = sh / w;
  A.a10 = w * sh;
  A.a11 = ch;
  A.b0 = 1 - ch;
  A.b1 = -w * sh;
  hipLaunchKernelGGL(step_closed_loop_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), A);
  CCC_HIP_CHECK(hipGetLastError());
  return CCC_OK;
}
