// preview_zmp.h -- device side of CCC::PreviewControlZmp and CCC::SingularPreviewControlZmp
// (/root/reference/src/PreviewControlZmp.cpp:15-76, src/SingularPreviewControlZmp.cpp:7-88).
//
// Both controllers are, per axis, u = -K x + sum_{i<N} w_i r_i and a two-line epilogue, so one pair of table-driven
// kernels serves both: the handle holds K [3], w [N] and the epilogue selector (csrc/preview_zmp.hip computes them).
//
// Layout (the house layout of csrc/step_mpc.h): one instance per 16-lane DPP row, four per wavefront, both axes carried
// together, the row sum through the DPP steps of wave_group.h.  A grid-stride loop over groups of sixteen instances keeps
// the per-handle tables resident: the sampled kernel holds its weights in registers for the lifetime of the wavefront,
// the knot kernel holds the suffix tables in LDS for the lifetime of the workgroup.
#pragma once

#include "../../include/ccc_amd.h"
#include "wave_group.h"

namespace ccc_amd
{
constexpr int kPvzMaxSteps = 512; // CCC_PVZ_MAX_STEPS
constexpr int kPvzMaxKnots = 32;  // CCC_PVZ_MAX_KNOTS
constexpr int kPvzTab = kPvzMaxSteps + 1;

struct PvzParams
{
  double K[3];
  double dt, inv_dt; // horizon_dt
  double c02;        // C(0, 2) of ComZmpModelJerkInput (PREVIEW)
  double off_dt;     // off * horizon_dt: the first sample is at current_time + off_dt
  int N, kind, off;  // off = 1 (PREVIEW: samples at t + (i + 1) dt) or 0 (SINGULAR: t + i dt)
};

// sum over the sixteen lanes of a DPP row, replicated in each of them
__device__ __forceinline__ double pvz_row_sum(double v)
{
  v += dpp_f64<kDppQuadXor1>(v);
  v += dpp_f64<kDppQuadXor2>(v);
  v += dpp_f64<kDppRowHalfMirror>(v);
  v += dpp_f64<kDppRowMirror>(v);
  return v;
}

// lane j of a row receives the value of lane (j + 1) % 16 (row_ror:15)
__device__ __forceinline__ int pvz_row_next(int v)
{
  return __builtin_amdgcn_mov_dpp(v, 0x12F, 0xf, 0xf, true);
}

// The feedback term and the epilogue of one axis, shared by both kernels: `s` is the preview sum, x the state in the
// order of the handle's K.  Returns the planned ZMP, u is the input (CoM jerk / ZMP velocity).
__device__ __forceinline__ double pvz_finish(const PvzParams & P, double control_dt, double x0, double x1, double x2, double s,
                                             double & u)
{
  u = s - fma(P.K[2], x2, fma(P.K[1], x1, P.K[0] * x0));
  if(P.kind == CCC_PVZ_PREVIEW)
  {
    // src/PreviewControlZmp.cpp:40-46
    const double cd = control_dt < 0 ? P.dt : control_dt;
    const double acc = x2 + cd * u;
    const double pos = x0 + cd * x1 + 0.5 * (cd * cd) * x2;
    return pos + P.c02 * acc;
  }
  // src/SingularPreviewControlZmp.cpp:54: control_dt as passed, never horizon_dt
  return x0 + control_dt * u;
}

// A pair of consecutive samples fetched by one 16-byte load; a row of an odd N starts on an odd double, so the pair is
// only 8-byte aligned (gfx950 global loads take that).
struct __attribute__((packed, aligned(8))) PvzPair
{
  double x, y;
};

// ------------------------------------------------------------------------------------------------ sampled kernel
// ref [n][2][N].  Lane l of a row owns samples 32 k + 2 l and 32 k + 2 l + 1, k < B, of each axis: one 16-byte load per
// lane, 256 contiguous bytes per row and load.  `w` is zero beyond N (kPvzTab entries), so tail samples are masked by
// their weights; their addresses are clamped into the row (the last row of the batch ends where the buffer ends).
// The 2 B loads of a row (both axes) are issued in stages of at most eight, one stage ahead of the stage being summed, so
// that the registers hold the 4 B weight registers and two stages of samples, without scratch: built for four or more
// resident wavefronts per SIMD at B = 2 and 4, three at B = 8 (N <= 256, the reference test's N = 200 among them) and two
// at B = 16 (215 VGPRs: 128 of them weights and samples, the rest the hoisted per-chunk offsets and masks).
template<int B>
struct PvzStage
{
  static constexpr int L = 2 * B, G = L < 8 ? L : 8, NG = L / G;
  PvzPair v[G];
  // stage `grp` holds the loads f = grp G + j, f = a B + k (axis a, chunk k)
  __device__ __forceinline__ void fetch(int grp, const double * const (&row)[2], int lane, int last_pair)
  {
#pragma unroll
    for(int j = 0; j < G; ++j)
    {
      const int f = grp * G + j, i = 32 * (f % B) + 2 * lane;
      v[j] = *reinterpret_cast<const PvzPair *>(row[f / B] + (i < last_pair ? i : last_pair));
    }
  }
  __device__ __forceinline__ void sum(int grp, const double (&w0)[B], const double (&w1)[B], int lane, int N, int last_pair,
                                      const int (&shift)[2], double (&acc)[2]) const
  {
#pragma unroll
    for(int j = 0; j < G; ++j)
    {
      const int f = grp * G + j, a = f / B, k = f % B, i = 32 * k + 2 * lane;
      // (the pair of sample N - 1 of an odd N starts one sample earlier, that of a clamped row `shift` earlier)
      const bool second = i + shift[a] != (i < last_pair ? i : last_pair);
      const double r0 = i < N ? (second ? v[j].y : v[j].x) : 0.0, r1 = i + 1 < N ? v[j].y : 0.0;
      acc[a] = fma(w0[k], r0, acc[a]);
      acc[a] = fma(w1[k], r1, acc[a]);
    }
  }
};

template<int B>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(B >= 16 ? 2 : (B >= 8 ? 3 : 4)))) void pvz_sampled_kernel(
    PvzParams P, long n, const double * __restrict__ w, const double * __restrict__ x0, const double * __restrict__ ref,
    double control_dt, double * __restrict__ zmp, double * __restrict__ input)
{
  using Stage = PvzStage<B>;
  const int tid = (int)threadIdx.x, lane = tid & 15, N = P.N;
  double w0[B], w1[B];
#pragma unroll
  for(int k = 0; k < B; ++k)
  {
    w0[k] = w[32 * k + 2 * lane];
    w1[k] = w[32 * k + 2 * lane + 1];
  }
  const long total = n * 2 * N, groups = (n + 15) / 16;
  const int last_pair = N >= 2 ? N - 2 : 0;
  for(long g = blockIdx.x; g < groups; g += gridDim.x)
  {
    const long inst = g * 16 + (tid >> 4);
    const bool present = inst < n;
    const long ic = present ? inst : n - 1;
    // (N = 1: the pair of the batch's last row would end past the buffer, so that row is read from one sample earlier)
    const long bx = ic * 2 * N, by = bx + N, cy = by < total - 2 ? by : total - 2;
    const double * const row[2] = {ref + bx, ref + cy};
    const int shift[2] = {0, (int)(by - cy)};
    double acc[2] = {0.0, 0.0};
    Stage st[2];
    st[0].fetch(0, row, lane, last_pair);
#pragma unroll
    for(int grp = 0; grp < Stage::NG; ++grp)
    {
      if(grp + 1 < Stage::NG) st[(grp + 1) & 1].fetch(grp + 1, row, lane, last_pair);
      __builtin_amdgcn_sched_barrier(0);
      st[grp & 1].sum(grp, w0, w1, lane, N, last_pair, shift, acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    const double sx = pvz_row_sum(acc[0]), sy = pvz_row_sum(acc[1]);
    const double * xs = x0 + ic * 6;
    double ux, uy;
    const double zx = pvz_finish(P, control_dt, xs[0], xs[1], xs[2], sx, ux);
    const double zy = pvz_finish(P, control_dt, xs[3], xs[4], xs[5], sy, uy);
    if(present && lane < 2)
    {
      zmp[inst * 2 + lane] = lane == 0 ? zx : zy;
      if(input) input[inst * 2 + lane] = lane == 0 ? ux : uy;
    }
  }
}

// ------------------------------------------------------------------------------------------------ knot kernel
// t_i = current_time + (i + off) * horizon_dt, rounded as the host's expression is (a product, then a sum: never an fma)
__device__ __forceinline__ double pvz_sample_time(const PvzParams & P, double ct, int i)
{
  return __dadd_rn(ct, __dmul_rn((double)(i + P.off), P.dt));
}

// The number of samples with t_i < tk (0 .. N): the first sample index of the segment that starts at knot time tk.
// Guessed by a division and corrected by the comparison itself; `ok` says whether the corrected guess IS the boundary.
__device__ __forceinline__ int pvz_boundary_guess(const PvzParams & P, double ct, double tk, bool & ok)
{
  const double gq = ceil((tk - ct) * P.inv_dt - (double)P.off);
  int g = gq > 0.0 ? (gq < (double)P.N ? (int)gq : P.N) : 0; // (NaN: 0)
#pragma unroll
  for(int r = 0; r < 2; ++r) g -= (g > 0 && !(pvz_sample_time(P, ct, g - 1) < tk)) ? 1 : 0;
#pragma unroll
  for(int r = 0; r < 2; ++r) g += (g < P.N && pvz_sample_time(P, ct, g) < tk) ? 1 : 0;
  ok = (g == 0 || pvz_sample_time(P, ct, g - 1) < tk) && (g == P.N || !(pvz_sample_time(P, ct, g) < tk));
  return g;
}

// The same by bisection on the comparison alone (ten steps cover N <= 512): taken by a whole wavefront when a guess of
// one of its lanes could not be corrected (horizon_dt near the spacing of doubles at current_time)
__device__ __forceinline__ int pvz_boundary_bisect(const PvzParams & P, double ct, double tk)
{
  int lo = 0, hi = P.N;
#pragma unroll
  for(int r = 0; r < 10; ++r)
  {
    const int mid = (lo + hi) >> 1;
    const bool open = lo < hi, below = pvz_sample_time(P, ct, mid) < tk;
    lo = open && below ? mid + 1 : lo;
    hi = open && !below ? mid : hi;
  }
  return lo;
}

// The preview sum over the samples [lo, hi) of the segment from (ta, za) to (tb, zb): r_i = alpha + i beta there, so the
// sum is alpha (W0[lo] - W0[hi]) + beta (W1[lo] - W1[hi]) with the suffix tables W0[j] = sum_{i >= j} w_i, W1[j] =
// sum_{i >= j} i w_i.
__device__ __forceinline__ void pvz_segment(const PvzParams & P, const double * sW0, const double * sW1, bool valid, int lo,
                                            int hi, double t0, double ta, double tb, double2 za, double2 zb, double & sx,
                                            double & sy)
{
  lo = valid ? lo : 0;
  hi = valid ? hi : 0;
  const double d0 = sW0[lo] - sW0[hi], d1 = sW1[lo] - sW1[hi];
  const double inv = 1.0 / (tb - ta), lead = t0 - ta;
  const double mx = (zb.x - za.x) * inv, my = (zb.y - za.y) * inv;
  const double cx = fma(za.x + lead * mx, d0, (P.dt * mx) * d1), cy = fma(za.y + lead * my, d0, (P.dt * my) * d1);
  sx += valid ? cx : 0.0;
  sy += valid ? cy : 0.0;
}

// num_knots [n], knot_time [n][32], knot_zmp [n][32][2]; tab = W0 [kPvzTab], W1 [kPvzTab].  Lane j of a row owns the
// segments j and j + 16 (segment s runs from knot s to knot s + 1).
__global__ __launch_bounds__(256) void pvz_knots_kernel(PvzParams P, long n, const double * __restrict__ tab,
                                                        const int * __restrict__ num_knots,
                                                        const double * __restrict__ knot_time,
                                                        const double * __restrict__ knot_zmp, const double * __restrict__ x0,
                                                        const double * __restrict__ current_time, double control_dt,
                                                        double * __restrict__ zmp, double * __restrict__ input,
                                                        int * __restrict__ status)
{
  __shared__ double sW0[kPvzTab], sW1[kPvzTab];
  const int tid = (int)threadIdx.x, lane = tid & 15, N = P.N;
  for(int i = tid; i <= N; i += 256)
  {
    sW0[i] = tab[i];
    sW1[i] = tab[kPvzTab + i];
  }
  __syncthreads();
  const unsigned rshift = (unsigned)(tid & 48); // this row's sixteen bits of a wavefront ballot
  const long groups = (n + 15) / 16;
  const int up = lane < 15 ? lane + 17 : 31; // (knot 32 does not exist: segment 31 is never valid)
  for(long g = blockIdx.x; g < groups; g += gridDim.x)
  {
    const long inst = g * 16 + (tid >> 4);
    const bool present = inst < n;
    const long ic = present ? inst : n - 1;
    // every array has a fixed stride of 32 knots per instance: in bounds whatever num_knots says
    const int nk = num_knots[ic];
    const bool nk_ok = nk >= 2 && nk <= kPvzMaxKnots;
    const double ct = current_time[ic];
    const double * kt = knot_time + ic * kPvzMaxKnots;
    const double2 * kz = reinterpret_cast<const double2 *>(knot_zmp) + ic * kPvzMaxKnots;
    const double ta1 = kt[lane], tb1 = kt[lane + 1], ta2 = kt[lane + 16], tb2 = kt[up];
    const double2 za1 = kz[lane], zb1 = kz[lane + 1], za2 = kz[lane + 16], zb2 = kz[up];

    bool ok1, ok2;
    int b1 = pvz_boundary_guess(P, ct, ta1, ok1), b2 = pvz_boundary_guess(P, ct, ta2, ok2);
    if(__any(!(ok1 && ok2)))
    {
      b1 = pvz_boundary_bisect(P, ct, ta1);
      b2 = pvz_boundary_bisect(P, ct, ta2);
    }
    const int r1 = pvz_row_next(b1), r2 = pvz_row_next(b2);
    const int e1 = lane < 15 ? r1 : r2; // boundary of knot lane + 1; (e2 = r2: that of knot lane + 17)

    const bool v1 = nk_ok && lane + 1 < nk, v2 = nk_ok && lane + 17 < nk;
    bool bad = (v1 && !(tb1 > ta1)) || (v2 && !(tb2 > ta2));      // knot times must increase (NaN included)
    bad = bad || (lane == 0 && b1 != 0);                           // a sample before the first knot
    bad = bad || (lane == nk - 1 && b1 != N) || (lane + 16 == nk - 1 && b2 != N); // a sample at or after the last
    const bool refused = !nk_ok || ((unsigned)(__ballot(bad) >> rshift) & 0xffffu) != 0u;

    const double t0 = ct + P.off_dt;
    double sx = 0.0, sy = 0.0;
    pvz_segment(P, sW0, sW1, v1, b1, e1, t0, ta1, tb1, za1, zb1, sx, sy);
    pvz_segment(P, sW0, sW1, v2, b2, r2, t0, ta2, tb2, za2, zb2, sx, sy);
    sx = pvz_row_sum(sx);
    sy = pvz_row_sum(sy);

    const double * xs = x0 + ic * 6;
    double ux, uy;
    const double zx = pvz_finish(P, control_dt, xs[0], xs[1], xs[2], sx, ux);
    const double zy = pvz_finish(P, control_dt, xs[3], xs[4], xs[5], sy, uy);
    if(present && lane < 2)
    {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      zmp[inst * 2 + lane] = refused ? nan : (lane == 0 ? zx : zy);
      if(input) input[inst * 2 + lane] = refused ? nan : (lane == 0 ? ux : uy);
      if(status && lane == 0) status[inst] = refused ? CCC_STATUS_INFEASIBLE : CCC_STATUS_SOLVED;
    }
  }
}
} // namespace ccc_amd
