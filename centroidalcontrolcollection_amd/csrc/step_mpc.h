// step_mpc.h -- CCC::StepMpc (footstep-adapting MPC, src/StepMpc.cpp:26-200) for one instance per 16-lane DPP row.
//
// The reference forms the normal matrix eq_mat = J'J of a linear least-squares problem in the n <= 16 piecewise-constant
// ZMPs u_0 .. u_{n-1} and solves it by a pivoted QR.  The rows of J hold the unstable mode e^{w t} over the whole
// horizon, so cond(eq_mat) = cond(J)^2 and the normal equations lose their digits from about 5 s of horizon on.  This
// kernel never forms J'J: it generates the weighted rows of J one at a time and rotates each into an upper-triangular
// R by Givens rotations (row-append QR), both axes as two right-hand sides of the one factorisation (the axes share the
// timeline, so they share J).
//
// Work split.  Lane j of a 16-lane row owns unknown j: column j of R in registers (Rc[k] = R[k][j], k a compile-time
// index in fully unrolled loops), entry j of both right-hand sides, the duration / flag / reference ZMP of element j
// and the two sensitivities of the modal state after the current stage to u_j:
//     xi = x + v / w,  zeta = x - v / w;   one element of duration T maps   xi <- e xi + (1 - e) u,
//     zeta <- zeta / e + (1 - 1 / e) u   with e = exp(w T)   (StepModel's Ad_, Bd_ in modal coordinates)
//     a_j = d xi / d u_j,  b_j = d zeta / d u_j:   one multiply each per stage, created as 1 - e_i, 1 - 1 / e_i at stage i.
// Position (a + b) / 2, velocity w (a - b) / 2, capture point a.  The free responses xi0, zeta0 of both axes advance the
// same way, redundantly in every lane.  A row of stage i is zero beyond column i: i + 1 rotations.  R[k][k], the row's
// k-th entry and d[k] reach the other lanes by DPP row_newbcast; a row that does not exist (another instance of the
// wavefront has it, this one has not) is the zero row with a zero right-hand side, whose rotations are identities --
// no divergent loop bounds.  The ZMP rows are diagonal and go first: they ARE the initial R and d.  No LDS, no scratch.
#pragma once

#include <cstdint>

#include "wave_group.h"

namespace ccc_amd
{
struct StepParams
{
  double omega;                                           // sqrt(g / com_height)
  double s_free, s_fixed, s_ds, s_pos, s_vel, s_cpa, s_cpr; // square roots of the weights (0: the rows are dropped)
};

template<int K>
__device__ __forceinline__ double step_bcast(double v)
{
  return dpp_f64<0x150 + K>(v); // DPP row_newbcast:K
}

__device__ __forceinline__ double step_row_sum(double v)
{
  v += dpp_f64<kDppQuadXor1>(v);
  v += dpp_f64<kDppQuadXor2>(v);
  v += dpp_f64<kDppRowHalfMirror>(v);
  v += dpp_f64<kDppRowMirror>(v);
  return v;
}

// Rotate the row (x: entry of this lane's column; yx, yy: its right-hand sides, the same in every lane of the row) into
// rows 0 .. I of R.  Rows beyond column I are zero by construction.
template<int I, int K = 0>
__device__ __forceinline__ void step_rotate(double (&Rc)[16], double & dx, double & dy, double x, double yx, double yy,
                                            int lane)
{
  const double rkk = step_bcast<K>(Rc[K]); // R[K][K] (> 0: it starts as the square root of a positive weight)
  const double xk = step_bcast<K>(x);
  const double dxk = step_bcast<K>(dx);
  const double dyk = step_bcast<K>(dy);
  const bool nz = xk != 0.0;
  const double rinv = 1.0 / sqrt(fma(rkk, rkk, xk * xk));
  const double c = nz ? rkk * rinv : 1.0;
  const double s = nz ? xk * rinv : 0.0;
  const double r_old = Rc[K];
  Rc[K] = fma(c, r_old, s * x);
  x = fma(c, x, -(s * r_old));
  const double ndx = fma(c, dxk, s * yx), ndy = fma(c, dyk, s * yy);
  yx = fma(c, yx, -(s * dxk));
  yy = fma(c, yy, -(s * dyk));
  dx = lane == K ? ndx : dx;
  dy = lane == K ? ndy : dy;
  if constexpr(K < I) step_rotate<I, K + 1>(Rc, dx, dy, x, yx, yy, lane);
}

// Per-row state of the stage recursion.
struct StepRow
{
  int lane, n;          // lane inside the row; elements (0 for an instance that is absent or refused)
  unsigned ss;          // bit i: element i is single support (bits at and beyond n clear)
  bool future_ss;       // some single-support element with index >= 1
  double e, einv, ce, cinv; // of this lane's element: exp(w T), its reciprocal, 1 - e, 1 - 1 / e   (1, 1, 0, 0 beyond n)
  double zx, zy;        // reference ZMP of this lane's element (0 beyond n)
  double a, b;          // sensitivities of xi, zeta after the current stage to this lane's unknown
  double xix, xiy, zex, zey; // free responses
};

// The (up to) six rows of stage I, generated first and then rotated in by ONE loop whose trip is not unrolled: the I + 1
// rotations are instantiated once per stage (136 bodies in all) instead of once per row kind.
template<typename T>
struct StepSix
{
  T v0, v1, v2, v3, v4, v5;
  // hand out the first, move the others up (the loop over the rows indexes nothing: a row picked by its number is
  // turned into a table in scratch by the compiler)
  __device__ __forceinline__ T pop()
  {
    const T r = v0;
    v0 = v1;
    v1 = v2;
    v2 = v3;
    v3 = v4;
    v4 = v5;
    return r;
  }
};
struct StepRows
{
  StepSix<double> x, yx, yy;
  StepSix<bool> has;
};

template<int I>
__device__ __forceinline__ void step_stage(const StepParams & P, StepRow & S, double (&Rc)[16], double & dx, double & dy)
{
  if(__ballot(I < S.n) == 0ull) return; // no instance of this wavefront has a stage I
  const bool live = I < S.n;
  const bool ss_i = (S.ss >> I) & 1u;
  const double dlt = S.lane == I ? 1.0 : 0.0;
  const double zxi = step_bcast<I>(S.zx), zyi = step_bcast<I>(S.zy);
  StepRows W;
  // -- rows on the state BEFORE element I (src/StepMpc.cpp:66-80, 135-145, 163-179)
  {
    // double support between two single supports: [1, -2, 1] on elements I - 2, I - 1, I
    W.has.v0 = I >= 2 && P.s_ds > 0.0 && live && ((S.ss >> (I >= 2 ? I - 2 : 0)) & 7u) == 5u;
    W.x.v0 = S.lane == I || S.lane == I - 2 ? P.s_ds : (S.lane == I - 1 ? -2.0 * P.s_ds : 0.0);
    W.yx.v0 = 0.0;
    W.yy.v0 = 0.0;
    // capture point after element I - 1 against the ZMP of the single-support element I: absolute, relative
    const bool has = I >= 1 && live && ss_i && S.future_ss;
    W.has.v1 = has && P.s_cpa > 0.0;
    W.x.v1 = P.s_cpa * S.a;
    W.yx.v1 = P.s_cpa * (zxi - S.xix);
    W.yy.v1 = P.s_cpa * (zyi - S.xiy);
    W.has.v2 = has && P.s_cpr > 0.0;
    W.x.v2 = P.s_cpr * (S.a - dlt);
    W.yx.v2 = -(P.s_cpr * S.xix);
    W.yy.v2 = -(P.s_cpr * S.xiy);
  }
  // -- element I
  {
    const double e = step_bcast<I>(S.e), einv = step_bcast<I>(S.einv);
    const double ce = step_bcast<I>(S.ce), cinv = step_bcast<I>(S.cinv);
    S.a = S.lane == I ? ce : (S.lane < I ? S.a * e : 0.0);
    S.b = S.lane == I ? cinv : (S.lane < I ? S.b * einv : 0.0);
    S.xix *= e;
    S.xiy *= e;
    S.zex *= einv;
    S.zey *= einv;
  }
  // -- rows on the state AFTER element I (src/StepMpc.cpp:82-109, 124-134)
  {
    // position against the ZMP of element min(I + 1, n - 1)
    const double zxn = step_bcast<(I < 15 ? I + 1 : 15)>(S.zx), zyn = step_bcast<(I < 15 ? I + 1 : 15)>(S.zy);
    const bool last = I + 1 >= S.n;
    W.has.v3 = live && P.s_pos > 0.0;
    W.x.v3 = P.s_pos * (0.5 * (S.a + S.b));
    W.yx.v3 = P.s_pos * ((last ? zxi : zxn) - 0.5 * (S.xix + S.zex));
    W.yy.v3 = P.s_pos * ((last ? zyi : zyn) - 0.5 * (S.xiy + S.zey));
    // velocity against zero
    const double sw = P.s_vel * (0.5 * P.omega);
    W.has.v4 = live && P.s_vel > 0.0;
    W.x.v4 = sw * (S.a - S.b);
    W.yx.v4 = -(sw * (S.xix - S.zex));
    W.yy.v4 = -(sw * (S.xiy - S.zey));
    // no single support ahead: the capture point after element I against the ZMP of element I
    W.has.v5 = live && P.s_cpa > 0.0 && !S.future_ss && (I >= 1 || !(S.ss & 1u));
    W.x.v5 = P.s_cpa * S.a;
    W.yx.v5 = P.s_cpa * (zxi - S.xix);
    W.yy.v5 = P.s_cpa * (zyi - S.xiy);
  }
#pragma unroll 1
  for(int s = 0; s < 6; ++s)
  {
    const bool has = W.has.pop();
    const double x = W.x.pop(), yx = W.yx.pop(), yy = W.yy.pop();
    if(__ballot(has) == 0ull) continue;
    // a row this instance does not have is the zero row: its rotations are identities
    step_rotate<I>(Rc, dx, dy, has ? x : 0.0, has ? yx : 0.0, has ? yy : 0.0, S.lane);
  }
}

// u = R^-1 d for both right-hand sides, row by row from the bottom: lane j holds R[k][j] and u_j, the products of row k
// are summed over the DPP row.
template<int K>
__device__ __forceinline__ void step_backsub(const double (&Rc)[16], double dx, double dy, double & ux, double & uy, int lane)
{
  const double sx = step_row_sum(lane > K ? Rc[K] * ux : 0.0);
  const double sy = step_row_sum(lane > K ? Rc[K] * uy : 0.0);
  if(lane == K)
  {
    ux = (dx - sx) / Rc[K];
    uy = (dy - sy) / Rc[K];
  }
  if constexpr(K > 0) step_backsub<K - 1>(Rc, dx, dy, ux, uy, lane);
}

template<int I>
__device__ __forceinline__ void step_all_stages(const StepParams & P, StepRow & S, double (&Rc)[16], double & dx, double & dy)
{
  if constexpr(I > 0) step_all_stages<I - 1>(P, S, Rc, dx, dy);
  step_stage<I>(P, S, Rc, dx, dy);
}
} // namespace ccc_amd

// the handle of the C-ABI (csrc/step_mpc.hip creates it, csrc/step_mpc_loop.hip reads P and device)
struct ccc_step
{
  int device = 0;
  ccc_amd::StepParams P;
  char * d_stage = nullptr;
  int64_t cap = 0;
  hipStream_t stream = nullptr;
};
