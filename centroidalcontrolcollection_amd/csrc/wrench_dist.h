// wrench_dist.h -- the box-constrained QP of ForceColl::WrenchDistribution::run() for one instance per 16-lane DPP row
// (four instances per wavefront), shared by the stand-alone kernel and the fused PreviewControlCentroidal kernel of
// csrc/wrench_dist.hip.
//
//   G (6 x m): column r = [(vertex_r - origin) x ridge_r; ridge_r]
//   minimise  1/2 (G s - w)' diag(ww) (G s - w) + 1/2 rho s's     s.t.  lo <= s_r <= hi
//
// Layout: ridge r = c + 16 j sits in lane c of the row, slot j < RPL (RPL = 1, 2, 4 for 16, 32, 64 ridge slots).  A lane
// keeps the six entries of its columns (scaled by sqrt(ww)), its s_r and its clamp state in registers; nothing M x M exists.
//
// One iteration, given the sets F (free), L (at lo), U (at hi):
//   1. A = G_F G_F' (21 sums) and r = w - G_B s_B (6 sums): 27 butterfly all-reductions over the row in DPP.  Every lane
//      needs all 27 (it factors redundantly), so the butterfly -- which leaves the sum in every lane -- replaces the packed
//      tree + broadcast that csrc/ddp_tile.h uses where one lane per sum is enough.
//   2. every lane: A = R'R (Cholesky with diagonal pivoting; rows whose pivot vanishes dropped: rank detection), then
//        z = (R R' + rho)^-1 R r,   v = R^+ z,   s_F = G_F' v.
//      This is the push-through solve  s_F = G_F'(rho + G_F G_F')^-1 r  written through the factor of G_F G_F' alone:
//      R R' is as well conditioned as the contact geometry whatever rho is, so neither 1/rho nor the huge
//      y = (unattainable part of r) / rho ever appears.  It covers |F| < 6 and rank-deficient G_F (two vertices) with the
//      same statements: the null directions of G_F G_F' are the dropped rows.  (The |F| x |F| primal system the design
//      note suggested for |F| < 6 would not cover |F| >= 6 at rank 5, and needs the free columns gathered into every lane.)
//      followed by one refinement step on the residual summed from the columns (six more row sums).
//   3. residual e = A v - r; every lane: s_r = g_r . v for its free ridges, gradient g_r . e + rho s_r for its clamped ones.
// Block mode (primal-dual active set): all sets change at once -- free ridges outside the box are clamped, clamped
// ridges whose multiplier has the wrong sign are freed -- until nothing changes.  If a set repeats (period 2) or the
// block budget runs out, the row restarts as a single-change primal active set from s = lo (ratio test, one release per
// step), which terminates on a strictly convex QP.  The answer is certified on the point itself (bounds, multiplier
// signs, scaled stationarity); a row that exhausts its budget or fails the certificate reports CCC_STATUS_MAX_ITER.
#pragma once

#include "common.h"
#include "wave_group.h"

namespace ccc_amd
{
struct WdConfig
{
  double sw[6];  // sqrt(wrench_weight)
  double isw[6]; // 1 / sqrt(wrench_weight)
  double rho, lo, hi;
};

constexpr int kWdBlockIters = 24; // block-mode budget before the single-change restart
constexpr double kWdRankTol = 1e-10; // a pivot below this fraction of A's largest diagonal entry: rank exhausted
constexpr double kWdCertTol = 1e-9;  // certificate: |gradient| <= this x (1 + |w|_inf) x max(1, |g_r|_inf)

__device__ __forceinline__ double wd_row_sum(double v)
{
  v += dpp_f64<kDppQuadXor1>(v);
  v += dpp_f64<kDppQuadXor2>(v);
  v += dpp_f64<kDppRowHalfMirror>(v);
  v += dpp_f64<kDppRowMirror>(v);
  return v;
}
__device__ __forceinline__ double wd_row_max(double v)
{
  v = max_raw(v, dpp_f64<kDppQuadXor1>(v));
  v = max_raw(v, dpp_f64<kDppQuadXor2>(v));
  v = max_raw(v, dpp_f64<kDppRowHalfMirror>(v));
  v = max_raw(v, dpp_f64<kDppRowMirror>(v));
  return v;
}
// the 16 ballot bits of the caller's row
__device__ __forceinline__ unsigned wd_row_ballot(bool p)
{
  return (unsigned)(__ballot(p) >> (threadIdx.x & 48)) & 0xffffu;
}

enum : int { kWdFree = 0, kWdLo = 1, kWdHi = 2, kWdNone = 3 };

// Solve one instance per row.  g[j][a]: column c + 16 j scaled by sw[a] (anything where st[j] == kWdNone); wt: desired
// wrench scaled by sw; m: ridges of the instance (0 for the rows beyond the batch, which run along with empty sets).  On return s[j]
// holds the ridge forces (0 where there is no ridge) and the return value is (iterations << 8) | CCC_STATUS_*.
template<int RPL>
__device__ __forceinline__ int wd_solve(const double (&g)[RPL][6], const double (&wt)[6], const WdConfig & C, int m,
                                        double (&s)[RPL])
{
  const int c = threadIdx.x & 15;
  int st[RPL];
  double gmax[RPL];
  double wmax = 0;
  for(int a = 0; a < 6; a++) wmax = fmax(wmax, fabs(wt[a]));
  for(int j = 0; j < RPL; j++)
  {
    const bool has = c + 16 * j < m;
    st[j] = has ? kWdLo : kWdNone;
    s[j] = has ? C.lo : 0.0;
    gmax[j] = 1.0;
    for(int a = 0; a < 6; a++) gmax[j] = fmax(gmax[j], fabs(g[j][a]));
  }
  const double ctol = kWdCertTol * (1.0 + wmax);
  // (releases use a tolerance well inside the certificate's, so that a released ridge is one the certificate would accept
  //  either way)
  const double gtol = 1e-3 * ctol;
  const int budget = kWdBlockIters + 8 * 16 * RPL + 64;
  bool single = false, active = true, certified = false;
  int iters = 0, prev1 = -1, prev2 = -2;

  while(__ballot(active) != 0ull)
  {
    // ---- 1. the 27 sums
    double acc[27];
    for(int i = 0; i < 27; i++) acc[i] = 0.0;
    for(int j = 0; j < RPL; j++)
    {
      const bool fr = st[j] == kWdFree, bd = st[j] == kWdLo || st[j] == kWdHi;
      int i = 0;
      for(int a = 0; a < 6; a++)
      {
        const double ga = fr ? g[j][a] : 0.0;
        for(int b = a; b < 6; b++, i++) acc[i] = fma(ga, g[j][b], acc[i]);
      }
      const double sb = bd ? s[j] : 0.0;
      for(int a = 0; a < 6; a++) acc[21 + a] = fma(sb, g[j][a], acc[21 + a]);
    }
    for(int i = 0; i < 27; i++) acc[i] = wd_row_sum(acc[i]);
    double A[6][6], r[6];
    {
      int i = 0;
      for(int a = 0; a < 6; a++)
        for(int b = a; b < 6; b++, i++) A[a][b] = A[b][a] = acc[i];
      for(int a = 0; a < 6; a++) r[a] = wt[a] - acc[21 + a];
    }
    // ---- 2. A = R'R by Cholesky with diagonal pivoting (outer-product form; the pivot row is picked with selects, nothing
    // is permuted in storage: row k of R has zeros in the columns of the earlier pivots).  Rank detection: once the
    // largest remaining diagonal is below kWdRankTol of the largest of A, that row and all later ones are zero (rinv = 0).
    // Without pivoting a rank-4 free set (four ridges of one vertex and a fifth) can meet a legitimate pivot of 5e-7 first
    // and noise just above any threshold after it: 8 instances in 65536 failed their certificate that way (measured).
    double S[6][6], R[6][6], rinv[6];
    int piv[6];
    bool used[6];
    double dmax0 = 0;
    for(int i = 0; i < 6; i++)
    {
      used[i] = false;
      dmax0 = fmax(dmax0, A[i][i]);
      for(int l = 0; l < 6; l++) S[i][l] = A[i][l];
    }
    for(int k = 0; k < 6; k++)
    {
      double best = -1.0;
      int p = 0;
      for(int j = 0; j < 6; j++)
      {
        const bool take = !used[j] && S[j][j] > best;
        best = take ? S[j][j] : best;
        p = take ? j : p;
      }
      const bool keep = best > kWdRankTol * dmax0;
      rinv[k] = keep ? rsqrt(best) : 0.0;
      piv[k] = p;
      for(int l = 0; l < 6; l++)
      {
        double t = S[0][l];
        for(int j = 1; j < 6; j++) t = p == j ? S[j][l] : t;
        R[k][l] = t * rinv[k];
      }
      for(int j = 0; j < 6; j++) used[j] = used[j] || p == j;
      for(int i = 0; i < 6; i++)
        for(int l = i; l < 6; l++) S[i][l] = S[l][i] = fma(-R[k][i], R[k][l], S[i][l]);
    }
    // M = R R' + rho (a dropped row: unit diagonal) = L L', in place (lower; the diagonal holds the reciprocals)
    double Mx[6][6];
    for(int i = 0; i < 6; i++)
    {
      for(int k = 0; k <= i; k++)
      {
        double t = 0;
        for(int l = 0; l < 6; l++) t = fma(R[i][l], R[k][l], t);
        Mx[i][k] = t;
      }
      Mx[i][i] += rinv[i] == 0.0 ? 1.0 : C.rho;
    }
    for(int j = 0; j < 6; j++)
    {
      double d = Mx[j][j];
      for(int k = 0; k < j; k++) d = fma(-Mx[j][k], Mx[j][k], d);
      const double di = rsqrt(d);
      Mx[j][j] = di;
      for(int i = j + 1; i < 6; i++)
      {
        double u = Mx[i][j];
        for(int k = 0; k < j; k++) u = fma(-Mx[i][k], Mx[j][k], u);
        Mx[i][j] = u * di;
      }
    }
    // x = R^+ (R R' + rho)^-1 R b: the range part of (rho + A)^-1 b
    auto back = [&](const double (&b)[6], double (&x)[6]) {
      double z[6];
      for(int j = 0; j < 6; j++)
      {
        double t = 0;
        for(int l = 0; l < 6; l++) t = fma(R[j][l], b[l], t);
        for(int k = 0; k < j; k++) t = fma(-Mx[j][k], z[k], t);
        z[j] = t * Mx[j][j];
      }
      for(int j = 5; j >= 0; j--)
      {
        double t = z[j];
        for(int i = j + 1; i < 6; i++) t = fma(-Mx[i][j], z[i], t);
        z[j] = t * Mx[j][j];
      }
      for(int l = 0; l < 6; l++) x[l] = 0.0;
      for(int k = 5; k >= 0; k--) // R x = z: row k meets the unknowns of the later pivots only
      {
        double t = z[k];
        for(int l = 0; l < 6; l++) t = fma(-R[k][l], x[l], t);
        t *= rinv[k];
        for(int l = 0; l < 6; l++) x[l] = piv[k] == l ? t : x[l];
      }
    };
    double v[6], dv[6], e[6], r2[6];
    back(r, v);
    // One step of refinement on the true residual r2 = r - G_F (G_F' v), summed from the columns (six more row sums):
    // A is a normal-equations matrix, so v carries eps x cond(G_F)^2 -- 1e-6 N on the wrench where four ridges of one
    // vertex and one of another are free and the desired wrench is far from attainable -- and the correction removes it.
    for(int a = 0; a < 6; a++) r2[a] = 0.0;
    for(int j = 0; j < RPL; j++)
    {
      double t = 0;
      for(int a = 0; a < 6; a++) t = fma(g[j][a], v[a], t);
      t = st[j] == kWdFree ? t : 0.0;
      for(int a = 0; a < 6; a++) r2[a] = fma(t, g[j][a], r2[a]);
    }
    for(int a = 0; a < 6; a++)
    {
      r2[a] = r[a] - wd_row_sum(r2[a]);
      e[a] = fma(-C.rho, v[a], r2[a]);
    }
    back(e, dv);
    for(int a = 0; a < 6; a++)
    {
      v[a] += dv[a];
      double t = -r2[a]; // e = A v - r = A dv - r2
      for(int b = 0; b < 6; b++) t = fma(A[a][b], dv[b], t);
      e[a] = t;
    }
    // ---- 3. every lane on its own ridges
    double val[RPL]; // free: the unconstrained s_r; clamped: the gradient
    bool cert = true;
    for(int j = 0; j < RPL; j++)
    {
      double t = 0, u = 0;
      for(int a = 0; a < 6; a++)
      {
        t = fma(g[j][a], v[a], t);
        u = fma(g[j][a], e[a], u);
      }
      u = fma(C.rho, st[j] == kWdFree ? t : s[j], u);
      val[j] = st[j] == kWdFree ? t : u;
      const double tol = ctol * gmax[j];
      // the certificate of the point (s_F = val, s_B at its bounds)
      if(st[j] == kWdFree) cert = cert && t >= C.lo && t <= C.hi && fabs(u) <= tol;
      if(st[j] == kWdLo) cert = cert && u >= -tol;
      if(st[j] == kWdHi) cert = cert && u <= tol;
    }
    iters += active ? 1 : 0;

    bool changed = false, restarted = false;
    if(__ballot(active && !single) != 0ull)
    {
      // block mode: every set changes at once
      int code = 0;
      for(int j = 0; j < RPL; j++)
      {
        int ns = st[j];
        if(st[j] == kWdFree) ns = val[j] < C.lo ? kWdLo : (val[j] > C.hi ? kWdHi : kWdFree);
        if(st[j] == kWdLo && val[j] < -gtol * gmax[j]) ns = kWdFree;
        if(st[j] == kWdHi && val[j] > gtol * gmax[j]) ns = kWdFree;
        code |= ns << (2 * j);
        if(active && !single)
        {
          changed = changed || ns != st[j];
          if(st[j] == kWdFree) s[j] = ns == kWdLo ? C.lo : (ns == kWdHi ? C.hi : val[j]);
          st[j] = ns;
        }
      }
      if(active && !single)
      {
        const bool row_changed = wd_row_ballot(changed) != 0u;
        const bool cycle = row_changed && (wd_row_ballot(code == prev2) == 0xffffu || iters >= kWdBlockIters);
        prev2 = prev1;
        prev1 = code;
        if(!row_changed)
        {
          active = false;
          certified = wd_row_ballot(cert) == 0xffffu;
        }
        else if(cycle)
        {
          single = true; // restart from the feasible corner s = lo
          for(int j = 0; j < RPL; j++)
            if(st[j] != kWdNone)
            {
              st[j] = kWdLo;
              s[j] = C.lo;
            }
          restarted = true;
        }
      }
    }
    const bool stepping = active && single && !restarted;
    if(__ballot(stepping) != 0ull)
    {
      // single-change primal active set: ratio test towards the solution of the current sets
      const double inf = __builtin_huge_val();
      double aj[RPL], wj[RPL], alpha = inf, viol = 0;
      for(int j = 0; j < RPL; j++)
      {
        // aj: the step at which free ridge j meets a bound; wj: by how much clamped ridge j's multiplier is wrong
        aj[j] = inf;
        if(st[j] == kWdFree && val[j] < C.lo) aj[j] = fmax((C.lo - s[j]) / (val[j] - s[j]), 0.0);
        if(st[j] == kWdFree && val[j] > C.hi) aj[j] = fmax((C.hi - s[j]) / (val[j] - s[j]), 0.0);
        wj[j] = st[j] == kWdLo ? -val[j] / gmax[j] - gtol : (st[j] == kWdHi ? val[j] / gmax[j] - gtol : -1.0);
        alpha = fmin(alpha, aj[j]);
        viol = fmax(viol, wj[j]);
      }
      const double amin = -wd_row_max(-alpha), vmax = wd_row_max(viol);
      const bool blocked = amin < 1.0;
      // the blocking ridge, or else the clamped ridge whose multiplier is most wrong (lowest index among ties)
      double pick = 1e9;
      for(int j = RPL - 1; j >= 0; j--)
        if(blocked ? aj[j] == amin : (vmax > 0.0 && wj[j] == vmax)) pick = (double)(c + 16 * j);
      const int sel = (int)(-wd_row_max(-pick));
      if(stepping)
      {
        for(int j = 0; j < RPL; j++)
        {
          const bool mine = sel == c + 16 * j;
          if(st[j] == kWdFree)
          {
            if(blocked)
            {
              s[j] = fma(amin, val[j] - s[j], s[j]);
              s[j] = fmin(fmax(s[j], C.lo), C.hi);
              if(mine)
              {
                st[j] = val[j] < C.lo ? kWdLo : kWdHi;
                s[j] = val[j] < C.lo ? C.lo : C.hi;
              }
            }
            else
              s[j] = val[j];
          }
          else if(!blocked && mine)
            st[j] = kWdFree;
        }
        if(!blocked && !(vmax > 0.0))
        {
          active = false;
          certified = wd_row_ballot(cert) == 0xffffu;
        }
      }
    }
    if(active && iters >= budget) active = false;
  }
  return (iters << 8) | (certified ? CCC_STATUS_SOLVED : CCC_STATUS_MAX_ITER);
}
} // namespace ccc_amd
