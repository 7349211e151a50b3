// ism_pcr_body.inc -- the solver body of the tridiagonal path of IntrinsicallyStableMpc, included by ism_plan_pcr_kernel
// (csrc/ism.hip, where the method is described) and by ism_closed_loop_kernel (csrc/ism_loop.hip): the safeguarded Newton
// iteration on the multiplier nu of the stability row around projected Newton on the box QP, parallel cyclic reduction
// as the tridiagonal solve.  One QP per wavefront; lane l holds rows idx[] = {l, l + 64} (in[u]: the row exists).
// The including scope provides
//   int N, max_outer; double e, c_eq            steps, outer budget, the off-diagonal -w_vel / dt^2, at'y = c_eq
//   int idx[2]; bool in[2], bad                 bad: some row has lo > hi (no iteration, CCC_STATUS_INFEASIBLE)
//   double lo[2], hi[2], q[2], at[2], dgn[2]    the box, the linear term, the stability row, the diagonal of the rows
//   double *Sy, *Sa, *Sr, *Sc, *Sd, *Se         the wavefront's six exchange arrays [kPcrNP] in LDS
//   bool pcr_warm                               the start: false = the equality-constrained first guess, nu from it, an
//                                               empty clamped set; true = y (clipped into [lo, hi] here), cl and nu as
//                                               they stand, the bracket of nu re-opened
//   double y[2], nu; bool cl[2]; int solves     in (warm) / out: the solution, its multiplier, its clamped set;
//                                               solves += the tridiagonal solves done
// and finds   int st   = CCC_STATUS_SOLVED, CCC_STATUS_MAX_ITER (a budget ran out) or CCC_STATUS_INFEASIBLE (bad).
  auto wsum = [&](double a, double b) { return WaveGroup<64>::sum(a + b); };
  // (H v)_i for the rows of this lane, v staged in Sy
  auto hmul = [&](const double (&v)[2], double (&hv)[2]) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for(int u = 0; u < 2; u++) Sy[idx[u]] = in[u] ? v[u] : 0.0;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for(int u = 0; u < 2; u++)
    {
      const int i = idx[u];
      const double vm = (i > 0) ? Sy[i - 1] : 0.0, vp = (i + 1 < N) ? Sy[i + 1] : 0.0;
      hv[u] = in[u] ? dgn[u] * v[u] + e * (vm + vp) : 0.0;
    }
  };
  // parallel cyclic reduction of the tridiagonal system (a, b, c) with the right-hand sides d and f; r = 1 / b on entry
  // and on exit the solutions are d * r and f * r
  auto pcr = [&](double (&a_)[2], double (&b_)[2], double (&c_)[2], double (&d_)[2], double (&f_)[2], double (&r_)[2]) {
    for(int s = 1; s < N; s <<= 1)
    {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for(int u = 0; u < 2; u++)
      {
        Sa[idx[u]] = a_[u];
        Sr[idx[u]] = r_[u];
        Sc[idx[u]] = c_[u];
        Sd[idx[u]] = d_[u];
        Se[idx[u]] = f_[u];
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for(int u = 0; u < 2; u++)
      {
        const int im = idx[u] - s, ip = idx[u] + s;
        const bool hm = im >= 0, hp = ip < kPcrNP;
        const double k1 = hm ? a_[u] * Sr[im] : 0.0, k2 = hp ? c_[u] * Sr[ip] : 0.0;
        const double am = hm ? Sa[im] : 0.0, cm = hm ? Sc[im] : 0.0, dm = hm ? Sd[im] : 0.0, fm = hm ? Se[im] : 0.0;
        const double ap = hp ? Sa[ip] : 0.0, cq = hp ? Sc[ip] : 0.0, dp = hp ? Sd[ip] : 0.0, fp = hp ? Se[ip] : 0.0;
        b_[u] = b_[u] - cm * k1 - ap * k2;
        d_[u] = d_[u] - dm * k1 - dp * k2;
        f_[u] = f_[u] - fm * k1 - fp * k2;
        a_[u] = -am * k1;
        c_[u] = -cq * k2;
        r_[u] = fast_rcp(b_[u]); // (v_rcp_f64 + two Newton steps: relative error ~1e-16, the pivots are >= w_zmp)
      }
    }
  };
  double nu_lo = -kIsmInf, nu_hi = kIsmInf; // (a warm start keeps nu and re-opens its bracket)
  if(!pcr_warm)
  {
    // first guess: the equality-constrained minimiser without the box, y = H^-1(-q) - nu H^-1 at with nu from at'y = c,
    // clamped -- the multiplier the outer iteration starts from is then usually within a step or two of the root
    nu = 0.0;
    double a_[2], b_[2], c_[2], d_[2], f_[2], r_[2];
#pragma unroll
    for(int u = 0; u < 2; u++)
    {
      a_[u] = (in[u] && idx[u] > 0) ? e : 0.0;
      c_[u] = (in[u] && idx[u] + 1 < N) ? e : 0.0;
      b_[u] = in[u] ? dgn[u] : 1.0;
      d_[u] = in[u] ? -q[u] : 0.0;
      f_[u] = in[u] ? at[u] : 0.0;
      r_[u] = fast_rcp(b_[u]);
    }
    pcr(a_, b_, c_, d_, f_, r_);
    ++solves;
    const double s0[2] = {d_[0] * r_[0], d_[1] * r_[1]}, s1[2] = {f_[0] * r_[0], f_[1] * r_[1]};
    const double num = wsum(at[0] * s0[0], at[1] * s0[1]) - c_eq, den = wsum(at[0] * s1[0], at[1] * s1[1]);
    if(den > 1e-300) nu = num / den;
#pragma unroll
    for(int u = 0; u < 2; u++) y[u] = in[u] ? fmin(fmax(s0[u] - nu * s1[u], lo[u]), hi[u]) : 0.0;
    cl[0] = false;
    cl[1] = false;
  }
  else
  {
#pragma unroll
    for(int u = 0; u < 2; u++) y[u] = in[u] ? fmin(fmax(y[u], lo[u]), hi[u]) : 0.0;
  }
  double sdir[2] = {0.0, 0.0}; // H_FF^-1 at of the last solve
  double hv[2] = {0.0, 0.0};   // H y, carried from the line search into the next iteration
  bool have_hv = false;
  bool exact_move = false;     // the last change of y was the affine move along the multiplier, unclipped
  int st = CCC_STATUS_MAX_ITER;
  if(__any(bad)) st = CCC_STATUS_INFEASIBLE;
  for(int outer = 0; outer < max_outer && st == CCC_STATUS_MAX_ITER; outer++)
  {
    bool first = true, full = true, inner_ok = false;
    for(int inner = 0; inner < kPcrInner; inner++)
    {
      double qq[2], g[2];
      if(!have_hv) hmul(y, hv);
      have_hv = true;
      bool ncl[2];
      bool changed = false;
#pragma unroll
      for(int u = 0; u < 2; u++)
      {
        qq[u] = q[u] + nu * at[u];
        g[u] = hv[u] + qq[u];
        ncl[u] = in[u] && ((y[u] <= lo[u] && g[u] > 0.0) || (y[u] >= hi[u] && g[u] < 0.0));
        changed = changed || (ncl[u] != cl[u]);
      }
      if((!first || exact_move) && !__any(changed) && full)
      {
        inner_ok = true;
        break;
      }
      first = false;
      const double J0 = wsum(in[0] ? y[0] * (0.5 * hv[0] + qq[0]) : 0.0, in[1] ? y[1] * (0.5 * hv[1] + qq[1]) : 0.0);
      // ---- Newton step: tridiagonal system on the free rows, identity on the clamped / padding rows; PCR
      double a_[2], b_[2], c_[2], d_[2], f_[2], r_[2];
#pragma unroll
      for(int u = 0; u < 2; u++)
      {
        cl[u] = ncl[u];
        const bool fr = in[u] && !cl[u];
        a_[u] = (fr && idx[u] > 0) ? e : 0.0;
        c_[u] = (fr && idx[u] + 1 < N) ? e : 0.0;
        b_[u] = fr ? dgn[u] : 1.0;
        d_[u] = fr ? -qq[u] : (in[u] ? y[u] : 0.0);
        f_[u] = fr ? at[u] : 0.0;
        r_[u] = fast_rcp(b_[u]);
      }
      pcr(a_, b_, c_, d_, f_, r_);
      ++solves;
      double xn[2];
#pragma unroll
      for(int u = 0; u < 2; u++)
      {
        xn[u] = d_[u] * r_[u];
        sdir[u] = f_[u] * r_[u];
      }
      // ---- projected step, halved until the objective does not increase
      double alpha = 1.0;
      for(;;)
      {
        double yt[2], ht[2];
#pragma unroll
        for(int u = 0; u < 2; u++) yt[u] = in[u] ? fmin(fmax(y[u] + alpha * (xn[u] - y[u]), lo[u]), hi[u]) : 0.0;
        hmul(yt, ht);
        const double Jt = wsum(in[0] ? yt[0] * (0.5 * ht[0] + qq[0]) : 0.0, in[1] ? yt[1] * (0.5 * ht[1] + qq[1]) : 0.0);
        if(Jt <= J0 + 1e-14 * fabs(J0) || alpha < 1e-8)
        {
          y[0] = yt[0];
          y[1] = yt[1];
          hv[0] = ht[0]; // H y of the accepted point: the gradient of the next iteration
          hv[1] = ht[1];
          break;
        }
        alpha *= 0.5;
      }
      full = alpha == 1.0;
    }
    if(!inner_ok) break; // inner iteration out of budget
    const double phi = wsum(at[0] * y[0], at[1] * y[1]) - c_eq;
    if(fabs(phi) <= 1e-13 * (1.0 + fabs(c_eq)))
    {
      st = CCC_STATUS_SOLVED;
      break;
    }
    if(phi > 0.0)
      nu_lo = nu;
    else
      nu_hi = nu;
    const double slope = wsum(at[0] * sdir[0], at[1] * sdir[1]); // > 0;  d phi / d nu = -slope
    double nn = slope > 1e-300 ? nu + phi / slope : (phi > 0.0 ? nu + 1.0 : nu - 1.0);
    if(!(nu_lo < nn && nn < nu_hi))
    {
      const bool both = nu_lo > -kIsmInf && nu_hi < kIsmInf;
      nn = both ? 0.5 * (nu_lo + nu_hi) : nu + (2.0 * fabs(nu) + 1.0) * (phi > 0.0 ? 1.0 : -1.0);
    }
    // on the current free set y is affine in the multiplier: y(nn) = y - (nn - nu) H_FF^-1 at.  If that move stays inside
    // the box, the next inner loop finds the clamped set unchanged and stops without a solve (and phi is then zero up
    // to rounding); otherwise it is the warm start
    {
      const double dn = nn - nu;
      bool clipped = false;
#pragma unroll
      for(int u = 0; u < 2; u++)
        if(in[u] && !cl[u])
        {
          const double t = y[u] - dn * sdir[u];
          const double tc = fmin(fmax(t, lo[u]), hi[u]);
          clipped = clipped || (tc != t);
          y[u] = tc;
        }
      exact_move = !__any(clipped);
      have_hv = false;
    }
    nu = nn;
  }
