// wrench_dist.hip -- ForceColl::WrenchDistribution::run() on MI355X (gfx950), stand-alone and fused behind
// CCC::PreviewControlCentroidal::planOnce(): kernels + C-ABI.
//
// Path replaced (reference file:line under /root/reference):
//   src/PreviewControlCentroidal.cpp:29-46    procOnce: jerk = -K x + F ref, force = inertia (acc + control_dt jerk)
//   src/PreviewControlCentroidal.cpp:97-129   planOnce: six axes, + m g on f_z, the wrench distribution about the CoM
//   include/CCC/PreviewControl.h:93-171       calcGain (host, at create): DARE by doubling, K, F with the last-column rule
//   ForceColl::WrenchDistribution::run        (external) the box-constrained QP over the ridge forces: csrc/wrench_dist.h
//
// Work split: one instance per 16-lane DPP row, four per wavefront, sixteen per 256-thread workgroup; ridge c + 16 j in lane
// c (csrc/wrench_dist.h).  The fused kernel stages the six gain rows once per workgroup in LDS, permuted into the flat
// order of an instance's reference block [N][12]; the 16 lanes of a row stream that block coalesced.  Flat element
// f = c + 16 t belongs to class (axis, kind) = f mod 12 = (c + 4 t) mod 12, which has period three in t: a lane meets three
// classes only, so three accumulators and a loop unrolled by three, then six row reductions (one per axis).
#include "wrench_dist.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ccc_amd
{
constexpr double kPccG = 9.80665; // CCC::constants::g

struct WdBatch
{
  long n;
  const int * dim;
  const double * vertex; // [n][M][3]
  const double * ridge;  // [n][M][3]
  double * wrench;       // [n][6]
  double * scales;       // [n][M] or null
  int * status;          // [n] or null
};

// loads the row's contact columns (scaled), solves, stores; w: desired wrench, o: moment origin (row uniform)
template<int RPL>
__device__ __forceinline__ void wd_instance(const WdBatch & B, const WdConfig & C, long k, bool live, const double (&w)[6],
                                            const double (&o)[3])
{
  constexpr int M = 16 * RPL;
  const int c = threadIdx.x & 15;
  const int m = live ? min(max(B.dim[k], 0), M) : 0;
  double g[RPL][6], wt[6], s[RPL];
  for(int j = 0; j < RPL; j++)
  {
    const int r = c + 16 * j;
    double p[3] = {0, 0, 0}, d[3] = {0, 0, 0};
    if(r < m)
    {
      const double * v = B.vertex + ((size_t)k * M + r) * 3;
      const double * q = B.ridge + ((size_t)k * M + r) * 3;
      for(int a = 0; a < 3; a++)
      {
        p[a] = v[a] - o[a];
        d[a] = q[a];
      }
    }
    g[j][0] = C.sw[0] * (p[1] * d[2] - p[2] * d[1]);
    g[j][1] = C.sw[1] * (p[2] * d[0] - p[0] * d[2]);
    g[j][2] = C.sw[2] * (p[0] * d[1] - p[1] * d[0]);
    for(int a = 0; a < 3; a++) g[j][3 + a] = C.sw[3 + a] * d[a];
  }
  for(int a = 0; a < 6; a++) wt[a] = C.sw[a] * w[a];
  const int status = wd_solve<RPL>(g, wt, C, m, s);
  // the projected wrench G s
  double out[6];
  for(int a = 0; a < 6; a++)
  {
    double t = 0;
    for(int j = 0; j < RPL; j++) t = fma(g[j][a], s[j], t);
    out[a] = wd_row_sum(t) * C.isw[a];
  }
  if(!live) return;
  if(B.scales)
    for(int j = 0; j < RPL; j++) B.scales[(size_t)k * M + c + 16 * j] = s[j];
  if(c == 0)
  {
    for(int a = 0; a < 6; a++) B.wrench[k * 6 + a] = out[a];
    if(B.status) B.status[k] = status;
  }
}

template<int RPL>
__global__ __launch_bounds__(256) void wrench_dist_kernel(WdBatch B, WdConfig C, const double * __restrict__ desired,
                                                          const double * __restrict__ origin)
{
  const long k = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool live = k < B.n;
  double w[6] = {0, 0, 0, 0, 0, 0}, o[3] = {0, 0, 0};
  if(live)
  {
    for(int a = 0; a < 6; a++) w[a] = desired[k * 6 + a];
    for(int a = 0; a < 3; a++) o[a] = origin[k * 3 + a];
  }
  wd_instance<RPL>(B, C, k, live, w, o);
}

struct PccParams
{
  int N;
  double K[6][3];
  double inertia[6]; // moment of inertia (3), mass (3)
  double mg, control_dt;
};

template<int RPL>
__global__ __launch_bounds__(256) void pcc_plan_kernel(WdBatch B, WdConfig C, PccParams P,
                                                       const double * __restrict__ gains, // [N][12], permuted (see create)
                                                       const double * __restrict__ x0,    // [n][18]
                                                       const double * __restrict__ ref,   // [n][N][12]
                                                       double * __restrict__ planned)     // [n][6] or null
{
  extern __shared__ double lds_gain[]; // [12 N]
  const int L = 12 * P.N;
  for(int i = threadIdx.x; i < L; i += 256) lds_gain[i] = gains[i];
  __syncthreads();
  const long k = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool live = k < B.n;
  const int c = threadIdx.x & 15;
  double acc[3] = {0, 0, 0};
  if(live)
  {
    const double * rk = ref + (size_t)k * L;
    int f = c;
    for(; f + 32 < L; f += 48) // three flat elements per turn: classes (c + 4 u) mod 12, u = 0, 1, 2
    {
      const double r0 = rk[f], r1 = rk[f + 16], r2 = rk[f + 32];
      acc[0] = fma(lds_gain[f], r0, acc[0]);
      acc[1] = fma(lds_gain[f + 16], r1, acc[1]);
      acc[2] = fma(lds_gain[f + 32], r2, acc[2]);
    }
    if(f < L) acc[0] = fma(lds_gain[f], rk[f], acc[0]);
    if(f + 16 < L) acc[1] = fma(lds_gain[f + 16], rk[f + 16], acc[1]);
  }
  double w[6], o[3] = {0, 0, 0};
  for(int a = 0; a < 6; a++)
  {
    double t = 0;
    for(int u = 0; u < 3; u++) t += (c + 4 * u) % 6 == a ? acc[u] : 0.0;
    const double fr = wd_row_sum(t); // F_a . ref_a
    double jerk = fr, xa2 = 0;
    if(live)
    {
      const double * x = x0 + k * 18;
      xa2 = x[12 + a];
      jerk = fr - (P.K[a][0] * x[a] + P.K[a][1] * x[6 + a] + P.K[a][2] * xa2);
    }
    w[a] = P.inertia[a] * fma(P.control_dt, jerk, xa2);
  }
  w[5] += P.mg;
  if(live)
  {
    for(int a = 0; a < 3; a++) o[a] = x0[k * 18 + 3 + a]; // initial_param.pos.linear()
    if(planned && c == 0)
      for(int a = 0; a < 6; a++) planned[k * 6 + a] = w[a];
  }
  wd_instance<RPL>(B, C, k, live, w, o);
}

static int make_config(const ccc_wrench_dist_config_t * cfg, WdConfig & C, const char * who)
{
  ccc_wrench_dist_config_t d;
  ccc_wrench_dist_default_config(&d);
  if(cfg) d = *cfg;
  for(int a = 0; a < 6; a++)
  {
    if(!(d.wrench_weight[a] > 0) || !std::isfinite(d.wrench_weight[a]))
      return fail(CCC_ERR_INVALID_ARGUMENT, "%s: wrench_weight[%d] must be > 0", who, a);
    C.sw[a] = std::sqrt(d.wrench_weight[a]);
    C.isw[a] = 1.0 / C.sw[a];
  }
  if(!(d.regular_weight > 0) || !std::isfinite(d.regular_weight))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: regular_weight must be > 0", who);
  if(!(d.ridge_force_min <= d.ridge_force_max) || !std::isfinite(d.ridge_force_min) || !std::isfinite(d.ridge_force_max))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: ridge_force_min <= ridge_force_max (finite) is required", who);
  C.rho = d.regular_weight;
  C.lo = d.ridge_force_min;
  C.hi = d.ridge_force_max;
  return CCC_OK;
}

static int check_ridges(int max_ridges, const char * who)
{
  if(max_ridges != 16 && max_ridges != 32 && max_ridges != 64)
    return fail(CCC_ERR_UNSUPPORTED, "%s: max_ridges = %d is not built into this library (16, 32 or 64)", who, max_ridges);
  return CCC_OK;
}

// include/CCC/PreviewControl.h:93-171 for the model of src/PreviewControlCentroidal.cpp:10-19, in extended precision
typedef long double real;
struct M3
{
  real v[3][3];
};
static M3 m3_zero()
{
  M3 r;
  for(auto & row : r.v)
    for(real & x : row) x = 0;
  return r;
}
static M3 m3_eye()
{
  M3 r = m3_zero();
  for(int i = 0; i < 3; i++) r.v[i][i] = 1;
  return r;
}
static M3 mul(const M3 & a, const M3 & b)
{
  M3 r = m3_zero();
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
      for(int k = 0; k < 3; k++) r.v[i][j] += a.v[i][k] * b.v[k][j];
  return r;
}
static M3 add(const M3 & a, const M3 & b, real sb = 1)
{
  M3 r;
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++) r.v[i][j] = a.v[i][j] + sb * b.v[i][j];
  return r;
}
static M3 tr(const M3 & a)
{
  M3 r;
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++) r.v[i][j] = a.v[j][i];
  return r;
}
static real fro(const M3 & a)
{
  real s = 0;
  for(auto & row : a.v)
    for(real x : row) s += x * x;
  return std::sqrt(s);
}
static M3 inv(const M3 & a)
{
  M3 r;
  const auto & m = a.v;
  const real c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2],
             c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const real det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
  r.v[0][0] = c00 / det;
  r.v[1][0] = c01 / det;
  r.v[2][0] = c02 / det;
  r.v[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det;
  r.v[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det;
  r.v[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
  r.v[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
  r.v[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
  r.v[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
  return r;
}

// one axis: K [3], F [2N], riccati_error
static void calc_gain(double inertia, double dt_, int N, double w_pos, double w_wrench, double w_jerk, double * K, double * F,
                      double * riccati_error)
{
  const real dt = dt_, q[2] = {w_pos, w_wrench}, Rw = w_jerk;
  // the chain of integrators is nilpotent: Ad = I + A dt + A^2 dt^2/2, Bd = [dt^3/6, dt^2/2, dt]
  M3 A = m3_eye();
  A.v[0][1] = A.v[1][2] = dt;
  A.v[0][2] = dt * dt / 2;
  const real Bv[3] = {dt * dt * dt / 6, dt * dt / 2, dt};
  const real Cm[2][3] = {{1, 0, 0}, {0, 0, (real)inertia}};
  M3 G0 = m3_zero(), H0 = m3_zero();
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
    {
      G0.v[i][j] = Bv[i] * Bv[j] / Rw;
      for(int o = 0; o < 2; o++) H0.v[i][j] += Cm[o][i] * q[o] * Cm[o][j];
    }
  const M3 CtQC = H0;
  M3 A0 = A, H1 = H0;
  for(int it = 0; it < 10000; it++)
  {
    const M3 Ii = inv(add(m3_eye(), mul(G0, H0)));
    const M3 A1 = mul(mul(A0, Ii), A0);
    const M3 G1 = add(G0, mul(mul(mul(A0, Ii), G0), tr(A0)));
    H1 = add(H0, mul(mul(mul(tr(A0), H0), Ii), A0));
    if(fro(add(H1, H0, -1)) / fro(H1) < 1e-8L) break;
    A0 = A1;
    G0 = G1;
    H0 = H1;
  }
  const M3 & Pm = H1;
  // B'P, R + B'PB
  real BtP[3] = {0, 0, 0}, BtPB = 0;
  for(int j = 0; j < 3; j++)
    for(int i = 0; i < 3; i++) BtP[j] += Bv[i] * Pm.v[i][j];
  for(int j = 0; j < 3; j++) BtPB += BtP[j] * Bv[j];
  const real rinv = 1 / (Rw + BtPB);
  real Kr[3] = {0, 0, 0};
  for(int j = 0; j < 3; j++)
  {
    for(int i = 0; i < 3; i++) Kr[j] += BtP[i] * A.v[i][j];
    Kr[j] *= rinv;
    K[j] = (double)Kr[j];
  }
  {
    // P - (A'PA + C'QC - A'PB (R + B'PB)^-1 B'PA)
    const M3 AtPA = mul(mul(tr(A), Pm), A);
    real AtPB[3] = {0, 0, 0};
    for(int i = 0; i < 3; i++)
      for(int j = 0; j < 3; j++) AtPB[i] += A.v[j][i] * BtP[j];
    M3 E;
    for(int i = 0; i < 3; i++)
      for(int j = 0; j < 3; j++) E.v[i][j] = Pm.v[i][j] - (AtPA.v[i][j] + CtQC.v[i][j] - AtPB[i] * rinv * AtPB[j]);
    *riccati_error = (double)fro(E);
  }
  M3 ABK; // A - B K
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++) ABK.v[i][j] = A.v[i][j] - Bv[i] * Kr[j];
  const M3 ABKt = tr(ABK);
  M3 fSub = m3_eye();
  for(int i = 0; i < N; i++)
  {
    real bf[3] = {0, 0, 0}; // B' fSub
    for(int j = 0; j < 3; j++)
      for(int l = 0; l < 3; l++) bf[j] += Bv[l] * fSub.v[l][j];
    for(int o = 0; o < 2; o++)
    {
      real t = 0;
      if(i < N - 1)
        for(int j = 0; j < 3; j++) t += bf[j] * Cm[o][j] * q[o];
      else // the last column: P C' (https://github.com/euslisp/jskeus/pull/551)
        for(int j = 0; j < 3; j++)
          for(int l = 0; l < 3; l++) t += bf[j] * Pm.v[j][l] * Cm[o][l];
      F[2 * i + o] = (double)(rinv * t);
    }
    fSub = mul(fSub, ABKt);
  }
}
} // namespace ccc_amd

using namespace ccc_amd;

extern "C" void ccc_wrench_dist_default_config(ccc_wrench_dist_config_t * cfg)
{
  if(!cfg) return;
  for(double & w : cfg->wrench_weight) w = 1.0;
  cfg->regular_weight = 1e-8;
  cfg->ridge_force_min = 3.0;
  cfg->ridge_force_max = 1000.0;
}

extern "C" int ccc_wrench_distribution_device(int64_t n, int max_ridges, const int32_t * dim, const double * vertex,
                                              const double * ridge, const double * desired_wrench, const double * origin,
                                              const ccc_wrench_dist_config_t * cfg, double * wrench_out, double * scales_out,
                                              int32_t * status, void * stream)
{
  const char * who = "ccc_wrench_distribution_device";
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(int rc = check_ridges(max_ridges, who)) return rc;
  WdConfig C;
  if(int rc = make_config(cfg, C, who)) return rc;
  if(n == 0) return CCC_OK;
  if(!dim || !vertex || !ridge || !desired_wrench || !origin || !wrench_out)
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  WdBatch B{(long)n, dim, vertex, ridge, wrench_out, scales_out, status};
  const dim3 grid((unsigned)((n + 15) / 16));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch(max_ridges)
  {
    case 16: hipLaunchKernelGGL(wrench_dist_kernel<1>, grid, dim3(256), 0, s, B, C, desired_wrench, origin); break;
    case 32: hipLaunchKernelGGL(wrench_dist_kernel<2>, grid, dim3(256), 0, s, B, C, desired_wrench, origin); break;
    default: hipLaunchKernelGGL(wrench_dist_kernel<4>, grid, dim3(256), 0, s, B, C, desired_wrench, origin); break;
  }
  CCC_HIP_CHECK(hipGetLastError());
  return CCC_OK;
}

struct ccc_pcc
{
  int device = 0, N = 0, max_ridges = 16;
  double mass = 0, dt = 0;
  PccParams P;
  WdConfig C;
  std::vector<double> K, F, err; // [6][3], [6][2N], [6]
  double * d_gains = nullptr;    // [N][12]
  char * d_stage = nullptr;
  int64_t cap = 0;
  hipStream_t stream = nullptr;
};

extern "C" int ccc_pcc_create(double mass, const double * moment_of_inertia, double horizon_duration, double horizon_dt,
                              const double * weight_pos, const double * weight_wrench, const double * weight_jerk,
                              const ccc_wrench_dist_config_t * cfg, int max_ridges, int device, ccc_pcc_t ** out)
{
  const char * who = "ccc_pcc_create";
  if(!out) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: out is NULL", who);
  *out = nullptr;
  if(!moment_of_inertia) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: moment_of_inertia is NULL", who);
  if(!(mass > 0) || !(horizon_duration > 0) || !(horizon_dt > 0) || !(moment_of_inertia[0] > 0) ||
     !(moment_of_inertia[1] > 0) || !(moment_of_inertia[2] > 0))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: mass, moment_of_inertia, horizon_duration and horizon_dt must be > 0", who);
  // WeightParam defaults of include/CCC/PreviewControlCentroidal.h:204-209 ([angular; linear])
  double wp[6] = {1e2, 1e2, 1e2, 2e2, 2e2, 2e2}, ww[6] = {5e-3, 5e-3, 5e-3, 5e-4, 5e-4, 5e-4},
         wj[6] = {1e-8, 1e-8, 1e-8, 1e-8, 1e-8, 1e-8};
  for(int a = 0; a < 6; a++)
  {
    if(weight_pos) wp[a] = weight_pos[a];
    if(weight_wrench) ww[a] = weight_wrench[a];
    if(weight_jerk) wj[a] = weight_jerk[a];
    if(!(wp[a] >= 0) || !(ww[a] >= 0) || !(wj[a] > 0))
      return fail(CCC_ERR_INVALID_ARGUMENT, "%s: weights must be >= 0 and the jerk weights > 0", who);
  }
  const double steps = std::ceil(horizon_duration / horizon_dt); // PreviewControl.h:71
  if(steps > CCC_PCC_MAX_STEPS)
    return fail(CCC_ERR_UNSUPPORTED, "%s: %.0f horizon steps > %d is not built into this library", who, steps,
                CCC_PCC_MAX_STEPS);
  if(int rc = check_ridges(max_ridges, who)) return rc;
  WdConfig C;
  if(int rc = make_config(cfg, C, who)) return rc;
  int rc = select_device(device);
  if(rc != CCC_OK) return rc;
  CCC_DEVICE_GUARD(device);
  ccc_pcc * h = new ccc_pcc();
  const int N = (int)steps;
  h->device = device;
  h->N = N;
  h->max_ridges = max_ridges;
  h->mass = mass;
  h->dt = horizon_dt;
  h->C = C;
  h->K.resize(18);
  h->F.resize((size_t)12 * N);
  h->err.resize(6);
  std::vector<double> perm((size_t)12 * N);
  h->P.N = N;
  h->P.mg = mass * kPccG;
  h->P.control_dt = horizon_dt;
  for(int a = 0; a < 6; a++)
  {
    const double inertia = a < 3 ? moment_of_inertia[a] : mass;
    h->P.inertia[a] = inertia;
    calc_gain(inertia, horizon_dt, N, wp[a], ww[a], wj[a], &h->K[3 * a], &h->F[(size_t)2 * N * a], &h->err[a]);
    for(int j = 0; j < 3; j++) h->P.K[a][j] = h->K[3 * a + j];
    // the reference block of an instance is [N][12] = (pos.vector(), wrench.vector()) per step
    for(int i = 0; i < N; i++)
      for(int kind = 0; kind < 2; kind++) perm[(size_t)12 * i + 6 * kind + a] = h->F[(size_t)2 * N * a + 2 * i + kind];
  }
  hipError_t e = hipMalloc(&h->d_gains, perm.size() * 8);
  if(e == hipSuccess) e = hipMemcpy(h->d_gains, perm.data(), perm.size() * 8, hipMemcpyHostToDevice);
  if(e != hipSuccess)
  {
    if(h->d_gains) (void)hipFree(h->d_gains);
    delete h;
    return fail(CCC_ERR_HIP, "%s: staging the gains failed: %s", who, hipGetErrorString(e));
  }
  *out = h;
  return CCC_OK;
}

extern "C" void ccc_pcc_destroy(ccc_pcc_t * h)
{
  if(!h) return;
  ccc_amd::DeviceGuard ccc_device_guard__(h->device);
  if(h->d_gains) (void)hipFree(h->d_gains);
  if(h->d_stage) (void)hipFree(h->d_stage);
  if(h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ccc_pcc_horizon_steps(const ccc_pcc_t * h)
{
  return h ? h->N : -1;
}

extern "C" int ccc_pcc_get_gains(const ccc_pcc_t * h, double * K, double * F, double * riccati_error)
{
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "ccc_pcc_get_gains: NULL handle");
  if(K) std::memcpy(K, h->K.data(), h->K.size() * 8);
  if(F) std::memcpy(F, h->F.data(), h->F.size() * 8);
  if(riccati_error) std::memcpy(riccati_error, h->err.data(), 48);
  return CCC_OK;
}

extern "C" int ccc_pcc_plan_batch_device(ccc_pcc_t * h, int64_t n, const double * x0, const double * ref, const int32_t * dim,
                                         const double * vertex, const double * ridge, double control_dt, double * wrench,
                                         double * planned_wrench, double * scales, int32_t * status, void * stream)
{
  const char * who = "ccc_pcc_plan_batch_device";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(n == 0) return CCC_OK;
  if(!x0 || !ref || !dim || !vertex || !ridge || !wrench) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CCC_DEVICE_GUARD(h->device);
  PccParams P = h->P;
  if(control_dt >= 0) P.control_dt = control_dt; // src/PreviewControlCentroidal.cpp:38-41
  WdBatch B{(long)n, dim, vertex, ridge, wrench, scales, status};
  const dim3 grid((unsigned)((n + 15) / 16));
  const size_t lds = (size_t)12 * h->N * 8;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch(h->max_ridges)
  {
    case 16: hipLaunchKernelGGL(pcc_plan_kernel<1>, grid, dim3(256), lds, s, B, h->C, P, h->d_gains, x0, ref, planned_wrench); break;
    case 32: hipLaunchKernelGGL(pcc_plan_kernel<2>, grid, dim3(256), lds, s, B, h->C, P, h->d_gains, x0, ref, planned_wrench); break;
    default: hipLaunchKernelGGL(pcc_plan_kernel<4>, grid, dim3(256), lds, s, B, h->C, P, h->d_gains, x0, ref, planned_wrench); break;
  }
  CCC_HIP_CHECK(hipGetLastError());
  return CCC_OK;
}

extern "C" int ccc_pcc_plan_batch(ccc_pcc_t * h, int64_t n, const double * x0, const double * ref, const int32_t * dim,
                                  const double * vertex, const double * ridge, double control_dt, double * wrench,
                                  double * planned_wrench, double * scales, int32_t * status)
{
  const char * who = "ccc_pcc_plan_batch";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(n == 0) return CCC_OK;
  if(!x0 || !ref || !dim || !vertex || !ridge || !wrench) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CCC_DEVICE_GUARD(h->device);
  const size_t M = (size_t)h->max_ridges, N = (size_t)h->N;
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t bx = (size_t)n * 18 * 8, br = (size_t)n * N * 12 * 8, bd = (size_t)n * 4, bv = (size_t)n * M * 24,
               bw = (size_t)n * 48, bs = (size_t)n * M * 8;
  const size_t ox = 0, orf = ox + up(bx), od = orf + up(br), ov = od + up(bd), ori = ov + up(bv), ow = ori + up(bv),
               op = ow + up(bw), os = op + up(bw), ost = os + up(bs), total = ost + up(bd);
  if(n > h->cap)
  {
    if(h->d_stage) (void)hipFree(h->d_stage);
    h->d_stage = nullptr;
    h->cap = 0;
    CCC_HIP_CHECK(hipMalloc(&h->d_stage, total));
    h->cap = n;
  }
  if(!h->stream) CCC_HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  char * d = h->d_stage;
  CCC_HIP_CHECK(hipMemcpyAsync(d + ox, x0, bx, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + orf, ref, br, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + od, dim, bd, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + ov, vertex, bv, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + ori, ridge, bv, hipMemcpyHostToDevice, h->stream));
  int rc = ccc_pcc_plan_batch_device(h, n, (const double *)(d + ox), (const double *)(d + orf), (const int32_t *)(d + od),
                                     (const double *)(d + ov), (const double *)(d + ori), control_dt, (double *)(d + ow),
                                     (double *)(d + op), (double *)(d + os), (int32_t *)(d + ost), h->stream);
  if(rc != CCC_OK) return rc;
  CCC_HIP_CHECK(hipMemcpyAsync(wrench, d + ow, bw, hipMemcpyDeviceToHost, h->stream));
  if(planned_wrench) CCC_HIP_CHECK(hipMemcpyAsync(planned_wrench, d + op, bw, hipMemcpyDeviceToHost, h->stream));
  if(scales) CCC_HIP_CHECK(hipMemcpyAsync(scales, d + os, bs, hipMemcpyDeviceToHost, h->stream));
  if(status) CCC_HIP_CHECK(hipMemcpyAsync(status, d + ost, bd, hipMemcpyDeviceToHost, h->stream));
  CCC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return CCC_OK;
}
