// preview_zmp.hip -- CCC::PreviewControlZmp (/root/reference/src/PreviewControlZmp.cpp:15-76, include/CCC/PreviewControl.h:
// 86-171) and CCC::SingularPreviewControlZmp (src/SingularPreviewControlZmp.cpp:7-88) batched on the device: the gain and
// weight tables of a handle, computed on the host in extended precision, and the C-ABI (include/ccc_amd.h) around the two
// kernels of csrc/preview_zmp.h.
#include "common.h"
#include "preview_zmp.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ccc_amd
{
namespace
{
constexpr double kPvzG = 9.80665; // include/CCC/Constants.h:10
typedef long double real;

struct Mat3
{
  real v[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  static Mat3 eye()
  {
    Mat3 r;
    r.v[0][0] = r.v[1][1] = r.v[2][2] = 1;
    return r;
  }
  Mat3 operator*(const Mat3 & b) const
  {
    Mat3 r;
    for(int i = 0; i < 3; i++)
      for(int j = 0; j < 3; j++)
        for(int k = 0; k < 3; k++) r.v[i][j] += v[i][k] * b.v[k][j];
    return r;
  }
  Mat3 plus(const Mat3 & b, real s = 1) const
  {
    Mat3 r;
    for(int i = 0; i < 3; i++)
      for(int j = 0; j < 3; j++) r.v[i][j] = v[i][j] + s * b.v[i][j];
    return r;
  }
  Mat3 t() const
  {
    Mat3 r;
    for(int i = 0; i < 3; i++)
      for(int j = 0; j < 3; j++) r.v[i][j] = v[j][i];
    return r;
  }
  real norm() const
  {
    real s = 0;
    for(auto & row : v)
      for(real x : row) s += x * x;
    return std::sqrt(s);
  }
  Mat3 inverse() const
  {
    Mat3 r;
    real det = 0;
    for(int i = 0; i < 3; i++)
      for(int j = 0; j < 3; j++) // cofactor of (j, i)
        r.v[i][j] = v[(j + 1) % 3][(i + 1) % 3] * v[(j + 2) % 3][(i + 2) % 3] - v[(j + 1) % 3][(i + 2) % 3] * v[(j + 2) % 3][(i + 1) % 3];
    for(int k = 0; k < 3; k++) det += v[0][k] * r.v[k][0];
    for(auto & row : r.v)
      for(real & x : row) x /= det;
    return r;
  }
};

// PreviewControl<3, 1, 1>::calcGain (PreviewControl.h:93-171) for ComZmpModelJerkInput(com_height) discretised at dt:
// K [3], F [N], riccati_error.  The chain of integrators is nilpotent, so the zero-order hold is a finite series.
void preview_gain(double com_height, double dt_, int N, double w_zmp, double w_jerk, double * K, double * F, double * riccati_error)
{
  const real dt = dt_, Q = w_zmp, R = w_jerk;
  Mat3 A = Mat3::eye();
  A.v[0][1] = A.v[1][2] = dt;
  A.v[0][2] = dt * dt / 2;
  const real Bv[3] = {dt * dt * dt / 6, dt * dt / 2, dt}, Cv[3] = {1, 0, -(real)com_height / (real)kPvzG};
  Mat3 G0, H0;
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
    {
      G0.v[i][j] = Bv[i] * Bv[j] / R;
      H0.v[i][j] = Cv[i] * Q * Cv[j];
    }
  const Mat3 CtQC = H0;
  Mat3 A0 = A, P = H0;
  for(int it = 0; it < 10000; it++) // the doubling iteration and its stopping rule (:121-143)
  {
    const Mat3 W = (Mat3::eye().plus(G0 * H0)).inverse();
    const Mat3 A1 = A0 * W * A0, G1 = G0.plus(A0 * W * G0 * A0.t());
    P = H0.plus(A0.t() * H0 * W * A0);
    if(P.plus(H0, -1).norm() / P.norm() < 1e-8L) break;
    A0 = A1;
    G0 = G1;
    H0 = P;
  }
  real BtP[3] = {0, 0, 0}, BtPB = 0, Kr[3] = {0, 0, 0}, AtPB[3] = {0, 0, 0};
  for(int j = 0; j < 3; j++)
    for(int i = 0; i < 3; i++) BtP[j] += Bv[i] * P.v[i][j];
  for(int j = 0; j < 3; j++) BtPB += BtP[j] * Bv[j];
  const real rinv = 1 / (R + BtPB);
  for(int j = 0; j < 3; j++)
  {
    for(int i = 0; i < 3; i++)
    {
      Kr[j] += BtP[i] * A.v[i][j];
      AtPB[j] += A.v[i][j] * BtP[i];
    }
    Kr[j] *= rinv;
    K[j] = (double)Kr[j];
  }
  Mat3 E = P.plus(A.t() * P * A, -1).plus(CtQC, -1), ABKt; // P - (A'PA + C'QC - A'PB (R + B'PB)^-1 B'PA)
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
    {
      E.v[i][j] += AtPB[i] * rinv * AtPB[j];
      ABKt.v[j][i] = A.v[i][j] - Bv[i] * Kr[j];
    }
  *riccati_error = (double)E.norm();
  Mat3 fSub = Mat3::eye();
  for(int i = 0; i < N; i++)
  {
    real f = 0;
    for(int j = 0; j < 3; j++)
    {
      real bf = 0, pc = 0; // (B' fSub)_j, (P C')_j
      for(int l = 0; l < 3; l++)
      {
        bf += Bv[l] * fSub.v[l][j];
        pc += P.v[j][l] * Cv[l];
      }
      f += bf * (i < N - 1 ? Cv[j] * Q : pc); // the last column: P C' (:165-169)
    }
    F[i] = (double)(rinv * f);
    fSub = fSub * ABKt;
  }
}

// src/SingularPreviewControlZmp.cpp:32-47: K of equation (16), and the backward recursion of :39-47 as the weights of
// ref_zmp_seq (its loop runs from size - 2 down to 1, so N = 1 folds both ends into w_0 and N = 2 has no interior)
void singular_gain(double com_height, double dt_, int N, double * K, double * w)
{
  const real dt = dt_, omega = std::sqrt((real)kPvzG / (real)com_height), od = omega * dt, rho = 1 / (1 + od);
  const real c = -omega * (2 + od) * rho * rho, end = (1 + od) / od;
  K[0] = (double)((1 + od) / dt + omega / (1 + od));
  K[1] = (double)(-(2 + od) / dt);
  K[2] = (double)(-(2 + od) / od);
  if(N == 1)
  {
    w[0] = (double)(1 / dt + c * end);
    return;
  }
  w[0] = (double)(1 / dt);
  real p = 1; // rho^(i - 1)
  for(int i = 1; i < N; i++, p *= rho) w[i] = (double)(i < N - 1 ? c * p : c * p * end);
}

template<int B>
void launch_sampled(const dim3 & grid, hipStream_t s, const PvzParams & P, long n, const double * w, const double * x0,
                    const double * ref, double control_dt, double * zmp, double * input)
{
  hipLaunchKernelGGL(pvz_sampled_kernel<B>, grid, dim3(256), 0, s, P, n, w, x0, ref, control_dt, zmp, input);
}
} // namespace
} // namespace ccc_amd

using namespace ccc_amd;

struct ccc_pvz
{
  int device = 0, max_blocks = 1;
  PvzParams P;
  std::vector<double> w;  // [N]
  double riccati_error = 0;
  double * d_tab = nullptr; // w [kPvzTab] (zero beyond N), W0 [kPvzTab], W1 [kPvzTab]
  char * d_stage = nullptr;
  size_t cap = 0;
  hipStream_t stream = nullptr;
};

extern "C" int ccc_pvz_create(int kind, double com_height, double horizon_duration, double horizon_dt, double weight_zmp,
                              double weight_com_jerk, int device, ccc_pvz_t ** out)
{
  const char * who = "ccc_pvz_create";
  if(!out) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: out is NULL", who);
  *out = nullptr;
  if(kind != CCC_PVZ_PREVIEW && kind != CCC_PVZ_SINGULAR) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: unknown kind %d", who, kind);
  if(!(com_height > 0) || !(horizon_duration > 0) || !(horizon_dt > 0))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: com_height, horizon_duration and horizon_dt must be > 0", who);
  const double steps = std::ceil(horizon_duration / horizon_dt); // PreviewControl.h:71, SingularPreviewControlZmp.h:44
  if(!(steps <= CCC_PVZ_MAX_STEPS))
    return fail(CCC_ERR_UNSUPPORTED, "%s: %.0f horizon steps > %d is not built into this library", who, steps, CCC_PVZ_MAX_STEPS);
  int rc = select_device(device);
  if(rc != CCC_OK) return rc;
  CCC_DEVICE_GUARD(device);
  const int N = (int)steps;
  ccc_pvz * h = new ccc_pvz();
  h->device = device;
  h->w.resize(N);
  PvzParams & P = h->P;
  P.N = N;
  P.kind = kind;
  P.off = kind == CCC_PVZ_PREVIEW ? 1 : 0;
  P.dt = horizon_dt;
  P.inv_dt = 1.0 / horizon_dt;
  P.off_dt = P.off * horizon_dt;
  P.c02 = -com_height / kPvzG; // src/CommonModels.cpp:16
  if(kind == CCC_PVZ_PREVIEW) // PreviewControlZmp.h:40: the defaults
    preview_gain(com_height, horizon_dt, N, weight_zmp > 0 ? weight_zmp : 1.0, weight_com_jerk > 0 ? weight_com_jerk : 1e-8, P.K,
                 h->w.data(), &h->riccati_error);
  else
    singular_gain(com_height, horizon_dt, N, P.K, h->w.data());
  // suffix sums of the double weights the sampled kernel multiplies by, accumulated from the small tail in extended
  // precision and rounded once
  std::vector<double> tab((size_t)3 * kPvzTab, 0.0);
  real s0 = 0, s1 = 0;
  for(int i = N - 1; i >= 0; i--)
  {
    tab[i] = h->w[i];
    s0 += (real)h->w[i];
    s1 += (real)i * (real)h->w[i];
    tab[kPvzTab + i] = (double)s0;
    tab[2 * kPvzTab + i] = (double)s1;
  }
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if(e == hipSuccess) h->max_blocks = prop.multiProcessorCount * 8;
  if(e == hipSuccess) e = hipMalloc(&h->d_tab, tab.size() * 8);
  if(e == hipSuccess) e = hipMemcpy(h->d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice);
  if(e != hipSuccess)
  {
    if(h->d_tab) (void)hipFree(h->d_tab);
    delete h;
    return fail(CCC_ERR_HIP, "%s: staging the tables failed: %s", who, hipGetErrorString(e));
  }
  *out = h;
  return CCC_OK;
}

extern "C" void ccc_pvz_destroy(ccc_pvz_t * h)
{
  if(!h) return;
  ccc_amd::DeviceGuard ccc_device_guard__(h->device);
  if(h->d_tab) (void)hipFree(h->d_tab);
  if(h->d_stage) (void)hipFree(h->d_stage);
  if(h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ccc_pvz_horizon_steps(const ccc_pvz_t * h)
{
  return h ? h->P.N : -1;
}

extern "C" int ccc_pvz_get_gains(const ccc_pvz_t * h, double * K, double * w, double * riccati_error)
{
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "ccc_pvz_get_gains: NULL handle");
  if(K) std::memcpy(K, h->P.K, 24);
  if(w) std::memcpy(w, h->w.data(), h->w.size() * 8);
  if(riccati_error) *riccati_error = h->riccati_error;
  return CCC_OK;
}

static dim3 pvz_grid(const ccc_pvz * h, int64_t n)
{
  const int64_t groups = (n + 15) / 16;
  return dim3((unsigned)(groups < h->max_blocks ? groups : h->max_blocks));
}

extern "C" int ccc_pvz_plan_batch_device(ccc_pvz_t * h, int64_t n, const double * x0, const double * ref, double control_dt,
                                         double * zmp, double * input, void * stream)
{
  const char * who = "ccc_pvz_plan_batch_device";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(n == 0) return CCC_OK;
  if(!x0 || !ref || !zmp) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CCC_DEVICE_GUARD(h->device);
  const dim3 grid = pvz_grid(h, n);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int chunks = (h->P.N + 31) / 32; // 32 samples per row and load
  if(chunks <= 2)
    launch_sampled<2>(grid, s, h->P, (long)n, h->d_tab, x0, ref, control_dt, zmp, input);
  else if(chunks <= 4)
    launch_sampled<4>(grid, s, h->P, (long)n, h->d_tab, x0, ref, control_dt, zmp, input);
  else if(chunks <= 8)
    launch_sampled<8>(grid, s, h->P, (long)n, h->d_tab, x0, ref, control_dt, zmp, input);
  else
    launch_sampled<16>(grid, s, h->P, (long)n, h->d_tab, x0, ref, control_dt, zmp, input);
  CCC_HIP_CHECK(hipGetLastError());
  return CCC_OK;
}

extern "C" int ccc_pvz_plan_knots_batch_device(ccc_pvz_t * h, int64_t n, const int32_t * num_knots, const double * knot_time,
                                               const double * knot_zmp, const double * x0, const double * current_time,
                                               double control_dt, double * zmp, double * input, int32_t * status, void * stream)
{
  const char * who = "ccc_pvz_plan_knots_batch_device";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(n == 0) return CCC_OK;
  if(!num_knots || !knot_time || !knot_zmp || !x0 || !current_time || !zmp)
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CCC_DEVICE_GUARD(h->device);
  hipLaunchKernelGGL(pvz_knots_kernel, pvz_grid(h, n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), h->P, (long)n,
                     h->d_tab + kPvzTab, num_knots, knot_time, knot_zmp, x0, current_time, control_dt, zmp, input, status);
  CCC_HIP_CHECK(hipGetLastError());
  return CCC_OK;
}

// The host entries: inputs staged through one device buffer of the handle (every piece on a 256-byte boundary), the
// device entry on the handle's stream, outputs copied back.
namespace
{
struct Piece
{
  const void * host_in;
  void * host_out;
  size_t bytes, offset;
};

int stage(ccc_pvz * h, Piece * pieces, int count)
{
  size_t total = 0;
  for(int i = 0; i < count; i++)
  {
    pieces[i].offset = total;
    total += (pieces[i].bytes + 255) / 256 * 256;
  }
  if(total > h->cap)
  {
    if(h->d_stage) (void)hipFree(h->d_stage);
    h->d_stage = nullptr;
    h->cap = 0;
    CCC_HIP_CHECK(hipMalloc(&h->d_stage, total));
    h->cap = total;
  }
  if(!h->stream) CCC_HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  for(int i = 0; i < count; i++)
    if(pieces[i].host_in)
      CCC_HIP_CHECK(hipMemcpyAsync(h->d_stage + pieces[i].offset, pieces[i].host_in, pieces[i].bytes, hipMemcpyHostToDevice, h->stream));
  return CCC_OK;
}

int unstage(ccc_pvz * h, const Piece * pieces, int count)
{
  for(int i = 0; i < count; i++)
    if(pieces[i].host_out)
      CCC_HIP_CHECK(hipMemcpyAsync(pieces[i].host_out, h->d_stage + pieces[i].offset, pieces[i].bytes, hipMemcpyDeviceToHost, h->stream));
  CCC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return CCC_OK;
}
} // namespace

extern "C" int ccc_pvz_plan_batch(ccc_pvz_t * h, int64_t n, const double * x0, const double * ref, double control_dt,
                                  double * zmp, double * input)
{
  const char * who = "ccc_pvz_plan_batch";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(n == 0) return CCC_OK;
  if(!x0 || !ref || !zmp) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CCC_DEVICE_GUARD(h->device);
  const size_t m = (size_t)n;
  Piece p[4] = {{x0, nullptr, m * 48, 0}, {ref, nullptr, m * 16 * h->P.N, 0}, {nullptr, zmp, m * 16, 0}, {nullptr, input, m * 16, 0}};
  if(int rc = stage(h, p, 4)) return rc;
  char * d = h->d_stage;
  if(int rc = ccc_pvz_plan_batch_device(h, n, (const double *)(d + p[0].offset), (const double *)(d + p[1].offset), control_dt,
                                        (double *)(d + p[2].offset), input ? (double *)(d + p[3].offset) : nullptr, h->stream))
    return rc;
  return unstage(h, p, 4);
}

extern "C" int ccc_pvz_plan_knots_batch(ccc_pvz_t * h, int64_t n, const int32_t * num_knots, const double * knot_time,
                                        const double * knot_zmp, const double * x0, const double * current_time,
                                        double control_dt, double * zmp, double * input, int32_t * status)
{
  const char * who = "ccc_pvz_plan_knots_batch";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(n == 0) return CCC_OK;
  if(!num_knots || !knot_time || !knot_zmp || !x0 || !current_time || !zmp)
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CCC_DEVICE_GUARD(h->device);
  const size_t m = (size_t)n;
  Piece p[8] = {{num_knots, nullptr, m * 4, 0},     {knot_time, nullptr, m * 8 * kPvzMaxKnots, 0},
                {knot_zmp, nullptr, m * 16 * kPvzMaxKnots, 0}, {x0, nullptr, m * 48, 0},
                {current_time, nullptr, m * 8, 0},  {nullptr, zmp, m * 16, 0},
                {nullptr, input, m * 16, 0},        {nullptr, status, m * 4, 0}};
  if(int rc = stage(h, p, 8)) return rc;
  char * d = h->d_stage;
  if(int rc = ccc_pvz_plan_knots_batch_device(
         h, n, (const int32_t *)(d + p[0].offset), (const double *)(d + p[1].offset), (const double *)(d + p[2].offset),
         (const double *)(d + p[3].offset), (const double *)(d + p[4].offset), control_dt, (double *)(d + p[5].offset),
         input ? (double *)(d + p[6].offset) : nullptr, status ? (int32_t *)(d + p[7].offset) : nullptr, h->stream))
    return rc;
  return unstage(h, p, 8);
}
