// step_mpc.hip -- CCC::StepMpc (/root/reference/include/CCC/StepMpc.h:163-240, src/StepMpc.cpp:26-247) batched on the
// device: the kernel of csrc/step_mpc.h (one instance per 16-lane DPP row, row-append Givens QR on the stacked
// least-squares rows, never the normal equations) and its C-ABI (include/ccc_amd.h).
#include "common.h"
#include "step_mpc.h"

#include <cmath>

namespace ccc_amd
{
namespace
{
constexpr double kStepG = 9.80665; // include/CCC/Constants.h:10

// 256 threads = four wavefronts = sixteen instances per workgroup.
__global__ __launch_bounds__(256) void step_mpc_kernel(StepParams P, long n_inst, const int * __restrict__ num_elements,
                                                       const int * __restrict__ is_single_support,
                                                       const double * __restrict__ end_time, const double * __restrict__ zmp,
                                                       const double * __restrict__ x0, const double * __restrict__ current_time,
                                                       double * __restrict__ current_zmp, double * __restrict__ next_foot_zmp,
                                                       int * __restrict__ status)
{
  const int tid = (int)threadIdx.x;
  const int lane = tid & 15;
  const long inst = (long)blockIdx.x * 16 + (tid >> 4);
  const bool present = inst < n_inst;
  const unsigned rshift = (unsigned)(tid & 48); // this row's sixteen bits of a wavefront ballot

  // ---- load and validate (every array has a fixed stride of 16 elements per instance: in bounds whatever n says)
  int n = 0, flag = 0;
  double te = 0.0, tp = 0.0, zx = 0.0, zy = 0.0, px = 0.0, py = 0.0, vx = 0.0, vy = 0.0;
  if(present)
  {
    n = num_elements[inst];
    flag = is_single_support[inst * 16 + lane];
    te = end_time[inst * 16 + lane];
    tp = lane == 0 ? current_time[inst] : end_time[inst * 16 + lane - 1];
    zx = zmp[(inst * 16 + lane) * 2];
    zy = zmp[(inst * 16 + lane) * 2 + 1];
    px = x0[inst * 4];
    py = x0[inst * 4 + 1];
    vx = x0[inst * 4 + 2];
    vy = x0[inst * 4 + 3];
  }
  const bool n_ok = n >= 1 && n <= 16;
  const bool mine = n_ok && lane < n; // this lane's element exists
  const double T = te - tp;
  const unsigned ss = (unsigned)(__ballot(mine && flag != 0) >> rshift) & 0xffffu;
  const unsigned have = (unsigned)(__ballot(mine) >> rshift) & 0xffffu;
  const unsigned bad_t = (unsigned)(__ballot(mine && !(T > 0.0)) >> rshift) & 0xffffu;
  const unsigned ds = have & ~ss;
  const bool valid = present && n_ok && bad_t == 0u && (ds & (ds >> 1)) == 0u; // no two double supports in a row

  StepRow S;
  S.lane = lane;
  S.n = valid ? n : 0;
  S.ss = valid ? ss : 0u;
  S.future_ss = (S.ss & ~1u) != 0u;
  const bool el = valid && mine;
  {
    // 1 - e and 1 - 1 / e through expm1: a first element of a few milliseconds keeps its digits
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

  // ---- the ZMP rows are diagonal: they are the initial R and d (src/StepMpc.cpp:51-64)
  double Rc[16];
#pragma unroll
  for(int k = 0; k < 16; ++k) Rc[k] = 0.0;
  const bool fixed = lane == 0 || (lane == 1 && S.n > 1 && !(S.ss & 1u));
  const double sz = fixed ? P.s_fixed : P.s_free;
#pragma unroll
  for(int k = 0; k < 16; ++k) Rc[k] = lane == k ? sz : Rc[k];
  double dx = sz * S.zx, dy = sz * S.zy;

  step_all_stages<15>(P, S, Rc, dx, dy);

  double ux = 0.0, uy = 0.0;
  step_backsub<15>(Rc, dx, dy, ux, uy, lane);

  // ---- outputs (src/StepMpc.cpp:185-199): u_0, and u of the first single-support element with index >= 1
  if(!present) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int foot = S.future_ss ? __ffs((int)(S.ss & ~1u)) - 1 : -1;
  if(lane == 0)
  {
    current_zmp[inst * 2] = valid ? ux : nan;
    current_zmp[inst * 2 + 1] = valid ? uy : nan;
    if(foot < 0)
    {
      next_foot_zmp[inst * 2] = valid ? 0.0 : nan;
      next_foot_zmp[inst * 2 + 1] = valid ? 0.0 : nan;
    }
    if(status) status[inst] = valid ? (CCC_STATUS_SOLVED | (foot >= 0 ? CCC_STEP_HAS_NEXT_FOOT : 0)) : CCC_STATUS_INFEASIBLE;
  }
  if(lane == foot)
  {
    next_foot_zmp[inst * 2] = ux;
    next_foot_zmp[inst * 2 + 1] = uy;
  }
}
} // namespace
} // namespace ccc_amd

using namespace ccc_amd;

extern "C" int ccc_step_create(double com_height, const ccc_step_weights_t * weights, int device, ccc_step_t ** out)
{
  const char * who = "ccc_step_create";
  if(!out) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: out is NULL", who);
  *out = nullptr;
  if(!(com_height > 0)) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: com_height must be > 0", who);
  const ccc_step_weights_t w = weights ? *weights : ccc_step_weights_t{1e-2, 1e0, 1e0, 0.0, 0.0, 1e1, 1e1}; // StepMpc.h:112-118
  // With a ZMP weight of zero R starts singular and the system can be rank deficient (the reference leans on column
  // pivoting there); this library refuses.
  if(!(w.free_zmp > 0) || !(w.fixed_zmp > 0))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: free_zmp and fixed_zmp must be > 0", who);
  if(!(w.double_support >= 0) || !(w.pos >= 0) || !(w.vel >= 0) || !(w.capture_point_abs >= 0) || !(w.capture_point_rel >= 0))
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: weights must be >= 0", who);
  int rc = select_device(device);
  if(rc != CCC_OK) return rc;
  ccc_step * h = new ccc_step();
  h->device = device;
  h->P.omega = std::sqrt(kStepG / com_height);
  h->P.s_free = std::sqrt(w.free_zmp);
  h->P.s_fixed = std::sqrt(w.fixed_zmp);
  h->P.s_ds = std::sqrt(w.double_support);
  h->P.s_pos = std::sqrt(w.pos);
  h->P.s_vel = std::sqrt(w.vel);
  h->P.s_cpa = std::sqrt(w.capture_point_abs);
  h->P.s_cpr = std::sqrt(w.capture_point_rel);
  *out = h;
  return CCC_OK;
}

extern "C" void ccc_step_destroy(ccc_step_t * h)
{
  if(!h) return;
  ccc_amd::DeviceGuard ccc_device_guard__(h->device);
  if(h->d_stage) (void)hipFree(h->d_stage);
  if(h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ccc_step_plan_batch_device(ccc_step_t * h, int64_t n, const int32_t * num_elements,
                                          const int32_t * is_single_support, const double * end_time, const double * zmp,
                                          const double * x0, const double * current_time, double * current_zmp,
                                          double * next_foot_zmp, int32_t * status, void * stream)
{
  const char * who = "ccc_step_plan_batch_device";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(n == 0) return CCC_OK;
  if(!num_elements || !is_single_support || !end_time || !zmp || !x0 || !current_time || !current_zmp || !next_foot_zmp)
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CCC_DEVICE_GUARD(h->device);
  const dim3 grid((unsigned)((n + 15) / 16));
  hipLaunchKernelGGL(step_mpc_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), h->P, (long)n, num_elements,
                     is_single_support, end_time, zmp, x0, current_time, current_zmp, next_foot_zmp, status);
  CCC_HIP_CHECK(hipGetLastError());
  return CCC_OK;
}

extern "C" int ccc_step_plan_batch(ccc_step_t * h, int64_t n, const int32_t * num_elements, const int32_t * is_single_support,
                                   const double * end_time, const double * zmp, const double * x0,
                                   const double * current_time, double * current_zmp, double * next_foot_zmp,
                                   int32_t * status)
{
  const char * who = "ccc_step_plan_batch";
  if(!h) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL handle", who);
  if(n < 0) return fail(CCC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", who, (long long)n);
  if(n == 0) return CCC_OK;
  if(!num_elements || !is_single_support || !end_time || !zmp || !x0 || !current_time || !current_zmp || !next_foot_zmp)
    return fail(CCC_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  CCC_DEVICE_GUARD(h->device);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t bn = (size_t)n * 4, bs = (size_t)n * 64, be = (size_t)n * 128, bz = (size_t)n * 256, bx = (size_t)n * 32,
               bt = (size_t)n * 8, bo = (size_t)n * 16;
  const size_t on = 0, os = on + up(bn), oe = os + up(bs), oz = oe + up(be), ox = oz + up(bz), ot = ox + up(bx),
               oc = ot + up(bt), of = oc + up(bo), ost = of + up(bo), total = ost + up(bn);
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
  CCC_HIP_CHECK(hipMemcpyAsync(d + on, num_elements, bn, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + os, is_single_support, bs, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + oe, end_time, be, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + oz, zmp, bz, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + ox, x0, bx, hipMemcpyHostToDevice, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(d + ot, current_time, bt, hipMemcpyHostToDevice, h->stream));
  int rc = ccc_step_plan_batch_device(h, n, (const int32_t *)(d + on), (const int32_t *)(d + os), (const double *)(d + oe),
                                      (const double *)(d + oz), (const double *)(d + ox), (const double *)(d + ot),
                                      (double *)(d + oc), (double *)(d + of), (int32_t *)(d + ost), h->stream);
  if(rc != CCC_OK) return rc;
  CCC_HIP_CHECK(hipMemcpyAsync(current_zmp, d + oc, bo, hipMemcpyDeviceToHost, h->stream));
  CCC_HIP_CHECK(hipMemcpyAsync(next_foot_zmp, d + of, bo, hipMemcpyDeviceToHost, h->stream));
  if(status) CCC_HIP_CHECK(hipMemcpyAsync(status, d + ost, bn, hipMemcpyDeviceToHost, h->stream));
  CCC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return CCC_OK;
}
