// gls_expr_device.hip -- gls_expr_eval_device: a gls_expr at n points on the device, and the device copy of an
// expression's program that every kernel with an expression in it reads (gls_expr_device.hpp has the
// interpreter).
//
// Work decomposition: one lane per point, every component of the expression in turn; the lane's variables are read
// from values[p][n_vars] when the program asks for them (PUSH_V) and the results go to out[p][n_comps]. The LDS
// stack is sized by the program: max_stack * 256 doubles, at most 32 KB at the cap of 16 entries. Every lane
// computes its own point from its own inputs: two calls on the same input are bitwise equal.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gls_native.h"
#include "gls_error.hpp"
#include "gls_expr_device.hpp"

namespace gls {
namespace expr {

namespace {

constexpr int kExprBlock = 256;  // 4 wave64 per block

struct DeviceCopy {
  FlatInstr *code = nullptr;
  int32_t *off = nullptr;
  int n_vars = 0, n_comps = 0, max_stack = 0;
};

__global__ void __launch_bounds__(kExprBlock)
    k_expr_eval(const DeviceProgram P, int64_t n_points, const double *__restrict__ values, double *__restrict__ out) {
  extern __shared__ double stack[];  // [max_stack][kExprBlock]
  const int64_t p = (int64_t)blockIdx.x * kExprBlock + threadIdx.x;
  if (p >= n_points) return;  // no barrier below
  const double *v = values + p * P.n_vars;
  for (int c = 0; c < P.n_comps; ++c)
    out[p * P.n_comps + c] =
        run(P.code, P.off[c], P.off[c + 1], stack + threadIdx.x, kExprBlock, [&](int i) { return v[i]; });
}

}  // namespace

void device_release(void *device_copy) {
  DeviceCopy *d = static_cast<DeviceCopy *>(device_copy);
  if (!d) return;
  if (d->code) (void)hipFree(d->code);
  if (d->off) (void)hipFree(d->off);
  delete d;
}

int device_program(const gls_expr *e, const char *who, DeviceProgram *out) {
  if (!e) return gls_io_set_error(GLS_EINVAL, "%s: null expression", who);
  void **slot = gls_io_expr_device_slot(e);
  if (!*slot) {
    FlatProgram F;
    gls_io_expr_flatten(e, F);
    if (F.max_stack > kDeviceMaxStack)
      return gls_io_set_error(GLS_EINVAL,
                              "%s: the expression needs an operand stack of %d entries, the device evaluator holds %d "
                              "(nest the expression less deeply)",
                              who, F.max_stack, kDeviceMaxStack);
    DeviceCopy *d = new DeviceCopy;
    d->n_vars = F.n_vars;
    d->n_comps = F.n_comps;
    d->max_stack = F.max_stack > 0 ? F.max_stack : 1;
    const size_t nb_code = F.code.size() * sizeof(FlatInstr), nb_off = F.off.size() * sizeof(int32_t);
    hipError_t rc = hipMalloc(&d->code, nb_code ? nb_code : sizeof(FlatInstr));
    if (rc == hipSuccess) rc = hipMalloc(&d->off, nb_off);
    if (rc == hipSuccess && nb_code) rc = hipMemcpy(d->code, F.code.data(), nb_code, hipMemcpyHostToDevice);
    if (rc == hipSuccess) rc = hipMemcpy(d->off, F.off.data(), nb_off, hipMemcpyHostToDevice);
    if (rc != hipSuccess) {
      device_release(d);
      return gls_io_set_error(GLS_EHIP, "%s: upload of the expression's program failed: %s", who, hipGetErrorString(rc));
    }
    *slot = d;
  }
  const DeviceCopy *d = static_cast<const DeviceCopy *>(*slot);
  out->code = d->code;
  out->off = d->off;
  out->n_vars = d->n_vars;
  out->n_comps = d->n_comps;
  out->max_stack = d->max_stack;
  return GLS_OK;
}

}  // namespace expr
}  // namespace gls

extern "C" int gls_expr_eval_device(const gls_expr *e, int64_t n_points, const double *values, double *out,
                                    void *hip_stream) {
  using namespace gls::expr;
  DeviceProgram P;
  const int rc = device_program(e, "gls_expr_eval_device", &P);
  if (rc < 0) return rc;
  if (n_points < 0 || (n_points > 0 && (!out || (!values && P.n_vars > 0))))
    return gls_io_set_error(GLS_EINVAL, "gls_expr_eval_device: bad arguments");
  if (n_points == 0 || P.n_comps == 0) return GLS_OK;
  const int64_t nb = (n_points + kExprBlock - 1) / kExprBlock;
  if (nb > 0x7fffffffLL) return gls_io_set_error(GLS_EINVAL, "gls_expr_eval_device: %lld points are too many for one launch", (long long)n_points);
  hipLaunchKernelGGL(k_expr_eval, dim3((unsigned)nb), dim3(kExprBlock), sizeof(double) * P.max_stack * kExprBlock,
                     static_cast<hipStream_t>(hip_stream), P, n_points, values, out);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return gls_io_set_error(GLS_EHIP, "gls_expr_eval_device: launch failed: %s", hipGetErrorString(le));
  return GLS_OK;
}
