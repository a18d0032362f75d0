// Stand-alone check of CoarseSolve's destruction order (csrc/gls_mg_coarse.hpp) for the sanitizers, without a GPU: the
// HIP and rocBLAS calls the header makes are the host stubs below (device memory = malloc). A worker that writes the
// check's result buffer (rel) after a short sleep is still running when the struct is destroyed, and again when it is
// move-assigned from an empty one (gls_mg_detach): both must join it before any buffer is freed. Exits 0.
//   c++ -std=c++17 -g -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -fsanitize=address,undefined
//       -fno-sanitize-recover=all -o coarse_solve_lifetime tools/coarse_solve_lifetime.cpp
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../softx_2020_200_amd/csrc/gls_mg_coarse.hpp"

int gls_impl::set_err(int code, const char *fmt, ...) {
  std::fprintf(stderr, "error %d: %s\n", code, fmt);
  return code;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return (*p = std::malloc(n)) ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { return std::free(p), hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { return std::memcpy(d, s, n), hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return *s = nullptr, hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return *e = nullptr, hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
rocblas_status rocblas_destroy_handle(rocblas_handle) { return rocblas_status_success; }
}

static void start_worker(gls_impl::CoarseSolve &cs) {
  if (cs.rel.alloc(1) != GLS_OK || cs.chk32.alloc(64) != GLS_OK) std::exit(2);
  // the band route's buffers (BandLU, a member declared before Side): its panels, scratch and check result
  if (cs.blu.panels.alloc(64) != GLS_OK || cs.blu.work.alloc(64) != GLS_OK || cs.blu.rel.alloc(1) != GLS_OK) std::exit(2);
  // (the pointers as the worker's queued device work holds them)
  cs.side.worker = std::thread([chk = cs.chk32.p, n = cs.chk32.n, rel = cs.rel.p, pan = cs.blu.panels.p, wrk = cs.blu.work.p,
                                brel = cs.blu.rel.p]() {
    std::this_thread::sleep_for(std::chrono::milliseconds(200));
    for (size_t i = 0; i < n; ++i) chk[i] = 1.0, pan[i] = 1.f, wrk[i] = 1.0;
    *rel = *brel = 64.0;  // what rocblas_dnrm2 writes in device pointer mode
  });
}

int main() {
  {
    gls_impl::CoarseSolve cs;
    start_worker(cs);
  }  // destroyed with the worker in flight
  gls_impl::CoarseSolve cs;
  start_worker(cs);
  cs = gls_impl::CoarseSolve();  // detached with the worker in flight
  std::printf("coarse_solve_lifetime: ok\n");
  return 0;
}
