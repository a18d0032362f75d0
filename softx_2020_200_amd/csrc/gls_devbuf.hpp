// gls_devbuf.hpp -- internal: the owning device buffer and the error macros of the library's host side, for the
// headers that hold device buffers without seeing the context struct (gls_ctx.hpp, gls_mg_coarse.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/gls_native.h"

namespace gls_impl {
// sets the thread-local last-error string (gls_last_error) and returns code (gls_api.cpp)
int set_err(int code, const char *fmt, ...);
}  // namespace gls_impl

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return ::gls_impl::set_err(GLS_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define GLS_TRY(expr)          \
  do {                         \
    int r_ = (expr);           \
    if (r_ < 0) return r_;     \
  } while (0)

namespace gls_impl {

template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  int alloc(size_t count) {
    release();
    if (count == 0) return GLS_OK;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) {
      p = nullptr;
      return set_err(GLS_ENOMEM, "hipMalloc of %zu bytes failed", count * sizeof(T));
    }
    n = count;
    return GLS_OK;
  }
  int upload(const T *h, size_t count) {
    GLS_TRY(alloc(count));
    if (count && hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      return set_err(GLS_EHIP, "upload failed");
    return GLS_OK;
  }
};

}  // namespace gls_impl
