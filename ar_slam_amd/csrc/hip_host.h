// hip_host.h -- the host side's HIP plumbing, shared by everything behind the
// C-ABIs (the LM handle, the localizer, the component entry points): a HIP
// error as an ApiError, an owned device buffer, a scope guard.
#pragma once
#include <hip/hip_runtime.h>

#include "api_error.h"

#include <string>
#include <utility>

#define HIP_CHECK(expr)                                                                      \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      throw arslam::ApiError(_e == hipErrorOutOfMemory ? ARSLAM_E_OUT_OF_MEMORY : ARSLAM_E_HIP, \
                             std::string(#expr) + ": " + hipGetErrorString(_e));             \
  } while (0)

namespace arslam {

// Device buffer; grow-only, so reloading a problem of the same or a smaller
// size (every optimize() of an incremental solve) does no hipMalloc/hipFree.
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0, cap = 0;
  void alloc(size_t count) {   // grows by half again (a growing incremental problem reallocates rarely)
    n = count;
    if (count <= cap) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = cap == 0 && count <= 16 ? count : count + count / 2;
    HIP_CHECK(hipMalloc(&p, want * sizeof(T)));
    cap = want;
  }
  void upload(const T *h, size_t count, hipStream_t s) {
    if (count) HIP_CHECK(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = cap = 0;
  }
  ~DevBuf() { release(); }
};

// runs f when the scope ends, however it ends (a stream to destroy, a plan to free)
template <class F>
struct ScopeExit {
  F f;
  explicit ScopeExit(F g) : f(std::move(g)) {}
  ScopeExit(const ScopeExit &) = delete;
  ScopeExit &operator=(const ScopeExit &) = delete;
  ~ScopeExit() { f(); }
};

}  // namespace arslam
