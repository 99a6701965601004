// dev_buf.h -- DevBuf<T>: the one owner of a block of device memory (no kernels).
// The including file supplies hipMalloc, hipFree, hipError_t and hipSuccess: the HIP runtime in the library, counting stand-ins
// in the CPU driver (tests/dev_buf_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

template <class T>
struct DevBuf {
  T* p = nullptr;
  int64_t cap = 0;                          // elements allocated; 0 iff p == nullptr
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p; }         // kernel-argument lists and `buf + off` read as with a raw pointer
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
  }
  // the old block goes first, then exactly max(n, 1) elements; a failure leaves the buffer empty (p and cap agree)
  hipError_t alloc(int64_t n) {
    release();
    if (n < 1) n = 1;
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (size_t)n * sizeof(T));
    if (e != hipSuccess) return e;
    p = static_cast<T*>(q); cap = n;
    return hipSuccess;
  }
  // nothing while need <= cap; otherwise alloc(alloc_elems) (a site that doubles or pads says so)
  hipError_t ensure(int64_t need, int64_t alloc_elems) { return need <= cap ? hipSuccess : alloc(alloc_elems); }
  hipError_t ensure(int64_t need) { return ensure(need, need); }
};
