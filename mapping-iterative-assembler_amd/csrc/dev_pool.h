// dev_pool.h -- DevPool and PoolLease<T>: device temporaries of the one-off calls (pass 1, Myers, adapter trimming), no kernels.
// hipMalloc / hipFree of twenty-odd buffers per call cost more than the kernels between them, so the context keeps the blocks and a
// call borrows them: a PoolLease is a block lent for the length of a scope, given back by its destructor on every way out.
// Like dev_buf.h this includes nothing of HIP: the including file supplies hipMalloc, hipFree, hipError_t and hipSuccess (the HIP
// runtime in the library, counting stand-ins in tests/dev_pool_driver.cpp).
#pragma once
#include <memory>
#include <utility>
#include <vector>

#include "dev_buf.h"

struct DevPool {
  struct Block { DevBuf<unsigned char> buf; bool lent = false; };
  // each block on the heap: a lease holds its block BY POINTER, and growing the pool erases an entry and appends one (an index would
  // shift, an element of the vector itself would move)
  std::vector<std::unique_ptr<Block>> blocks;

  // Best fit among the idle blocks; when nothing fits, the largest idle block goes (rather than keep one that nothing fits any more)
  // and a block of exactly `bytes` is made.  nullptr and *e on a refused allocation: the pool is as usable as before.
  Block* lend(int64_t bytes, hipError_t* e) {
    *e = hipSuccess;
    Block* best = nullptr;
    for (auto& b : blocks)
      if (!b->lent && b->buf.cap >= bytes && (!best || b->buf.cap < best->buf.cap)) best = b.get();
    if (!best) {
      size_t idle = blocks.size();
      for (size_t k = 0; k < blocks.size(); k++)
        if (!blocks[k]->lent && (idle == blocks.size() || blocks[k]->buf.cap > blocks[idle]->buf.cap)) idle = k;
      if (idle < blocks.size()) blocks.erase(blocks.begin() + (ptrdiff_t)idle);
      auto fresh = std::make_unique<Block>();
      if ((*e = fresh->buf.alloc(bytes)) != hipSuccess) return nullptr;
      blocks.push_back(std::move(fresh));
      best = blocks.back().get();
    }
    best->lent = true;
    return best;
  }
};

// Move-only; reads as a T* (kernel-argument lists, `lease + off`), null while it holds nothing.  Must not outlive its pool.
template <class T>
struct PoolLease {
  T* p = nullptr;
  DevPool::Block* block = nullptr;
  PoolLease() = default;
  PoolLease(const PoolLease&) = delete;
  PoolLease& operator=(const PoolLease&) = delete;
  PoolLease(PoolLease&& o) noexcept : p(o.p), block(o.block) { o.p = nullptr; o.block = nullptr; }
  PoolLease& operator=(PoolLease&& o) noexcept {
    if (this != &o) { give_back(); p = o.p; block = o.block; o.p = nullptr; o.block = nullptr; }
    return *this;
  }
  ~PoolLease() { give_back(); }
  operator T*() const { return p; }
  void give_back() {
    if (block) block->lent = false;
    block = nullptr; p = nullptr;
  }
  // n elements (a zero request is one element); what it held before goes back first; a failure leaves the lease empty
  hipError_t take(DevPool& pool, size_t n) {
    give_back();
    hipError_t e;
    block = pool.lend((int64_t)((n ? n : 1) * sizeof(T)), &e);
    if (block) p = reinterpret_cast<T*>(block->buf.p);
    return e;
  }
};
