// CPU driver of csrc/dev_pool.h: hipMalloc / hipFree are counting stand-ins over malloc / free (an address or leak sanitizer sees every
// block), the nth hipMalloc can be told to fail.  `dev_pool_driver <case>` runs one case and exits 0 iff every check of it held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
struct Event { char kind; void* p; size_t bytes; };      // 'm' malloc, 'x' refused malloc, 'f' free
static std::vector<Event> g_log;
static int g_mallocs = 0, g_frees = 0, g_calls = 0, g_fail_at = 0;      // g_fail_at: the 1-based hipMalloc call that is refused (0: none)
static hipError_t hipMalloc(void** p, size_t bytes) {
  if (++g_calls == g_fail_at) { g_log.push_back({'x', nullptr, bytes}); *p = nullptr; return hipErrorOutOfMemory; }
  *p = malloc(bytes);
  g_log.push_back({'m', *p, bytes});
  g_mallocs++;
  return hipSuccess;
}
static hipError_t hipFree(void* p) {
  g_log.push_back({'f', p, 0});
  g_frees++;
  free(p);
  return hipSuccess;
}

#include "../mapping-iterative-assembler_amd/csrc/dev_pool.h"

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); g_bad++; } } while (0)
static std::string kinds() { std::string s; for (auto& e : g_log) s += e.kind; return s; }
static int idle_blocks(const DevPool& pool) { int k = 0; for (auto& b : pool.blocks) k += !b->lent; return k; }

// three idle blocks of 100, 400 and 200 bytes (made in that order)
static void three_blocks(DevPool& pool, void** b100, void** b400, void** b200) {
  PoolLease<char> a, b, c;
  CHECK(a.take(pool, 100) == hipSuccess && b.take(pool, 400) == hipSuccess && c.take(pool, 200) == hipSuccess);
  *b100 = a.p; *b400 = b.p; *b200 = c.p;
}

// best fit: the smallest idle block that holds the request, and no malloc
static void case_best_fit(DevPool& pool) {
  void *b100, *b400, *b200;
  three_blocks(pool, &b100, &b400, &b200);
  CHECK(g_mallocs == 3 && idle_blocks(pool) == 3);
  PoolLease<char> x;
  CHECK(x.take(pool, 150) == hipSuccess && x.p == b200);
  PoolLease<int32_t> y;                                           // (sizes are in elements: 50 words are 200 bytes, the 200-byte block is lent)
  CHECK(y.take(pool, 50) == hipSuccess && (void*)y.p == b400);
  PoolLease<char> z;
  CHECK(z.take(pool, 100) == hipSuccess && z.p == b100);           // an exact fit is a fit
  PoolLease<char> zero;
  CHECK(g_mallocs == 3);
  CHECK(zero.take(pool, 0) == hipSuccess && zero.p != nullptr && g_mallocs == 4 && g_log.back().bytes == 1);      // a zero request is one element
  zero.p[0] = 1;                                                  // (the sanitizer watches)
}

// a request nothing fits frees the largest idle block first and allocates exactly the request
static void case_grow(DevPool& pool) {
  void *b100, *b400, *b200;
  three_blocks(pool, &b100, &b400, &b200);
  PoolLease<char> held;
  CHECK(held.take(pool, 300) == hipSuccess && held.p == b400);      // the largest block is lent: the largest IDLE one is the 200-byte block
  PoolLease<int16_t> big;
  CHECK(big.take(pool, 250) == hipSuccess);
  CHECK(kinds() == "mmmfm" && g_log[3].p == b200 && g_log[4].bytes == 500 && pool.blocks.size() == 3);
  PoolLease<char> small;
  CHECK(small.take(pool, 10) == hipSuccess && small.p == b100 && g_mallocs == 4);
  PoolLease<char> none_idle;                                      // nothing idle: nothing freed, one more block
  CHECK(none_idle.take(pool, 10) == hipSuccess && kinds() == "mmmfmm" && g_log.back().bytes == 10 && pool.blocks.size() == 4);
}

static hipError_t nest_with_early_return(DevPool& pool, void** outer, void** inner) {
  PoolLease<char> a;
  if (a.take(pool, 64) != hipSuccess) return hipErrorOutOfMemory;
  *outer = a.p;
  {
    PoolLease<char> b;
    if (b.take(pool, 32) != hipSuccess) return hipErrorOutOfMemory;
    *inner = b.p;
    PoolLease<char> c;
    g_fail_at = g_calls + 1;
    if (c.take(pool, 4096) != hipSuccess) return hipErrorOutOfMemory;      // out of a nest of leases
  }
  return hipSuccess;
}

// a lease that goes out of scope makes its block idle again: the next equal request gets the same block and no malloc
static void case_scope(DevPool& pool) {
  void* first = nullptr;
  {
    PoolLease<int32_t> a;
    CHECK(a.take(pool, 25) == hipSuccess && a.block && a.block->lent);
    first = a.p;
  }
  CHECK(idle_blocks(pool) == 1 && g_mallocs == 1);
  {
    PoolLease<int32_t> a;
    CHECK(a.take(pool, 25) == hipSuccess && (void*)a.p == first && g_mallocs == 1);
    CHECK(a.take(pool, 25) == hipSuccess && (void*)a.p == first && g_mallocs == 1);      // taking again gives back first
    a.give_back();
    CHECK(a.p == nullptr && static_cast<int32_t*>(a) == nullptr && idle_blocks(pool) == 1);
  }
  void *outer = nullptr, *inner = nullptr;
  CHECK(nest_with_early_return(pool, &outer, &inner) == hipErrorOutOfMemory);
  CHECK(idle_blocks(pool) == (int)pool.blocks.size());             // every lease of the nest gave its block back
  PoolLease<char> a, b;
  const int before = g_mallocs;
  CHECK(a.take(pool, 64) == hipSuccess && b.take(pool, 32) == hipSuccess && g_mallocs == before && a.p == outer && b.p == inner);
}

// two live leases never share a block
static void case_distinct(DevPool& pool) {
  std::vector<PoolLease<char>> v(12);
  for (size_t k = 0; k < v.size(); k++) CHECK(v[k].take(pool, 16 + 8 * (k % 3)) == hipSuccess);
  for (size_t k = 0; k < v.size(); k += 2) v[k].give_back();
  for (size_t k = 0; k < v.size(); k += 2) CHECK(v[k].take(pool, 16 + 8 * (k % 3)) == hipSuccess);
  for (size_t i = 0; i < v.size(); i++)
    for (size_t j = i + 1; j < v.size(); j++) CHECK(v[i].p != v[j].p && v[i].block != v[j].block);
  CHECK(g_mallocs == 12 && idle_blocks(pool) == 0);
  for (auto& l : v) memset(l.p, 0x5a, 16);                        // (the sanitizer watches)
}

// a refused allocation leaves the lease empty and the pool usable
static void case_refused(DevPool& pool) {
  PoolLease<char> keep;
  CHECK(keep.take(pool, 50) == hipSuccess);
  { PoolLease<char> t; CHECK(t.take(pool, 80) == hipSuccess); }
  PoolLease<char> a;
  CHECK(a.take(pool, 60) == hipSuccess && g_mallocs == 2);         // (holds the 80-byte block when the next request arrives)
  g_fail_at = g_calls + 1;
  CHECK(a.take(pool, 1000) == hipErrorOutOfMemory);                // its own block went back first, was the largest idle one and is freed
  CHECK(a.p == nullptr && a.block == nullptr && kinds() == "mmfx" && pool.blocks.size() == 1 && keep.block->lent);
  CHECK(a.take(pool, 70) == hipSuccess && a.p != nullptr && kinds() == "mmfxm" && pool.blocks.size() == 2);
  PoolLease<char> first;                                          // ... and a refusal in an empty pool
  DevPool other;
  g_fail_at = g_calls + 1;
  CHECK(first.take(other, 8) == hipErrorOutOfMemory && first.p == nullptr && other.blocks.empty());
  CHECK(first.take(other, 8) == hipSuccess && other.blocks.size() == 1);
  first.give_back();
}

// a moved-from lease gives nothing back, the target gives back once
static void case_move(DevPool& pool) {
  PoolLease<int32_t> a;
  CHECK(a.take(pool, 10) == hipSuccess);
  DevPool::Block* blk = a.block;
  {
    PoolLease<int32_t> b(std::move(a));
    CHECK(a.p == nullptr && a.block == nullptr && b.block == blk && blk->lent);
    a.give_back();                                                // nothing to give
    CHECK(blk->lent);
    { PoolLease<int32_t> gone(std::move(a)); }                     // ... nor does a lease made of an empty one
    CHECK(blk->lent);
    PoolLease<int32_t> c;
    CHECK(c.take(pool, 10) == hipSuccess && c.block != blk);
    DevPool::Block* cblk = c.block;
    c = std::move(b);                                             // the target's own block goes back, the source is left empty
    CHECK(!cblk->lent && blk->lent && c.block == blk && b.block == nullptr && b.p == nullptr);
    std::vector<PoolLease<int32_t>> v;                            // (a vector that grows moves its elements)
    v.push_back(std::move(c));
    for (int k = 0; k < 8; k++) v.emplace_back();
    CHECK(blk->lent && v[0].block == blk);
  }
  CHECK(!blk->lent && idle_blocks(pool) == 2 && g_mallocs == 2 && g_frees == 0);
}

// a lease taken before the pool grows still returns its own block: erasing an entry shifts the others, appending may move the vector
static void case_by_pointer(DevPool& pool) {
  void* mine = nullptr;
  DevPool::Block* blk = nullptr;
  {
    PoolLease<char> t, a;
    CHECK(t.take(pool, 1000) == hipSuccess);                       // blocks[0]: the one growth will erase
    CHECK(a.take(pool, 2000) == hipSuccess && pool.blocks.size() == 2 && pool.blocks[1].get() == a.block);
    t.give_back();
    mine = a.p; blk = a.block;
    std::vector<PoolLease<char>> more(40);
    for (size_t k = 0; k < more.size(); k++) CHECK(more[k].take(pool, 3000 + k) == hipSuccess);      // the first erases blocks[0], the rest append
    CHECK(g_frees == 1 && pool.blocks.size() == 41 && pool.blocks[0].get() == blk && a.p == mine && blk->lent);
    a.p[1999] = 1;
    more.clear();
    CHECK(idle_blocks(pool) == 40 && blk->lent);
  }
  CHECK(!blk->lent && idle_blocks(pool) == 41);
  PoolLease<char> again;
  CHECK(again.take(pool, 2000) == hipSuccess && again.p == mine);
}

int main(int argc, char** argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  {
    DevPool pool;
    if (which == "best_fit") case_best_fit(pool);
    else if (which == "grow") case_grow(pool);
    else if (which == "scope") case_scope(pool);
    else if (which == "distinct") case_distinct(pool);
    else if (which == "refused") case_refused(pool);
    else if (which == "move") case_move(pool);
    else if (which == "by_pointer") case_by_pointer(pool);
    else { fprintf(stderr, "usage: dev_pool_driver best_fit|grow|scope|distinct|refused|move|by_pointer\n"); return 2; }
    CHECK(idle_blocks(pool) == (int)pool.blocks.size());           // every lease of the case is gone
  }
  // ... and so is the pool: frees equal successful mallocs, and no block was freed twice or not at all
  CHECK(g_frees == g_mallocs);
  std::vector<void*> live;
  for (auto& e : g_log) {
    if (e.kind == 'm') live.push_back(e.p);
    if (e.kind == 'f') { size_t k = 0; while (k < live.size() && live[k] != e.p) k++; CHECK(k < live.size()); if (k < live.size()) live.erase(live.begin() + k); }
  }
  CHECK(live.empty());
  printf("%s: %d mallocs, %d frees, %d failed checks\n", which.c_str(), g_mallocs, g_frees, g_bad);
  return g_bad ? 1 : 0;
}
