// CPU driver of csrc/dev_buf.h: hipMalloc / hipFree are counting stand-ins over malloc / free (an address or leak sanitizer sees every
// block), the nth hipMalloc can be told to fail.  `dev_buf_driver <case>` runs one case and exits 0 iff every check of it held.
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

#include "../mapping-iterative-assembler_amd/csrc/dev_buf.h"

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); g_bad++; } } while (0)
static std::string kinds() { std::string s; for (auto& e : g_log) s += e.kind; return s; }

// ensure does nothing while need <= cap, and allocates exactly alloc_elems otherwise
static void case_ensure() {
  DevBuf<int32_t> b;
  CHECK(b.p == nullptr && b.cap == 0 && static_cast<int32_t*>(b) == nullptr);
  CHECK(b.ensure(0, 0) == hipSuccess && b.p == nullptr && g_log.empty());      // nothing wanted of an empty buffer: nothing made
  CHECK(b.ensure(100, 200) == hipSuccess && b.cap == 200 && g_log.size() == 1 && g_log[0].bytes == 200 * sizeof(int32_t));
  int32_t* first = b;
  for (int64_t need : {0, 1, 100, 199, 200}) CHECK(b.ensure(need, need * 2) == hipSuccess && b.p == first && b.cap == 200);
  CHECK(g_log.size() == 1);
  CHECK(b.ensure(201, 201 + 64) == hipSuccess && b.cap == 265 && g_log.back().bytes == 265 * sizeof(int32_t));      // a padded site
  CHECK(b.ensure(300) == hipSuccess && b.cap == 300 && g_log.back().bytes == 300 * sizeof(int32_t));                // an exact one
  CHECK(b + 3 == b.p + 3 && &b[5] == b.p + 5);      // reads as a pointer
  DevBuf<uint64_t> w;
  CHECK(w.ensure(7, 7) == hipSuccess && g_log.back().bytes == 56);
}

// the old block is freed before the new one is requested (as dev_alloc did)
static void case_order() {
  DevBuf<char> b;
  CHECK(b.alloc(10) == hipSuccess);
  void* old = b.p;
  CHECK(b.alloc(20) == hipSuccess);
  CHECK(kinds() == "mfm" && g_log[1].p == old && g_log[2].bytes == 20 && b.cap == 20);
  CHECK(b.ensure(21, 42) == hipSuccess && kinds() == "mfmfm" && g_log[3].p == g_log[2].p);
}

// a refused allocation leaves p == nullptr AND cap == 0: the next, smaller request allocates again
static void case_failure() {
  DevBuf<int16_t> b;
  CHECK(b.ensure(1000, 2000) == hipSuccess && b.cap == 2000);
  g_fail_at = g_calls + 1;
  CHECK(b.ensure(5000, 5000) == hipErrorOutOfMemory);
  CHECK(b.p == nullptr && b.cap == 0 && kinds() == "mfx");      // (the old block went first, as in the parent)
  CHECK(b.ensure(10, 10) == hipSuccess && b.p != nullptr && b.cap == 10 && kinds() == "mfxm");
  DevBuf<int16_t> c;                                            // ... and a first allocation that is refused
  g_fail_at = g_calls + 1;
  CHECK(c.alloc(4) == hipErrorOutOfMemory && c.p == nullptr && c.cap == 0);
  CHECK(c.ensure(1, 1) == hipSuccess && c.cap == 1);
}

// move leaves the source empty; destructor and release free exactly once
static void case_move() {
  void* blk = nullptr;
  {
    DevBuf<int32_t> a;
    CHECK(a.alloc(8) == hipSuccess);
    blk = a.p;
    DevBuf<int32_t> b(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0 && b.p == blk && b.cap == 8 && g_frees == 0);
    DevBuf<int32_t> c;
    CHECK(c.alloc(3) == hipSuccess);
    void* cblk = c.p;
    c = std::move(b);                                            // the target's own block goes, the source is left empty
    CHECK(g_frees == 1 && g_log.back().kind == 'f' && g_log.back().p == cblk && c.p == blk && c.cap == 8 && b.p == nullptr && b.cap == 0);
    std::vector<DevBuf<int32_t>> v;                              // (owned_links: a vector that grows moves its elements)
    v.push_back(std::move(c));
    for (int k = 0; k < 8; k++) { DevBuf<int32_t> d; CHECK(d.alloc(1) == hipSuccess); v.push_back(std::move(d)); }
    CHECK(g_frees == 1 && v[0].p == blk);
    v[0].release();
    CHECK(g_frees == 2 && v[0].p == nullptr && v[0].cap == 0);
    v[0].release();                                              // an empty buffer has nothing to free
    CHECK(g_frees == 2);
  }
  CHECK(g_frees == 10 && g_mallocs == 10);
  int of_blk = 0;
  for (auto& e : g_log) of_blk += e.kind == 'f' && e.p == blk;
  CHECK(of_blk == 1);
}

// alloc(0) yields a valid one-element block, as dev_alloc does
static void case_zero() {
  DevBuf<int64_t> b;
  CHECK(b.alloc(0) == hipSuccess && b.p != nullptr && b.cap == 1 && g_log.back().bytes == sizeof(int64_t));
  b.p[0] = 7;                                                    // (the sanitizer watches)
  CHECK(b.ensure(1, 1) == hipSuccess && g_log.size() == 1);
}

int main(int argc, char** argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  if (which == "ensure") case_ensure();
  else if (which == "order") case_order();
  else if (which == "failure") case_failure();
  else if (which == "move") case_move();
  else if (which == "zero") case_zero();
  else { fprintf(stderr, "usage: dev_buf_driver ensure|order|failure|move|zero\n"); return 2; }
  // every buffer of the case is gone: frees equal successful mallocs, and no block was freed twice or not at all
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
