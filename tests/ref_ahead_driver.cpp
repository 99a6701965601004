// Driver of tests/test_ref_ahead_cpu.py over csrc/ref_ahead.h and the ref_ready input of csrc/align_route.h (plain C++17, no HIP).
//   ref_ahead_driver hit     stdin: lines "<built key: 9 numbers> <wanted key: 9 numbers> <kept string> <new string>", the key's fields in
//                            the order of KEY_FIELDS.  The new call's length and circular flag are the wanted key's.  Per line, to stdout:
//                            "<same_string> <hit>".
//   ref_ahead_driver route   stdin as tests/align_route_driver.cpp takes it.  For every point five 64-bit words: the route with
//                            ref_ready = false packed as that driver packs it, its two plan grids, the same two words with
//                            ref_ready = true, and prep_none of the two (bit 0: without, bit 1: with).
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/align_route.h"
#include "../mapping-iterative-assembler_amd/csrc/ref_ahead.h"

using namespace mia;

#define KEY_FIELDS(X) X(L) X(circular) X(n_other) X(kh_entries) X(kslots) X(kwild) X(plane_words) X(nib_words) X(bits)

static bool read_key(std::istream& s, RefAheadKey& k) {
  long long v;
#define X(f) if (!(s >> v)) return false; k.f = (decltype(k.f))v;
  KEY_FIELDS(X)
#undef X
  return true;
}

static int run_hit() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream s(line);
    RefAheadKey built, want;
    std::string kept, fresh;
    if (!read_key(s, built) || !read_key(s, want) || !(s >> kept >> fresh)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
    // (the context keeps built.L characters; a wanted length beyond the new string would read past it)
    if ((long long)kept.size() < built.L || (long long)fresh.size() < want.L) { fprintf(stderr, "string shorter than its key says\n"); return 2; }
    const bool same = ref_ahead_same_string(built, kept.data(), fresh.data(), want.L, want.circular);
    printf("%d %d\n", same ? 1 : 0, ref_ahead_hit(built, want, kept.data(), fresh.data()) ? 1 : 0);
  }
  return 0;
}

#define IN_FIELDS(X) X(n) X(max_len) X(wrap) X(L) X(plane_words) X(kh_entries) X(flat) X(ref_mostly_bases) X(ref_few_n) X(bx_ok) X(explicit_win) \
  X(deferred) X(pend_encode) X(own_umax) X(rejects) X(use_filter) X(use_banddp) X(use_bx) X(use_lanes) X(use_fine) X(use_quick) X(bx_serial) \
  X(plan_split) X(use_direct_open) X(no_prep_fuse) X(ext_events) X(dbg) X(bx_dbg)
// (name, bits): tests/align_route_driver.cpp's list, in its order
#define FIELDS(X) X(nwords, 3) X(bx, 1) X(run_filter, 1) X(fused_prep, 1) X(filtered, 1) X(kocc, 1) X(banded, 1) X(want_bits, 1) X(new_flow, 1) X(split, 1) \
  X(fork_by_launch, 1) X(fine, 1) X(many_rejects, 1) X(planner_head_first, 1) X(direct_open, 1) X(maxw, 7) X(quick, 1) X(quick_lds, 1) X(one_launch, 1) \
  X(fork_at_quick, 1) X(qch, 4) X(quick_phase, 3) X(full_first, 3) X(full_last, 3) X(grid_cap, 9) X(three_streams, 1) X(two_streams, 1) X(values_aside, 1) \
  X(trace_signals, 1) X(planner_aside, 1) X(use_plain, 1) X(plan_count_late, 1)

static void set_field(AlignRouteIn& in, const std::string& name, long long v) {
#define X(f) if (name == #f) { in.f = (decltype(in.f))v; return; }
  IN_FIELDS(X)
#undef X
  fprintf(stderr, "unknown input field %s\n", name.c_str());
  exit(2);
}

static bool pack(const AlignRouteIn& in, unsigned long long* w) {
  const AlignRoute r = align_route(in);
  int at = 0;
  w[0] = 0;
#define X(f, bits) { const unsigned long long v = (unsigned long long)r.f; if (v >> bits) { fprintf(stderr, #f " does not fit its field\n"); exit(3); } w[0] |= v << at; at += bits; }
  FIELDS(X)
#undef X
  if (at > 64 || r.plane_words != in.plane_words) exit(4);
  w[1] = (unsigned long long)align_route_plan_grid(r, r.full_first, in.n) | ((unsigned long long)align_route_plan_grid(r, r.full_last, in.n) << 32);
  return r.prep_none;
}

static void emit(AlignRouteIn in) {
  unsigned long long w[5];
  in.ref_ready = false;
  const bool none_off = pack(in, w);
  in.ref_ready = true;
  const bool none_on = pack(in, w + 2);
  w[4] = (none_off ? 1ull : 0ull) | (none_on ? 2ull : 0ull);
  fwrite(w, 8, 5, stdout);
}

struct Axis { std::string name; std::vector<long long> v; };

static void product(const std::vector<Axis>& axes, size_t k, AlignRouteIn& in) {
  if (k == axes.size()) { emit(in); return; }
  for (long long v : axes[k].v) { set_field(in, axes[k].name, v); product(axes, k + 1, in); }
}

static int run_route() {
  std::string line, word;
  int K = 0, M = 0;
  std::vector<Axis> axes;
  std::getline(std::cin, line);
  { std::istringstream s(line); s >> word >> K; }
  for (int k = 0; k < K; k++) {
    std::getline(std::cin, line);
    std::istringstream s(line);
    Axis a; long long v;
    s >> a.name;
    while (s >> v) a.v.push_back(v);
    axes.push_back(a);
  }
  std::getline(std::cin, line);
  std::vector<std::string> names;
  { std::istringstream s(line); s >> word >> M; while (s >> word) names.push_back(word); }
  for (int m = 0; m < M; m++) {
    std::getline(std::cin, line);
    std::istringstream s(line);
    AlignRouteIn in;
    for (const std::string& nm : names) { long long v; s >> v; set_field(in, nm, v); }
    product(axes, 0, in);
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "hit") return run_hit();
  if (mode == "route") return run_route();
  fprintf(stderr, "usage: ref_ahead_driver hit | route\n");
  return 2;
}
