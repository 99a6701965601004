// Driver of tests/test_align_route_cpu.py over csrc/align_route.h (plain C++17, no HIP).  stdin: "axes K", K lines "<field> v1 v2 ...",
// "cfgs M <field> <field> ...", M lines of values for those fields.  For every cfg line (outermost) and every point of the axes' product
// (first axis slowest) two 64-bit words go to stdout: the route packed field by field (FIELDS below, in that order, lowest bits first),
// and the grids of the full plan's first and last launch.
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/align_route.h"

using namespace mia;

#define IN_FIELDS(X) X(n) X(max_len) X(wrap) X(L) X(plane_words) X(kh_entries) X(flat) X(ref_mostly_bases) X(ref_few_n) X(bx_ok) X(explicit_win) \
  X(deferred) X(pend_encode) X(own_umax) X(rejects) X(use_filter) X(use_banddp) X(use_bx) X(use_lanes) X(use_fine) X(use_quick) X(bx_serial) \
  X(plan_split) X(use_direct_open) X(no_prep_fuse) X(ext_events) X(dbg) X(bx_dbg)
// (name, bits): tests/test_align_route_cpu.py carries the same list
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

static void emit(const AlignRouteIn& in) {
  const AlignRoute r = align_route(in);
  unsigned long long w[2] = {0, 0};
  int at = 0;
#define X(f, bits) { const unsigned long long v = (unsigned long long)r.f; if (v >> bits) { fprintf(stderr, #f " does not fit its field\n"); exit(3); } w[0] |= v << at; at += bits; }
  FIELDS(X)
#undef X
  if (at > 64 || r.plane_words != in.plane_words) exit(4);
  w[1] = (unsigned long long)align_route_plan_grid(r, r.full_first, in.n) | ((unsigned long long)align_route_plan_grid(r, r.full_last, in.n) << 32);
  fwrite(w, 8, 2, stdout);
}

struct Axis { std::string name; std::vector<long long> v; };

static void product(const std::vector<Axis>& axes, size_t k, AlignRouteIn& in) {
  if (k == axes.size()) { emit(in); return; }
  for (long long v : axes[k].v) { set_field(in, axes[k].name, v); product(axes, k + 1, in); }
}

int main() {
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
