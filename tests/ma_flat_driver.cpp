// ma_flat_driver.cpp -- the shared walk over the flat columns (csrc/ma_flat_body.h) on the host, against a plain loop.
// A program of its own (tests/test_ma_flat_cpu.py compiles it with -fsanitize=address,undefined and runs it): ma_flat_stretch, in both
// EVERY_POSITION forms, over every stretch of hand-made geometries -- and over one stretch behind the last --, compared with a loop
// record by record and column by column that shares nothing with the walk.  Every array is a heap block of exactly its size, so the
// sanitizer sees every index; the reference is a null pointer, which the walk must never read.
// Prints one line per geometry and selection, "name use stretches columns leaves whole beyond", and "ok" at the end; the first
// disagreement is reported on stderr and ends the program with status 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_flat_body.h"
#include "ma_driver_util.h"

using namespace mia;

namespace {

// one call of either callable: kind 'C' (column) or 'L' (leave)
struct Event {
  char kind;
  int64_t r, col, p;
  bool rc, used, whole;
  char seq_ch, smp_ch;
  bool operator==(const Event& o) const {
    return kind == o.kind && r == o.r && col == o.col && p == o.p && rc == o.rc && used == o.used && whole == o.whole && seq_ch == o.seq_ch && smp_ch == o.smp_ch;
  }
};

struct Geometry {
  const char* name;
  int32_t L;
  std::vector<int64_t> lens;               // columns of every record
  std::vector<int32_t> starts;
  // worked out by hand: leave calls over all stretches, those with `whole`, and columns with p >= L
  long long leaves, whole, beyond;
};

const int32_t BIG = 1000;
std::vector<int32_t> ramp(size_t n) { std::vector<int32_t> s(n); for (size_t r = 0; r < n; r++) s[r] = (int32_t)(7 * r + 1); return s; }

const std::vector<Geometry>& geometries() {
  static const std::vector<Geometry> g = {
      {"empty", BIG, {}, {}, 0, 0, 0},
      {"one_column", BIG, {1}, ramp(1), 1, 1, 0},
      {"T15", BIG, {15}, ramp(1), 1, 1, 0},
      {"T16", BIG, {16}, ramp(1), 1, 1, 0},
      {"T17", BIG, {17}, ramp(1), 2, 0, 0},                                      // the record spans two stretches
      {"seam_on_16", BIG, {16, 5}, ramp(2), 2, 2, 0},
      {"seam_on_16_inside", BIG, {10, 6, 20}, ramp(3), 4, 2, 0},                 // records 0 and 1 whole; record 2 in stretches 1 and 2
      {"sixteen_ones", BIG, std::vector<int64_t>(16, 1), ramp(16), 16, 16, 0},
      {"empty_records", BIG, {0, 0, 3, 0, 0, 4, 0}, ramp(7), 2, 2, 0},           // in front, between two others, at the very end
      {"empty_records_on_16", BIG, {16, 0, 0, 5, 0}, ramp(5), 2, 2, 0},          // stretch 1 begins with record 3, not 1 or 2
      {"three_stretches", BIG, {5, 30, 4}, ramp(3), 5, 2, 0},                    // record 1: columns 5 .. 34, whole in none
      {"exactly_one_stretch", BIG, {16, 16, 16}, ramp(3), 3, 3, 0},
      {"beyond_L", 40, {6, 4}, {0, 37}, 2, 2, 1},                                // record 1: p = 37 .. 40, the last one is L
  };
  return g;
}

int64_t padded(int64_t T) { return (T + MA_FLAT_LANE - 1) / MA_FLAT_LANE * MA_FLAT_LANE; }

[[noreturn]] void fail(const Geometry& g, int use_kind, int64_t base, const char* what) {
  fprintf(stderr, "ma_flat_driver: %s (use %d), stretch at %lld: %s\n", g.name, use_kind, (long long)base, what);
  exit(1);
}

// use_kind 0: a null pointer; 1: an array with zeros (every record r with r % 3 == 1 is left out)
void run(const Geometry& g, int use_kind) {
  const int64_t n = (int64_t)g.lens.size();
  Exact<int64_t> col_off((size_t)n + 1);
  for (int64_t r = 0; r < n; r++) col_off.p[r + 1] = col_off.p[r] + g.lens[(size_t)r];
  const int64_t T = col_off.p[n];
  Exact<int32_t> start((size_t)n);
  Exact<uint8_t> revcom((size_t)n), use(use_kind ? (size_t)n : 0);
  for (int64_t r = 0; r < n; r++) {
    start.p[r] = g.starts[(size_t)r];
    revcom.p[r] = (uint8_t)(r % 2);
    if (use_kind) use.p[r] = r % 3 == 1 ? 0 : (uint8_t)(1 + r % 5);            // (any value but 0 means "counts")
  }
  Exact<char> seq((size_t)padded(T), MA_FLAT_LANE), smp((size_t)padded(T), MA_FLAT_LANE);
  for (int64_t x = 0; x < T; x++) { seq.p[x] = (char)('a' + x % 26); smp.p[x] = (char)('A' + (x * 7) % 31); }
  const MaFlatView v(n, T, g.L, start.p, revcom.p, col_off.p, seq.p, smp.p, nullptr, use.p);

  long long stretches = 0, columns = 0, leaves = 0, whole = 0, beyond = 0;
  for (int64_t base = 0; base <= padded(T); base += MA_FLAT_LANE, stretches++) {     // (the last one lies wholly behind T)
    // the plain loop: every record, every column, kept where it lies inside the stretch
    std::vector<Event> want;
    for (int64_t r = 0; r < n; r++) {
      bool inside = false;
      for (int64_t c = 0; c < g.lens[(size_t)r]; c++) {
        const int64_t pos = col_off.p[r] + c;
        if (pos < base || pos >= base + MA_FLAT_LANE) continue;
        inside = true;
        want.push_back(Event{'C', r, c, (int64_t)g.starts[(size_t)r] + c, r % 2 == 1, !use_kind || r % 3 != 1, false, seq.p[pos], smp.p[pos]});
        columns++;
        if ((int64_t)g.starts[(size_t)r] + c >= g.L) beyond++;
      }
      if (!inside) continue;
      const bool w = col_off.p[r] >= base && col_off.p[r + 1] <= base + MA_FLAT_LANE;
      want.push_back(Event{'L', r, 0, 0, false, false, w, 0, 0});
      leaves++;
      whole += w ? 1 : 0;
    }
    // the walk, both forms
    for (int every = 0; every < 2; every++) {
      std::vector<Event> got;
      int calls = 0;
      auto column = [&](const MaFlatColumn& c) {
        const int64_t pos = base + calls++;
        if (!every && !c.live) fail(g, use_kind, base, "a position that is not live was handed over without EVERY_POSITION");
        if (every && c.live != (pos < T)) fail(g, use_kind, base, "EVERY_POSITION: `live` is not `the position lies in front of T`");
        if (c.live) got.push_back(Event{'C', c.r, c.col, c.p, c.rc, c.used, false, c.seq_ch, c.smp_ch});
      };
      auto leave = [&](int64_t r, bool w) { got.push_back(Event{'L', r, 0, 0, false, false, w, 0, 0}); };
      if (every) ma_flat_stretch<true>(v, base, column, leave);
      else ma_flat_stretch<false>(v, base, column, leave);
      if (every && calls != MA_FLAT_LANE) fail(g, use_kind, base, "EVERY_POSITION: not exactly 16 column calls");
      if (!every && calls != (int)(T - base < 0 ? 0 : T - base < MA_FLAT_LANE ? T - base : MA_FLAT_LANE)) fail(g, use_kind, base, "wrong number of column calls");
      if (got.size() != want.size()) fail(g, use_kind, base, every ? "EVERY_POSITION: the number of calls differs from the plain loop's" : "the number of calls differs from the plain loop's");
      for (size_t k = 0; k < want.size(); k++)
        if (!(got[k] == want[k])) {
          fprintf(stderr, "call %zu: got %c r=%lld col=%lld p=%lld rc=%d used=%d whole=%d '%c' '%c', want %c r=%lld col=%lld p=%lld rc=%d used=%d whole=%d '%c' '%c'\n", k,
                  got[k].kind, (long long)got[k].r, (long long)got[k].col, (long long)got[k].p, got[k].rc, got[k].used, got[k].whole, got[k].seq_ch ? got[k].seq_ch : '.',
                  got[k].smp_ch ? got[k].smp_ch : '.', want[k].kind, (long long)want[k].r, (long long)want[k].col, (long long)want[k].p, want[k].rc, want[k].used,
                  want[k].whole, want[k].seq_ch ? want[k].seq_ch : '.', want[k].smp_ch ? want[k].smp_ch : '.');
          fail(g, use_kind, base, every ? "EVERY_POSITION: a call differs from the plain loop's" : "a call differs from the plain loop's");
        }
    }
    // the bisection on its own: the last r with col_off[r] <= pos
    for (int64_t pos = base; pos < base + MA_FLAT_LANE && pos < T; pos++) {
      int64_t r = n - 1;
      while (col_off.p[r] > pos) r--;
      if (ma_flat_record_of(v, pos) != r) fail(g, use_kind, base, "ma_flat_record_of is not the last record that begins at or in front of the position");
    }
  }
  if (columns != T) fail(g, use_kind, 0, "the plain loop did not meet every column once");
  if (leaves != g.leaves || whole != g.whole || beyond != g.beyond) {
    fprintf(stderr, "leaves %lld whole %lld beyond %lld\n", leaves, whole, beyond);
    fail(g, use_kind, 0, "the geometry is not what its hand-made figures say");
  }
  printf("%s %d %lld %lld %lld %lld %lld\n", g.name, use_kind, stretches, columns, leaves, whole, beyond);
}

}  // namespace

int main() {
  for (const Geometry& g : geometries())
    for (int use_kind = 0; use_kind < 2; use_kind++) run(g, use_kind);
  printf("ok\n");
  return 0;
}
