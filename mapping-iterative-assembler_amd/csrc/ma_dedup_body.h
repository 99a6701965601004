// ma_dedup_body.h -- the duplicate filter (ma_hip -u, -t) as functions of one record, one molecule or one run.  The rule is
// the reference's sort_fsdb + set_uniq_in_fsdb with just_outer_coords and a tolerance (src/fsdb.c:13-88,440-508); DESIGN.md,
// "Duplicate filter", states it in full and tests/ma_dedup_ref.py restates it.
//
// MOLECULES.  Record r has START s, END e (e = s - 1: no columns), strand rc, SCORE and mate[r]: MA_DEDUP_NONE (a molecule of its
// own), MA_DEDUP_ORPHAN (a half without its other half: always kept, never clustered) or the record number of its other half.  Of
// two halves the FRONT is the one with the greater START (the back half begins at column 0 of a circular reference; equal STARTs:
// the lower record number); the molecule is (rc, a = s(front), e = e(back) + L) with the front's SCORE.  Its index is the lower of
// the two record numbers.
// KEY.  With E = 2 L and e1 = e + 1 (so that a record without columns at column 0 has no negative coordinate) both a and e1 lie in
// 0 .. E.  The reverse strand is mirrored, a' = E - e1 and e' = E - a, after which BOTH strands sort as "a' ascending, e' descending":
//     key = forward << 2 W  |  a' << W  |  E - e'          W = the bits of E
// (reverse molecules first, as fs_comp has them).  Equal keys are a RUN.  |a - a0| <= t and |e - e0| <= t are the same tests on the
// mirrored coordinates, and within a strand a' never falls from one run to the next.
// BEST of a run: the highest SCORE, then the lowest index -- the maximum of  (score ^ 0x80000000) << 32 | ~index  as one 64-bit word
// (never 0: an index is below 2^31).
// NEXT of run k: the first later run that is not a duplicate of k (R if there is none).  The anchors are the orbit of run 0 under
// NEXT: what set_uniq_in_fsdb's walk visits, because it compares with the latest anchor only.
//
// Plain C++ behind MIA_HD.  The kernels of mia_ma_dedup_kernels.h call these per lane; tests/ma_dedup_driver.cpp runs the same
// functions in the same stages (runs, next, doubling, scan) on the host against a serial walk.
#pragma once
#include <stdint.h>

#include "ma_molecule_body.h"

namespace mia {

constexpr int64_t MA_DEDUP_NONE = MA_MOL_NONE, MA_DEDUP_ORPHAN = MA_MOL_ORPHAN;   // the one encoding of mate (ma_molecule_body.h)
constexpr int MA_DEDUP_MAX_TOL = 100;
constexpr int MA_DEDUP_SIZES = 1025;                       // bins 1 .. 1023, bin 1024 = larger; bin 0 unused
constexpr int MA_DEDUP_HIST = 2 * MA_DEDUP_SIZES;          // [strand][size]
constexpr int32_t MA_DEDUP_MAX_L = 1 << 29;                // 2 W + 1 <= 63 bits with room to spare
constexpr uint64_t MA_DEDUP_NO_KEY = ~0ull;                // a record that is no molecule (a back half, an orphan): sorts behind every key

MIA_HD inline int ma_dedup_width(int32_t L) {              // W: the bits of E = 2 L
  int w = 1;
  while ((2ll * L) >> w) w++;
  return w;
}
MIA_HD inline int ma_dedup_key_bits(int32_t L) { return 2 * ma_dedup_width(L) + 1; }
MIA_HD inline int ma_dedup_passes(int32_t L) { return (ma_dedup_key_bits(L) + 7) / 8; }      // 8-bit passes of the radix sort

MIA_HD inline uint64_t ma_dedup_key(int32_t L, int W, bool rc, int64_t a, int64_t e) {
  const int64_t E = 2ll * L, e1 = e + 1;
  const int64_t am = rc ? E - e1 : a, em = rc ? E - a : e1;
  return ((uint64_t)(rc ? 0 : 1) << (2 * W)) | ((uint64_t)am << W) | (uint64_t)(E - em);
}

// is `r` the front of the pair (r, m)
MIA_HD inline bool ma_dedup_front(const int32_t* start, int64_t r, int64_t m) { return start[r] > start[m] || (start[r] == start[m] && r < m); }

// the key of record r, MA_DEDUP_NO_KEY if it is no molecule's first record
MIA_HD inline uint64_t ma_dedup_record_key(int32_t L, int W, const int32_t* start, const int32_t* end, const uint8_t* revcom, const int64_t* mate, int64_t r) {
  const int64_t m = mate ? mate[r] : MA_DEDUP_NONE;
  if (m == MA_DEDUP_ORPHAN) return MA_DEDUP_NO_KEY;
  if (m < 0) return ma_dedup_key(L, W, revcom[r] != 0, start[r], end[r]);
  if (!ma_dedup_front(start, r, m)) return MA_DEDUP_NO_KEY;
  return ma_dedup_key(L, W, revcom[r] != 0, start[r], (int64_t)end[m] + L);
}

MIA_HD inline int64_t ma_dedup_index(const int64_t* mate, int64_t r) {
  const int64_t m = mate ? mate[r] : MA_DEDUP_NONE;
  return m >= 0 && m < r ? m : r;
}

MIA_HD inline uint64_t ma_dedup_pack(int32_t score, int64_t index) { return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint32_t)~(uint32_t)index; }
MIA_HD inline int64_t ma_dedup_packed_index(uint64_t packed) { return (int64_t)(uint32_t)~(uint32_t)packed; }

// is the run with key kj a duplicate of the (earlier) run with key kk under tolerance t
MIA_HD inline bool ma_dedup_is_dup(uint64_t kk, uint64_t kj, int W, int32_t t) {
  const uint64_t mask = (1ull << W) - 1;
  if ((kk >> (2 * W)) != (kj >> (2 * W))) return false;
  const int64_t da = (int64_t)((kj >> W) & mask) - (int64_t)((kk >> W) & mask);
  const int64_t de = (int64_t)(kj & mask) - (int64_t)(kk & mask);
  return da <= t && da >= -(int64_t)t && de <= t && de >= -(int64_t)t;
}

// the first run behind k that is no duplicate of k; R if every later run is
MIA_HD inline int64_t ma_dedup_next(const uint64_t* run_key, int64_t R, int64_t k, int W, int32_t t) {
  const uint64_t kk = run_key[k];
  int64_t j = k + 1;
  while (j < R && ma_dedup_is_dup(kk, run_key[j], W, t)) j++;
  return j;
}

MIA_HD inline bool ma_dedup_key_forward(uint64_t key, int W) { return ((key >> (2 * W)) & 1u) != 0; }
MIA_HD inline int ma_dedup_size_bin(bool forward, int64_t size) { return (forward ? 0 : MA_DEDUP_SIZES) + (int)(size < MA_DEDUP_SIZES - 1 ? size : MA_DEDUP_SIZES - 1); }

// doubling rounds that reach every run from run 0: the least j with 2^j >= R
MIA_HD inline int ma_dedup_rounds(int64_t R) {
  int j = 0;
  while (((int64_t)1 << j) < R) j++;
  return j;
}

}  // namespace mia
