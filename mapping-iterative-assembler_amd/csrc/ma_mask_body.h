// ma_mask_body.h -- the end mask of a .maln (ma_hip -E, -x, -f 96) as functions of one column, of one stretch of flat positions and of
// one record.  The reference has no such step: the rule is this project's own ("End mask"), defined on the depth codes as
// the substitution profile reads them (ma_prof_bin, ma_profile_body.h: d' in the read's orientation):
//     5' zone at k = 1 .. n5     d' = k - 1
//     3' zone at k = 1 .. n3     d' = 31 - k
// MIDDLE and columns with a bad code are in no zone.  Trim mode keeps columns a .. b-1 of a record: a1 = its first column in no zone,
// b1 = one behind its last (b1 = a1 when every column is in a zone), then a walks forward from a1 and b backward from b1 over '-'
// columns; a >= b empties the record.  Substitution mode writes N over a zone column whose base, in the read's orientation, is the one
// deamination makes (5': T; 3': A, single-stranded T).
//
// Plain C++ behind MIA_HD.  k_ma_mask_bounds (mia_ma_mask_kernels.h) gives every lane a stretch of MA_MASK_LANE flat positions:
// ma_mask_stretch is the shared walk (ma_flat_body.h) with this rule: it keeps a1 / b1 of the record it is in in registers, hands them
// to its caller when the walk leaves the record, and hands every zone column (substitution mode: every substituted column) to a counter.
// k_ma_mask_layout gives every lane a record: ma_mask_record walks the '-' columns and decides.  k_ma_mask_apply gives every lane a
// stretch of the NEW layout: ma_mask_gather reads its 16 columns from where they were.  The counts of trim mode are a difference: the
// bounds stage counts every zone column, the apply stage every zone column that stays (in a mia-written file: none), since a column's
// fate is known only behind the layout.  A host caller (tests/ma_mask_driver.cpp) runs the same code.
#pragma once
#include <stdint.h>

#include "ma_profile_body.h"

namespace mia {

constexpr int MA_MASK_LANE = MA_FLAT_LANE;
constexpr int MA_MASK_MAX_POS = 15;                                    // n5, n3 lie in 0 .. 15, k in 1 .. 15
constexpr int MA_MASK_K = MA_MASK_MAX_POS + 1;
constexpr int MA_MASK_HIST = 2 * 2 * MA_MASK_K;                        // hist[strand][end][k]
// the bins of one call: hist | the zone columns that stay (trim mode) | emptied[2] | stripped | pairs dropped | records kept
constexpr int MA_MASK_STAY = MA_MASK_HIST, MA_MASK_EMPTIED = MA_MASK_STAY + MA_MASK_HIST, MA_MASK_STRIPPED = MA_MASK_EMPTIED + 2,
              MA_MASK_PAIRS = MA_MASK_STRIPPED + 1, MA_MASK_KEPT = MA_MASK_PAIRS + 1, MA_MASK_BINS = MA_MASK_KEPT + 1;   // 133
constexpr int MA_MASK_TRIM = 0, MA_MASK_N = 1;
constexpr uint32_t MA_MASK_NO_COLUMN = 0xffffffffu;                    // a1 of a record no column of which is outside the zones

MIA_HD inline bool ma_mask_args_ok(int n5, int n3, int mode, int single_stranded) {
  return n5 >= 0 && n5 <= MA_MASK_MAX_POS && n3 >= 0 && n3 <= MA_MASK_MAX_POS && (n5 | n3) != 0 && (mode == MA_MASK_TRIM || mode == MA_MASK_N) &&
         (!single_stranded || mode == MA_MASK_N);
}

// The zone of a column: 0 = none, +k = the 5' zone at position k, -k = the 3' zone at position k.  The code is decoded by ma_prof_bin
// (a '-' column's bin is MA_PROF_DEL + d'), so that the mirroring of an RC record stays written once.
MIA_HD inline int ma_mask_zone(char smp_ch, bool rc, int n5, int n3) {
  const int bin = ma_prof_bin(false, '\0', '-', smp_ch, rc);
  if (bin == MA_PROF_BAD) return 0;
  const int d = bin - MA_PROF_DEL;
  if (d < n5) return d + 1;
  if (d > MA_PROF_DEPTHS - 1 - n3) return -(MA_PROF_DEPTHS - d);
  return 0;
}
MIA_HD inline int ma_mask_hist_bin(bool rc, int zone) { return ((rc ? 2 : 0) + (zone < 0 ? 1 : 0)) * MA_MASK_K + (zone < 0 ? -zone : zone); }

// substitution mode: does the column of zone `zone` (not 0) become N
MIA_HD inline bool ma_mask_substituted(char seq_ch, int zone, bool rc, bool single_stranded) {
  int j = ma_prof_class(seq_ch);
  if (rc) j = ma_prof_mirror(j);
  return j == (zone > 0 || single_stranded ? 3 : 0);
}

// The stretch of flat positions base .. base + MA_MASK_LANE - 1 (base a multiple of MA_MASK_LANE).  Trim mode: found(r, lo, hi, whole)
// is called once for every record r of the stretch, lo = the first column of r inside the stretch that is in no zone
// (MA_MASK_NO_COLUMN: none), hi = one behind the last such column (0: none), whole = every column of r lies inside the stretch; and
// count(bin) for every zone column.  Substitution mode: no found, count(bin) for every substituted column.
template <class Found, class Count>
MIA_HD inline void ma_mask_stretch(const MaFlatView& v, int n5, int n3, int mode, bool single_stranded, int64_t base, Found&& found, Count&& count) {
  uint32_t lo = MA_MASK_NO_COLUMN, hi = 0;
  ma_flat_stretch<false>(
      v, base,
      [&](const MaFlatColumn& c) {
        const int zone = ma_mask_zone(c.smp_ch, c.rc, n5, n3);
        const uint32_t col = (uint32_t)c.col;
        if (mode == MA_MASK_TRIM) {
          if (zone) count(ma_mask_hist_bin(c.rc, zone));
          else { if (lo == MA_MASK_NO_COLUMN) lo = col; hi = col + 1; }
        } else if (zone && ma_mask_substituted(c.seq_ch, zone, c.rc, single_stranded)) {
          count(ma_mask_hist_bin(c.rc, zone));
        }
      },
      [&](int64_t r, bool whole) {
        if (mode == MA_MASK_TRIM) found(r, lo, hi, whole);
        lo = MA_MASK_NO_COLUMN; hi = 0;
      });
}

// The layout stage's view: the records, what the bounds stage left per record, and the new record view's scalars per record.
struct MaMaskRecView {
  MaFlatView v;
  int32_t n5, n3, mode;
  const uint32_t* lo;        // [n]: a1, or MA_MASK_NO_COLUMN (trim mode)
  const uint32_t* hi;        // [n]: b1, or 0
  int32_t* first;            // [n] out: a
  int32_t* count;            // [n] out: b - a, 0 = emptied
  int32_t* start;            // [n] out: START of the masked record
};

// Record r: a and b from a1 and b1, first / count / start, and count(bin) for what the record adds to the scalars.  Returns the columns
// the record keeps.  A record of more than 2^31 - 1 columns is not supported (mia_hip_ma_tally takes fewer characters than that per
// record: a SEQ line is at most MAX_LINE_LEN long).
template <class Count>
MIA_HD inline int64_t ma_mask_record(const MaMaskRecView& m, int64_t r, Count&& count) {
  const int64_t o0 = m.v.col_off[r], n = m.v.col_off[r + 1] - o0;
  const bool rc = m.v.revcom[r] != 0;
  m.start[r] = m.v.start[r];
  if (m.mode == MA_MASK_N) {
    m.first[r] = 0; m.count[r] = (int32_t)n;
    count(MA_MASK_KEPT);
    return n;
  }
  int64_t a = m.lo[r] == MA_MASK_NO_COLUMN || (int64_t)m.lo[r] > n ? n : (int64_t)m.lo[r];
  int64_t b = (int64_t)m.hi[r] > n ? n : (int64_t)m.hi[r];
  if (b < a) b = a;
  const char *s = m.v.seq + o0, *p = m.v.smp + o0;
  for (; a < b && s[a] == '-'; a++) if (!ma_mask_zone(p[a], rc, m.n5, m.n3)) count(MA_MASK_STRIPPED);
  for (; b > a && s[b - 1] == '-'; b--) if (!ma_mask_zone(p[b - 1], rc, m.n5, m.n3)) count(MA_MASK_STRIPPED);
  if (a >= b) {
    m.first[r] = 0; m.count[r] = 0;
    count(MA_MASK_EMPTIED + (rc ? 1 : 0));
    return 0;
  }
  m.first[r] = (int32_t)a; m.count[r] = (int32_t)(b - a);
  m.start[r] = m.v.start[r] + (int32_t)a;
  count(MA_MASK_KEPT);
  return b - a;
}

// The apply stage's view: the records as they were, where every record's columns go, and the question asked.
struct MaMaskApplyView {
  MaFlatView v;              // the records as tallied
  int32_t n5, n3, mode, single_stranded;
  const int32_t* first;      // [n]
  const int64_t* new_off;    // [n+1]: record r's kept columns are flat positions new_off[r] .. new_off[r+1) of the new strings
  int64_t new_T;             // new_off[n]
};

// the record that holds position pos (0 <= pos < new_T) of the new layout: the last r with new_off[r] <= pos
MIA_HD inline int64_t ma_mask_new_record_of(const MaMaskApplyView& m, int64_t pos) {
  int64_t lo = 0, hi = m.v.n;
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (m.new_off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// 16 characters from p + at (at >= 0, any alignment; every character up to `limit`, the string's readable end, a multiple of 16, may be
// read): two aligned words and a byte shift -- the words are selected by constants, so that they stay registers.
MIA_HD inline MaRecWord ma_mask_load_unaligned(const char* p, int64_t at, int64_t limit) {
  const int64_t word = at & ~(int64_t)(MA_REC_LANE - 1);
  const MaRecWord x = ma_rec_load(p + word);
  MaRecWord y{{0, 0, 0, 0}};
  if (word + MA_REC_LANE < limit) y = ma_rec_load(p + word + MA_REC_LANE);
  const int q = (int)(at & 15) >> 2, t = ((int)at & 3) * 8;
  uint32_t w0 = x.w[0], w1 = x.w[1], w2 = x.w[2], w3 = x.w[3], w4 = y.w[0], w5 = y.w[1], w6 = y.w[2], w7 = y.w[3];
  if (q & 2) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; w5 = w7; }
  if (q & 1) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; }
  MaRecWord out;
  out.w[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> t);
  out.w[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> t);
  out.w[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> t);
  out.w[3] = (uint32_t)((((uint64_t)w4 << 32) | w3) >> t);
  return out;
}

// The stretch base .. base + MA_MASK_LANE - 1 of the NEW layout (base a multiple of MA_MASK_LANE, base < new_T rounded up): its SEQ and
// SMP characters, 0 behind new_T.  The columns of the stretch's first record come out of two unaligned 16-character loads; those of
// the records behind it (the seams) are read one by one.  Trim mode: count(bin) for every zone column met -- it stays.  Substitution
// mode: the substituted columns are N.
template <class Count>
MIA_HD inline void ma_mask_gather(const MaMaskApplyView& m, int64_t base, MaRecWord* seq_out, MaRecWord* smp_out, Count&& count) {
  MaRecWord so{{0, 0, 0, 0}}, mo{{0, 0, 0, 0}};
  if (base < m.new_T) {
    int64_t r = ma_mask_new_record_of(m, base);
    int64_t end = m.new_off[r + 1];
    int64_t delta = m.v.col_off[r] + m.first[r] - m.new_off[r];              // old flat position - new flat position, inside record r
    bool rc = m.v.revcom[r] != 0, head = true;
    const int64_t limit = (m.v.T + MA_REC_LANE - 1) & ~(int64_t)(MA_REC_LANE - 1);
    const MaRecWord sq = ma_mask_load_unaligned(m.v.seq, base + delta, limit), sm = ma_mask_load_unaligned(m.v.smp, base + delta, limit);
    MA_FLAT_UNROLL
    for (int w = 0; w < MA_MASK_LANE / 4; w++) {
      uint32_t a = sq.w[w], b = sm.w[w], sa = 0, sb = 0;
      MA_FLAT_NOUNROLL
      for (int q = 0; q < 4; q++, a >>= 8, b >>= 8) {
        const int64_t pos = base + w * 4 + q;
        if (pos >= m.new_T) continue;
        if (pos >= end) {                  // (pos < new_T = new_off[n]: r stays below n)
          do { r++; end = m.new_off[r + 1]; } while (pos >= end);
          delta = m.v.col_off[r] + m.first[r] - m.new_off[r];
          rc = m.v.revcom[r] != 0; head = false;
        }
        uint32_t ch = head ? (a & 0xffu) : (uint32_t)(unsigned char)m.v.seq[pos + delta];
        const uint32_t code = head ? (b & 0xffu) : (uint32_t)(unsigned char)m.v.smp[pos + delta];
        const int zone = ma_mask_zone((char)code, rc, m.n5, m.n3);
        if (zone) {
          if (m.mode == MA_MASK_TRIM) count(ma_mask_hist_bin(rc, zone));
          else if (ma_mask_substituted((char)ch, zone, rc, m.single_stranded != 0)) ch = 'N';
        }
        sa |= ch << (8 * q); sb |= code << (8 * q);
      }
      so.w[w] = sa; mo.w[w] = sb;
    }
  }
  *seq_out = so; *smp_out = mo;
}

// Pair e of record r: does it stay, and its position in the masked record (0 when it leaves).  Trim mode: a < pos < b.
MIA_HD inline bool ma_mask_pair(int mode, int32_t first, int32_t count, int32_t pos, int32_t* new_pos) {
  if (mode == MA_MASK_N) { *new_pos = pos; return true; }
  const bool stays = count > 0 && pos > first && (int64_t)pos < (int64_t)first + count;
  *new_pos = stays ? pos - first : 0;
  return stays;
}

}  // namespace mia
