// ma_ends_body.h -- fragment-end context (ma_hip -f 92) and read lengths (-f 93) of a .maln as functions of one record.  The
// reference has neither report: the rule is this project's own ("Fragment ends and read lengths").  A record that
// counts, with s = START, n columns, e = s + n - 1, strand rc, segment character seg and d = rc ? -1 : +1, has
//     a 5' end  at anchor column  rc ? e : s   unless seg is  rc ? 'f' : 'b'
//     a 3' end  at anchor column  rc ? s : e   unless seg is  rc ? 'b' : 'f'
// (a read split at the origin is two records; only the front record's START and the back record's END are ends of the read:
// starts_f, ends_r, ends_f, starts_r of col_print_cons, src/map_align.c:789-825).  Every end that is there yields 20 events, one per
// position k = -10 .. -1, +1 .. +10 (o = k + 10 for k < 0, k + 9 for k > 0), on column
//     5' end:  k > 0 (inside)  a + d (k - 1)      k < 0 (in front)  a + d k
//     3' end:  k < 0 (inside)  a + d (k + 1)      k > 0 (behind)    a + d k
// The class of column p: 5 outside 0 .. L-1 (no wrap), else A C G T -> 0 .. 3 and anything else 4 of toupper(ref[p]); for rc a class
// c < 4 becomes 3 - c.  The event's bin is (end * 20 + o) * 6 + class.  A record that is whole (seg neither 'f' nor 'b') also yields
// one length event, bin MA_ENDS_LEN + rc * 513 + min(length, 512): length = its columns that are not '-' plus the characters other
// than '-' of the INS_POS pairs that count -- position in 0 .. n-1 and no later pair of the record at the same position (read_ma's
// overwrite); a half yields bin MA_ENDS_HALVES instead.  A record without columns is not special.
//
// Plain C++ behind MIA_HD.  k_ma_ends (mia_ma_ends_kernels.h) gives every lane a record and adds every bin that ma_ends_record
// hands it to the wavefront's histogram; a host caller (tests/ma_ends_driver.cpp) runs the same code record by record.
#pragma once
#include <stdint.h>

#include "ma_profile_body.h"               // ma_prof_class, ma_prof_mirror and MA_FLAT_UNROLL
#include "ma_records.h"

namespace mia {

constexpr int MA_ENDS_REACH = 10, MA_ENDS_POS = 2 * MA_ENDS_REACH, MA_ENDS_CLASSES = 6, MA_ENDS_OUTSIDE = 5;
constexpr int MA_ENDS_CTX = 2 * MA_ENDS_POS * MA_ENDS_CLASSES;                  // 240: ctx[end][o][class]
constexpr int MA_ENDS_MAX_LEN = 512, MA_ENDS_LENS = MA_ENDS_MAX_LEN + 1;        // bin 512 holds everything longer than 511
constexpr int MA_ENDS_LEN = MA_ENDS_CTX, MA_ENDS_HALVES = MA_ENDS_LEN + 2 * MA_ENDS_LENS, MA_ENDS_BINS = MA_ENDS_HALVES + 1;   // 240, 1 266, 1 267

// The records (ma_records.h: seq and ins_bases are loaded in whole 16-byte words), the reference, the segments and the selection.
struct MaEndsView : MaRecords {
  const char* ref;           // [L]
  const uint8_t* segment;    // [n]: the SEG character; NULL = every record is whole
  const uint8_t* use;        // [n]: 0 = the record is left out; NULL = every record counts
  MaEndsView(const MaRecords& recs, const char* ref, const uint8_t* segment, const uint8_t* use) : MaRecords(recs), ref(ref), segment(segment), use(use) {}
  // ... or from the arrays this export reads alone, for a caller that holds no more (the host drivers): the rest of MaRecords is null
  MaEndsView(int64_t n, int32_t L, const int32_t* start, const uint8_t* revcom, const int64_t* col_off, const char* seq, const int32_t* rec_ins,
             const int32_t* ins_list, const int32_t* ins_pos, const int64_t* ins_off, const char* ins_bases, const char* ref, const uint8_t* segment,
             const uint8_t* use)
      : MaRecords{n, L, start, revcom, col_off, seq, rec_ins, ins_list, ins_pos, ins_off, ins_bases, nullptr}, ref(ref), segment(segment), use(use) {}
};

// is the end there (end 0 = 5', 1 = 3'), and on which column
MIA_HD inline bool ma_ends_has(int end, bool rc, char seg) { return seg != ((end == 0) != rc ? 'b' : 'f'); }
MIA_HD inline int64_t ma_ends_anchor(int end, bool rc, int64_t s, int64_t e) { return (end == 0) != rc ? s : e; }
MIA_HD inline int ma_ends_k(int o) { return o < MA_ENDS_REACH ? o - MA_ENDS_REACH : o - MA_ENDS_REACH + 1; }
// the column of position k: inside the read the anchor is the first one (5': k = +1, 3': k = -1), outside nothing is skipped
MIA_HD inline int64_t ma_ends_column(int end, int64_t a, int d, int k) {
  const bool inside = end == 0 ? k > 0 : k < 0;
  return a + (int64_t)d * (inside ? (k > 0 ? k - 1 : k + 1) : k);
}
MIA_HD inline int ma_ends_class(const char* ref, int32_t L, int64_t p, bool rc) {
  if (p < 0 || p >= L) return MA_ENDS_OUTSIDE;
  const int c = ma_prof_class(ref[p]);
  return rc ? ma_prof_mirror(c) : c;
}
MIA_HD inline int ma_ends_ctx_bin(int end, int o, int cls) { return (end * MA_ENDS_POS + o) * MA_ENDS_CLASSES + cls; }

// 0x80 in every byte of w that is '-' (exact: no carry leaves a byte)
MIA_HD inline uint32_t ma_ends_dash_flags(uint32_t w) {
  const uint32_t x = w ^ 0x2d2d2d2du;
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
// The characters other than '-' of seq[off .. off + n): whole 16-byte words from the one that holds seq[off] to the one that holds
// seq[off + n - 1], the bytes of the first and the last that are not the record's masked out.  n == 0: nothing is read.
MIA_HD inline int64_t ma_ends_bases(const char* seq, int64_t off, int64_t n) {
  int64_t dashes = 0;
  const int64_t end = off + n;
  for (int64_t base = off & ~(int64_t)(MA_REC_LANE - 1); base < end; base += MA_REC_LANE) {
    const MaRecWord x = ma_rec_load(seq + base);
    uint32_t m = 0;                        // bit b: byte b of the word is '-'
    MA_FLAT_UNROLL
    for (int w = 0; w < MA_REC_LANE / 4; w++) m |= (((ma_ends_dash_flags(x.w[w]) >> 7) * 0x00204081u >> 21) & 0xfu) << (4 * w);
    const int lo = off > base ? (int)(off - base) : 0, hi = end - base < MA_REC_LANE ? (int)(end - base) : MA_REC_LANE;
    dashes += __builtin_popcount(m & ((1u << hi) - 1u) & ~((1u << lo) - 1u));
  }
  return n - dashes;
}

// the characters other than '-' of the record's INS_POS pairs that count
MIA_HD inline int64_t ma_ends_inserted(const MaEndsView& v, int64_t r, int64_t ncols) {
  int64_t bases = 0;
  for (int32_t k = v.rec_ins[r], hi = v.rec_ins[r + 1]; k < hi; k++) {
    if (!ma_rec_pair_counts(v, k, hi, ncols)) continue;
    const int32_t e = v.ins_list[k];
    bases += ma_ends_bases(v.ins_bases, v.ins_off[e], v.ins_off[e + 1] - v.ins_off[e]);
  }
  return bases;
}

MIA_HD inline int ma_ends_len_bin(bool rc, int64_t length) {
  return MA_ENDS_LEN + (rc ? MA_ENDS_LENS : 0) + (int)(length < MA_ENDS_MAX_LEN ? length : MA_ENDS_MAX_LEN);
}

// Every event of record r (0 <= r < n): emit(bin) once per event -- none for a record that is left out, else 20 per end that is
// there and one for its length or for its being a half.
template <class Emit>
MIA_HD inline void ma_ends_record(const MaEndsView& v, int64_t r, Emit&& emit) {
  if (v.use && v.use[r] == 0) return;
  const int64_t off = v.col_off[r], n = v.col_off[r + 1] - off, s = v.start[r], e = s + n - 1;
  const bool rc = v.revcom[r] != 0;
  const char seg = v.segment ? (char)v.segment[r] : 'n';
  const int d = rc ? -1 : 1;
  for (int end = 0; end < 2; end++) {
    if (!ma_ends_has(end, rc, seg)) continue;
    const int64_t a = ma_ends_anchor(end, rc, s, e);
    for (int o = 0; o < MA_ENDS_POS; o++) emit(ma_ends_ctx_bin(end, o, ma_ends_class(v.ref, v.L, ma_ends_column(end, a, d, ma_ends_k(o)), rc)));
  }
  if (seg == 'f' || seg == 'b') emit(MA_ENDS_HALVES);
  else emit(ma_ends_len_bin(rc, ma_ends_bases(v.seq, off, n) + ma_ends_inserted(v, r, n)));
}

}  // namespace mia
