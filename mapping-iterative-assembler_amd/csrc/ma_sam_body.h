// ma_sam_body.h -- CIGAR, SEQ and NM of ma_hip's SAM export (-f 8) as functions of one record.  The reference has no SAM output:
// the rule is this project's own ("SAM export").  A record of columns START .. END (n of them) on a reference of L
// columns is WALKED: for c = 0 .. n-1 first the characters of the insert the record has at position c (of several INS_POS pairs
// of one position the last one given; pairs outside 0 .. n-1 are never looked at, as in the ACE export), then the column's own
// character.  Every walk position yields at most one CIGAR op and at most one SEQ character:
//     insert character   '-': nothing            else: SEQ, op I -- op S when START + c >= L
//     column character   '-': op D, no SEQ       else: SEQ, op M -- op S when START + c >= L;  '-' when START + c >= L: nothing
// Equal neighbouring ops merge (a position that yields nothing does not separate them); a run prints as its decimal length and
// its letter.  NM = the D ops + the I ops + the M columns whose character differs from ref[START + c], both upper-cased.
// A record whose walk yields no SEQ character prints CIGAR "*" and SEQ "*" (its NM is still the count above).
//
// Plain C++ behind MIA_HD.  The kernels of mia_ma_sam_kernels.h put the 64 lanes of a wavefront on a stretch of 64 walk
// positions and hand the ballots of the lanes' ops to the mask functions below; a host caller (tests/ma_sam_driver.cpp) makes
// the same masks in a loop -- the same code either way.
#pragma once
#include <stdint.h>

#include "ma_records.h"

namespace mia {

constexpr int MA_SAM_NONE = 0, MA_SAM_M = 1, MA_SAM_I = 2, MA_SAM_D = 3, MA_SAM_S = 4, MA_SAM_OPS = 5;
// a record's body is <CIGAR> MA_SAM_MID <SEQ>: fields 6-10 of its line (RNEXT *, PNEXT 0, TLEN 0 between them)
#define MA_SAM_MID "\t*\t0\t0\t"
#define MA_SAM_EMPTY "*\t*\t0\t0\t*"
constexpr int MA_SAM_MID_BYTES = 7, MA_SAM_EMPTY_BYTES = 9;

// The records (ma_records.h), the reference, and the index of every record's inserts that ma_sam_index writes.
struct MaSamView : MaRecords {
  const char* ref;           // [L]
  // [pairs + n + 1]: record r owns cum[rec_ins[r] + r .. rec_ins[r+1] + r], one word per listed pair and one behind them:
  // word j = the insert characters the walk holds in front of pair j's own (pairs that do not count hold none)
  int64_t* cum;
  MaSamView(const MaRecords& recs, const char* ref, int64_t* cum) : MaRecords(recs), ref(ref), cum(cum) {}
  // ... or from the arrays this export reads alone, for a caller that holds no more (the host drivers): the rest of MaRecords is null
  MaSamView(int64_t n, int32_t L, const int32_t* start, const int64_t* col_off, const char* seq, const int32_t* rec_ins, const int32_t* ins_list,
            const int32_t* ins_pos, const int64_t* ins_off, const char* ins_bases, const char* ref, int64_t* cum)
      : MaRecords{n, L, start, nullptr, col_off, seq, rec_ins, ins_list, ins_pos, ins_off, ins_bases, nullptr}, ref(ref), cum(cum) {}
};

MIA_HD inline int64_t ma_sam_ncols(const MaSamView& v, int64_t r) { return v.col_off[r + 1] - v.col_off[r]; }

// Fills the record's words of v.cum and returns the length of its walk: its columns and the characters of the pairs that count.
MIA_HD inline int64_t ma_sam_index(const MaSamView& v, int64_t r) {
  const int32_t lo = v.rec_ins[r], cnt = v.rec_ins[r + 1] - lo;
  const int64_t ncols = ma_sam_ncols(v, r);
  int64_t* cum = v.cum + lo + r;
  int64_t run = 0;
  for (int32_t j = 0; j < cnt; j++) {
    cum[j] = run;
    const int32_t e = v.ins_list[lo + j];
    if (ma_rec_pair_counts(v, lo + j, lo + cnt, ncols)) run += v.ins_off[e + 1] - v.ins_off[e];
  }
  cum[cnt] = run;
  return ncols + run;
}

MIA_HD inline int64_t ma_sam_walk_len(const MaSamView& v, int64_t r) { return ma_sam_ncols(v, r) + v.cum[v.rec_ins[r + 1] + r]; }

MIA_HD inline char ma_sam_upper(char c) { return c >= 'a' && c <= 'z' ? (char)(c - 32) : c; }

// what walk position w (0 <= w < walk length) of record r yields
struct MaSamElem {
  int op;        // MA_SAM_NONE .. MA_SAM_S
  char ch;       // its SEQ character, for M, I and S
  bool nm;       // it counts for NM
};

// Pair j's characters begin at walk position ins_pos + cum[j], a key that never falls along the record's list and is the same
// for the pairs of one position only (those in front of the last hold no characters): the last pair whose key is <= w is found by
// bisection.  w lies inside its characters, or on a column behind them.
MIA_HD inline MaSamElem ma_sam_elem(const MaSamView& v, int64_t r, int64_t w) {
  const int32_t lo = v.rec_ins[r], cnt = v.rec_ins[r + 1] - lo;
  const int64_t* cum = v.cum + lo + r;
  int32_t a = 0, b = cnt;
  while (a < b) {
    const int32_t mid = a + ((b - a) >> 1);
    if ((int64_t)v.ins_pos[v.ins_list[lo + mid]] + cum[mid] <= w) a = mid + 1; else b = mid;
  }
  int64_t c = w;
  bool inserted = false;
  char ch = 0;
  if (a > 0) {
    const int32_t e = v.ins_list[lo + a - 1];
    const int64_t d = w - ((int64_t)v.ins_pos[e] + cum[a - 1]);
    if (d < cum[a] - cum[a - 1]) { inserted = true; c = v.ins_pos[e]; ch = v.ins_bases[v.ins_off[e] + d]; }
    else c = w - cum[a];
  }
  const int64_t p = (int64_t)v.start[r] + c;
  const bool clip = p >= v.L;
  MaSamElem x{MA_SAM_NONE, 0, false};
  if (!inserted) ch = v.seq[v.col_off[r] + c];
  if (ch == '-') {
    if (!inserted && !clip) { x.op = MA_SAM_D; x.nm = true; }
    return x;
  }
  x.ch = ch;
  if (clip) x.op = MA_SAM_S;
  else if (inserted) { x.op = MA_SAM_I; x.nm = true; }
  else { x.op = MA_SAM_M; x.nm = ma_sam_upper(ch) != ma_sam_upper(v.ref[p]); }
  return x;
}

// ---- a stretch of 64 walk positions, as masks ------------------------------------------------------------------------------------
struct MaSamStretch {
  uint64_t m[MA_SAM_OPS];    // m[op]: the positions of the stretch whose op it is (m[MA_SAM_NONE] is not used)
  uint64_t act;              // m[M] | m[I] | m[D] | m[S]
};
// the run that is open in front of a stretch (op MA_SAM_NONE: none), or one that a position closes
struct MaSamRun {
  int op;
  int64_t len;
};

MIA_HD inline uint64_t ma_sam_below(int lane) { return (1ull << lane) - 1ull; }
MIA_HD inline int ma_sam_top(uint64_t x) { return 63 - __builtin_clzll(x); }   // (x != 0)
MIA_HD inline int ma_sam_count(uint64_t x) { return __builtin_popcountll(x); }

// (selects, not an index that varies: the masks stay in registers)
MIA_HD inline uint64_t ma_sam_mask(const MaSamStretch& s, int op) {
  return op == MA_SAM_M ? s.m[MA_SAM_M] : op == MA_SAM_I ? s.m[MA_SAM_I] : op == MA_SAM_D ? s.m[MA_SAM_D] : op == MA_SAM_S ? s.m[MA_SAM_S] : 0ull;
}
MIA_HD inline int ma_sam_op_at(const MaSamStretch& s, int lane) {
  return (s.m[MA_SAM_M] >> lane) & 1ull ? MA_SAM_M : (s.m[MA_SAM_I] >> lane) & 1ull ? MA_SAM_I : (s.m[MA_SAM_D] >> lane) & 1ull ? MA_SAM_D :
         (s.m[MA_SAM_S] >> lane) & 1ull ? MA_SAM_S : MA_SAM_NONE;
}

// A run begins at position `lane` (whose op is `op`): the nearest position to its left that has an op has another one -- or there
// is none in the stretch and the open run has another one.
MIA_HD inline bool ma_sam_head(const MaSamStretch& s, int lane, int op, int open_op) {
  if (op == MA_SAM_NONE) return false;
  const uint64_t left = s.act & ma_sam_below(lane);
  return left ? !((ma_sam_mask(s, op) >> ma_sam_top(left)) & 1ull) : open_op != op;
}

// The run that ends where the head at `lane` begins its own: the one of the head before it in the stretch, or the open run
// (op MA_SAM_NONE in front of the record's first).  heads = the stretch's positions for which ma_sam_head holds.
MIA_HD inline MaSamRun ma_sam_closed(const MaSamStretch& s, uint64_t heads, int lane, const MaSamRun& open) {
  const uint64_t left = s.act & ma_sam_below(lane), heads_left = heads & ma_sam_below(lane);
  if (!heads_left) return MaSamRun{open.op, open.op != MA_SAM_NONE ? open.len + ma_sam_count(left) : 0};
  const int h = ma_sam_top(heads_left);
  return MaSamRun{ma_sam_op_at(s, h), (int64_t)ma_sam_count(left >> h)};
}

// the run that is open behind the stretch
MIA_HD inline MaSamRun ma_sam_carry(const MaSamStretch& s, uint64_t heads, const MaSamRun& open) {
  if (!heads) return MaSamRun{open.op, open.len + ma_sam_count(s.act)};
  const int h = ma_sam_top(heads);
  return MaSamRun{ma_sam_op_at(s, h), (int64_t)ma_sam_count(s.act >> h)};
}

// a run's text: decimal length, letter
MIA_HD inline int ma_sam_run_bytes(int64_t len) {
  int k = 2;
  for (; len >= 10; len /= 10) k++;
  return k;
}
MIA_HD inline void ma_sam_run_text(const MaSamRun& run, char* out) {
  int k = ma_sam_run_bytes(run.len) - 1;
  out[k] = "?MIDS"[run.op];
  for (int64_t x = run.len; k > 0; x /= 10) out[--k] = (char)('0' + x % 10);
}

// bytes of a record's body from the bytes of its CIGAR and of its SEQ
MIA_HD inline int64_t ma_sam_body_bytes(int64_t cigar_bytes, int64_t seq_len) {
  return seq_len > 0 ? cigar_bytes + MA_SAM_MID_BYTES + seq_len : MA_SAM_EMPTY_BYTES;
}

// Host side: a negative GAPS value is a malformed file; GAPS[0] > 0 is fine here (SAM never looks at the gapped consensus)
inline bool ma_sam_gaps_ok(const int32_t* gaps, int64_t L) {
  for (int64_t p = 0; p < L; p++) if (gaps[p] < 0) return false;
  return true;
}

}  // namespace mia
