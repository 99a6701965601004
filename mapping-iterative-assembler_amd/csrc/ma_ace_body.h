// ma_ace_body.h -- the read blocks of ma's ACE export (-f 7; ace_output, reference src/io.c:756-913) as functions of one
// record: where it sits in the padded contig (the AF line), how long its padded read is, and the text of that read,
// already cut into lines of 50 with their newlines (:844-880).  Plain C++ behind MIA_HD: the kernels of
// mia_ma_ace_kernels.h run it with the lanes of a wavefront over a record's bytes, a host caller
// (tests/ma_ace_driver.cpp) one record at a time -- the same code either way.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>

#ifndef MIA_HD
#if defined(__HIPCC__)
#define MIA_HD __host__ __device__
#else
#define MIA_HD
#endif
#endif

namespace mia {

constexpr int MA_ACE_LINE = 50;   // max_line_length, src/io.c:767

// The records of a .maln as mia_hip_ma_tally receives them, the INS_POS pairs listed by record in ascending position
// (ma_ace_order_inserts), and the running sum of ref->gaps.
struct MaAceView {
  int64_t n;
  const int32_t* start;      // [n]
  const int64_t* col_off;    // [n+1]: record r owns seq[col_off[r] .. col_off[r+1]) = columns start .. end
  const char* seq;
  const int32_t* rec_ins;    // [n+1]: record r owns ins_list[rec_ins[r] .. rec_ins[r+1])
  const int32_t* ins_list;   // pair numbers, by record, ascending ins_pos; pairs of one position in the order they were given
  const int32_t* ins_pos;    // per pair: the insert sits in front of column start + ins_pos
  const int64_t* ins_off;    // per pair (+1): its bases are ins_bases[ins_off[e] .. ins_off[e+1])
  const char* ins_bases;
  // [L+2]: G[p] = gaps[0] + .. + gaps[p-1] (sum_of_gaps, src/map_alignment.c:658-664) with gaps[L] = 0 as ace_output sets it
  // (src/io.c:826): the record of a circular assembly may end on column L.  Every gaps[p] >= 0.
  const int64_t* G;
};

// One record's place in the export: columns, insert columns in front of and between them, length and bytes of its text
struct MaAceRec {
  int32_t start, ncols;
  int64_t g0;                // G[start]
  int64_t len;               // characters of the padded read: ncols + gaps[start] + .. + gaps[end] (j of src/io.c:848-866)
  int64_t bytes;             // len + one newline per full line + the newline of the remainder line (:868-879)
};

MIA_HD inline MaAceRec ma_ace_rec(const MaAceView& v, int64_t r) {
  MaAceRec q;
  q.start = v.start[r];
  q.ncols = (int32_t)(v.col_off[r + 1] - v.col_off[r]);
  q.g0 = v.G[q.start];
  q.len = (int64_t)q.ncols + (v.G[q.start + q.ncols] - q.g0);
  q.bytes = q.len + q.len / MA_ACE_LINE + 1;
  return q;
}

// the position the AF line prints: aln_seq->start + sum_of_gaps(start) + 1 (src/io.c:812-814)
MIA_HD inline int64_t ma_ace_af_pos(const MaAceRec& q) { return (int64_t)q.start + q.g0 + 1; }

// aln_seq->ins[pos]: read_ma lets a later pair of the same position replace an earlier one (src/map_alignment.c:602-605).
// The record's pairs are in ascending position, so the last pair of `pos` is found by bisection however many there are.
MIA_HD inline int ma_ace_insert(const MaAceView& v, int64_t r, int32_t pos, const char** bases) {
  int32_t lo = v.rec_ins[r], hi = v.rec_ins[r + 1];
  const int32_t first = lo;
  while (lo < hi) {                                  // first pair with a position above pos
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (v.ins_pos[v.ins_list[mid]] <= pos) lo = mid + 1; else hi = mid;
  }
  if (lo > first) {
    const int32_t e = v.ins_list[lo - 1];
    if (v.ins_pos[e] == pos) { *bases = v.ins_bases + v.ins_off[e]; return (int)(v.ins_off[e + 1] - v.ins_off[e]); }
  }
  *bases = nullptr;
  return 0;
}

// Character c (0 <= c < q.len) of the padded read of record r (src/io.c:849-870): column k of the record owns gaps[start + k]
// insert characters -- its inserted bases, cut off at gaps, then '*' -- and then its own character; '-' is printed as '*'.
// Column k's own character is character k + G[start + k + 1] - G[start]: the column is found by bisection over that.
MIA_HD inline char ma_ace_char(const MaAceView& v, int64_t r, const MaAceRec& q, int64_t c) {
  const int64_t* G = v.G + q.start;
  int32_t lo = 0, hi = q.ncols - 1;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)mid + (G[mid + 1] - q.g0) >= c) hi = mid; else lo = mid + 1;
  }
  const int32_t k = lo;
  const int64_t g = G[k + 1] - G[k], slot = c - ((int64_t)k + (G[k] - q.g0));
  char ch;
  if (slot >= g) ch = v.seq[v.col_off[r] + k];
  else {
    const char* bases = nullptr;
    const int len = ma_ace_insert(v, r, k, &bases);
    ch = slot < (int64_t)len ? bases[slot] : '*';
  }
  return ch == '-' ? '*' : ch;
}

// Byte o (0 <= o < q.bytes) of the record's text: lines of 50 characters, a newline behind each, and the remainder line
// (empty when the length is a multiple of 50) with its own
MIA_HD inline char ma_ace_byte(const MaAceView& v, int64_t r, const MaAceRec& q, int64_t o) {
  const int64_t c = o - o / (MA_ACE_LINE + 1);
  if (o % (MA_ACE_LINE + 1) == MA_ACE_LINE || c >= q.len) return '\n';
  return ma_ace_char(v, r, q, c);
}

// The whole text of record r at out[0 .. q.bytes).  Lane `lane` of `nlanes` writes its share -- single bytes up to the first
// address that is a multiple of four, whole 32-bit words from there, single bytes behind the last whole word; (0, 1)
// writes all of it.
MIA_HD inline void ma_ace_body(const MaAceView& v, int64_t r, char* out, int lane, int nlanes) {
  const MaAceRec q = ma_ace_rec(v, r);
  int64_t head = (int64_t)((4 - ((uintptr_t)out & 3)) & 3);
  if (head > q.bytes) head = q.bytes;
  const int64_t words = (q.bytes - head) >> 2, tail = head + (words << 2);
  for (int64_t o = lane; o < head; o += nlanes) out[o] = ma_ace_byte(v, r, q, o);
  for (int64_t w = lane; w < words; w += nlanes) {
    const int64_t o = head + (w << 2);
    const uint32_t x = (uint32_t)(unsigned char)ma_ace_byte(v, r, q, o) | (uint32_t)(unsigned char)ma_ace_byte(v, r, q, o + 1) << 8 |
                       (uint32_t)(unsigned char)ma_ace_byte(v, r, q, o + 2) << 16 | (uint32_t)(unsigned char)ma_ace_byte(v, r, q, o + 3) << 24;
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint32_t*>(out + o) = x;
#else
    memcpy(out + o, &x, 4);                          // (little-endian hosts, as the device is)
#endif
  }
  for (int64_t o = tail + lane; o < q.bytes; o += nlanes) out[o] = ma_ace_byte(v, r, q, o);
}

// Host side.  A record's pairs list[0 .. count) into ascending position, pairs of one position staying in the order they
// were given (so that the last one given is the last one listed); what mia writes is in that order already.
inline void ma_ace_order_inserts(int32_t* list, int32_t count, const int32_t* ins_pos) {
  bool sorted = true;
  for (int32_t k = 1; k < count && sorted; k++) sorted = ins_pos[list[k - 1]] <= ins_pos[list[k]];
  if (!sorted) std::stable_sort(list, list + count, [ins_pos](int32_t a, int32_t b) { return ins_pos[a] < ins_pos[b]; });
}

// ace_output reads consensus[0 .. seq_len + sum of gaps) but get_consensus leaves out the insert columns of column 0
// (src/map_alignment.c:222-227,249): with gaps[0] > 0 it reads past its string.  Such a file, and one with a negative
// GAPS value, has no ACE export.
inline bool ma_ace_gaps_ok(const int32_t* gaps, int64_t L) {
  if (L > 0 && gaps[0] > 0) return false;
  for (int64_t p = 0; p < L; p++) if (gaps[p] < 0) return false;
  return true;
}

}  // namespace mia
