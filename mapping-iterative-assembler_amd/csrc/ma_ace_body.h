// ma_ace_body.h -- the read blocks of ma's ACE export (-f 7; ace_output, reference src/io.c:756-913) as functions of one
// record: where it sits in the padded contig (the AF line), how long its padded read is, and the text of that read,
// already cut into lines of 50 with their newlines (:844-880).  Plain C++ behind MIA_HD: the kernels of
// mia_ma_ace_kernels.h run it with the lanes of a wavefront over a record's bytes, a host caller
// (tests/ma_ace_driver.cpp) one record at a time -- the same code either way.
#pragma once
#include <stdint.h>
#include <string.h>

#include "ma_records.h"

namespace mia {

constexpr int MA_ACE_LINE = 50;   // max_line_length, src/io.c:767

// The records (ma_records.h) and the running sum of ref->gaps.
struct MaAceView : MaRecords {
  // [L+2]: G[p] = gaps[0] + .. + gaps[p-1] (sum_of_gaps, src/map_alignment.c:658-664) with gaps[L] = 0 as ace_output sets it
  // (src/io.c:826): the record of a circular assembly may end on column L.  Every gaps[p] >= 0.
  const int64_t* G;
  MaAceView(const MaRecords& recs, const int64_t* G) : MaRecords(recs), G(G) {}
  // ... or from the arrays this export reads alone, for a caller that holds no more (the host drivers): the rest of MaRecords is null, L 0
  MaAceView(int64_t n, const int32_t* start, const int64_t* col_off, const char* seq, const int32_t* rec_ins, const int32_t* ins_list,
            const int32_t* ins_pos, const int64_t* ins_off, const char* ins_bases, const int64_t* G)
      : MaRecords{n, 0, start, nullptr, col_off, seq, rec_ins, ins_list, ins_pos, ins_off, ins_bases, nullptr}, G(G) {}
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
    const int len = ma_rec_insert(v, r, k, &bases);
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

// Host side.  ace_output reads consensus[0 .. seq_len + sum of gaps) but get_consensus leaves out the insert columns of column 0
// (src/map_alignment.c:222-227,249): with gaps[0] > 0 it reads past its string.  Such a file, and one with a negative
// GAPS value, has no ACE export.
inline bool ma_ace_gaps_ok(const int32_t* gaps, int64_t L) {
  if (L > 0 && gaps[0] > 0) return false;
  for (int64_t p = 0; p < L; p++) if (gaps[p] < 0) return false;
  return true;
}

}  // namespace mia
