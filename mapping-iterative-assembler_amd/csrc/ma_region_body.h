// ma_region_body.h -- the region view of ma (print_region, reference src/map_align.c:543-759) as functions of one record
// and one region: which records overlap it (alnseq_ol_reg, src/map_align.c:44-46) and what text row a record gives
// (:687-736).  Plain C++ behind MIA_HD: the kernels of mia_ma_region_kernels.h run it one wavefront per row, a host
// caller (tests/ma_region_driver.cpp) one row at a time -- the same code either way.
#pragma once
#include <stdint.h>
#include <string.h>

#include "ma_records.h"

namespace mia {

// The records (ma_records.h) and one region.
struct MaRegionView : MaRecords {
  const int32_t* gaps;       // [L]: ref->gaps
  int32_t first, last;       // 0-based inclusive reference columns
  // colmap[k], k = 0 .. last - first + 1: text offset of the first insert column in front of reference column first + k
  // (every column p owns gaps[p] insert columns, p == 0 and p == first included); colmap[last - first + 1] = the row's width
  const int64_t* colmap;
  MaRegionView(const MaRecords& recs, const int32_t* gaps, int32_t first, int32_t last, const int64_t* colmap)
      : MaRecords(recs), gaps(gaps), first(first), last(last), colmap(colmap) {}
  // ... or from the arrays this export reads alone, for a caller that holds no more (the host drivers): the rest of MaRecords is null, L 0
  MaRegionView(int64_t n, const int32_t* start, const int64_t* col_off, const char* seq, const int32_t* rec_ins, const int32_t* ins_list,
               const int32_t* ins_pos, const int64_t* ins_off, const char* ins_bases, const int32_t* gaps, int32_t first, int32_t last, const int64_t* colmap)
      : MaRecords{n, 0, start, nullptr, col_off, seq, rec_ins, ins_list, ins_pos, ins_off, ins_bases, nullptr}, gaps(gaps), first(first), last(last),
        colmap(colmap) {}
};

MIA_HD inline int ma_region_gap(int32_t g) { return g > 0 ? g : 0; }

// alnseq_ol_reg: a record of columns start .. end is shown when it reaches into first .. last
MIA_HD inline bool ma_region_overlaps(int32_t start, int32_t end, int32_t first, int32_t last) { return start <= last && end >= first; }

MIA_HD inline int32_t ma_region_end(const MaRegionView& v, int64_t r) { return v.start[r] + (int32_t)(v.col_off[r + 1] - v.col_off[r]) - 1; }

// '.' over row[a .. b): lane `lane` of `nlanes` takes its share; whole 16-byte words where the address allows
MIA_HD inline void ma_region_dots(char* row, int64_t a, int64_t b, int lane, int nlanes) {
  if (a >= b) return;
#if defined(__HIP_DEVICE_COMPILE__)
  const int64_t head = (int64_t)((16 - ((uintptr_t)(row + a) & 15)) & 15);
  const int64_t a16 = a + head < b ? a + head : b;
  const int64_t words = (b - a16) >> 4, b16 = a16 + (words << 4);
  for (int64_t i = a + lane; i < a16; i += nlanes) row[i] = '.';
  uint4* w = reinterpret_cast<uint4*>(row + a16);
  const uint4 d = make_uint4(0x2e2e2e2eu, 0x2e2e2e2eu, 0x2e2e2e2eu, 0x2e2e2e2eu);
  for (int64_t i = lane; i < words; i += nlanes) w[i] = d;
  for (int64_t i = b16 + lane; i < b; i += nlanes) row[i] = '.';
#else
  if (lane == 0) memset(row + a, '.', (size_t)(b - a));
#endif
}

// The gaps[p] + 1 characters of reference column p = first + k in the row of record r, which covers p
// (src/map_align.c:691-724): the insert columns -- dots on the record's own first column, else its inserted bases and
// then '-' -- and the record's character.
MIA_HD inline void ma_region_column(const MaRegionView& v, int64_t r, int32_t k, char* row) {
  const int32_t p = v.first + k, s = v.start[r];
  const int g = ma_region_gap(v.gaps[p]);
  char* out = row + v.colmap[k];
  if (g > 0) {
    if (p == s) {
      for (int i = 0; i < g; i++) out[i] = '.';
    } else {
      const char* bases = nullptr;
      int len = ma_rec_insert(v, r, p - s, &bases);
      if (len > g) len = g;                      // (an insert longer than ref->gaps says: the reference writes past its row)
      for (int i = 0; i < len; i++) out[i] = bases[i];
      for (int i = len; i < g; i++) out[i] = '-';
    }
  }
  out[g] = v.seq[v.col_off[r] + (p - s)];
}

// The whole row of record r (colmap[last - first + 1] bytes, no terminator): dots left and right of the columns it
// covers, ma_region_column over those.  Lane `lane` of `nlanes` writes its share; (0, 1) writes all of it.
MIA_HD inline void ma_region_row(const MaRegionView& v, int64_t r, char* row, int lane, int nlanes) {
  if (v.first > v.last) return;
  const int32_t s = v.start[r], e = ma_region_end(v, r), ncol = v.last - v.first + 1;
  int32_t ka = (s > v.first ? s : v.first) - v.first, kb = (e < v.last ? e : v.last) + 1 - v.first;   // covered: [ka, kb)
  if (ka > ncol) ka = ncol;
  if (kb < ka) kb = ka;
  ma_region_dots(row, 0, v.colmap[ka], lane, nlanes);
  for (int32_t k = ka + lane; k < kb; k += nlanes) ma_region_column(v, r, k, row);
  ma_region_dots(row, v.colmap[kb], v.colmap[ncol], lane, nlanes);
}

}  // namespace mia
