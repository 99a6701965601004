// ma_flat_body.h -- the walk over the FLAT columns of a .maln that the profile, the deaminated-fragment filter, the damage score and
// the end mask share.  The records' SEQ and SMP strings lie end to end (col_off): flat position x is one column of one record.  A
// caller takes MA_FLAT_LANE = 16 positions at a time, a STRETCH whose base is a multiple of 16:
//     two 16-byte loads, one of SEQ and one of SMP;
//     one bisection of col_off for the record of the first position (ma_flat_record_of);
//     then forward from record to record: where a position lies behind the record's end, the next record that has a column.
// What a column contributes and what a record hands over when the walk leaves it are the caller's, as two callables: ma_prof_stretch
// (ma_profile_body.h), ma_dmg_stretch (ma_damage_body.h), ma_pmd_stretch (ma_pmd_body.h) and ma_mask_stretch (ma_mask_body.h) are
// this walk with their rule.  The 16 positions are four unrolled words, so that each is a register, and the four characters of a
// word one loop that is not unrolled, so that the code stays short: no scratch.
//
// Plain C++ behind MIA_HD: the kernels run it per lane, tests/ma_flat_driver.cpp runs it stretch by stretch against a plain loop.
#pragma once
#include <stdint.h>

#include "ma_records.h"

#if defined(__clang__)
#define MA_FLAT_UNROLL _Pragma("unroll")
#define MA_FLAT_NOUNROLL _Pragma("nounroll")
#else
#define MA_FLAT_UNROLL
#define MA_FLAT_NOUNROLL
#endif

namespace mia {

constexpr int MA_FLAT_LANE = MA_REC_LANE;  // flat positions of one stretch: one 16-byte word of SEQ and one of SMP

// The records (ma_records.h: seq and smp are loaded in whole 16-byte words), the reference and the selection.
struct MaFlatView : MaRecords {
  int64_t T;                 // col_off[n] flat positions
  const char* ref;           // [L]; the walk does not read it (the end mask passes NULL)
  const uint8_t* use;        // [n]: 0 = the record is left out; NULL = every record counts
  MaFlatView(const MaRecords& recs, int64_t T, const char* ref, const uint8_t* use) : MaRecords(recs), T(T), ref(ref), use(use) {}
  // ... or from the arrays the walk reads alone, for a caller that holds no more (the host drivers): the rest of MaRecords is null
  MaFlatView(int64_t n, int64_t T, int32_t L, const int32_t* start, const uint8_t* revcom, const int64_t* col_off, const char* seq, const char* smp,
             const char* ref, const uint8_t* use)
      : MaRecords{n, L, start, revcom, col_off, seq, nullptr, nullptr, nullptr, nullptr, nullptr, smp}, T(T), ref(ref), use(use) {}
};

// the record that holds flat position pos (0 <= pos < T): the last r with col_off[r] <= pos -- records without columns hold none
MIA_HD inline int64_t ma_flat_record_of(const MaFlatView& v, int64_t pos) {
  int64_t lo = 0, hi = v.n;                // col_off[lo] <= pos < col_off[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v.col_off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// One flat position as the walk hands it to `column`.  Of a position that is not live only `live` means anything.
struct MaFlatColumn {
  int64_t r;                 // the record
  int64_t col;               // the column inside the record: pos - col_off[r]
  int64_t p;                 // the reference column START + col (p >= L: the record of a circular assembly that runs past column L)
  bool rc, used;             // the record's strand; does it count (use)
  bool live;                 // the position lies in front of T
  char seq_ch, smp_ch;
};

// The stretch of flat positions base .. base + MA_FLAT_LANE - 1 (base a multiple of MA_FLAT_LANE).
// column(c) is called in order for every position of the stretch in front of T.  leave(r, whole) is called once for every record
// that has a column inside the stretch, behind that record's last column there: when the record changes and at the stretch's end;
// whole = every column of r lies inside the stretch.
// EVERY_POSITION: column is called exactly MA_FLAT_LANE times whatever the base, the positions at or behind T not live, and nothing
// is loaded for a stretch that lies wholly behind T -- so a wavefront's lanes reach each call together and the callable may hold a
// ballot.  Otherwise the walk returns at once for such a stretch.
template <bool EVERY_POSITION, class Column, class Leave>
MIA_HD inline void ma_flat_stretch(const MaFlatView& v, int64_t base, Column&& column, Leave&& leave) {
  const bool any = base < v.T;
  if (!EVERY_POSITION && !any) return;
  MaRecWord sq{{0, 0, 0, 0}}, sm{{0, 0, 0, 0}};
  int64_t r = 0, end = 0, o0 = 0;
  int32_t start = 0;
  bool rc = false, used = false;
  if (any) {
    sq = ma_rec_load(v.seq + base);
    sm = ma_rec_load(v.smp + base);
    r = ma_flat_record_of(v, base);
    o0 = v.col_off[r]; end = v.col_off[r + 1];
    start = v.start[r]; rc = v.revcom[r] != 0; used = !v.use || v.use[r] != 0;
  }
  MA_FLAT_UNROLL
  for (int w = 0; w < MA_FLAT_LANE / 4; w++) {
    uint32_t a = sq.w[w], b = sm.w[w];
    MA_FLAT_NOUNROLL
    for (int q = 0; q < 4; q++, a >>= 8, b >>= 8) {
      const int64_t pos = base + w * 4 + q;
      const bool live = pos < v.T;
      if (!EVERY_POSITION && !live) continue;
      if (live && pos >= end) {            // (pos < T = col_off[n]: r stays below n)
        leave(r, o0 >= base);
        do { r++; end = v.col_off[r + 1]; } while (pos >= end);
        o0 = v.col_off[r];
        start = v.start[r]; rc = v.revcom[r] != 0; used = !v.use || v.use[r] != 0;
      }
      column(MaFlatColumn{r, pos - o0, (int64_t)start + (pos - o0), rc, used, live, (char)(a & 0xffu), (char)(b & 0xffu)});
    }
  }
  if (any) leave(r, o0 >= base && end <= base + MA_FLAT_LANE);
}

}  // namespace mia
