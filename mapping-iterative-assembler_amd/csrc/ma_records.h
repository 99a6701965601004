// ma_records.h -- the records of a .maln as mia_hip_ma_tally leaves them on the device, and what every export of ma_hip needs of them:
// the one view of the arrays (MaRecords), the 16-byte load of their character strings, the INS_POS pairs listed by record (host:
// ma_list_pairs) and the pair that counts at a position (ma_rec_insert, ma_rec_pair_counts).  Plain C++ behind MIA_HD: the kernels
// and the host callers under tests/ run the same code.  The views of the exports (ma_*_body.h) derive from MaRecords and add
// what is their own.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#ifndef MIA_HD
#if defined(__HIPCC__)
#define MIA_HD __host__ __device__
#else
#define MIA_HD
#endif
#endif

namespace mia {

constexpr int MA_REC_LANE = 16;            // seq, smp and ins_bases are read in words of this many characters

struct MaRecords {
  int64_t n;
  int32_t L;                 // reference columns
  const int32_t* start;      // [n]
  const uint8_t* revcom;     // [n]
  const int64_t* col_off;    // [n+1]: record r owns seq / smp[col_off[r] .. col_off[r+1]) = columns start .. end
  const char* seq;           // 16-byte aligned and readable up to the next multiple of MA_REC_LANE behind col_off[n] (what lies there is not looked at)
  // The INS_POS pairs by record (ma_list_pairs)
  const int32_t* rec_ins;    // [n+1]: record r owns ins_list[rec_ins[r] .. rec_ins[r+1])
  const int32_t* ins_list;   // pair numbers, by record, ascending ins_pos; pairs of one position in the order they were given
  const int32_t* ins_pos;    // per pair: the insert sits in front of column start + ins_pos
  const int64_t* ins_off;    // per pair (+1): its characters are ins_bases[ins_off[e] .. ins_off[e+1])
  const char* ins_bases;     // 16-byte aligned and readable up to the next multiple of MA_REC_LANE behind its last character, as seq is
  // The depth codes: last, since only the tally and the profile read them
  const char* smp;           // [col_off[n]] beside seq, aligned and readable as seq is
};

struct MaRecWord { uint32_t w[4]; };
MIA_HD inline MaRecWord ma_rec_load(const char* p) {         // (p: 16-byte aligned)
  MaRecWord x;
  __builtin_memcpy(&x, __builtin_assume_aligned(p, 16), sizeof x);
  return x;
}

// aln_seq->ins[pos]: read_ma lets a later pair of the same position replace an earlier one (src/map_alignment.c:602-605).
// The record's pairs are in ascending position and those of one position in the order they were given, so the pair that
// counts is the last one listed for `pos`: found by bisection however many there are.  Returns the length of its characters
// (0 and *bases = nullptr when the record has no pair there).
MIA_HD inline int ma_rec_insert(const MaRecords& v, int64_t r, int32_t pos, const char** bases) {
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

// Does the pair listed at ins_list[k] count, for one who walks the list of a record of `ncols` columns whose pairs end at
// `hi` = rec_ins[r + 1]: its position lies inside the record and it is the last pair listed for that position.
MIA_HD inline bool ma_rec_pair_counts(const MaRecords& v, int32_t k, int32_t hi, int64_t ncols) {
  const int32_t pos = v.ins_pos[v.ins_list[k]];
  return pos >= 0 && pos < ncols && (k + 1 == hi || v.ins_pos[v.ins_list[k + 1]] != pos);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// A record's pairs list[0 .. count) into ascending position, pairs of one position staying in the order they were given (so
// that the last one given is the last one listed); what mia writes is in that order already.
inline void ma_ace_order_inserts(int32_t* list, int32_t count, const int32_t* ins_pos) {
  bool sorted = true;
  for (int32_t k = 1; k < count && sorted; k++) sorted = ins_pos[list[k - 1]] <= ins_pos[list[k]];
  if (!sorted) std::stable_sort(list, list + count, [ins_pos](int32_t a, int32_t b) { return ins_pos[a] < ins_pos[b]; });
}

// rec_ins [n+1] and ins_list [n_ins] of MaRecords from the pairs' record numbers (each in 0 .. n-1): a stable counting sort of
// the pair numbers by record, then ma_ace_order_inserts inside every record.
inline void ma_list_pairs(int64_t n, int64_t n_ins, const int32_t* ins_record, const int32_t* ins_pos, std::vector<int32_t>* rec_ins,
                          std::vector<int32_t>* ins_list) {
  rec_ins->assign((size_t)n + 1, 0);
  ins_list->assign((size_t)n_ins, 0);
  for (int64_t e = 0; e < n_ins; e++) (*rec_ins)[(size_t)ins_record[e] + 1]++;
  for (int64_t r = 0; r < n; r++) (*rec_ins)[(size_t)r + 1] += (*rec_ins)[(size_t)r];
  std::vector<int32_t> cursor(rec_ins->begin(), rec_ins->end() - 1);
  for (int64_t e = 0; e < n_ins; e++) (*ins_list)[(size_t)cursor[(size_t)ins_record[e]]++] = (int32_t)e;
  for (int64_t r = 0; r < n; r++)
    ma_ace_order_inserts(ins_list->data() + (*rec_ins)[(size_t)r], (*rec_ins)[(size_t)r + 1] - (*rec_ins)[(size_t)r], ins_pos);
}

}  // namespace mia
