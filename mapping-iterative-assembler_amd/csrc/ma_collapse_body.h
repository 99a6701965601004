// ma_collapse_body.h -- the duplicate consensus (ma_hip -u -j, -f 98; mia_hip_ma_collapse) as functions of one character, one voter,
// one column and one cluster.  The rule is this project's own (the reference's collapse_FSDB, src/mia.c:140-233, works on raw reads
// with qualities, which a .maln does not hold); DESIGN.md, "Duplicate consensus", states it in full and tests/ma_collapse_ref.py
// restates it.
//
// VOTERS.  The clusters, their representative and the sorted molecule order are those of the duplicate filter (ma_dedup_body.h); the
// members of a cluster are consecutive entries of that order.  Entry i names the molecule's whole or front record in the numbers the
// filter was given; rec_of turns those into the numbers of the tallied records (MaRecords), whose SEQ strings hold the votes.  A
// molecule votes at reference column p with its whole or front record if that covers p, otherwise with its back half if that does;
// a molecule whose whole or front record has vote == 0 votes nowhere (its column counts are 0 here: MaColVoter).
// CLASSES.  A, C, G, T and '-' in either case; every other character is no vote.  At the first and the last column of the
// representative's record '-' votes do not count (the edge flag of ma_col_decide).
// DECISION.  One class strictly ahead: the column becomes that class unless it is the representative's own; several ahead: the own
// character stays if it is one of them, else the column becomes N.  A column counts as changed only when its byte changes.
// CHUNKS.  The sorted order is cut into chunks of MA_COL_K entries, one wavefront each.  A cluster that lies inside one chunk is
// decided there; one that straddles a chunk boundary adds its counts to five words per column in a count array and is decided by a
// stage of its own (ma_col_straddles: the plan and the count stage must agree on it).
//
// Plain C++ behind MIA_HD.  The kernels of mia_ma_collapse_kernels.h call these per lane; tests/ma_collapse_driver.cpp runs the same
// functions in the same stages on the host against a serial walk.
#pragma once
#include <stdint.h>

#include "ma_dedup_body.h"
#include "ma_records.h"

namespace mia {

constexpr int MA_COL_K = 64;                               // members of one work unit: a chunk of the sorted order
constexpr int MA_COL_CLASSES = 5, MA_COL_NO_CLASS = 5;     // A C G T '-', and everything else
constexpr int MA_COL_SIZE_BINS = 6;                        // molecules in the cluster: 2, 3, 4, 5-8, 9-16, 17 and more
constexpr int MA_COL_CLUSTERS = 0, MA_COL_COLUMNS = 1, MA_COL_SPLIT = 2, MA_COL_TO_BASE = 3, MA_COL_TO_GAP = 4, MA_COL_TO_N = 5, MA_COL_COUNTS = 6;
constexpr int MA_COL_HIST = 2 * MA_COL_SIZE_BINS * MA_COL_COUNTS;      // [strand][size bin][count]
constexpr int64_t MA_COL_MAX_MEMBERS = 0x7fffffff;

MIA_HD inline int ma_col_class(char ch) {
  switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    case '-': return 4;
    default: return MA_COL_NO_CLASS;
  }
}
MIA_HD inline char ma_col_char(int cls) { return cls == 0 ? 'A' : cls == 1 ? 'C' : cls == 2 ? 'G' : cls == 3 ? 'T' : '-'; }

MIA_HD inline int ma_col_size_bin(int64_t size) { return size <= 4 ? (int)size - 2 : size <= 8 ? 3 : size <= 16 ? 4 : 5; }      // (size >= 2)
MIA_HD inline int ma_col_bin(bool revcom, int64_t size, int what) { return ((revcom ? 1 : 0) * MA_COL_SIZE_BINS + ma_col_size_bin(size)) * MA_COL_COUNTS + what; }

// does the cluster of sorted entries lo .. hi - 1 lie in more than one chunk
MIA_HD inline bool ma_col_straddles(int64_t lo, int64_t hi) { return lo / MA_COL_K != (hi - 1) / MA_COL_K; }
MIA_HD inline int64_t ma_col_chunks(int64_t M) { return (M + MA_COL_K - 1) / MA_COL_K; }

// What the collapse reads of the duplicate filter's results (all in the filter's own record numbers but rec_of and vote)
struct MaColDedup {
  int64_t M, C;                          // molecules, clusters
  const uint32_t* sm;                    // [M] the sorted order: the molecule's whole or front record
  const uint32_t* run_id;                // [M]
  const uint32_t* run_first;             // [R + 1]
  const uint32_t* cluster_of;            // [R]
  const uint32_t* anchor;                // [C + 1]
  const unsigned long long* best;        // [R]
  const int64_t* mate;                   // [n] or NULL
  const int32_t* start;                  // [n]
  const int32_t* rec_of;                 // [n] the tallied record of a filter's record, NULL: the same number
  const uint8_t* vote;                   // [n] per TALLIED record, NULL: everyone votes
};

MIA_HD inline int64_t ma_col_rec(const MaColDedup& d, int64_t f) { return d.rec_of ? d.rec_of[f] : f; }

// A molecule as a voter: START, columns and the place of the SEQ string of its whole or front record (F) and of its back half (B).
// No columns: that record votes nowhere.
struct MaColVoter { int32_t sF, nF, sB, nB; int64_t oF, oB; };

MIA_HD inline MaColVoter ma_col_voter(const MaRecords& v, const MaColDedup& d, int64_t i) {
  MaColVoter q{0, 0, 0, 0, 0, 0};
  const int64_t f = d.sm[i], F = ma_col_rec(d, f);
  if (d.vote && !d.vote[F]) return q;
  q.sF = v.start[F]; q.oF = v.col_off[F]; q.nF = (int32_t)(v.col_off[F + 1] - q.oF);
  const int64_t m = d.mate ? d.mate[f] : MA_DEDUP_NONE;
  if (m >= 0) {
    const int64_t B = ma_col_rec(d, m);
    q.sB = v.start[B]; q.oB = v.col_off[B]; q.nB = (int32_t)(v.col_off[B + 1] - q.oB);
  }
  return q;
}

// the class the voter casts at reference column p (no modulo: each half lies in 0 .. L - 1)
MIA_HD inline int ma_col_vote(const char* seq, const MaColVoter& q, int64_t p) {
  if (p >= q.sF && p < (int64_t)q.sF + q.nF) return ma_col_class(seq[q.oF + (p - q.sF)]);
  if (p >= q.sB && p < (int64_t)q.sB + q.nB) return ma_col_class(seq[q.oB + (p - q.sB)]);
  return MA_COL_NO_CLASS;
}

// Cluster c: its size in molecules and the tallied records of its representative (the front or whole one, and the back half or -1)
MIA_HD inline int64_t ma_col_cluster(const MaColDedup& d, int64_t c, int64_t* lo, int64_t* hi, int32_t* F, int32_t* B) {
  const uint32_t ka = d.anchor[c];
  *lo = d.run_first[ka];
  *hi = d.run_first[d.anchor[c + 1]];
  const int64_t idx = ma_dedup_packed_index(d.best[ka]), m = d.mate ? d.mate[idx] : MA_DEDUP_NONE;
  const int64_t front = m >= 0 && !ma_dedup_front(d.start, idx, m) ? m : idx;
  *F = (int32_t)ma_col_rec(d, front);
  *B = m >= 0 ? (int32_t)ma_col_rec(d, front == idx ? m : idx) : -1;
  return *hi - *lo;
}

MIA_HD inline uint32_t ma_col_pick(uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint32_t gap, int cls) {
  return cls == 0 ? a : cls == 1 ? c : cls == 2 ? g : cls == 3 ? t : gap;
}

// The decision for one column from the five counts, the representative's own character and the edge flag.  what: 0 = the byte stays,
// otherwise MA_COL_TO_BASE, MA_COL_TO_GAP or MA_COL_TO_N and `out` is the new byte.
struct MaColDecision { char out; bool voted, split; int what; };

MIA_HD inline MaColDecision ma_col_decide(uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint32_t gap, char own, bool edge) {
  if (edge) gap = 0;
  uint32_t top = a;
  if (c > top) top = c;
  if (g > top) top = g;
  if (t > top) top = t;
  if (gap > top) top = gap;
  MaColDecision d{own, top > 0, false, 0};
  if (top == 0) return d;
  const int classes = (a > 0) + (c > 0) + (g > 0) + (t > 0) + (gap > 0);
  const int ahead = (a == top) + (c == top) + (g == top) + (t == top) + (gap == top);
  d.split = classes > 1;
  const int mine = ma_col_class(own);
  if (ahead == 1) {
    const int win = a == top ? 0 : c == top ? 1 : g == top ? 2 : t == top ? 3 : 4;
    if (win == mine) return d;
    d.out = ma_col_char(win);
    d.what = win == 4 ? MA_COL_TO_GAP : MA_COL_TO_BASE;
    return d;
  }
  if (mine != MA_COL_NO_CLASS && ma_col_pick(a, c, g, t, gap, mine) == top) return d;
  if (own == 'N') return d;                                 // (a tie over an N: the byte stays, nothing is counted)
  d.out = 'N';
  d.what = MA_COL_TO_N;
  return d;
}

}  // namespace mia
