// mia_ma_collapse_kernels.h -- the duplicate consensus (ma_hip -u -j, -f 98; mia_hip_ma_collapse) on the device, over the records
// mia_hip_ma_tally left there and the sorted order, runs, clusters and anchors mia_hip_ma_dedup left there.  What one character, voter,
// column or cluster yields is in ma_collapse_body.h; this file is the data movement around it.  Three timed stages, all on the
// context's stream, launched only when the filter found a cluster of two or more molecules:
//
// k_ma_collapse_plan    first SEQ' = SEQ, sixteen bytes a lane (k_ma_collapse_copy).  Then a lane per cluster: its size, the tallied
//                       records of its representative (repF, repB), `members` of those records, the cluster counted into hist, and --
//                       for a cluster whose members lie in more than one chunk of MA_COL_K sorted entries -- the representative's
//                       columns as its own sum of the ordered scan of ma_scan_dev.h (a workgroup's place is its ticket): cnt_off[c] is
//                       where the cluster's five words per column begin in the count array, and the scan's total sizes that array (the
//                       host reads it back once).  Clusters inside one chunk add nothing, so cnt_off is monotone over all clusters.
// k_ma_collapse_count   a wavefront per chunk of MA_COL_K = 64 sorted entries, lane l holding entry l as a voter (MaColVoter: where
//                       its records' SEQ strings lie; no columns if it does not vote) and its cluster number.  The wavefront walks the
//                       clusters of its chunk; for one of two or more molecules its lanes run over the representative's columns, 64 at
//                       a time, and over the cluster's members inside the chunk, whose voters come out of the lanes' registers one by
//                       one (v_readlane), with five counters in registers per column.  A cluster inside the chunk is decided on the
//                       spot: the changed bytes are stored into SEQ' and the counts of the columns go through ballots into the
//                       wavefront's own copy of hist in LDS.  A cluster that straddles a boundary adds its non-zero counters with 32-bit
//                       vector atomics at cnt_off[c]: a pile of 70 000 copies on one key is 1 094 wavefronts, none of which waits.
// k_ma_collapse_decide  a lane per column of the count array: its cluster by bisecting cnt_off (the last cluster that begins at or in
//                       front of it), the five words, the decision, the byte, hist through LDS atomics.
//
// hist goes through the wavefronts' own copies in LDS (ma_wave_bins.h).  No workgroup waits for another except inside
// ma_scan_before.  No scratch; vector stores only; no inline assembly, no cooperative launch.  All counts are integer sums and every
// byte of SEQ' is written by the one lane that decides its column: the result does not depend on the grid or on the records' order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_collapse_body.h"
#include "ma_scan_dev.h"
#include "ma_wave_bins.h"

namespace mia {

constexpr int MAJ_THREADS = 256, MAJ_WAVES = MAJ_THREADS / 64;
constexpr int MAJ_WGS_PER_CU = 8;           // grid-stride kernels: at most this many workgroups per compute unit

MIA_HD inline int64_t ma_collapse_wgs(int64_t items) { return (items + MAJ_THREADS - 1) / MAJ_THREADS; }

__device__ __forceinline__ uint32_t maj_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ int32_t maj_from(int32_t x, int lane) { return __builtin_amdgcn_readlane(x, lane); }
__device__ __forceinline__ int64_t maj_from64(int64_t x, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)x, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)((uint64_t)x >> 32), lane);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint32_t maj_count(bool flag) { return (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(flag)); }

// SEQ' = SEQ: words = the 16-byte words of the string, its last one padded (both buffers are allocated that far)
__global__ __launch_bounds__(MAJ_THREADS) void k_ma_collapse_copy(const char* seq, char* out, int64_t words) {
  for (int64_t w = (int64_t)blockIdx.x * MAJ_THREADS + threadIdx.x; w < words; w += (int64_t)gridDim.x * MAJ_THREADS)
    reinterpret_cast<uint4*>(out)[w] = reinterpret_cast<const uint4*>(seq)[w];
}

// Launched with exactly n_wgs = ma_collapse_wgs(C) workgroups; ctl (MAR_STATE + n_wgs words), members and hist are zero.
__global__ __launch_bounds__(MAJ_THREADS) void k_ma_collapse_plan(MaRecords v, MaColDedup d, unsigned long long* ctl, int32_t n_wgs, int32_t* rep_f, int32_t* rep_b,
                                                                   int64_t* cnt_off, int32_t* members, unsigned long long* hist) {
  __shared__ unsigned long long s_first;
  __shared__ long long s_len[MAJ_THREADS];
  __shared__ uint32_t s_bins[MAJ_WAVES][MA_COL_HIST];
  const int tid = threadIdx.x;
  uint32_t* const mine = ma_wave_bins_mine(s_bins);
  if (tid == 0) s_first = ma_scan_ticket(ctl);
  ma_wave_bins_zero(s_bins);
  const int64_t t = (int64_t)s_first;
  if (t >= n_wgs) return;
  const int64_t c = t * MAJ_THREADS + tid;
  long long own = 0;
  if (c < d.C) {
    int64_t lo, hi;
    int32_t F, B;
    const int64_t size = ma_col_cluster(d, c, &lo, &hi, &F, &B);
    if (size >= 2) {
      const int32_t m = (int32_t)(size < MA_COL_MAX_MEMBERS ? size : MA_COL_MAX_MEMBERS);
      members[F] = m;
      if (B >= 0) members[B] = m;
      atomicAdd(&mine[ma_col_bin(v.revcom[F] != 0, size, MA_COL_CLUSTERS)], 1u);
      if (ma_col_straddles(lo, hi)) own = (v.col_off[F + 1] - v.col_off[F]) + (B >= 0 ? v.col_off[B + 1] - v.col_off[B] : 0);
    } else {
      F = B = -1;
    }
    rep_f[c] = F;
    rep_b[c] = B;
  }
  s_len[tid] = own;
  __syncthreads();
  if (tid == 0) {
    unsigned long long sum = 0;
    for (int i = 0; i < MAJ_THREADS; i++) { const long long x = s_len[i]; s_len[i] = (long long)sum; sum += (unsigned long long)x; }
    const unsigned long long before = ma_scan_before(ctl, t, n_wgs, sum);
    if (t == n_wgs - 1) cnt_off[d.C] = (int64_t)(before + sum);
    s_first = before;
  }
  __syncthreads();
  if (c < d.C) cnt_off[c] = (int64_t)s_first + s_len[tid];
  ma_wave_bins_flush(s_bins, hist);
}

// cnt: five words per column of the straddling clusters, zero; out: SEQ' (a copy of SEQ)
__global__ __launch_bounds__(MAJ_THREADS) void k_ma_collapse_count(MaRecords v, MaColDedup d, const int32_t* rep_f, const int32_t* rep_b, const int64_t* cnt_off,
                                                                    uint32_t* cnt, char* out, unsigned long long* hist) {
  __shared__ uint32_t s_bins[MAJ_WAVES][MA_COL_HIST];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)maj_lane();
  uint32_t* const mine = s_bins[wave];
  ma_wave_bins_zero(s_bins);
  const int64_t n_chunks = ma_col_chunks(d.M);
  for (int64_t g = (int64_t)blockIdx.x * MAJ_WAVES + wave; g < n_chunks; g += (int64_t)gridDim.x * MAJ_WAVES) {
    const int64_t g0 = g * MA_COL_K;
    const int held = (int)(d.M - g0 < MA_COL_K ? d.M - g0 : MA_COL_K);
    MaColVoter q{0, 0, 0, 0, 0, 0};
    int32_t cl = 0;
    if (lane < held) { q = ma_col_voter(v, d, g0 + lane); cl = (int32_t)d.cluster_of[d.run_id[g0 + lane]]; }
    for (int j = 0; j < held;) {
      const int64_t c = (uint32_t)maj_from(cl, j);
      const int64_t lo = d.run_first[d.anchor[c]], hi = d.run_first[d.anchor[c + 1]];
      int jend = (int)((hi < g0 + held ? hi : g0 + held) - g0);
      if (jend <= j) jend = j + 1;                            // (entry g0 + j lies in cluster c, so hi > g0 + j: the loop moves on whatever it reads)
      if (hi - lo >= 2) {
        const bool whole = !ma_col_straddles(lo, hi);
        const int32_t F = rep_f[c], B = rep_b[c];
        const int bin = ma_col_bin(v.revcom[F] != 0, hi - lo, 0);
        uint32_t n_cols = 0, n_split = 0, n_base = 0, n_gap = 0, n_N = 0;
        int64_t slot = whole ? 0 : cnt_off[c];
        for (int half = 0; half < 2; half++) {
          const int32_t R = half ? B : F;
          if (R < 0) continue;
          const int64_t sR = v.start[R], oR = v.col_off[R], n = v.col_off[R + 1] - oR;
          for (int64_t col0 = 0; col0 < n; col0 += 64) {
            const int64_t col = col0 + lane, p = sR + col;
            const bool active = col < n;
            uint32_t ca = 0, cc = 0, cg = 0, ct = 0, cgap = 0;
            for (int k = j; k < jend; k++) {
              const MaColVoter x{maj_from(q.sF, k), maj_from(q.nF, k), maj_from(q.sB, k), maj_from(q.nB, k), maj_from64(q.oF, k), maj_from64(q.oB, k)};
              if (!active) continue;
              const int cls = ma_col_vote(v.seq, x, p);
              ca += cls == 0; cc += cls == 1; cg += cls == 2; ct += cls == 3; cgap += cls == 4;
            }
            if (whole) {
              MaColDecision dec{0, false, false, 0};
              if (active) {
                dec = ma_col_decide(ca, cc, cg, ct, cgap, v.seq[oR + col], col == 0 || col == n - 1);
                if (dec.what) out[oR + col] = dec.out;
              }
              n_cols += maj_count(dec.voted); n_split += maj_count(dec.split); n_base += maj_count(dec.what == MA_COL_TO_BASE);
              n_gap += maj_count(dec.what == MA_COL_TO_GAP); n_N += maj_count(dec.what == MA_COL_TO_N);
            } else if (active) {
              uint32_t* const w = cnt + (slot + col) * MA_COL_CLASSES;
              if (ca) atomicAdd(w + 0, ca);
              if (cc) atomicAdd(w + 1, cc);
              if (cg) atomicAdd(w + 2, cg);
              if (ct) atomicAdd(w + 3, ct);
              if (cgap) atomicAdd(w + 4, cgap);
            }
          }
          slot += n;
        }
        if (whole && lane == 0) {                             // (the wavefront's own copy: no other wavefront touches it)
          mine[bin + MA_COL_COLUMNS] += n_cols; mine[bin + MA_COL_SPLIT] += n_split; mine[bin + MA_COL_TO_BASE] += n_base;
          mine[bin + MA_COL_TO_GAP] += n_gap; mine[bin + MA_COL_TO_N] += n_N;
        }
      }
      j = jend;
    }
  }
  ma_wave_bins_flush(s_bins, hist);
}

// Q = cnt_off[C]: the columns of the count array
__global__ __launch_bounds__(MAJ_THREADS) void k_ma_collapse_decide(MaRecords v, MaColDedup d, const int32_t* rep_f, const int32_t* rep_b, const int64_t* cnt_off,
                                                                     const uint32_t* cnt, int64_t Q, char* out, unsigned long long* hist) {
  __shared__ uint32_t s_bins[MAJ_WAVES][MA_COL_HIST];
  uint32_t* const mine = ma_wave_bins_mine(s_bins);
  ma_wave_bins_zero(s_bins);
  for (int64_t s = (int64_t)blockIdx.x * MAJ_THREADS + threadIdx.x; s < Q; s += (int64_t)gridDim.x * MAJ_THREADS) {
    int64_t lo = 0, hi = d.C;                                 // the last cluster with cnt_off[c] <= s: cnt_off[lo] <= s < cnt_off[hi]
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (cnt_off[mid] <= s) lo = mid; else hi = mid;
    }
    const int64_t c = lo;
    const int32_t F = rep_f[c], B = rep_b[c];
    if (F < 0) continue;                                      // (never: a column of the array belongs to a straddling cluster)
    int64_t col = s - cnt_off[c];
    const int64_t nF = v.col_off[F + 1] - v.col_off[F];
    int32_t R = F;
    if (col >= nF) { col -= nF; R = B; }
    if (R < 0) continue;
    const int64_t oR = v.col_off[R], n = v.col_off[R + 1] - oR;
    if (col >= n) continue;
    const uint32_t* const w = cnt + s * MA_COL_CLASSES;
    const MaColDecision dec = ma_col_decide(w[0], w[1], w[2], w[3], w[4], v.seq[oR + col], col == 0 || col == n - 1);
    if (dec.what) out[oR + col] = dec.out;
    const int64_t size = (int64_t)d.run_first[d.anchor[c + 1]] - (int64_t)d.run_first[d.anchor[c]];
    const int bin = ma_col_bin(v.revcom[F] != 0, size, 0);
    if (dec.voted) atomicAdd(&mine[bin + MA_COL_COLUMNS], 1u);
    if (dec.split) atomicAdd(&mine[bin + MA_COL_SPLIT], 1u);
    if (dec.what) atomicAdd(&mine[bin + dec.what], 1u);
  }
  ma_wave_bins_flush(s_bins, hist);
}

}  // namespace mia
