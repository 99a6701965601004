// mia_ma_dedup_kernels.h -- the duplicate filter (ma_hip -u, -t; mia_hip_ma_dedup) on the device.  What one record, molecule
// or run yields is in ma_dedup_body.h; this file is the data movement around it.  Six timed stages, all on the context's stream:
//
// k_ma_dedup_keys      a lane per record: the molecule's 64-bit key (ma_dedup_record_key; the back half of a pair and an orphan get
//                      MA_DEDUP_NO_KEY, which sorts behind every key) and the record's number as the value; an orphan's keep and rep.
// k_ma_dedup_sort      a stable LSD radix sort of the (key, record) pairs over the 2 W + 1 bits that L needs, 8 bits a pass and three
//                      launches a pass: counts per workgroup and digit, one workgroup that scans the 256 x workgroups table digit by
//                      digit, and the scatter.  A workgroup owns 2 048 consecutive entries and goes through them in tiles of 256.  The
//                      lanes of a wavefront that hold the same digit find each other with eight ballots (mad_match): the lowest of them
//                      posts their count, each takes its rank among them, so a pile of equal keys costs one LDS word per wavefront, not
//                      one atomic per entry, and the order of equal digits -- tile, wavefront, lane -- is the order they came in.
// k_ma_dedup_runs      head flags by comparing neighbours, run numbers by the ordered scan of ma_scan_dev.h (a workgroup's place is
//                      its ticket), the first entry and the key of every run, and the run's best molecule: a segmented max over the
//                      workgroup's 256 packed (score, ~index) words in LDS, then ONE 64-bit atomic max per workgroup and run -- a
//                      pile of 70 000 molecules on one key is 274 atomics, not 70 000.
// k_ma_dedup_next      a lane per run: the first later run that is no duplicate (ma_dedup_next), a forward walk that ends at the
//                      first run outside the tolerance; t = 0 walks one step like any other.  Run 0 is marked.
// k_ma_dedup_anchors   pointer doubling, ceil(log2(runs)) launches: every marked run marks jump[k], then jump is squared into the
//                      other of two buffers.  A mark written in the same launch may or may not be seen; either way only runs of the
//                      orbit of run 0 are ever marked, and after round j all of them within 2^(j+1) steps are.
// k_ma_dedup_clusters  the ordered scan again, over the marks: a run's cluster number and the anchor run of every cluster.  Runs of a
//                      cluster are consecutive, so a cluster's size is the distance between the first entries of two anchor runs and no
//                      sum is needed; the histogram goes through a copy per wavefront in LDS (ma_wave_bins.h); keep and rep are
//                      scattered to the records of every molecule.
//
// No workgroup waits for another except inside ma_scan_before.  No scratch; vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_dedup_body.h"
#include "ma_scan_dev.h"
#include "ma_wave_bins.h"

namespace mia {

constexpr int MAD_THREADS = 256, MAD_WAVES = MAD_THREADS / 64;
constexpr int MAD_SORT_TILES = 8, MAD_SORT_CHUNK = MAD_THREADS * MAD_SORT_TILES;   // entries of one workgroup of a sort pass
constexpr int MAD_RADIX = 256;
constexpr int MAD_WGS_PER_CU = 8;           // grid-stride kernels: at most this many workgroups per compute unit

MIA_HD inline int64_t ma_dedup_wgs(int64_t n) { return (n + MAD_THREADS - 1) / MAD_THREADS; }
MIA_HD inline int64_t ma_dedup_sort_wgs(int64_t n) { return (n + MAD_SORT_CHUNK - 1) / MAD_SORT_CHUNK; }

__device__ __forceinline__ uint32_t mad_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint64_t mad_below(uint32_t lane) { return (1ull << lane) - 1; }

// the lanes of this wavefront that are valid and hold the same 8-bit digit as this one (every lane of the wavefront calls it)
__device__ __forceinline__ uint64_t mad_match(uint32_t digit, bool valid) {
  uint64_t peers = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (digit >> b) & 1u;
    const uint64_t m = __builtin_amdgcn_ballot_w64(bit);
    peers &= bit ? m : ~m;
  }
  return peers;
}

__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_keys(int64_t n, int32_t L, int W, const int32_t* start, const int32_t* end, const uint8_t* revcom,
                                                               const int64_t* mate, unsigned long long* key, uint32_t* val, uint8_t* keep, int64_t* rep) {
  for (int64_t r = (int64_t)blockIdx.x * MAD_THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * MAD_THREADS) {
    key[r] = ma_dedup_record_key(L, W, start, end, revcom, mate, r);
    val[r] = (uint32_t)r;
    if (mate && mate[r] == MA_DEDUP_ORPHAN) { keep[r] = 1; rep[r] = r; }
  }
}

// counts[digit * n_wgs + workgroup] = entries of the workgroup's chunk with that digit
__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_sort_count(const unsigned long long* key, int64_t n, int shift, uint32_t* counts, int64_t n_wgs) {
  __shared__ uint32_t s_cnt[MAD_RADIX];
  const int tid = threadIdx.x;
  const uint32_t lane = mad_lane();
  s_cnt[tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * MAD_SORT_CHUNK;
  for (int tile = 0; tile < MAD_SORT_TILES; tile++) {
    const int64_t i = base + tile * MAD_THREADS + tid;
    const bool valid = i < n;
    const uint32_t digit = valid ? (uint32_t)(key[i] >> shift) & 255u : 0u;
    const uint64_t peers = mad_match(digit, valid);
    if (valid && (peers & mad_below(lane)) == 0) atomicAdd(&s_cnt[digit], (uint32_t)__popcll(peers));
  }
  __syncthreads();
  counts[(int64_t)tid * n_wgs + blockIdx.x] = s_cnt[tid];
}

// exclusive scan of the table in place, digit-major: one workgroup, a contiguous stretch per thread
__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_sort_scan(uint32_t* counts, int64_t total) {
  __shared__ uint32_t s_sum[2][MAD_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = (total + MAD_THREADS - 1) / MAD_THREADS;
  int64_t lo = per * tid, hi = lo + per;
  if (lo > total) lo = total;
  if (hi > total) hi = total;
  uint32_t sum = 0;
  for (int64_t i = lo; i < hi; i++) sum += counts[i];
  s_sum[0][tid] = sum;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < MAD_THREADS; d <<= 1) {
    uint32_t x = s_sum[cur][tid];
    if (tid >= d) x += s_sum[cur][tid - d];
    s_sum[cur ^ 1][tid] = x;
    __syncthreads();
    cur ^= 1;
  }
  uint32_t run = s_sum[cur][tid] - sum;
  for (int64_t i = lo; i < hi; i++) { const uint32_t c = counts[i]; counts[i] = run; run += c; }
}

__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_sort_scatter(const unsigned long long* key_in, const uint32_t* val_in, unsigned long long* key_out,
                                                                       uint32_t* val_out, int64_t n, int shift, const uint32_t* offsets, int64_t n_wgs) {
  __shared__ uint32_t s_base[MAD_RADIX];
  __shared__ uint32_t s_cnt[MAD_WAVES][MAD_RADIX];
  const int tid = threadIdx.x, wave = tid >> 6;
  const uint32_t lane = mad_lane();
  s_base[tid] = offsets[(int64_t)tid * n_wgs + blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * MAD_SORT_CHUNK;
  for (int tile = 0; tile < MAD_SORT_TILES; tile++) {
#pragma unroll
    for (int w = 0; w < MAD_WAVES; w++) s_cnt[w][tid] = 0;
    __syncthreads();
    const int64_t i = base + tile * MAD_THREADS + tid;
    const bool valid = i < n;
    const unsigned long long k = valid ? key_in[i] : 0ull;
    const uint32_t v = valid ? val_in[i] : 0u;
    const uint32_t digit = (uint32_t)(k >> shift) & 255u;
    const uint64_t peers = mad_match(digit, valid);
    const uint32_t rank = (uint32_t)__popcll(peers & mad_below(lane));
    if (valid && rank == 0) s_cnt[wave][digit] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t off = s_base[digit] + rank;
      for (int w = 0; w < wave; w++) off += s_cnt[w][digit];
      // off < n is an invariant (the offsets are the scan of the counts of these very keys); the test only keeps a store inside the
      // buffer should it ever break: a wrong result that the tests catch, not a write outside the allocation
      if ((int64_t)off < n) { key_out[off] = k; val_out[off] = v; }
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (int w = 0; w < MAD_WAVES; w++) add += s_cnt[w][tid];
    s_base[tid] += add;
  }
}

// The ordered scan of one flag per thread that the runs and the clusters share: the number of flags in front of this thread over the
// whole launch plus its own (an inclusive count), and the launch's total in *total for the last place.  t: the workgroup's ticket.
__device__ __forceinline__ unsigned long long mad_ordered_count(bool flag, unsigned long long* ctl, int64_t t, int32_t n_wgs, uint32_t* s_wsum,
                                                                unsigned long long* s_before, unsigned long long* total) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const uint32_t lane = mad_lane();
  const uint64_t b = __builtin_amdgcn_ballot_w64(flag);
  if (lane == 0) s_wsum[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  if (tid == 0) {
    unsigned long long own = 0;
    for (int w = 0; w < MAD_WAVES; w++) own += s_wsum[w];
    *s_before = ma_scan_before(ctl, t, n_wgs, own);
  }
  __syncthreads();
  unsigned long long incl = *s_before + (unsigned long long)__popcll(b & mad_below(lane)) + (flag ? 1u : 0u);
  unsigned long long all = *s_before;
  for (int w = 0; w < MAD_WAVES; w++) { if (w < wave) incl += s_wsum[w]; all += s_wsum[w]; }
  *total = all;
  return incl;
}

// sk, sm: the sorted keys and records, the first M of them molecules.  Launched with exactly n_wgs = ma_dedup_wgs(M) workgroups; ctl
// (MAR_STATE + n_wgs words) and best (M words) are zero.
__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_runs(const unsigned long long* sk, const uint32_t* sm, int64_t M, const int32_t* score,
                                                               const int64_t* mate, unsigned long long* ctl, int32_t n_wgs, uint32_t* run_id,
                                                               uint32_t* run_first, unsigned long long* run_key, unsigned long long* best) {
  __shared__ long long s_t;
  __shared__ unsigned long long s_before;
  __shared__ uint32_t s_wsum[MAD_WAVES];
  __shared__ unsigned long long s_val[2][MAD_THREADS];
  __shared__ uint32_t s_run[MAD_THREADS];
  const int tid = threadIdx.x;
  if (tid == 0) s_t = (long long)ma_scan_ticket(ctl);
  __syncthreads();
  const int64_t t = s_t;
  if (t >= n_wgs) return;
  const int64_t i = t * MAD_THREADS + tid;
  const bool valid = i < M;
  const unsigned long long k = valid ? sk[i] : 0ull;
  const bool head = valid && (i == 0 || sk[i - 1] != k);
  unsigned long long total = 0;
  const unsigned long long incl = mad_ordered_count(head, ctl, t, n_wgs, s_wsum, &s_before, &total);
  const uint32_t run = (uint32_t)(incl - 1);              // (a valid entry has a head at or in front of it)
  if (valid) run_id[i] = run;
  if (head) { run_first[run] = (uint32_t)i; run_key[run] = k; }
  if (t == n_wgs - 1 && tid == 0) run_first[total] = (uint32_t)M;
  // the best molecule of every run, as far as it lies in this workgroup
  unsigned long long v = 0;
  if (valid) { const int64_t f = sm[i]; v = ma_dedup_pack(score[f], ma_dedup_index(mate, f)); }
  s_run[tid] = valid ? run : 0xffffffffu;
  s_val[0][tid] = v;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < MAD_THREADS; d <<= 1) {
    unsigned long long x = s_val[cur][tid];
    if (tid >= d && s_run[tid - d] == s_run[tid]) { const unsigned long long y = s_val[cur][tid - d]; x = y > x ? y : x; }
    s_val[cur ^ 1][tid] = x;
    __syncthreads();
    cur ^= 1;
  }
  if (valid && (tid == MAD_THREADS - 1 || s_run[tid + 1] != run)) atomicMax(&best[run], s_val[cur][tid]);
}

// jump[k] for k = 0 .. R (jump[R] = R), mark[k] = (k == 0)
__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_next(const unsigned long long* run_key, int64_t R, int W, int32_t tol, uint32_t* jump, uint32_t* mark) {
  for (int64_t k = (int64_t)blockIdx.x * MAD_THREADS + threadIdx.x; k <= R; k += (int64_t)gridDim.x * MAD_THREADS) {
    if (k == R) { jump[k] = (uint32_t)R; continue; }
    jump[k] = (uint32_t)ma_dedup_next((const uint64_t*)run_key, R, k, W, tol);
    mark[k] = k == 0 ? 1u : 0u;
  }
}

__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_double(const uint32_t* jump_in, uint32_t* jump_out, uint32_t* mark, int64_t R) {
  for (int64_t k = (int64_t)blockIdx.x * MAD_THREADS + threadIdx.x; k <= R; k += (int64_t)gridDim.x * MAD_THREADS) {
    uint32_t j = jump_in[k];
    if ((int64_t)j > R) j = (uint32_t)R;
    if (k < R && (int64_t)j < R && mark[k]) mark[j] = 1u;
    jump_out[k] = jump_in[j];
  }
}

// cluster numbers of the runs and the anchor run of every cluster (anchor[C] = R); exactly n_wgs = ma_dedup_wgs(R) workgroups, ctl zero
__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_cluster_scan(const uint32_t* mark, int64_t R, unsigned long long* ctl, int32_t n_wgs,
                                                                       uint32_t* cluster_of, uint32_t* anchor) {
  __shared__ long long s_t;
  __shared__ unsigned long long s_before;
  __shared__ uint32_t s_wsum[MAD_WAVES];
  const int tid = threadIdx.x;
  if (tid == 0) s_t = (long long)ma_scan_ticket(ctl);
  __syncthreads();
  const int64_t t = s_t;
  if (t >= n_wgs) return;
  const int64_t k = t * MAD_THREADS + tid;
  const bool valid = k < R;
  const bool flag = valid && mark[k] != 0;
  unsigned long long total = 0;
  const unsigned long long incl = mad_ordered_count(flag, ctl, t, n_wgs, s_wsum, &s_before, &total);
  if (valid) cluster_of[k] = (uint32_t)(incl - 1);        // (run 0 is an anchor)
  if (flag) anchor[incl - 1] = (uint32_t)k;
  if (t == n_wgs - 1 && tid == 0) anchor[total] = (uint32_t)R;
}

// the histogram of cluster sizes per strand; ctl[MAR_ROWS] holds the number of clusters
__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_hist(const uint32_t* anchor, const unsigned long long* ctl, const uint32_t* run_first,
                                                               const unsigned long long* run_key, int W, unsigned long long* hist) {
  __shared__ uint32_t s_bins[MAD_WAVES][MA_DEDUP_HIST];
  const int tid = threadIdx.x;
  uint32_t* const mine = ma_wave_bins_mine(s_bins);
  ma_wave_bins_zero(s_bins);
  const int64_t C = (int64_t)ctl[MAR_ROWS];
  for (int64_t c = (int64_t)blockIdx.x * MAD_THREADS + tid; c < C; c += (int64_t)gridDim.x * MAD_THREADS) {
    const uint32_t ka = anchor[c], kb = anchor[c + 1];
    const int64_t size = (int64_t)run_first[kb] - (int64_t)run_first[ka];
    atomicAdd(&mine[ma_dedup_size_bin(ma_dedup_key_forward(run_key[ka], W), size)], 1u);
  }
  ma_wave_bins_flush(s_bins, hist);
}

// keep and rep of the records of every molecule
__global__ __launch_bounds__(MAD_THREADS) void k_ma_dedup_scatter(const uint32_t* sm, int64_t M, const uint32_t* run_id, const uint32_t* cluster_of,
                                                                  const uint32_t* anchor, const unsigned long long* best, const int64_t* mate, uint8_t* keep,
                                                                  int64_t* rep) {
  for (int64_t i = (int64_t)blockIdx.x * MAD_THREADS + threadIdx.x; i < M; i += (int64_t)gridDim.x * MAD_THREADS) {
    const int64_t f = sm[i];
    const int64_t r = ma_dedup_packed_index(best[anchor[cluster_of[run_id[i]]]]);
    const uint8_t kp = ma_dedup_index(mate, f) == r ? 1 : 0;
    keep[f] = kp;
    rep[f] = r;
    const int64_t m = mate ? mate[f] : MA_DEDUP_NONE;
    if (m >= 0) { keep[m] = kp; rep[m] = r; }
  }
}

}  // namespace mia
