// mia_ma_region_kernels.h -- ma's region view (-f 6 / -f 61; print_region, reference src/map_align.c:543-759) over the
// records mia_hip_ma_tally left on the device.  Two launches:
//   k_ma_region_select   the records that overlap the region, in record order (ordered compaction: a scan of the
//                        workgroups' counts by look-back, no atomic append), and beside them the region's column map
//   k_ma_region_render   one wavefront per selected record, lanes over the region's columns; bytes gathered and stored,
//                        nothing else
// What a record's row holds is ma_region_body.h, shared with the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mia_layout.h"
#include "ma_region_body.h"

namespace mia {

constexpr int MAR_THREADS = 256, MAR_ITEMS = 4, MAR_PER_WG = MAR_THREADS * MAR_ITEMS;
// the select launch's words (64 bits each): arrival tickets, number of rows, width of a row, then one state per workgroup
constexpr int MAR_TICKET = 0, MAR_ROWS = 1, MAR_WIDTH = 2, MAR_STATE = 4;
// state of workgroup t: its own count (MAR_OWN) or the count of workgroups 0 .. t (MAR_UPTO) in the low 62 bits
constexpr unsigned long long MAR_OWN = 1ull << 62, MAR_UPTO = 2ull << 62, MAR_VALUE = (1ull << 62) - 1;

// Workgroups take their place by ticket, so a workgroup only ever waits for workgroups that already run.  Tickets
// 0 .. n_wgs - 1 select MAR_PER_WG records each; ticket n_wgs writes the column map.
__global__ __launch_bounds__(MAR_THREADS) void k_ma_region_select(MaRegionView v, int32_t n_wgs, unsigned long long* ctl, int64_t* colmap,
                                                                   int64_t* rows) {
  __shared__ unsigned long long s_first;
  __shared__ long long s_part[MAR_THREADS];
  __shared__ int s_cnt[MAR_ITEMS * (MAR_THREADS / 64)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_first = atomicAdd(&ctl[MAR_TICKET], 1ull);
  __syncthreads();
  const int64_t t = (int64_t)s_first;
  if (t >= n_wgs) {
    // column map: colmap[k] = sum over q < k of gaps[first + q] + 1; a run of columns per thread, the runs' sums scanned by one
    if (t > n_wgs || v.first > v.last) return;
    const int64_t ncol = (int64_t)v.last - v.first + 1, per = (ncol + MAR_THREADS - 1) / MAR_THREADS;
    const int64_t k0 = tid * per < ncol ? tid * per : ncol, k1 = k0 + per < ncol ? k0 + per : ncol;
    long long sum = 0;
    for (int64_t k = k0; k < k1; k++) sum += ma_region_gap(v.gaps[v.first + k]) + 1;
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      long long run = 0;
      for (int i = 0; i < MAR_THREADS; i++) { const long long x = s_part[i]; s_part[i] = run; run += x; }
      colmap[ncol] = run;
      ctl[MAR_WIDTH] = (unsigned long long)run;
    }
    __syncthreads();
    long long at = s_part[tid];
    for (int64_t k = k0; k < k1; k++) { colmap[k] = at; at += ma_region_gap(v.gaps[v.first + k]) + 1; }
    return;
  }
  bool take[MAR_ITEMS];
  int rank[MAR_ITEMS];
#pragma unroll
  for (int i = 0; i < MAR_ITEMS; i++) {
    const int64_t r = t * MAR_PER_WG + i * MAR_THREADS + tid;
    take[i] = r < v.n && ma_region_overlaps(v.start[r], ma_region_end(v, r), v.first, v.last);
    const unsigned long long m = __ballot(take[i]);
    rank[i] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[i * (MAR_THREADS / 64) + wave] = __popcll(m);
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long own = 0, before = 0;
    for (int i = 0; i < MAR_ITEMS * (MAR_THREADS / 64); i++) own += (unsigned long long)s_cnt[i];
    unsigned long long* state = ctl + MAR_STATE;
    if (t > 0) {
      __hip_atomic_store(&state[t], MAR_OWN | own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int64_t j = t - 1;;) {              // (workgroup 0 publishes MAR_UPTO and nothing else: j never passes it)
        const unsigned long long x = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((x & ~MAR_VALUE) == 0) { __builtin_amdgcn_s_sleep(1); continue; }
        before += x & MAR_VALUE;
        if ((x & ~MAR_VALUE) == MAR_UPTO) break;
        j--;
      }
    }
    __hip_atomic_store(&state[t], MAR_UPTO | (before + own), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == n_wgs - 1) ctl[MAR_ROWS] = before + own;
    s_first = before;
  }
  __syncthreads();
  const int64_t base = (int64_t)s_first;
#pragma unroll
  for (int i = 0; i < MAR_ITEMS; i++) {
    if (!take[i]) continue;
    int64_t at = base + rank[i];
    for (int j = 0; j < i * (MAR_THREADS / 64) + wave; j++) at += s_cnt[j];
    rows[at] = t * MAR_PER_WG + i * MAR_THREADS + tid;
  }
}

// text[i * width ..): the row of record rows[i].  v.colmap is the map the select launch wrote.
__global__ __launch_bounds__(MAR_THREADS) void k_ma_region_render(MaRegionView v, const int64_t* rows, int64_t n_rows, int64_t width, char* text) {
  const int64_t i = (int64_t)blockIdx.x * (MAR_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= n_rows) return;
  ma_region_row(v, rows[i], text + i * width, (int)(threadIdx.x & 63), 64);
}

}  // namespace mia
