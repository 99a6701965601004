// mia_ma_region_kernels.h -- ma's region view (-f 6 / -f 61; print_region, reference src/map_align.c:543-759) over the
// records mia_hip_ma_tally left on the device.  Two launches:
//   k_ma_region_select   the records that overlap the region, in record order (ordered compaction: the scan of the
//                        workgroups' counts of ma_scan_dev.h), and beside them the region's column map
//   k_ma_region_render   one wavefront per selected record, lanes over the region's columns; bytes gathered and stored,
//                        nothing else
// What a record's row holds is ma_region_body.h, shared with the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mia_layout.h"
#include "ma_region_body.h"
#include "ma_scan_dev.h"

namespace mia {

constexpr int MAR_THREADS = 256, MAR_ITEMS = 4, MAR_PER_WG = MAR_THREADS * MAR_ITEMS;

// Workgroups take their place by ticket (ma_scan_dev.h; ctl[MAR_ROWS] = number of rows, ctl[MAR_WIDTH] = width of a row).  Tickets
// 0 .. n_wgs - 1 select MAR_PER_WG records each; ticket n_wgs writes the column map.
__global__ __launch_bounds__(MAR_THREADS) void k_ma_region_select(MaRegionView v, int32_t n_wgs, unsigned long long* ctl, int64_t* colmap,
                                                                   int64_t* rows) {
  __shared__ unsigned long long s_first;
  __shared__ long long s_part[MAR_THREADS];
  __shared__ int s_cnt[MAR_ITEMS * (MAR_THREADS / 64)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_first = ma_scan_ticket(ctl);
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
    unsigned long long own = 0;
    for (int i = 0; i < MAR_ITEMS * (MAR_THREADS / 64); i++) own += (unsigned long long)s_cnt[i];
    s_first = ma_scan_before(ctl, t, n_wgs, own);
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
