// mia_ma_ace_kernels.h -- the read blocks of ma's ACE export (-f 7; ace_output, reference src/io.c:756-913) over the records
// mia_hip_ma_tally left on the device.  Three launches:
//   k_ma_ace_gaps     G[p] = gaps[0] + .. + gaps[p-1] in 64 bits for p = 0 .. L + 1 (gaps[L] = 0), one workgroup: sum_of_gaps for
//                     every column at once
//   k_ma_ace_layout   per record its AF position, the length of its padded read and the bytes of its text; the records'
//                     offsets in the text buffer are an ordered scan of those bytes (the workgroups' sums by the scan of
//                     ma_scan_dev.h: the order of the records is the order of the output)
//   k_ma_ace_render   one wavefront per record, lanes over the bytes of its text (newlines included): every lane finds the
//                     column of its characters by bisection over G inside the record's span; whole 32-bit words are stored
//                     where the address allows
// What a record's text holds is ma_ace_body.h, shared with the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mia_ma_region_kernels.h"
#include "ma_ace_body.h"

namespace mia {

constexpr int MAA_SCAN_THREADS = 1024;

__global__ __launch_bounds__(MAA_SCAN_THREADS) void k_ma_ace_gaps(const int32_t* gaps, int32_t L, int64_t* G) {
  __shared__ long long s_part[MAA_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = ((int64_t)L + MAA_SCAN_THREADS - 1) / MAA_SCAN_THREADS;
  const int64_t p0 = tid * per < L ? tid * per : L, p1 = p0 + per < L ? p0 + per : L;
  long long sum = 0;
  for (int64_t p = p0; p < p1; p++) sum += gaps[p];
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < MAA_SCAN_THREADS; i++) { const long long x = s_part[i]; s_part[i] = run; run += x; }
    G[L] = run;
    G[(int64_t)L + 1] = run;
  }
  __syncthreads();
  long long at = s_part[tid];
  for (int64_t p = p0; p < p1; p++) { G[p] = at; at += gaps[p]; }
}

// Workgroups take their place by ticket (ma_scan_dev.h; ctl[MAR_ROWS] = bytes of the whole text).  Workgroup t lays out records
// t * MAR_PER_WG .., MAR_ITEMS consecutive records per thread.
__global__ __launch_bounds__(MAR_THREADS) void k_ma_ace_layout(MaAceView v, int32_t n_wgs, unsigned long long* ctl, int64_t* af_pos,
                                                                int64_t* padded_len, int64_t* body_off) {
  __shared__ unsigned long long s_first;
  __shared__ long long s_part[MAR_THREADS];
  const int tid = threadIdx.x;
  if (tid == 0) s_first = ma_scan_ticket(ctl);
  __syncthreads();
  const int64_t t = (int64_t)s_first;
  if (t >= n_wgs) return;
  long long bytes[MAR_ITEMS], sum = 0;
#pragma unroll
  for (int i = 0; i < MAR_ITEMS; i++) {
    const int64_t r = t * MAR_PER_WG + (int64_t)tid * MAR_ITEMS + i;
    bytes[i] = 0;
    if (r < v.n) {
      const MaAceRec q = ma_ace_rec(v, r);
      af_pos[r] = ma_ace_af_pos(q);
      padded_len[r] = q.len;
      bytes[i] = q.bytes;
    }
    sum += bytes[i];
  }
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    unsigned long long own = 0;
    for (int i = 0; i < MAR_THREADS; i++) { const long long x = s_part[i]; s_part[i] = (long long)own; own += (unsigned long long)x; }
    const unsigned long long before = ma_scan_before(ctl, t, n_wgs, own);
    if (t == n_wgs - 1) body_off[v.n] = (int64_t)(before + own);
    s_first = before;
  }
  __syncthreads();
  long long at = (long long)s_first + s_part[tid];
#pragma unroll
  for (int i = 0; i < MAR_ITEMS; i++) {
    const int64_t r = t * MAR_PER_WG + (int64_t)tid * MAR_ITEMS + i;
    if (r < v.n) body_off[r] = at;
    at += bytes[i];
  }
}

// body[body_off[r] ..): the text of record r
__global__ __launch_bounds__(MAR_THREADS) void k_ma_ace_render(MaAceView v, const int64_t* body_off, char* body) {
  const int64_t r = (int64_t)blockIdx.x * (MAR_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= v.n) return;
  ma_ace_body(v, r, body + body_off[r], (int)(threadIdx.x & 63), 64);
}

}  // namespace mia
