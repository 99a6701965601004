// mia_ma_pmd_kernels.h -- the damage score (ma_hip -L, -K, -S, -f 97) over the records mia_hip_ma_tally left on the device.  Two
// launches (ma_pmd_body.h holds what a lane does in either):
//
// k_ma_score_cols runs over the FLAT columns (the shared walk: ma_flat_body.h): a lane takes a stretch of MA_PMD_LANE = 16 positions at
// a time, a workgroup 4 096, the grid strides over those chunks.  The 775 words of the weight table are staged in LDS once per workgroup, in
// front of the chunks, so a column costs one LDS read on top of what the profile does with it.  A lane sums the weights of the record
// it is in in one register (|w| <= 2^20: sixteen of them stay inside int32) and sends the sum when the record changes and at the end
// of its stretch: at most one 64-bit vector atomic add per (lane, record) whose sum is NOT zero, into score[r], which only needs to be
// zeroed (one memset).  Integer adds: the result does not depend on the order in which lanes arrive.  With the model's table every C
// and G column carries a weight, so a long record gets an add from most of the lanes that cross it -- a sixteenth of its columns --,
// never one per column.  No scratch.
//
// k_ma_score_molecules runs a RECORD PER LANE: the lower-numbered record of a molecule adds the halves, decides keep against the
// threshold, stores S and keep to both records (plain vector stores: no other lane writes them) and adds the molecule to
// hist[strand][bin] -- with the orphan and kept-record counts 130 bins, one LDS atomic on the wavefront's own copy (ma_wave_bins.h: 4
// copies, 2 KiB per workgroup).  A record adds at most three events and mia_hip_ma_tally takes fewer than 2^31 records: a 32-bit LDS
// word does not overflow before the one flush.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_pmd_body.h"
#include "ma_wave_bins.h"

namespace mia {

constexpr int MAQ_THREADS = 256, MAQ_WAVES = MAQ_THREADS / 64;
constexpr int MAQ_WG_COLS = MAQ_THREADS * MA_PMD_LANE;     // 4 096
constexpr int MAQ_WGS_PER_CU = 4;          // persistent grids: at most this many workgroups per compute unit

MIA_HD inline int64_t ma_pmd_chunks(int64_t T) { return (T + MAQ_WG_COLS - 1) / MAQ_WG_COLS; }
MIA_HD inline int64_t ma_pmd_record_wgs(int64_t n) { return (n + MAQ_THREADS - 1) / MAQ_THREADS; }

__global__ __launch_bounds__(MAQ_THREADS) void k_ma_score_cols(MaFlatView v, const int32_t* __restrict__ w, unsigned long long* score) {
  __shared__ int32_t s_w[MA_PMD_WEIGHTS];
  for (int b = threadIdx.x; b < MA_PMD_WEIGHTS; b += MAQ_THREADS) s_w[b] = w[b];
  __syncthreads();
  const int64_t n_chunks = ma_pmd_chunks(v.T);
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x)
    ma_pmd_stretch(v, s_w, c * MAQ_WG_COLS + (int64_t)threadIdx.x * MA_PMD_LANE, [&](int64_t r, int32_t sum) {
      atomicAdd(&score[r], (unsigned long long)(int64_t)sum);          // (two's complement: a negative sum wraps to the right total)
    });
}

__global__ __launch_bounds__(MAQ_THREADS) void k_ma_score_molecules(MaPmdMolView v, unsigned long long* out) {
  __shared__ uint32_t s_bins[MAQ_WAVES][MA_PMD_BINS];
  ma_wave_bins_records(s_bins, v.n, out, [&](int64_t r, auto&& count) { ma_pmd_record(v, r, count); });
}

}  // namespace mia
