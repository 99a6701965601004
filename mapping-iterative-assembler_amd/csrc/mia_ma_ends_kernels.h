// mia_ma_ends_kernels.h -- fragment-end context (ma_hip -f 92) and read lengths (-f 93) over the records mia_hip_ma_tally left on
// the device.  One launch, k_ma_ends, a RECORD PER LANE (ma_ends_record, ma_ends_body.h): up to 40 characters of a reference that
// fits in cache for the two ends, the record's own columns in 16-byte words for its '-' count (a walk per record: the word that
// holds its first column to the word that holds its last, about ten loads for a read of 150), and its INS_POS pairs from the list
// by record that mia_hip_ma_tally already keeps (ascending position, so a pair counts when the next one has another position),
// their characters in the same 16-byte words.
//
// HISTOGRAM.  1 267 bins (ctx[2][20][6] | len[2][513] | halves), few and unevenly hit: a pile of duplicate reads puts every event
// of a wavefront into the same 41.  Every event is one LDS atomic on the wavefront's own copy of the bins (ma_wave_bins.h: 4 copies
// of 1 267 words, 19.8 KiB per workgroup).
// WIDTH.  The LDS words are 32-bit.  A record adds at most one event to a bin and mia_hip_ma_tally takes fewer than 2^31 records,
// so no word overflows however long the grid strides.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_ends_body.h"
#include "ma_wave_bins.h"

namespace mia {

constexpr int MAE_THREADS = 256, MAE_WAVES = MAE_THREADS / 64;
constexpr int MAE_WGS_PER_CU = 4;          // persistent grid: at most this many workgroups per compute unit

MIA_HD inline int64_t ma_ends_chunks(int64_t n) { return (n + MAE_THREADS - 1) / MAE_THREADS; }

__global__ __launch_bounds__(MAE_THREADS) void k_ma_ends(MaEndsView v, unsigned long long* out) {
  __shared__ uint32_t s_bins[MAE_WAVES][MA_ENDS_BINS];
  ma_wave_bins_records(s_bins, v.n, out, [&](int64_t r, auto&& count) { ma_ends_record(v, r, count); });
}

}  // namespace mia
