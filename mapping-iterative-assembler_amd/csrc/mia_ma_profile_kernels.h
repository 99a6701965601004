// mia_ma_profile_kernels.h -- the substitution profile (ma_hip -f 9, -f 91) over the records mia_hip_ma_tally left on the device.
// One launch, k_ma_profile, over the FLAT columns: the records' SEQ and SMP strings lie end to end (col_off), flat position x is
// one column event.  A lane takes a stretch of MA_PROF_LANE = 16 positions at a time (the shared walk: ma_flat_body.h, with the
// profile's rule ma_prof_stretch, ma_profile_body.h); a wavefront takes 1 024 consecutive positions, a workgroup 4 096, the grid
// strides over the workgroup chunks.
//
// HISTOGRAM.  808 bins (count[31][5][5] | del[31] | bad_code | beyond), filled very unevenly: in a real assembly most events are
// (MIDDLE, X, X).  Those four bins never touch memory in the loop: per position a ballot per bin and a population count into a
// wave-uniform register (MA_PROF_HOT counters per wavefront).  Every other event is one LDS atomic on the wavefront's own copy of
// the bins (ma_wave_bins.h: 4 copies of 808 words, 12.6 KiB per workgroup), so a wavefront's lanes contend only where they hit the
// same rare bin at the same step.
// WIDTH.  The LDS words and the hot counters are 32-bit.  A wavefront adds at most 1 024 events per chunk and a workgroup flushes
// after at most MAP_FLUSH_CHUNKS = 2^20 chunks: no word exceeds 2^30 between flushes.  (With a grid of g workgroups that is
// reached from T = g * 2^32 flat positions on.)
// FLUSH.  ma_wave_bins_flush, followed by a barrier where the copies are zeroed again for the next MAP_FLUSH_CHUNKS chunks.
// No scratch (the 16 positions are four unrolled words of four characters each, all in registers), no launch but this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_profile_body.h"
#include "ma_wave_bins.h"

namespace mia {

constexpr int MAP_THREADS = 256, MAP_WAVES = MAP_THREADS / 64;
constexpr int MAP_WAVE_COLS = 64 * MA_PROF_LANE, MAP_WG_COLS = MAP_THREADS * MA_PROF_LANE;        // 1 024, 4 096
constexpr int64_t MAP_FLUSH_CHUNKS = (int64_t)1 << 20;
constexpr int MAP_WGS_PER_CU = 4;          // persistent grid: at most this many workgroups per compute unit

MIA_HD inline int64_t ma_prof_chunks(int64_t T) { return (T + MAP_WG_COLS - 1) / MAP_WG_COLS; }

__global__ __launch_bounds__(MAP_THREADS) void k_ma_profile(MaFlatView v, unsigned long long* out) {
  __shared__ uint32_t s_bins[MAP_WAVES][MA_PROF_BINS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* const mine = ma_wave_bins_mine(s_bins);
  const int64_t n_chunks = ma_prof_chunks(v.T);
  int64_t c = blockIdx.x;
  while (c < n_chunks) {                                    // (c is the same in every thread of the workgroup)
    ma_wave_bins_zero(s_bins);
    uint32_t hot0 = 0, hot1 = 0, hot2 = 0, hot3 = 0;
    for (int64_t k = 0; k < MAP_FLUSH_CHUNKS && c < n_chunks; k++, c += gridDim.x) {
      const int64_t base = c * MAP_WG_COLS + (int64_t)tid * MA_PROF_LANE;
      if (c * MAP_WG_COLS + (int64_t)wave * MAP_WAVE_COLS >= v.T) continue;       // the whole wavefront lies behind T
      ma_prof_stretch(v, base, [&](int bin) {
        const int h = ma_prof_hot(bin);
        hot0 += (uint32_t)__popcll(__ballot(h == 0));
        hot1 += (uint32_t)__popcll(__ballot(h == 1));
        hot2 += (uint32_t)__popcll(__ballot(h == 2));
        hot3 += (uint32_t)__popcll(__ballot(h == 3));
        if (bin >= 0 && h < 0) atomicAdd(&mine[bin], 1u);
      });
    }
    if (lane == 0) {
      atomicAdd(&mine[ma_prof_hot_bin(0)], hot0);
      atomicAdd(&mine[ma_prof_hot_bin(1)], hot1);
      atomicAdd(&mine[ma_prof_hot_bin(2)], hot2);
      atomicAdd(&mine[ma_prof_hot_bin(3)], hot3);
    }
    ma_wave_bins_flush(s_bins, out);
    __syncthreads();
  }
}

}  // namespace mia
