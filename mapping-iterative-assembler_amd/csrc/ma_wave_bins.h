// ma_wave_bins.h -- the histogram of the ma kernels: every wavefront of a workgroup counts into its own copy of BINS 32-bit words in
// LDS, so wavefronts never contend with each other and no event reaches global memory before the flush; the flush sums the copies per
// bin and adds what is not zero to the int64 result with one 64-bit vector atomic per bin and workgroup -- integer adds: the result
// does not depend on the grid or on the order of the events.  The array, __shared__ uint32_t s_bins[WAVES][BINS], is declared in the
// kernel, so that a kernel's LDS stays visible there; WAVES and BINS are read off its type, and the workgroup has WAVES * 64 threads.
// A 32-bit word holds while a wavefront adds fewer than 2^32 events to a bin between zero and flush: every kernel says why it does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mia {

// every copy to zero; ends on a barrier
template <int WAVES, int BINS>
__device__ __forceinline__ void ma_wave_bins_zero(uint32_t (&s_bins)[WAVES][BINS]) {
  for (int b = threadIdx.x; b < WAVES * BINS; b += WAVES * 64) (&s_bins[0][0])[b] = 0;
  __syncthreads();
}

// the calling wavefront's own copy
template <int WAVES, int BINS>
__device__ __forceinline__ uint32_t* ma_wave_bins_mine(uint32_t (&s_bins)[WAVES][BINS]) { return s_bins[threadIdx.x >> 6]; }

// begins on a barrier; out[b] += the copies' sum for every bin b whose sum is not zero
template <int WAVES, int BINS>
__device__ __forceinline__ void ma_wave_bins_flush(uint32_t (&s_bins)[WAVES][BINS], unsigned long long* out) {
  __syncthreads();
  for (int b = threadIdx.x; b < BINS; b += WAVES * 64) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) sum += s_bins[w][b];
    if (sum) atomicAdd(&out[b], sum);
  }
}

// A whole kernel of the simplest shape, a RECORD PER LANE over a persistent grid: record(r, count) is called for every r < n and
// calls count(bin) for every event.
template <int WAVES, int BINS, class Record>
__device__ __forceinline__ void ma_wave_bins_records(uint32_t (&s_bins)[WAVES][BINS], int64_t n, unsigned long long* out, Record&& record) {
  constexpr int THREADS = WAVES * 64;
  uint32_t* const mine = ma_wave_bins_mine(s_bins);
  ma_wave_bins_zero(s_bins);
  for (int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * THREADS)
    record(r, [&](int bin) { atomicAdd(&mine[bin], 1u); });
  ma_wave_bins_flush(s_bins, out);
}

}  // namespace mia
