// mia_ma_cols_kernels.h -- the strand-split column table (ma_hip -f 42) over the records mia_hip_ma_tally left on the device: sixteen
// words per reference column (ma_cols_body.h).  One launch, k_ma_cols.
//
// TILES AND SLICES.  The reference is cut into tiles of MA_COLS_TILE columns and the records, in whatever order they were given, into
// n_slices stretches of per_slice records.  A workgroup takes one (tile, slice) job at a time (a persistent grid strides over them)
// and holds the tile's 16 x 512 words in LDS.  It scans its slice MAC_THREADS records at a time: every thread looks at START and the
// two offsets of one record -- a few bytes -- and, if the record has columns in the tile, lists that part of it in LDS (twelve bytes:
// where it begins in SEQ, how long it is, its first column in the tile, its strand); no sort is needed.  The thread adds the record's
// START and END events itself, to the tile that holds the anchor.  Then a wavefront per listed part walks it, lanes over adjacent
// aligned words of four columns, so a record of up to 256 columns is one load per lane.  EVERY EVENT IS ONE LDS ADD; an atomic one,
// since wavefronts meet on a word.  What lies on no reference column (`beyond`, `ends_outside`) is counted by the workgroups of tile
// 0, per thread, and added up once per job.
// WIDTH.  The LDS words are 32-bit: a record adds at most one event to a word and mia_hip_ma_tally takes fewer than 2^31 records.
// FLUSH.  Every word of the tile that is not zero is added to the table once, with one 32-bit vector atomic -- integer adds: the result
// depends neither on the grid nor on the order of the records.  No column event reaches global memory as an atomic of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_cols_body.h"

namespace mia {

constexpr int MAC_THREADS = 512, MAC_WAVES = MAC_THREADS / 64;
constexpr int MAC_WGS_PER_CU = 4;          // 38 KiB of LDS each: four fit beside each other on a compute unit's 160 KiB, 32 wavefronts

constexpr int MAC_SLICE_MIN = 128;         // records of the shortest slice: sixteen parts per wavefront when all of them lie in the tile

// how the records are cut for `wgs` resident workgroups: as many slices as keep them all busy, none shorter than MAC_SLICE_MIN (a
// wavefront walks its parts one after the other, a load each: on a short reference few long slices leave the device idle)
MIA_HD inline int64_t ma_cols_slices(int64_t n, int32_t L, int64_t wgs) {
  const int64_t tiles = ma_cols_tiles(L), most = (n + MAC_SLICE_MIN - 1) / MAC_SLICE_MIN;
  int64_t s = wgs / tiles;
  if (s > most) s = most;
  return s < 1 ? 1 : s;
}

__global__ __launch_bounds__(MAC_THREADS) void k_ma_cols(MaColsView v, int64_t n_slices, int64_t per_slice, uint32_t* table,
                                                         unsigned long long* totals) {
  __shared__ uint32_t s_tab[MA_COLS_WORDS * MA_COLS_TILE];
  __shared__ int64_t s_at[MAC_THREADS];                      // the listed parts (MaColsPart)
  __shared__ int32_t s_meta[MAC_THREADS];
  __shared__ int32_t s_listed;
  __shared__ unsigned long long s_out[2];                    // beyond, ends_outside
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tiles = ma_cols_tiles(v.L), jobs = tiles * n_slices;
  const auto add = [&](int word, int col) { atomicAdd(&s_tab[word * MA_COLS_TILE + col], 1u); };
  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int64_t tile = job % tiles, slice = job / tiles;
    const int64_t r0 = slice * per_slice, r1 = r0 + per_slice < v.n ? r0 + per_slice : v.n;
    for (int i = tid; i < MA_COLS_WORDS * MA_COLS_TILE; i += MAC_THREADS) s_tab[i] = 0;
    if (tid < 2) s_out[tid] = 0;
    int64_t beyond = 0, outside = 0;
    for (int64_t base = r0; base < r1; base += MAC_THREADS) {
      if (tid == 0) s_listed = 0;
      __syncthreads();                                       // (the first scan: the tile is zero; later ones: the list has been read)
      const int64_t r = base + tid;
      if (r < r1) {
        const int64_t s = v.start[r], n = v.col_off[r + 1] - v.col_off[r];
        const bool here = ma_cols_touches(s, n, v.L, tile);
        const bool far = tile == 0 && (s < 0 || s >= v.L || s + n < 1 || s + n > v.L);       // an anchor or a column on no reference column
        if ((here || far) && ma_cols_counts(v, r)) {
          if (far) ma_cols_outside(v, r, &beyond, &outside);
          MaColsPart part;
          if (here) {
            ma_cols_ends(v, r, tile, add);
            if (ma_cols_part(v, r, tile, &part)) {
              const int q = atomicAdd(&s_listed, 1);         // one per thread at most: the list holds them
              s_at[q] = part.at;
              s_meta[q] = part.meta;
            }
          }
        }
      }
      __syncthreads();
      const int listed = s_listed;
      for (int q = wave; q < listed; q += MAC_WAVES) ma_cols_walk(v.seq, MaColsPart{s_at[q], s_meta[q]}, lane, 64, add);
      __syncthreads();
    }
    if (beyond) atomicAdd(&s_out[0], (unsigned long long)beyond);
    if (outside) atomicAdd(&s_out[1], (unsigned long long)outside);
    __syncthreads();
    const int64_t t0 = tile * MA_COLS_TILE;
    for (int i = tid; i < MA_COLS_WORDS * MA_COLS_TILE; i += MAC_THREADS) {
      const uint32_t x = s_tab[i];
      const int64_t p = t0 + i % MA_COLS_TILE;
      if (x && p < v.L) atomicAdd(&table[(int64_t)(i / MA_COLS_TILE) * v.L + p], x);
    }
    if (tid < 2 && s_out[tid]) atomicAdd(&totals[tid], s_out[tid]);
    __syncthreads();                                         // (the next job zeroes what was just read)
  }
}

}  // namespace mia
