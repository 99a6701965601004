// mia_ma_damage_kernels.h -- the deaminated-fragment filter (ma_hip -D, -e, -S, -f 95) over the records mia_hip_ma_tally left on the
// device.  Two launches (ma_damage_body.h holds what a lane does in either):
//
// k_ma_damage_hits runs over the FLAT columns (the shared walk: ma_flat_body.h): a lane takes a stretch of MA_DMG_LANE = 16 positions
// at a time, a workgroup 4 096, the grid strides over those chunks.  A lane keeps the best hit per end of the record it is in in two
// registers and sends them when the record changes and at the end of its stretch: at most one 32-bit vector atomic per (lane, record,
// end) that HAS a hit, on hit5[r] / hit3[r].  The value is 16 - k and the atomic a maximum, so the arrays only need to be zeroed
// (one memset) and the smallest k wins in whatever order lanes arrive.  In real data a few per cent of the records have a hit at all;
// adversarial data (every column a hit) is bounded by one atomic per lane, record and end -- a sixteenth of the columns for long
// records -- never one per column.  No LDS, no scratch.
//
// k_ma_damage_molecules runs a RECORD PER LANE: it turns the record's two values into pos5 / pos3, and the lower-numbered record of a
// molecule joins the halves, decides keep for N and the ends mode, stores keep to both records (plain vector stores: no other lane
// writes them) and adds the molecule to hist[strand][m5][m3] -- with the orphan and kept-record counts 514 bins, one LDS atomic on the
// wavefront's own copy (ma_wave_bins.h: 4 copies, 8 KiB per workgroup).  A record adds at most three events and mia_hip_ma_tally
// takes fewer than 2^31 records: a 32-bit LDS word does not overflow before the one flush.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_damage_body.h"
#include "ma_wave_bins.h"

namespace mia {

constexpr int MAG_THREADS = 256, MAG_WAVES = MAG_THREADS / 64;
constexpr int MAG_WG_COLS = MAG_THREADS * MA_DMG_LANE;     // 4 096
constexpr int MAG_WGS_PER_CU = 4;          // persistent grids: at most this many workgroups per compute unit

MIA_HD inline int64_t ma_dmg_chunks(int64_t T) { return (T + MAG_WG_COLS - 1) / MAG_WG_COLS; }
MIA_HD inline int64_t ma_dmg_record_wgs(int64_t n) { return (n + MAG_THREADS - 1) / MAG_THREADS; }

__global__ __launch_bounds__(MAG_THREADS) void k_ma_damage_hits(MaFlatView v, int32_t single_stranded, uint32_t* hit5, uint32_t* hit3) {
  const int64_t n_chunks = ma_dmg_chunks(v.T);
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x)
    ma_dmg_stretch(v, single_stranded != 0, c * MAG_WG_COLS + (int64_t)threadIdx.x * MA_DMG_LANE, [&](int64_t r, uint32_t h5, uint32_t h3) {
      if (h5) atomicMax(&hit5[r], h5);
      if (h3) atomicMax(&hit3[r], h3);
    });
}

__global__ __launch_bounds__(MAG_THREADS) void k_ma_damage_molecules(MaDmgMolView v, unsigned long long* out) {
  __shared__ uint32_t s_bins[MAG_WAVES][MA_DMG_BINS];
  ma_wave_bins_records(s_bins, v.n, out, [&](int64_t r, auto&& count) { ma_dmg_record(v, r, count); });
}

}  // namespace mia
