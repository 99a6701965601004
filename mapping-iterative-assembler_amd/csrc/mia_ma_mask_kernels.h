// mia_ma_mask_kernels.h -- the end mask (ma_hip -E, -x, -f 96) over the records mia_hip_ma_tally left on the device.  Three launches
// (ma_mask_body.h holds what a lane does in each):
//
// k_ma_mask_bounds runs over the FLAT columns (the shared walk: ma_flat_body.h): a lane takes a stretch of MA_MASK_LANE = 16 positions
// at a time, a workgroup 4 096, the grid strides over those chunks.  A lane keeps the first and the last column outside the zones of the record
// it is in in two registers and sends them when the record changes and at the end of its stretch: one 32-bit vector atomic minimum on
// lo[r] and one maximum on hi[r] per (lane, record), none where the lane met no such column, and plain stores where the record lies
// wholly inside the lane's stretch (no other lane sees it).  lo is preset to all ones and hi to 0, so the order of arrival does not
// matter.  Every zone column (substitution mode: every substituted column) is one LDS atomic on the wavefront's own copy of
// hist[2][2][16] (ma_wave_bins.h).  A workgroup meets fewer than 2^32 columns, so the 32-bit LDS words hold.
//
// k_ma_mask_layout runs a RECORD PER LANE: ma_mask_record walks a over the '-' columns behind a1 and b over those in front of b1
// (bounded by the record's own '-' runs at its two seams), writes first, count and start', and the workgroup's kept columns go through
// the ordered scan of ma_scan_dev.h into col_off' -- the scan k_ma_sam_layout and the other exports use, tickets and all.  The scalars
// (emptied per strand, stripped, records kept) go through LDS as above.
//
// k_ma_mask_apply runs over the NEW flat layout: a lane makes 16 positions of SEQ' and SMP' and stores each with one 16-byte vector
// store -- the strings are padded to a multiple of 16, the padding is written as 0, and no two lanes share a word.  The columns of the
// stretch's first record are fetched with two aligned 16-byte loads and a byte shift (ma_mask_load_unaligned); the columns of records
// that begin inside the stretch, the seams, byte by byte.  In trim mode a zone column that STAYS (a hand-made file: mia writes none)
// is counted into a second histogram, which the host subtracts from the first.  In substitution mode the layout is the old one and the
// substituted columns are written as N.  Behind the strings, one lane per listed INS_POS pair: the pair's record by bisecting
// rec_ins, pair_keep and ins_pos', and the dropped pairs of surviving records counted per wavefront.
//
// Vector stores only, no scratch, no inline assembly, no cooperative launch.  All counts are integer sums: the result does not
// depend on the grid or on the records' order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_mask_body.h"
#include "ma_scan_dev.h"
#include "ma_wave_bins.h"

namespace mia {

constexpr int MAM_THREADS = 256, MAM_WAVES = MAM_THREADS / 64;
constexpr int MAM_WG_COLS = MAM_THREADS * MA_MASK_LANE;    // 4 096
constexpr int MAM_WGS_PER_CU = 4;          // persistent grids: at most this many workgroups per compute unit
constexpr int MAM_PER_WG = MAM_THREADS;    // records of one workgroup of the layout

MIA_HD inline int64_t ma_mask_chunks(int64_t T) { return (T + MAM_WG_COLS - 1) / MAM_WG_COLS; }
MIA_HD inline int64_t ma_mask_layout_wgs(int64_t n) { return (n + MAM_PER_WG - 1) / MAM_PER_WG; }
MIA_HD inline int64_t ma_mask_padded(int64_t T) { return (T + MA_MASK_LANE - 1) / MA_MASK_LANE * MA_MASK_LANE; }

__global__ __launch_bounds__(MAM_THREADS) void k_ma_mask_bounds(MaFlatView v, int32_t n5, int32_t n3, int32_t mode, int32_t single_stranded, uint32_t* lo,
                                                                 uint32_t* hi, unsigned long long* bins) {
  __shared__ uint32_t s_bins[MAM_WAVES][MA_MASK_HIST];
  uint32_t* const mine = ma_wave_bins_mine(s_bins);
  ma_wave_bins_zero(s_bins);
  const int64_t n_chunks = ma_mask_chunks(v.T);
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x)
    ma_mask_stretch(
        v, n5, n3, mode, single_stranded != 0, c * MAM_WG_COLS + (int64_t)threadIdx.x * MA_MASK_LANE,
        [&](int64_t r, uint32_t a1, uint32_t b1, bool whole) {
          if (whole) { lo[r] = a1; hi[r] = b1; return; }
          if (a1 != MA_MASK_NO_COLUMN) atomicMin(&lo[r], a1);
          if (b1) atomicMax(&hi[r], b1);
        },
        [&](int bin) { atomicAdd(&mine[bin], 1u); });
  ma_wave_bins_flush(s_bins, bins);
}

// Workgroups take their place by ticket (ma_scan_dev.h; ctl[MAR_ROWS] = the kept columns of the whole file).  Workgroup t decides
// records t * MAM_PER_WG .., a record per lane.
__global__ __launch_bounds__(MAM_THREADS) void k_ma_mask_layout(MaMaskRecView m, int32_t n_wgs, unsigned long long* ctl, int64_t* new_off,
                                                                 unsigned long long* bins) {
  constexpr int SCALARS = MA_MASK_BINS - MA_MASK_EMPTIED;
  __shared__ unsigned long long s_first;
  __shared__ long long s_len[MAM_PER_WG];
  __shared__ uint32_t s_bins[MAM_WAVES][SCALARS];
  const int tid = threadIdx.x;
  uint32_t* const mine = ma_wave_bins_mine(s_bins);
  if (tid == 0) s_first = ma_scan_ticket(ctl);
  ma_wave_bins_zero(s_bins);
  const int64_t t = (int64_t)s_first;
  if (t >= n_wgs) return;
  const int64_t r = t * MAM_PER_WG + tid;
  s_len[tid] = r < m.v.n ? ma_mask_record(m, r, [&](int bin) { atomicAdd(&mine[bin - MA_MASK_EMPTIED], 1u); }) : 0;
  __syncthreads();
  if (tid == 0) {
    unsigned long long own = 0;
    for (int i = 0; i < MAM_PER_WG; i++) { const long long x = s_len[i]; s_len[i] = (long long)own; own += (unsigned long long)x; }
    const unsigned long long before = ma_scan_before(ctl, t, n_wgs, own);
    if (t == n_wgs - 1) new_off[m.v.n] = (int64_t)(before + own);
    s_first = before;
  }
  __syncthreads();
  if (r < m.v.n) new_off[r] = (int64_t)s_first + s_len[tid];
  ma_wave_bins_flush(s_bins, bins + MA_MASK_EMPTIED);
}

// chunks = ma_mask_chunks(padded new_T) workgroup-sized pieces of the new strings, then the pairs in pieces of MAM_THREADS
__global__ __launch_bounds__(MAM_THREADS) void k_ma_mask_apply(MaMaskApplyView m, const int32_t* count, int64_t n_ins, char* seq_out, char* smp_out,
                                                                uint8_t* pair_keep, int32_t* new_ins_pos, unsigned long long* bins) {
  __shared__ uint32_t s_bins[MAM_WAVES][MA_MASK_HIST];
  uint32_t* const mine = ma_wave_bins_mine(s_bins);
  ma_wave_bins_zero(s_bins);
  const int64_t padded = ma_mask_padded(m.new_T), n_chunks = ma_mask_chunks(padded);
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t base = c * MAM_WG_COLS + (int64_t)threadIdx.x * MA_MASK_LANE;
    if (base >= padded) continue;
    MaRecWord so, mo;
    ma_mask_gather(m, base, &so, &mo, [&](int bin) { atomicAdd(&mine[bin], 1u); });
    *reinterpret_cast<uint4*>(seq_out + base) = make_uint4(so.w[0], so.w[1], so.w[2], so.w[3]);
    *reinterpret_cast<uint4*>(smp_out + base) = make_uint4(mo.w[0], mo.w[1], mo.w[2], mo.w[3]);
  }
  ma_wave_bins_flush(s_bins, bins + MA_MASK_STAY);
  uint32_t dropped = 0;
  for (int64_t k = (int64_t)blockIdx.x * MAM_THREADS + threadIdx.x; k < n_ins; k += (int64_t)gridDim.x * MAM_THREADS) {
    int64_t lo = 0, hi = m.v.n;            // the record of the k-th listed pair: rec_ins[lo] <= k < rec_ins[hi]
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if ((int64_t)m.v.rec_ins[mid] <= k) lo = mid; else hi = mid;
    }
    const int32_t e = m.v.ins_list[k];
    int32_t pos = 0;
    const bool stays = ma_mask_pair(m.mode, m.first[lo], count[lo], m.v.ins_pos[e], &pos);
    pair_keep[e] = stays ? 1 : 0;
    new_ins_pos[e] = pos;
    dropped += !stays && count[lo] > 0 ? 1u : 0u;
  }
  if (dropped) atomicAdd(&bins[MA_MASK_PAIRS], (unsigned long long)dropped);
}

}  // namespace mia
