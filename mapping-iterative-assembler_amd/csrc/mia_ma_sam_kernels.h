// mia_ma_sam_kernels.h -- CIGAR, SEQ and NM of ma_hip's SAM export (-f 8) over the records mia_hip_ma_tally left on the device.
// Two launches:
//   k_ma_sam_layout   per record the index of its inserts (ma_sam_index, one thread per record), then one wavefront per record
//                     over its walk: the bytes of its CIGAR, the length of its SEQ, its NM.  The records' offsets in the text
//                     buffer are an ordered scan of their bodies' bytes (the workgroups' sums by the scan of ma_scan_dev.h: the
//                     order of the records is the order of the output)
//   k_ma_sam_render   one wavefront per record over the same walk, writing: every run of ops is written by the lane on which the
//                     next run begins (the last one by lane 0), every SEQ character by the lane that holds it
// Both walk a record in stretches of 64 positions (ma_sam_wave): the lanes' ops become ballots, a run begins where a lane's op
// differs from that of the nearest lane to its left that has one, the run open at the end of a stretch is carried into the
// next, the offsets of the runs' texts are a prefix sum over the lanes (DPP), the SEQ characters are compacted by ballot.
// What a walk position yields and what the masks mean is ma_sam_body.h, shared with the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ma_sam_body.h"
#include "ma_scan_dev.h"
#include "wave_dev.h"

namespace mia {

constexpr int MAS_THREADS = 256, MAS_WAVES = MAS_THREADS / 64;
// records a workgroup of the layout takes, two per wavefront: a wavefront's records are chains of dependent loads one after the
// other, so few of them per wavefront and many workgroups ("SAM export", has the times of 64 and of 8 per workgroup)
constexpr int MAS_PER_WG = 8;

// The walk of record r (`walk` positions) by one wavefront, every lane of it active.  WRITE: the CIGAR goes to cigar[0 ..), the
// SEQ to seq[0 ..).  Returns in every lane the bytes of the CIGAR, the SEQ characters and NM.
template <bool WRITE>
__device__ __forceinline__ void ma_sam_wave(const MaSamView& v, int64_t r, int64_t walk, int lane, char* cigar, char* seq, int64_t* cigar_bytes,
                                            int64_t* seq_len, int64_t* nm) {
  const DevWave wv(nullptr, nullptr);
  MaSamRun open{MA_SAM_NONE, 0};
  int64_t c_at = 0, s_at = 0, n_nm = 0;
  for (int64_t w0 = 0; w0 < walk; w0 += 64) {
    MaSamElem e{MA_SAM_NONE, 0, false};
    if (w0 + lane < walk) e = ma_sam_elem(v, r, w0 + lane);
    MaSamStretch s;
    s.m[MA_SAM_NONE] = 0;
    s.m[MA_SAM_M] = __ballot(e.op == MA_SAM_M);
    s.m[MA_SAM_I] = __ballot(e.op == MA_SAM_I);
    s.m[MA_SAM_D] = __ballot(e.op == MA_SAM_D);
    s.m[MA_SAM_S] = __ballot(e.op == MA_SAM_S);
    s.act = s.m[MA_SAM_M] | s.m[MA_SAM_I] | s.m[MA_SAM_D] | s.m[MA_SAM_S];
    n_nm += ma_sam_count(__ballot(e.nm));
    const bool head = ma_sam_head(s, lane, e.op, open.op);
    const uint64_t heads = __ballot(head);
    // the runs that end in this stretch, each on the lane of the head behind it
    MaSamRun closed{MA_SAM_NONE, 0};
    uint32_t bytes = 0;
    if (head) {
      closed = ma_sam_closed(s, heads, lane, open);
      if (closed.op != MA_SAM_NONE) bytes = (uint32_t)ma_sam_run_bytes(closed.len);
    }
    const uint32_t upto = wv.scan_add(bytes);
    if (WRITE && bytes) ma_sam_run_text(closed, cigar + c_at + (upto - bytes));
    c_at += wv.lane_val(upto, 63);
    const uint64_t chars = s.m[MA_SAM_M] | s.m[MA_SAM_I] | s.m[MA_SAM_S];
    if (WRITE && ((chars >> lane) & 1ull)) seq[s_at + ma_sam_count(chars & ma_sam_below(lane))] = e.ch;
    s_at += ma_sam_count(chars);
    open = ma_sam_carry(s, heads, open);
  }
  if (open.op != MA_SAM_NONE) {
    if (WRITE && lane == 0) ma_sam_run_text(open, cigar + c_at);
    c_at += ma_sam_run_bytes(open.len);
  }
  *cigar_bytes = c_at;
  *seq_len = s_at;
  *nm = n_nm;
}

// Workgroups take their place by ticket (ma_scan_dev.h; ctl[MAR_ROWS] = bytes of the whole text).  Workgroup t lays out records
// t * MAS_PER_WG .., wavefront w of it records w, w + MAS_WAVES, ..  cigar_bytes[r] = 0 marks a record without SEQ ("*", "*").
__global__ __launch_bounds__(MAS_THREADS) void k_ma_sam_layout(MaSamView v, int32_t n_wgs, unsigned long long* ctl, int32_t* nm, int64_t* cigar_bytes,
                                                                int64_t* body_off) {
  __shared__ unsigned long long s_first;
  __shared__ long long s_walk[MAS_PER_WG], s_bytes[MAS_PER_WG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_first = ma_scan_ticket(ctl);
  __syncthreads();
  const int64_t t = (int64_t)s_first;
  if (t >= n_wgs) return;
  if (tid < MAS_PER_WG) {
    const int64_t r = t * MAS_PER_WG + tid;
    s_walk[tid] = r < v.n ? ma_sam_index(v, r) : 0;
  }
  __syncthreads();                            // (v.cum of this workgroup's records is read by its other wavefronts from here on)
  for (int i = wave; i < MAS_PER_WG; i += MAS_WAVES) {
    const int64_t r = t * MAS_PER_WG + i;
    long long bytes = 0;
    if (r < v.n) {
      int64_t cb = 0, sl = 0, n_nm = 0;
      ma_sam_wave<false>(v, r, s_walk[i], lane, nullptr, nullptr, &cb, &sl, &n_nm);
      bytes = ma_sam_body_bytes(cb, sl);
      if (lane == 0) { nm[r] = (int32_t)n_nm; cigar_bytes[r] = sl > 0 ? cb : 0; }
    }
    if (lane == 0) s_bytes[i] = bytes;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long own = 0;
    for (int i = 0; i < MAS_PER_WG; i++) { const long long x = s_bytes[i]; s_bytes[i] = (long long)own; own += (unsigned long long)x; }
    const unsigned long long before = ma_scan_before(ctl, t, n_wgs, own);
    if (t == n_wgs - 1) body_off[v.n] = (int64_t)(before + own);
    s_first = before;
  }
  __syncthreads();
  if (tid < MAS_PER_WG) {
    const int64_t r = t * MAS_PER_WG + tid;
    if (r < v.n) body_off[r] = (int64_t)s_first + s_bytes[tid];
  }
}

// body[body_off[r] ..): <CIGAR> MA_SAM_MID <SEQ> of record r, at the sizes the layout found
__global__ __launch_bounds__(MAS_THREADS) void k_ma_sam_render(MaSamView v, const int64_t* cigar_bytes, const int64_t* body_off, char* body) {
  const int64_t r = (int64_t)blockIdx.x * MAS_WAVES + (threadIdx.x >> 6);
  if (r >= v.n) return;
  const int lane = (int)(threadIdx.x & 63);
  char* out = body + body_off[r];
  const int64_t cb = cigar_bytes[r];
  if (cb == 0) {
    if (lane < MA_SAM_EMPTY_BYTES) out[lane] = MA_SAM_EMPTY[lane];
    return;
  }
  if (lane < MA_SAM_MID_BYTES) out[cb + lane] = MA_SAM_MID[lane];
  int64_t got_cb = 0, sl = 0, n_nm = 0;
  ma_sam_wave<true>(v, r, ma_sam_walk_len(v, r), lane, out, out + cb + MA_SAM_MID_BYTES, &got_cb, &sl, &n_nm);
}

}  // namespace mia
