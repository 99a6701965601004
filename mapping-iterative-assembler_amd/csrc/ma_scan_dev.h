// ma_scan_dev.h -- the ordered scan over the workgroups of one launch that k_ma_region_select, k_ma_ace_layout and k_ma_sam_layout
// share: every workgroup has a sum of its own (rows selected, bytes of text) and learns the sum of all workgroups in front of it, so
// that the order of the records is the order of the output with no atomic append.  The only inter-workgroup synchronisation of ma's
// exports.
//
// The launch has control words of 64 bits, zeroed by the host in front of it: an arrival ticket, two results, and one state per
// workgroup.  A workgroup's place t is the ticket its thread 0 takes (ma_scan_ticket), not its blockIdx: tickets are handed out in
// the order workgroups start to run, so a workgroup only ever waits for workgroups that already run and the scan cannot deadlock
// however few of the grid are resident.  Thread 0 of place t then calls ma_scan_before with the workgroup's sum: it publishes
// MAR_OWN | own, walks back over state[t-1], state[t-2], .. adding what it finds -- sleeping on a word that is still empty -- until
// it meets a MAR_UPTO, and publishes MAR_UPTO | (before + own).  Place 0 publishes MAR_UPTO and nothing else, so the walk never
// passes it.  Place n_wgs - 1 stores the total to ctl[MAR_ROWS].  All accesses are relaxed atomics of agent scope on single words
// that carry their own tag: nothing else is communicated through them, so no fence is needed.
//
// Neither function holds a barrier: the caller hands thread 0's results to the other threads through LDS between its own
// __syncthreads().  The grid may hold more workgroups than n_wgs (the region select's ticket n_wgs writes the column map): what a
// ticket at or above n_wgs does is the caller's business, and it must not call ma_scan_before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mia {

// the control words: arrival tickets, the scan's total, a second result of the caller's own (the region's row width), then one
// state per workgroup
constexpr int MAR_TICKET = 0, MAR_ROWS = 1, MAR_WIDTH = 2, MAR_STATE = 4;
// state of workgroup t: its own sum (MAR_OWN) or the sum of workgroups 0 .. t (MAR_UPTO) in the low 62 bits
constexpr unsigned long long MAR_OWN = 1ull << 62, MAR_UPTO = 2ull << 62, MAR_VALUE = (1ull << 62) - 1;

__device__ __forceinline__ unsigned long long ma_scan_ticket(unsigned long long* ctl) { return atomicAdd(&ctl[MAR_TICKET], 1ull); }

// the sum of the workgroups in front of place t (0 <= t < n_wgs), whose own sum is `own`
__device__ __forceinline__ unsigned long long ma_scan_before(unsigned long long* ctl, int64_t t, int32_t n_wgs, unsigned long long own) {
  unsigned long long before = 0;
  unsigned long long* state = ctl + MAR_STATE;
  if (t > 0) {
    __hip_atomic_store(&state[t], MAR_OWN | own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int64_t j = t - 1;;) {
      const unsigned long long x = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((x & ~MAR_VALUE) == 0) { __builtin_amdgcn_s_sleep(1); continue; }
      before += x & MAR_VALUE;
      if ((x & ~MAR_VALUE) == MAR_UPTO) break;
      j--;
    }
  }
  __hip_atomic_store(&state[t], MAR_UPTO | (before + own), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t == n_wgs - 1) ctl[MAR_ROWS] = before + own;
  return before;
}

}  // namespace mia
