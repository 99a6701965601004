// align_route.h -- which kernels take the reads of one alignment, in which order and on which stream: THE one place where that is
// decided.  Plain C++17, no HIP: align_route() reads its argument and nothing else, so a CPU test (tests/test_align_route_cpu.py)
// enumerates it against a restatement of every rule and pins the routes of the benched workloads.  align_all (mia_hip.hip) fills
// AlignRouteIn from the context, asks once, and its stages only follow the answer.  The comments are the record of why each threshold
// is what it is: a rule and its measurements live here, once.
#pragma once
#include <stdint.h>

namespace mia {

constexpr int ROUTE_QCH = 8, ROUTE_MAXW = 64;      // = BX_QCH, BX_MAXW (bandx_kernels.h, bandx_body.h; held together by mia_hip.hip)

struct AlignRouteIn {
  int64_t n = 0;                       // reads
  int max_len = 0, wrap = 0, L = 0;    // longest read; reference columns with and without the wrapped stretch
  int64_t plane_words = 0;             // words of one bit plane of the wrapped reference (diag_filter.h: plane_words(wrap + 64))
  int64_t kh_entries = 0;              // > 0: the reference has N columns and its 10-mer table lists them
  bool flat = false, ref_mostly_bases = true, ref_few_n = true, bx_ok = false, explicit_win = false, deferred = false, pend_encode = false;
  bool own_umax = false;               // the context's own reads, their U at hand (a borrowed read set has none)
  bool ref_ready = false;              // codes, planes, nibbles, table and bitmaps of this reference stand, and the control block is clear (ref_ahead.h: a hit)
  int64_t rejects = 0;                 // reads the plan of the alignment before gave up on: sum of bx_last[BXC_FAIL0 + k], k = 1 .. BXF_KINDS - 1
  // the alt switches (read_alt_switches); the release build only ever holds the defaults
  int use_filter = 1, use_banddp = 1, use_bx = 1, use_lanes = 1, use_fine = 1, use_quick = 1;
  bool bx_serial = false, plan_split = true, use_direct_open = true, no_prep_fuse = false;
  uint32_t ext_events = 31u, dbg = 0, bx_dbg = 0;
};

struct AlignRoute {
  int64_t plane_words = 0;             // (the caller's)
  int nwords = 0;                      // 64-row words of the longest read
  bool bx = false, run_filter = false, fused_prep = false, filtered = false, kocc = false, banded = false;
  bool prep_none = false;              // the reference preparation launches nothing: it only hands the stages the views of what stands
  bool want_bits = false, new_flow = false, split = false, fork_by_launch = false, fine = false;
  bool many_rejects = false;           // THE many-rejects predicate: one answer for fine, planner_head_first / direct_open and use_plain
  bool planner_head_first = false, direct_open = false;
  int maxw = 0;                        // widest band class in use (BxTab::maxw)
  bool quick = false, quick_lds = false, one_launch = false, fork_at_quick = false;
  int qch = 4;                         // stretches of 256 reads per workgroup of the quick plan
  int quick_phase = 0;                 // k_bx_plan<NW, 4 | 5> (0: no quick plan)
  int full_first = 0, full_last = 0;   // the full plan's launches k_bx_plan<NW, full_first .. full_last>: 0, 1..2, 1..3, or 6 (one looped launch)
  int grid_cap = 0;                    // its grid rule: phases 2 and 3 at most 1 024 workgroups, the ones before at most this many (0: one per 256 reads)
  bool three_streams = false, two_streams = false;      // the band DPs' order (neither: MIA_HIP_DEBUG_SKIP & 256, no band DPs at all)
  bool values_aside = false;           // three streams: values DP and late trace on stream2 (else on the context's stream)
  bool trace_signals = false;          // ... the trace DP signals ev_join3 itself
  bool planner_aside = false;          // ... planner and full-window kernels on stream2
  bool use_plain = false;              // the values-only quad pass
  bool plan_count_late = false;        // k_plan_count behind the band launches (not in front of the fork, not left out)
};

// (one per 256 reads, capped: one_launch is a grid the chip holds at once, looping over the list -- see PH 6 in bandx_kernels.h)
inline unsigned align_route_plan_grid(const AlignRoute& r, int phase, int64_t n) {
  const int64_t g = (n + 255) / 256, cap = (phase == 2 || phase == 3) ? 1024 : r.grid_cap;
  return (unsigned)(cap && g > cap ? cap : g);
}

inline AlignRoute align_route(const AlignRouteIn& in) {
  AlignRoute r;
  const int64_t n = in.n;
  r.nwords = (in.max_len + 63) >> 6;
  r.plane_words = in.plane_words;
  const bool filter_ok = in.flat && in.use_filter && in.ref_mostly_bases;
  // the band pipeline for any matrix (bandx_kernels.h); it needs the 10-mer table and windows free of N
  r.bx = in.bx_ok && in.use_bx && (in.ref_mostly_bases || in.kh_entries > 0) && in.wrap <= (1 << 22) && !(in.dbg & 128u);
  r.run_filter = filter_ok && !r.bx;
  // mia_hip_iterate with the band pipeline alone: codes, control block, planes, nibbles and 10-mer table in one launch (k_ref_prep)
  r.fused_prep = in.pend_encode && r.bx && !in.no_prep_fuse;
  // ... or none at all: the last call of mia_hip_iterate made all of it behind its consensus, for the string it returned, and this call
  // brings that string (only the band pipeline's set is prepared ahead)
  r.prep_none = in.ref_ready && r.bx;
  r.filtered = r.run_filter || r.bx;            // bin_of carries marks for the planner
  // the 10-mer table of this reference (rule (c) looks long clean stretches up instead of sliding over every diagonal;
  // the band plans are made of its anchors); not for the very long concatenated strings mia_hip_align_windows may be given
  r.kocc = r.filtered && in.wrap <= (1 << 22) && !r.bx;
  // what the filter leaves over goes through a banded DP first (bandx_kernels.h, or round 1's band_body.h); both need the table
  r.banded = r.bx || (r.filtered && in.use_banddp && r.kocc && !(in.dbg & 128u));
  // MANY REJECTS: the plan gives up on many reads -- against a reference full of ambiguity codes (every run's first iteration
  // against mt311: the N columns alone exhaust the loss budget of one read in twenty, one in five with the ancient matrix),
  // or when it did so in the iteration before.
  const bool many = !in.ref_mostly_bases || in.rejects * 20 > n;
  r.many_rejects = r.bx && many;
  // behind the banded DP the values-only pass has nothing left to prove: what the band could not take nearly always needs a trace
  // ... unless the plan gives up on many reads.  Most of those reads are gap-free; the values-only pass finishes them at
  // half the trace kernel's price (first iteration 2.84 -> 2.59 ms flat, 5.35 -> 4.08 ms ancient, per 1 M reads).
  // Either way every read gets the reference's alignment: the choice only moves work between exact kernels.
  r.use_plain = !r.banded || r.many_rejects;
  r.plan_count_late = true;
  if (!r.bx) return r;

  // (the quick plan's bitmaps: made wherever the table is made, unless the reference is N all over -- hardly a window without one then)
  r.want_bits = in.use_quick && (in.kh_entries <= 0 || in.ref_few_n);
  // MIA_HIP_BX_SERIAL=1: round 2's order (band kernels, then the planner over everything they left open)
  // (caller-supplied windows -- mia_hip_align_windows -- can be of any length: the retry list's window kernel is picked by read length)
  r.new_flow = in.use_lanes && !in.bx_serial && !(in.dbg & 256u) && !in.explicit_win;
  // the plan in two launches (bandx_kernels.h, phase): the reads with anchors on two diagonals are finished by a second launch
  // with every lane at work (MIA_HIP_NO_PLAN_SPLIT=1: by the first threads of their blocks, one launch)
  r.split = in.plan_split;
  r.fork_by_launch = (in.ext_events & 1u) && r.new_flow;
  // a third launch for the reads whose loss exceeds what the 10-mers vouch for (bx_fine_anchors; MIA_HIP_NO_FINE=1: given up as before)
  // ... with a position-specific matrix (two reads in a hundred exceed the 10-mers' budget in every iteration, and the full-window
  // kernels they went to were the largest consumer of vector instructions at 10 M reads: configs[3] 8.47 -> 7.44 ms, configs[2]
  // 1.41 -> 1.35 ms), with many reads (the launch costs next to nothing where the step is bound by throughput), and whenever
  // the plan gives up on many reads: against a reference full of ambiguity codes (every run's first iteration), or when it did so
  // in the iteration before.  With the flat matrix and a million reads the launch would sit on the step's critical path (~55 us)
  // for the sake of a few thousand reads whose full-window kernels run beside the band DPs anyway.
  r.fine = r.split && in.use_fine && (in.use_fine > 1 || !in.flat || n >= 4000000 || many);
  // PLANNER FIRST.  Where the plan gives up on many reads (against a reference full of ambiguity codes -- every run's first
  // iteration --, or when it did so in the iteration before) the planner's chain on stream2 -- count, scan, fill, the values-only
  // quad kernel, the re-plan, the trace quad kernel -- is the longest of the three, and its three small head kernels, launched
  // beside the persistent band grids, wait for wave slots: k_plan_scan's single workgroup 70 us, the other two 65-80 us each
  // instead of 10 (first iteration of 1 M flat reads; at 10 M reads 1 ms and 0.8 ms).  They go in front of the fork then: ~35 us
  // later for the band DPs, ~190 us earlier for the chain that the step waits for.  (Not at steady state, where the
  // planner's chain has slack and the band DPs' start is the step's critical path.)
  r.planner_head_first = r.new_flow && in.deferred && many;
  // DIRECT OPEN LIST (round 6).  At steady state the plan leaves a few hundred reads per million open.  For their sake the planner
  // counted, scanned and filled over ALL reads (three launches beside the persistent band grids: 13 + 7 + 71 us), a quad kernel took
  // them four to a wavefront (110 us: one quad's latency), three window-class launches and a retry launch followed -- nine launches,
  // 270 us, the longest of the step's three DP chains.  Now the plan appends such a read to a list as it gives up on it and
  // k_align_open takes the list, one read per wavefront (90-115 us beside the band DPs, 35 on an idle chip: off the step's chain either way).  Where the plan gives up on MANY reads (the values-only quad pass is on:
  // every run's first iteration, N-rich references) the planner and the quad kernels stay: four reads per wavefront is what pays there.
  r.direct_open = r.new_flow && in.deferred && in.use_direct_open && !many && !(in.bx_dbg & (4u | 8u));
  // (the widest class needs a read spread over eight lanes)
  // ... and where the plan's third launch is off (flat matrix, a million reads, hardly any rejects: the step is a chain of
  // latencies) the widest class is not used at all: those few reads keep going to the full-window kernels on the planner's stream,
  // whose chain is as long with them as without (measured: 0.960 against 0.944 ms per step with the class in use)
  r.maxw = (in.use_lanes && (r.fine || in.use_fine >= 2)) ? ROUTE_MAXW : 32;
  // THE QUICK PLAN FIRST (round 6; bandx_body.h: bx_quick, k_bx_plan<NW, 4>): every read on the diagonal it was aligned on before -- nine
  // in ten of a steady-state iteration are finished or listed there for a tenth of the full plan's instructions; the rest goes on a
  // list (the diagonal filter's: d_left_list, d_filter_n[1]) that the full plan's launches take as their in_list.  Not against a reference
  // that is N all over (every run's first iteration; one with a few N columns: the windows that hold none, want_bits above).
  // (... and with the fine blocks on only from two million reads: the three launches of the full plan stay behind it then, each with a
  // launch's floor of 30-90 us for the few reads it has left -- 1 M ancient reads 1.12 ms without it, 1.15 with; 10 M solexa 6.0 / 5.4)
  r.quick = r.split && r.new_flow && r.want_bits && !(in.bx_dbg & 32u) && in.own_umax &&      // (the context's own reads: their U is at hand)
            (!r.fine || n >= 2000000 || in.use_quick > 1);
  // mia_hip_iterate: the fork is behind the QUICK plan (BxDev::to_late) -- values DP and late trace are on the context's stream there, behind
  // the full plan's launch, so no wait between streams is added; mia_hip_realign keeps every launch of the plan in front of the fork
  // (... and only where the plan lists its open reads itself: the planner's kernels on stream2 would want every read's mark at the fork)
  // (... and not with the fine blocks: the three launches of the full plan are then a chain of their own, longer beside the DPs than
  // both DPs together -- configs[2]: 45 + 174 + 114 us and 211 for their lists' trace against 280 for the DPs; in front of the fork)
  r.fork_at_quick = r.quick && r.direct_open && !r.fine;
  // (the reference's planes in LDS for the quick plan while they are small: 38 KB holds a hundred thousand columns)
  r.quick_lds = r.quick && r.plane_words * 24 <= 38 * 1024;
  r.quick_phase = r.quick ? (r.quick_lds ? 5 : 4) : 0;
  // (eight stretches per workgroup where the lists' counters are the wait -- many reads -- and the planes in LDS are small: with a
  // 100 kb reference's 37 KB of planes the larger per-read arrays cost the third workgroup per compute unit, configs[4] 7.85 -> 8.05 ms)
  r.qch = (r.quick && n >= 4000000 && r.plane_words * 24 <= 16 * 1024) ? ROUTE_QCH : 4;
  // behind the quick plan the full plan has one read in a hundred left: without fine blocks ONE launch (phase 0: the reads with anchors on
  // two diagonals by the block's first threads -- a second launch would be a second chain through the table, 40 us, for fifty workgroups)
  r.one_launch = r.quick && !r.fine;
  r.full_first = r.one_launch ? 6 : r.split ? 1 : 0;
  r.full_last = r.one_launch ? 6 : r.split ? (r.fine ? 3 : 2) : 0;
  r.grid_cap = r.one_launch ? 256 : 0;
  // BAND DPs.  Three things that do not depend on each other run side by side: the trace DP of the plan's own lists (stream3),
  // the values DP with one more trace launch behind it for what it could not finish (stream2), and -- on the
  // context's stream -- the planner and the full-window kernels for the reads the plan gave up on.  The
  // step pays the longest of the three instead of their sum; what no band kernel can finish (the reference's
  // index-0 quirk: next to nothing) goes on a retry list that a window kernel reads behind the join.
  // mia_hip_iterate (deferred): the values DP and the trace launch behind it ARE the step's critical path, so they
  // stay on the context's stream, right behind the plan -- a cross-stream wait costs 20-30 us each way, and it is the
  // planner with the full-window kernels (short, done long before) that moves to stream2.
  // fork_at_quick (round 6): the context's stream holds the full plan's launch for the reads the quick plan left and the trace launch
  // of what THAT lists (the second late lists); values DP and late trace run beside them on stream2, the trace DP on stream3 -- three
  // chains of about the same length instead of plan -> values DP -> late trace one after the other, and the join waits for all
  r.three_streams = r.new_flow;
  r.two_streams = !r.new_flow && !(in.dbg & 256u);
  r.values_aside = r.three_streams && !(in.deferred && !r.fork_at_quick);
  r.trace_signals = r.three_streams && (in.ext_events & 2u) && !(in.bx_dbg & 8u);
  r.planner_aside = r.three_streams && in.deferred;
  r.plan_count_late = !r.planner_head_first && !r.direct_open;
  return r;
}

}  // namespace mia
