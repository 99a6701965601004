// mia_hip.hip -- libmia_hip.so: C ABI (include/mia_hip.h) over the gfx950 kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared (see __graft_entry__.build()).
#include <hip/hip_runtime.h>
#include <atomic>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <optional>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/mia_hip.h"
#include "dev_buf.h"
#include "ref_ahead.h"
#include "dev_pool.h"
#include "mia_comm.h"
#include "mia_consensus_kernels.h"
#include "mia_kernels.h"
#include "bandx_kernels.h"
#include "align_route.h"
#include "pass1_route.h"
#include "mia_pass1_kernels.h"
#include "mia_myers_kernels.h"
#include "mia_trim_kernels.h"
#include "mia_peak_kernels.h"
#include "mia_iter_kernels.h"
#include "mia_ma_region_kernels.h"
#include "mia_ma_ace_kernels.h"
#include "mia_ma_sam_kernels.h"
#include "mia_ma_profile_kernels.h"
#include "mia_ma_ends_kernels.h"
#include "mia_ma_cols_kernels.h"
#include "mia_ma_dedup_kernels.h"
#include "mia_ma_damage_kernels.h"
#include "mia_ma_mask_kernels.h"
#include "mia_ma_pmd_kernels.h"
#include "mia_ma_collapse_kernels.h"

using namespace mia;

// timed stages (HIP events on the context's stream around the kernel launches of that kind)
enum Stage { STG_TRACE = 0, STG_PLAIN, STG_FILTER, STG_BAND, STG_BX_PLAN, STG_BX_VALUES, STG_BX_TRACE, STG_TALLY, STG_PASS1, STG_MA_SELECT, STG_MA_RENDER, STG_MA_ACE_LAYOUT, STG_MA_ACE_RENDER, STG_MA_MASK_BOUNDS, STG_MA_MASK_LAYOUT, STG_MA_MASK_APPLY, STG_MA_SCORE_COLS, STG_MA_SCORE_MOLECULES, STG_MA_SAM_LAYOUT, STG_MA_SAM_RENDER, STG_MA_DAMAGE_HITS, STG_MA_DAMAGE_MOLECULES, STG_MA_PROFILE, STG_MA_DEDUP_KEYS, STG_MA_DEDUP_SORT, STG_MA_DEDUP_RUNS, STG_MA_DEDUP_NEXT, STG_MA_DEDUP_ANCHORS, STG_MA_DEDUP_CLUSTERS, STG_MA_TALLY, STG_MA_COLS, STG_MA_ENDS, STG_COUNT };
static const char* const STAGE_NAMES[STG_COUNT] = {"k_align_quad", "k_align_quad_plain", "k_diag_filter", "k_band_align", "k_bx_plan",
                                                   "k_bx_values", "k_bx_trace", "k_tally_binned", "k_pass1", "k_ma_region_select",
                                                   "k_ma_region_render", "k_ma_ace_layout", "k_ma_ace_render", "k_ma_mask_bounds", "k_ma_mask_layout", "k_ma_mask_apply", "k_ma_score_cols", "k_ma_score_molecules", "k_ma_sam_layout",
                                                   "k_ma_sam_render", "k_ma_damage_hits", "k_ma_damage_molecules", "k_ma_profile", "k_ma_dedup_keys", "k_ma_dedup_sort", "k_ma_dedup_runs",
                                                   "k_ma_dedup_next", "k_ma_dedup_anchors", "k_ma_dedup_clusters", "k_ma_tally", "k_ma_cols", "k_ma_ends"};
// The stages behind the 32 that mia_hip_set_stage_mask has a bit for: always timed, listed behind the others by mia_hip_stage_stats.
enum StageMore { STG_MA_COLLAPSE_PLAN = STG_COUNT, STG_MA_COLLAPSE_COUNT, STG_MA_COLLAPSE_DECIDE, STG_ALL };
static const char* const STAGE_NAMES_MORE[STG_ALL - STG_COUNT] = {"k_ma_collapse_plan", "k_ma_collapse_count", "k_ma_collapse_decide"};
static inline const char* stage_name(int k) { return k < STG_COUNT ? STAGE_NAMES[k] : STAGE_NAMES_MORE[k - STG_COUNT]; }

// One device block for every small counter of an iteration (planner bins and header, filter / band-pipeline counters, link
// count, cull and tally flags, insert-event count): one memset at the start of the alignment clears them all, and one copy
// brings back what the host wants to see.  Offsets in 32-bit words.
constexpr int OPEN_WGS = 1024;                                   // k_align_open's persistent grid (one read per wavefront; a steady-state list holds a few hundred)
constexpr int64_t OPEN_SLAB_BYTES = (int64_t)MAX_READ * 64 * 12;   // its trace slab: the widest window class's
constexpr int CTRL_BINS = 0;                                   // [count N_BINS][off N_BINS][cursor N_BINS][wide_count][retry_count]
constexpr int CTRL_HDR = (3 * N_BINS + 2 + 1) & ~1;            // PH_* (8-byte aligned: the DP kernels fetch their range as a pair)
constexpr int CTRL_FILTER = CTRL_HDR + PH_WORDS;               // 4 words (k_diag_filter / k_band_align)
constexpr int CTRL_LKN = CTRL_FILTER + 4, CTRL_CULLF = CTRL_LKN + 1, CTRL_NEV = CTRL_CULLF + 1, CTRL_TFLAGS = CTRL_NEV + 1;
constexpr int CTRL_GENN = CTRL_TFLAGS + 2;                           // reads k_tally_binned left to k_tally_general (the word in front of it is reserved: the block's layout stays as it was)
constexpr int CTRL_BXC = (CTRL_GENN + 1 + 63) & ~63;           // BXC_* counters, a cache line each
constexpr int CTRL_WORDS = CTRL_BXC + BXC_WORDS;
constexpr int CTRL_C0 = CTRL_BINS + 3 * N_BINS, CTRL_CN = CTRL_WORDS - CTRL_C0;    // what the host looks at behind an alignment: wide / retry counts, planner header, filter and band counters

// Environment switches.  The release library reads FIVE (documented in DESIGN.md 1): MIA_HIP_SPIN_WAIT and MIA_HIP_LOOPBACK_TIMEOUT
// here, MIA_HIP_THREADS, MIA_HIP_TIMING and MIA_DATA_PATH in the host programs.  Everything else -- the "off" sides of the
// differential tests, the round-1 and one-lane routes, the profiling switches that make results wrong on purpose
// (MIA_HIP_DEBUG_SKIP, MIA_HIP_BX_DEBUG) -- exists only in libmia_hip_alt.so, built with -DMIA_HIP_ALT_PATHS; the Python binding
// loads that build for a context made while such a variable is set (tests, tools), and nothing else does.
#ifdef MIA_HIP_ALT_PATHS
static inline const char* alt_env(const char* name) { return getenv(name); }
#define ALT_KERNEL(k) ((const void*)(k))
#else
static inline const char* alt_env(const char*) { return nullptr; }
#define ALT_KERNEL(k) ((const void*)nullptr)        // (the one-lane band kernels are not part of the release build's code object)
#endif
static inline std::optional<int> alt_int(const char* name) {
  const char* v = alt_env(name);
  return v ? std::optional<int>(atoi(v)) : std::nullopt;
}

struct mia_hip_ctx {
  int device = 0;
  int cus = 1;
  std::string err;
  DevPool pool;                            // device temporaries of the one-off calls (dev_pool.h; pool_take)
  // pinned staging: small copies to and from pageable memory wait for the stream, pinned ones do not
  unsigned char* h_pin = nullptr; static constexpr size_t PIN_BYTES = 1 << 20, PIN_MISC = 64 << 10;
  // the control block (CTRL_*), twice: the views below look at one half (ctrl_bind); k_ref_prep's shadow launch clears the other, and
  // the call that adopts the shadow's work turns to it -- what the getters read from the device after a step stays as the step left it
  DevBuf<int32_t> d_ctrl; int ctrl_half = 0;
  int32_t* ctrl = nullptr;                 // the current half (view)
  int32_t* d_genn = nullptr;               // CTRL_GENN (view)
  const int32_t* d_ctr0 = nullptr;         // CTRL_C0: the CTRL_CN words the host looks at behind an alignment (view)
  uint32_t dbg = 0;                        // timing experiments only, results are wrong when set (read_alt_switches)

  // ---- streams and events ------------------------------------------------------------------------------------------------
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // the trace DP of the plan's own lists runs beside the values DP
  hipEvent_t ev_cons = nullptr;            // k_cons_scatter's own end, where a shadow launch follows it (ref_ahead_speculate)
  hipStream_t stream3 = nullptr; hipEvent_t ev_join3 = nullptr;                      // ... and both beside the planner and the full-window kernels of the reads the plan gave up on
  // the launches other streams wait for signal their events themselves (launch_k) instead of a marker behind them: a bit per launch, all or none
  uint32_t ext_events = 31u; bool align_end_signalled = false;      // (the alignment's last launch on the context's stream has signalled ev_fork: bx_join_and_retry)
  bool spin_wait = true;                   // mia_hip_iterate's one wait asks (hipStreamQuery) instead of sleeping on an interrupt; MIA_HIP_SPIN_WAIT=0: hipStreamSynchronize
  // HIP-event timers of the kernels bench.py reports, one per stage (mia_hip_stage_stats); pairs are recycled through ev_free
  uint32_t stage_mask = ~0u;               // timed stages (mia_hip_set_stage_mask): an event pair costs the stream a few microseconds
  struct StageTimer { std::vector<std::pair<hipEvent_t, hipEvent_t>> pending; double ms = 0; int64_t launches = 0; };
  StageTimer stg[STG_ALL];
  bool stage_timed(int st) const { return st >= STG_COUNT || ((stage_mask >> st) & 1u); }
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_free;

  // ---- reads (and the matrices they are scored with), reference --------------------------------------------------------------
  // PSSMs (fwd, rc)
  DevBuf<int32_t> d_pssm;
  int max_abs = 0;
  int max_pos = 0;   // largest positive PSSM entry: bounds any score by rows * max_pos
  bool have_pssm = false;
  bool flat = false;
  PackSet packs;
  ReadSet rs{};
  DevBuf<uint8_t> d_packed; DevBuf<uint32_t> d_roff; DevBuf<uint16_t> d_len;
  DevBuf<uint8_t> d_rc, d_sk;
  DevBuf<int32_t> d_as, d_ae, d_score, d_refstart;
  DevBuf<int16_t> d_abr; DevBuf<uint32_t> d_status; DevBuf<int16_t> d_cols;
  int max_len = 0;
  int min_len = 0;                          // shortest stored read
  std::vector<int32_t> h_len;               // read lengths on the host (the score-cut regression of reads of different lengths)
  DevBuf<uint64_t> d_rplanes; int rplane_words = 0;   // bit planes of the stored reads (k_read_planes)
  DevBuf<int32_t> d_umax; bool umax_valid = false;
  // reference
  DevBuf<uint8_t> d_ref; int L = 0, wrap = 0; int explicit_win = 0; bool have_ref = false; bool aligned = false;
  bool ref_mostly_bases = true;            // fewer than 2 % of the reference columns are N
  bool ref_few_n = true;                   // ... fewer than 0.2 %: four windows in five hold none (the quick plan asks those even where the table spells out N columns)
  int64_t kh_entries = 0;                  // > 0: the reference has N columns and its 10-mer table lists them (bandx_body.h, N COLUMNS)

  // ---- plan and full-window kernels ----------------------------------------------------------------------------------------
  DevBuf<int32_t> d_bin_of, d_list, d_wide_list, d_retry_list;
  int32_t* d_bins = nullptr;  // [count N_BINS][off N_BINS][cursor N_BINS][wide_count 1]
  int32_t* d_plan_hdr = nullptr;            // PH_* (k_plan_scan)
  bool deferred = false;                    // align_all: no host round trip before its end
  // trace slabs of the persistent DP grid (one per workgroup, per CPL class)
  DevBuf<unsigned char> d_slabs[N_CPL];
  DevBuf<unsigned char> d_slabs_retry[3];                             // trace slabs of the band kernels' retry launch (see launch_window)
  DevBuf<unsigned char> d_quad_slabs;
  int quad_wgs = 0;
  int grid_wgs = 0;
  int window_wgs[N_CPL] = {0, 0, 0};
  int64_t plain_retried = 0, plain_total = 0;
  bool wide_to_caller = false;             // run_wide marks its reads ST_ESCAPE instead of aligning them (the anchored pass 1)
  // wide scratch
  DevBuf<int32_t> d_scratch; DevBuf<int64_t> d_scratch_off;
  // round 6: the band plan lists the reads it leaves open itself and k_align_open takes them one per wavefront (align_route.h: direct_open):
  // the plan's own open list (n entries), k_align_open's trace slabs (one per workgroup of its grid)
  DevBuf<int32_t> d_open_list; DevBuf<unsigned char> d_slabs_open; bool use_direct_open = true; int64_t direct_open_steps = 0;

  // ---- band pipeline, round 1: the diagonal filter (diag_filter.h) and its banded DP (band_body.h), flat matrix only -----------
  int use_filter = 1;
  DevBuf<int32_t> d_kocc_cnt, d_kocc_pos;   // 10-mer table of the reference (diag_filter.h: KmerOcc)
  DevBuf<uint64_t> d_planes;                // lo | hi | ok, a third of the block each (plane_stride)
  uint32_t* d_filter_n = nullptr; int64_t filter_proven = 0, filter_seen = 0;   // device: {finished by the filter, left over, finished by the banded DP}
  int use_banddp = 1;
  DevBuf<int32_t> d_left_list;
  DevBuf<uint32_t> d_band_slabs;
  int64_t band_done = 0;

  // ---- band pipeline for any PSSM (bandx_kernels.h): plan -> values-only DP -> trace DP ------------------------------------------
  bool bx_ok = false;                       // the matrices allow it (bx_make_tables)
  int use_bx = 1, use_lanes = 1; bool bx_serial = false; uint32_t bx_dbg = 0;
  DevBuf<int32_t> d_bx_sub, d_bx_mrow; DevBuf<int16_t> d_bx_loss, d_bx_dl;   // sub | sub * 256; M; losses; block costs
  int32_t bx_min_m = 0, bx_max_m = 0;
  DevBuf<uint32_t> d_refnib;
  DevBuf<uint32_t> d_khash; DevBuf<int32_t> d_khash_ovf;   // 10-mers of the reference (bandx_body.h: KmerHash)
  DevBuf<KbPair> d_kbits;               // the quick plan's bitmaps over all 4^10 10-mers (bandx_body.h: KmerBits), remade with the table
  int use_quick = 1; int64_t quick_steps = 0;      // the quick plan in front of k_bx_plan's launches
  DevBuf<uint32_t> d_prep_bar; uint32_t prep_bar_count = 0; bool no_prep_fuse = false;   // k_ref_prep's grid barrier
  // REFERENCE AHEAD (ref_ahead.h): a second set of everything k_ref_prep writes.  mia_hip_iterate launches k_ref_prep
  // into it behind the consensus it returns (the string is the next call's reference in every real loop); the next call, if it brings
  // that string, swaps the set into place instead of preparing anything (ref_ahead_adopt).  Barrier counter and `stuck` word are shared
  // with the ordinary launch: both are on the context's stream, one after the other.
  struct RefAhead {
    DevBuf<uint8_t> d_ref; DevBuf<uint64_t> d_planes; DevBuf<uint32_t> d_refnib, d_khash; DevBuf<int32_t> d_khash_ovf; DevBuf<KbPair> d_kbits;
    bool queued = false;                    // a speculative launch with `key` is queued behind this call's k_cons_scatter (not settled yet)
    bool valid = false;                     // a shadow launch is queued or done, `key` and `str` describe it
    RefAheadKey key; std::string str;       // what it was built with; the string as returned
  } ahead;
  bool no_ref_ahead = false;               // (alt build, MIA_HIP_NO_REF_AHEAD=1) no shadow launch
  bool ref_ready = false;                  // this call adopted the shadow's work (AlignRouteIn::ref_ready); never outlives the call
  bool last_route_bx = false;              // the last alignment took the band pipeline
  DevBuf<uint32_t> d_bx_plan; DevBuf<int32_t> d_bx_expect, d_bx_lists;
  DevBuf<BxCandRec> d_bx_cand; bool plan_split = true;      // k_bx_plan's hand-over list between its two launches
  DevBuf<BxCandRec> d_bx_cand2; int use_fine = 1;      // the third launch's list (reads for the fine blocks)
  uint32_t* d_bx_ctr = nullptr;
  DevBuf<uint32_t> d_bx_slabs;
  int bx_values_wgs = 0, bx_trace_wgs = 0;
  DevBuf<uint32_t> d_bx_slabs_late; int bx_late_wgs = 0;
  DevBuf<uint32_t> d_bx_slabs_late2;         // the second late trace's slabs (align_route.h: fork_at_quick)
  DevBuf<int32_t> d_retry2;                                                         // reads no band kernel could finish
  bool diag_scripts_missing = false;       // the last alignment left the scripts of its ST_DIAG reads unwritten (k_diag_scripts)
  int64_t bx_seen = 0, bx_done[3] = {0, 0, 0};   // reads planned on; finished by the plan / the values DP / the trace DP
  int64_t bx_launches = 0;
  uint32_t bx_last[BXC_COUNTERS] = {0};     // counters of the last call (list lengths, reasons a read was not planned)

  // ---- cull ----------------------------------------------------------------------------------------------------------------
  DevBuf<int64_t> d_slot, d_partial, d_total;
  DevBuf<uint8_t> d_slot_dropped, d_drop_f, d_drop_b; int64_t n_slots = 0;
  // stale back_asp emulation (mia_consensus_kernels.h, k_cull_mark)
  DevBuf<int64_t> d_back_slot;             // per read, persistent across iterations
  DevBuf<int64_t> d_front_slot0;           // per read: pass-1 front slot (followed for strand-unknown reads only)
  DevBuf<uint8_t> d_link_mark;             // per read: which of the two is set (cull_body.h: cull_link_mark), kept wherever one of them is written
  DevBuf<int32_t> d_link_act;
  // the kernels take ri, si, lk and tb by value: views, set beside their owners' allocation (mia_hip_upload_reads, ensure_tally, ensure_events)
  RecInfo ri{};                            // per read, per iteration
  DevBuf<int32_t> d_ri_flen, d_ri_blen, d_ri_actf, d_ri_trec;
  SlotInfo si{};                           // per local slot, per iteration
  DevBuf<int32_t> d_si_reclen, d_si_recact, d_si_mult; DevBuf<unsigned long long> d_si_writer;
  Links lk{};                              // links produced by this context in the last cull
  DevBuf<int64_t> d_lk_rec;
  int64_t* d_links_all = nullptr; int32_t n_links_all = 0;   // links to apply (own, or gathered from all ranks): lk.rec or owned_links.back()
  int32_t* d_n_links_all = nullptr; int64_t links_cap_all = 0; DevBuf<int32_t> d_n_links_gathered;
  DevBuf<int32_t> d_link_len;
  uint32_t* d_cull_flags = nullptr;
  DevBuf<uint32_t> d_cull_sync;             // k_slot_count's arrival counter (zero between launches)
  DevBuf<unsigned long long> d_sums;
  int64_t read_base = 0;                   // global index of this context's first read (sharded runs)
  int64_t slot_base = 0;
  bool culled = false, links_applied = false;
  std::vector<DevBuf<int64_t>> owned_links;   // gathered link buffers (mia_hip_set_links)
  bool cull_scan = false, tail_scans = false;
  bool cull_with_records = true;           // k_cull_records writes the tally records of an iteration without links itself
  // lean cull (k_cull_records, lean_ok): mia_hip_iterate without a communicator lets an iteration without a link leave d_slot and the
  // side arrays of ri / si unwritten.  d_cull_stats: {links counted before the cull or -1, 1 if the lean form ran}, written by the kernel
  bool no_cull_lean = false;
  bool no_cull_apply = false;              // the links of such an iteration by a launch of k_links_apply, not by k_cull_records' last workgroup
  bool cull_applied = false;               // the last cull was launched with the ticket: its own links are applied already
  bool cull_lean_ok = false;               // the last cull was launched with lean_ok: whether it ran lean is d_cull_stats[1]
  DevBuf<int32_t> d_cull_stats;
  int64_t pre_cull_records = 0, pre_cull_links = 0; bool pre_cull_valid = false;   // mia_hip_score_sums' by-products

  // ---- tally and consensus -------------------------------------------------------------------------------------------------
  TallyBuf tb{}; DevBuf<int32_t> d_tb_tally, d_ins_off, d_ins_total; DevBuf<uint64_t> d_tb_events;
  DevBuf<int32_t> d_ins_tally; DevBuf<char> d_calls, d_ins_calls;
  int64_t ins_tally_cap = 0;               // insert slots d_ins_tally and d_ins_calls both hold: a kernel argument (like tb.cap_events), set with them in mia_hip_consensus
  int32_t n_events_host = 0; bool tallied = false;
  int64_t ins_total_host = 0;
  bool consensus_done = false;
  bool fake_event_overflow = false;
  bool no_linear_tally = false, sort2_unpacked = false;
  bool tally_linear = false;               // the score words of a column are linear in its base counts: the tally counts only (mia_hip_set_pssm)
  int tally_pk_bias = -1;                   // the tally's packed end-base sums (k_tally_binned): the bias that makes every score positive, or -1: entries too large
  // read bucketing for the LDS-privatised tally
  int use_binned_tally = 1;
  DevBuf<int32_t> d_bucket, d_order;
  int bucket_clean_nb = -1;                 // the tally's bucket counts are zero for this bucket count (k_bucket_scan leaves them so)
  int buckets_queued = 0;                   // the tally's counting sort is already queued: 1 on the context's stream, 2 on stream2 (ev_join behind it)
  bool no_side_buckets = false;
  DevBuf<int32_t> d_tally_slabs;   // one LDS window per tally workgroup, summed by k_tally_reduce
  DevBuf<int32_t> d_gen_list;             // the reads k_tally_binned leaves to k_tally_reduce's extra workgroups (a thousand in a million; room for all)
  bool tally_defer = true;                 // ... false: they are taken inside k_tally_binned, one per wavefront
  // position-specific matrices: a workgroup's reads all of one strand, sorted by start (round 5).  Measured against round 4's tally:
  // configs[2] 1.313 -> 1.306 ms, configs[4] at 5 M reads 9.91 -> 10.2 ms (twice the part-filled workgroups and slabs; the end rows'
  // packed atomics are what the kernel waits for either way)
  bool tally_strand_split = true;
  bool tally_rall = true;                  // reads of 129 .. 256 bases: every row through the runs
  bool tally_runs = true;                  // ... and the rows at either end of a read reduced over runs of equal starts
  DevBuf<int32_t> d_order2; DevBuf<uint8_t> d_okey; DevBuf<int32_t> d_sort2;      // the reads of every bucket by start; histogram + cursors of that sort

  // ---- iterate: one iteration with the planner's answers, the cut line and the insert-event count left on the device ------------
  bool in_iterate = false;                  // the control block was cleared as a whole by the alignment's one memset
  // no host wait behind the alignment: cull, tally and consensus are queued at once and every one of their kernels returns at its
  // first instruction if *abort_if != 0 (reads are waiting for the exact one-read-per-thread kernel: the host sees that with the
  // consensus, runs it, and queues the chain again)
  const int32_t* abort_if = nullptr;
  bool spec_ok = false, spec_pending = false, spec_filtered = false, spec_bx = false, spec_plain = false;
  int64_t spec_redone = 0;                  // iterations whose cull / tally / consensus were queued twice (reads for the exact kernel)
  bool no_spec = false;
  bool spec_force = false; DevBuf<int32_t> d_one;      // (tests) every iteration takes the second round; a word that holds 1
  bool pend_encode = false; int32_t pend_L = 0, pend_wl = 0, pend_total = 0;      // d_ascii holds the new reference, d_ref not yet
  bool zero_copy = true;                   // the last kernel writes consensus and counters into pinned host memory itself
  const double* dev_cut = nullptr; DevBuf<double> d_cut_buf;
  DevBuf<char> d_ascii; const char* ascii_src = nullptr;     // ascii_src: where the pending reference is read from (d_ascii, or the pinned staging area)
  DevBuf<char> d_cons;                                       // result of an iteration: [CH_WORDS header][consensus string]
  DevBuf<int32_t> d_cons_pos;
  unsigned char* h_pin2 = nullptr; size_t pin2_bytes = 0;   // results of an iteration (header + consensus string)
  int64_t iter_fallbacks = 0;

  // ---- one-off calls: pass 1, Myers, trimming ---------------------------------------------------------------------------------
  double pass1_ms = 0; int64_t pass1_filtered = 0, pass1_anchored = 0;   // reads of the last pass-1 call that the diagonal filter decided
  double myers_kernel_ms = 0; bool myers_no_lanes = false, myers_no_ond = false;   // the kernels of the last mia_hip_myers call (HIP events)
  int64_t trim_escapes = 0;   // reads of the last mia_hip_trim call that took the exact scalar path
  int64_t trim_launches = 0, trim_scratch_bytes = 0;   // ... in how many k_trim_wide launches, on how large a scratch
  bool trim_exact = false;    // (alt build) every read of a mia_hip_trim call is re-run by the exact scalar kernel
  // the records of the last mia_hip_ma_tally stay on the device for mia_hip_ma_region: start, col_off, seq, the INS_POS pairs (and
  // which pairs each record owns), ref->gaps; the region's column map, selected records and text
  bool ma_resident = false; int64_t ma_n = 0, ma_n_ins = 0; int32_t ma_L = 0;
  DevBuf<int32_t> d_ma_start, d_ma_gaps, d_ma_ipos, d_ma_rec_ins, d_ma_ins_list;
  DevBuf<int64_t> d_ma_coff, d_ma_ioff, d_ma_colmap, d_ma_rows;
  DevBuf<char> d_ma_seq, d_ma_ib, d_ma_text;
  DevBuf<unsigned long long> d_ma_ctl;
  // what the exports' calls found, per export (the big results are further down): mia_hip_ma_tally forgets all of it at once
  struct MaOut {
    bool region_done = false, ace_done = false, sam_done = false, prof_done = false, ends_done = false, cols_done = false, damage_done = false, mask_done = false, score_done = false;
    int32_t first = 0, last = -1; int64_t rows = 0, width = 0, ace_bytes = 0, sam_bytes = 0;
  } ma_out;
  // ... and for mia_hip_ma_ace: whether the job has an ACE export at all (GAPS, the records' columns), the running sum of ref->gaps,
  // per record the AF position, the padded length and the offset of its text, the text
  bool ma_ace_gaps_ok = false, ma_ace_cols_ok = false;
  DevBuf<int64_t> d_ace_g, d_ace_af, d_ace_len, d_ace_off; DevBuf<char> d_ace_body;
  // ... and for mia_hip_ma_sam: whether GAPS is well-formed, the reference, the index of the records' inserts, per record NM, the bytes
  // of its CIGAR and the offset of its body, the bodies, the layout's control words
  bool ma_sam_gaps_ok = false;
  DevBuf<char> d_sam_ref, d_sam_body; DevBuf<int64_t> d_sam_cum, d_sam_cig, d_sam_off; DevBuf<int32_t> d_sam_nm;
  DevBuf<unsigned long long> d_sam_ctl;
  // ... and for mia_hip_ma_profile: strands and depth codes stay behind the tally as well; the reference, the selection, the 808 bins
  // (ma_profile_body.h) on the device and, after the call, here
  DevBuf<uint8_t> d_ma_rev, d_prof_use; DevBuf<char> d_ma_smp, d_prof_ref; DevBuf<unsigned long long> d_prof_bins;
  int64_t ma_cols = 0; int64_t ma_prof_bins[MA_PROF_BINS] = {0};
  // ... and for mia_hip_ma_ends, which shares the reference's and the selection's buffers with the profile (either call's results are on
  // the host when it returns): the segment characters, the 1 267 bins (ma_ends_body.h) on the device and, after the call, here
  DevBuf<uint8_t> d_ends_seg; DevBuf<unsigned long long> d_ends_bins;
  int64_t ma_ends_bins[MA_ENDS_BINS] = {0};
  // ... and for mia_hip_ma_cols, which takes the segments and the selection into the same buffers: the sixteen words per reference
  // column (ma_cols_body.h) and the two counts of what lies on no column, on the device and, after the call, here
  DevBuf<uint32_t> d_cols_tab; DevBuf<unsigned long long> d_cols_out;
  std::vector<int32_t> ma_cols_tab;
  // ... and mia_hip_ma_dedup, which needs no tally in front of it: the records' coordinates, strands, scores and mates, the two sides
  // of the radix sort and its counts, runs, jumps, marks, clusters (mia_ma_dedup_kernels.h); keep and rep stay on the device until
  // mia_hip_get_ma_dedup, the histogram and the totals are here
  struct MaDedup {
    bool done = false; int64_t n = 0, molecules = 0, clusters = 0, orphans = 0;
    DevBuf<int32_t> d_start, d_end, d_score; DevBuf<uint8_t> d_rc, d_keep; DevBuf<int64_t> d_mate, d_rep;
    DevBuf<unsigned long long> d_key[2], d_runkey, d_best, d_ctl, d_hist;
    DevBuf<uint32_t> d_val[2], d_jump[2], d_counts, d_runid, d_first, d_mark, d_cluster, d_anchor;
    int64_t hist[MA_DEDUP_HIST] = {0};
    // ... and what mia_hip_ma_collapse needs of the call behind it: the side of the sort that holds the sorted order, the runs, whether
    // mates were given, the reference length, and the tally the call came after (0: none)
    int sorted_side = 0; int64_t runs = 0; bool has_mate = false; int32_t L = 0; uint64_t tally_no = 0;
  } dedup;
  uint64_t ma_tally_no = 0;                 // counts the successful mia_hip_ma_tally calls

  // ... and mia_hip_ma_collapse, which reads the tallied records and what mia_hip_ma_dedup left: the tallied record of every record of
  // the filter and the votes, per cluster the representative's records and the place of its counts, the count array, members, SEQ', the
  // scan's control words, and the 72 bins (ma_collapse_body.h) on the device and, after the call, here.  The next mia_hip_ma_tally or
  // mia_hip_ma_dedup invalidates it.
  struct MaCollapse {
    bool done = false, launched = false; int64_t n = 0, cols = 0, collapsed = 0, changed = 0;
    DevBuf<int32_t> d_rec_of, d_rep_f, d_rep_b, d_members; DevBuf<uint8_t> d_vote; DevBuf<int64_t> d_cnt_off; DevBuf<uint32_t> d_cnt; DevBuf<char> d_seq;
    DevBuf<unsigned long long> d_ctl, d_hist;
    int64_t hist[MA_COL_HIST] = {0};
  } collapse;

  // ... and mia_hip_ma_damage, which reads the tallied records and shares the reference's and the selection's buffers with the profile:
  // the pairing, per record 16 - k of its best hit at either end (hit5 | hit3, zeroed before the launch), pos5 | pos3 and keep, which
  // stay on the device until mia_hip_get_ma_damage; the 514 bins (ma_damage_body.h) on the device and, after the call, here
  struct MaDamage {
    DevBuf<int64_t> d_mate; DevBuf<uint32_t> d_hit; DevBuf<uint8_t> d_pos, d_keep; DevBuf<unsigned long long> d_bins;
    int64_t bins[MA_DMG_BINS] = {0};
  } damage;

  // ... and mia_hip_ma_mask, which reads the tallied records alone: per record a1 | b1 of the bounds stage (lo preset to all ones, hi
  // to 0), first | count | start' and col_off' of the layout, the new strings (padded to a multiple of 16), the pairs' fate, the scan's
  // control words, and the 133 bins (ma_mask_body.h) on the device and, after the call, here.  All of it stays on the device until
  // mia_hip_get_ma_mask; the next mia_hip_ma_tally invalidates it.
  struct MaMask {
    DevBuf<uint32_t> d_lohi; DevBuf<int32_t> d_rec, d_ipos; DevBuf<int64_t> d_off; DevBuf<char> d_seq, d_smp; DevBuf<uint8_t> d_pair_keep;
    DevBuf<unsigned long long> d_ctl, d_bins;
    int64_t bins[MA_MASK_BINS] = {0}, cols_kept = 0; int32_t mode = 0;
  } mask;

  // ... and mia_hip_ma_score, which reads the tallied records and shares the reference's and the selection's buffers with the profile:
  // the pairing, the 775 weights, per record the sum of its weights (zeroed before the launch), its molecule's score and keep, which
  // stay on the device until mia_hip_get_ma_score; the 130 bins (ma_pmd_body.h) on the device and, after the call, here
  struct MaScore {
    DevBuf<int64_t> d_mate, d_mol; DevBuf<int32_t> d_w; DevBuf<uint8_t> d_keep; DevBuf<unsigned long long> d_rec, d_bins;
    int64_t bins[MA_PMD_BINS] = {0};
  } score;

  // ---- comm: sharded runs, one context per GPU; the exchanges go through a table of collectives (RCCL over xGMI from
  // mia_hip_comm_init, or whatever mia_hip_comm_attach was given), on the context's own stream ------------------------------------
  mia_hip_collectives coll{}; bool comm = false; int comm_ranks = 1, comm_rank = 0; std::string coll_name;
  DevBuf<unsigned long long> d_gather;      // [PRE_WORDS * ranks] score sums, record, link and exact-kernel counts of every rank
  std::vector<int64_t> h_gather;            // ... on the host, once the alignment's one wait is over
  int64_t ev_pad = 0;                       // insert events per rank the event all-gather is sized for (0: not known yet)
  DevBuf<int64_t> d_lstage, d_lmine, d_lall;                 // links / insert events of all ranks, padded to the longest
  DevBuf<int32_t> d_scores_all;
};

// The alternative routes and diagnostics of libmia_hip_alt.so (alt_env reads nothing in the release build), one line each.  What the
// alignment's switches do to the route is decided in ONE place, align_route.h (align_route); these lines only set the fields.  The rest
// are read where they apply: MIA_HIP_ITER_DEBUG and MIA_HIP_EV_PAD (mia_hip_iterate), MIA_HIP_P1_TIMING (mia_hip_pass1),
// MIA_HIP_PEAK_DEBUG (mia_hip_peak).  MIA_HIP_P1_CPL and MIA_HIP_P1_PLAIN are parsed in one spot, with every call (pass1_route_input),
// and handed to pass1_route.h, which decides what they do.
static void read_alt_switches(mia_hip_ctx* ctx) {
  auto on = [](const char* name) { const char* v = alt_env(name); return v && atoi(v) != 0; };
  // alignment: which kernels take the reads
  if (on("MIA_HIP_NO_DIAG_FILTER")) { ctx->use_filter = 0; ctx->use_bx = 0; }      // every shortcut off: the full-window DP kernels only
  if (on("MIA_HIP_NO_BAND_DP")) { ctx->use_banddp = 0; ctx->use_bx = 0; }          // flat matrix: the filter's left-overs go straight to the full-window kernels
  if (on("MIA_HIP_NO_BANDX")) ctx->use_bx = 0;                 // the round-1 path (flat: filter + k_band_align; PSSM: full-window kernels)
  if (on("MIA_HIP_NO_LANES")) ctx->use_lanes = 0;              // the band DPs one read per lane (k_bx_values / k_bx_trace) instead of W/8 lanes per read
  if (on("MIA_HIP_BX_SERIAL")) ctx->bx_serial = true;          // round 2's order: band kernels, then the planner over everything they left open
  if (on("MIA_HIP_NO_PLAN_SPLIT")) ctx->plan_split = false;    // k_bx_plan in one launch
  if (on("MIA_HIP_NO_FINE")) ctx->use_fine = 0;                // no third launch of the plan (fine blocks)
  if (const char* v = alt_env("MIA_HIP_FINE")) ctx->use_fine = atoi(v);            // 2: the third launch in every iteration
  if (on("MIA_HIP_NO_QUICK_PLAN")) ctx->use_quick = 0;         // the full plan for every read
  if (const char* v = alt_env("MIA_HIP_QUICK_PLAN")) ctx->use_quick = atoi(v);     // 2: the quick plan also where align_all's size rule says no
  if (on("MIA_HIP_NO_DIRECT_OPEN")) ctx->use_direct_open = false;                  // open reads through the planner's count / scan / fill and the quad kernels
  if (on("MIA_HIP_NO_PREP_FUSE")) ctx->no_prep_fuse = true;    // six launches instead of k_ref_prep
  if (on("MIA_HIP_NO_REF_AHEAD")) ctx->no_ref_ahead = true;    // no k_ref_prep behind the consensus for the next call (ref_ahead.h)
  // mia_hip_iterate: what is queued when
  if (on("MIA_HIP_NO_SPEC")) ctx->no_spec = true;              // wait for the alignment's counters before the cull is queued
  if (on("MIA_HIP_SPEC_TEST")) ctx->spec_force = true;         // every iteration queues cull / tally / consensus twice
  if (on("MIA_HIP_NO_SIDE_BUCKETS")) ctx->no_side_buckets = true;                  // the tally's counting sort behind the cull, not beside it
  if (on("MIA_HIP_NO_ZERO_COPY")) ctx->zero_copy = false;      // consensus and counters by two copies
  if (on("MIA_HIP_NO_EXT_EVENTS")) ctx->ext_events = 0u;       // marker events behind the launches other streams wait for
  if (on("MIA_HIP_FAKE_EVENT_OVERFLOW")) ctx->fake_event_overflow = true;          // (tests) this rank pretends its insert-event list overflowed
  // cull and tally
  if (on("MIA_HIP_CULL_SCAN")) ctx->cull_scan = true;          // the slot scan as a kernel of its own (k_scan_partials)
  if (on("MIA_HIP_TAIL_SCANS")) ctx->tail_scans = true;        // the consensus tail's scans as single-workgroup kernels of their own
  if (on("MIA_HIP_NO_CULL_RECORDS")) ctx->cull_with_records = false;               // k_rec_params writes every tally record
  if (on("MIA_HIP_NO_CULL_LEAN")) ctx->no_cull_lean = true;    // k_cull_records writes d_slot and the side arrays in every iteration
  if (on("MIA_HIP_NO_CULL_APPLY")) ctx->no_cull_apply = true;  // k_links_apply as a launch of its own in every iteration
  if (on("MIA_HIP_NO_BINNED_TALLY")) ctx->use_binned_tally = 0;                    // plain global-atomic tally
  if (on("MIA_HIP_NO_LINEAR_TALLY")) ctx->no_linear_tally = true;                // the tally adds the four scores of every base even where counting would do
  if (on("MIA_HIP_SORT2_UNPACKED")) ctx->sort2_unpacked = true;                  // the second sort's key in a byte array beside the entries, as from 2^24 reads
  if (on("MIA_HIP_TALLY_INLINE")) ctx->tally_defer = false;    // gapped reads inside k_tally_binned, one per wavefront
  if (const char* v = alt_env("MIA_HIP_STRAND_SPLIT")) ctx->tally_strand_split = atoi(v) != 0;      // 0: round 4's tally for position-specific matrices
  if (on("MIA_HIP_NO_TALLY_RUNS")) ctx->tally_runs = false;    // end rows per read, not per run of equal starts
  if (on("MIA_HIP_NO_TALLY_RALL")) ctx->tally_rall = false;    // round 4's tally for reads of 129 .. 256 bases
  // Myers
  if (on("MIA_HIP_MYERS_NO_LANES")) ctx->myers_no_lanes = true;                    // every pair through k_myers
  if (on("MIA_HIP_MYERS_NO_OND")) ctx->myers_no_ond = true;    // no O(ND) kernel
  // trimming
  if (on("MIA_HIP_TRIM_EXACT")) ctx->trim_exact = true;        // every read through k_trim_wide, after k_trim has run
  // profiling: results are wrong on purpose
  if (const char* v = alt_env("MIA_HIP_DEBUG_SKIP")) ctx->dbg = (uint32_t)atoi(v);                  // bits: see the kernels' dbg tests
  if (const char* v = alt_env("MIA_HIP_BX_DEBUG")) ctx->bx_dbg = (uint32_t)atoi(v);                 // 1 no traceback, 2 one DP row, 4 no values launch, 8 no trace launch, ...
}

#define HIPCHK(call)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess) {                                                                            \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                                    \
      return MIA_HIP_ERR_DEVICE;                                                                       \
    }                                                                                                  \
  } while (0)

// what a DevBuf's alloc / ensure answered, as the ABI's code (and the context's message)
static int dev_nomem(mia_hip_ctx* ctx, hipError_t e) {
  if (e == hipSuccess) return MIA_HIP_OK;
  ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
  return MIA_HIP_ERR_NOMEM;
}
template <class T>
static int dev_alloc(mia_hip_ctx* ctx, DevBuf<T>& b, int64_t n) { return dev_nomem(ctx, b.alloc(n)); }
template <class T>
static int dev_ensure(mia_hip_ctx* ctx, DevBuf<T>& b, int64_t need, int64_t alloc_elems) { return dev_nomem(ctx, b.ensure(need, alloc_elems)); }
template <class T>
static int dev_ensure(mia_hip_ctx* ctx, DevBuf<T>& b, int64_t need) { return dev_nomem(ctx, b.ensure(need, need)); }

// A temporary of a one-off call (pass 1, Myers): a block of the context's pool, lent until the lease goes out of scope (dev_pool.h)
template <class T>
static int pool_take(mia_hip_ctx* ctx, PoolLease<T>& lease, size_t n) { return dev_nomem(ctx, lease.take(ctx->pool, n)); }

// THE one place where the views into the control block are set: at context creation, and when a call adopts the tables prepared
// ahead together with the half of the block that was cleared for them (ref_ahead_adopt).  A view that is derived from one of these
// (d_n_links_all while it names this context's own link count) follows.
static_assert(CTRL_WORDS % 64 == 0, "the second half of the control block starts on a cache line, as the first does");
static void ctrl_bind(mia_hip_ctx* ctx, int half) {
  const bool own_links = ctx->d_n_links_all && ctx->d_n_links_all == ctx->lk.n;
  int32_t* b = ctx->d_ctrl + (size_t)half * CTRL_WORDS;
  ctx->ctrl_half = half;
  ctx->ctrl = b;
  ctx->d_bins = b + CTRL_BINS;
  ctx->d_plan_hdr = b + CTRL_HDR;
  ctx->d_filter_n = reinterpret_cast<uint32_t*>(b + CTRL_FILTER);
  ctx->lk.n = b + CTRL_LKN;
  ctx->d_cull_flags = reinterpret_cast<uint32_t*>(b + CTRL_CULLF);
  ctx->tb.n_events = b + CTRL_NEV;
  ctx->tb.flags = reinterpret_cast<uint32_t*>(b + CTRL_TFLAGS);
  ctx->d_genn = b + CTRL_GENN;
  ctx->d_bx_ctr = reinterpret_cast<uint32_t*>(b + CTRL_BXC);
  ctx->d_ctr0 = b + CTRL_C0;
  if (own_links) ctx->d_n_links_all = ctx->lk.n;
}

extern "C" const char* mia_hip_last_error(const mia_hip_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int mia_hip_create(mia_hip_ctx** out, int device_index) {
  if (!out) return MIA_HIP_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MIA_HIP_ERR_DEVICE;   // no CPU fallback, by design
  if (device_index < 0 || device_index >= ndev) return MIA_HIP_ERR_ARG;
  mia_hip_ctx* ctx = new mia_hip_ctx();
  ctx->device = device_index;
  const unsigned evf = hipEventDisableTiming;
  if (hipSetDevice(device_index) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_join3, evf) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_cons, evf) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_fork, evf) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_join, evf) != hipSuccess) {
    delete ctx;
    return MIA_HIP_ERR_DEVICE;
  }
  {
    // persistent DP grid: one 64-lane workgroup per wave slot of the chip (8 waves/SIMD x 4 SIMDs x CUs)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_index) != hipSuccess) { delete ctx; return MIA_HIP_ERR_DEVICE; }
    ctx->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
    ctx->grid_wgs = prop.multiProcessorCount * 32;
    ctx->quad_wgs = prop.multiProcessorCount * 16;   // 128 VGPRs -> 4 waves per SIMD
    read_alt_switches(ctx);
    if (const char* sw = getenv("MIA_HIP_SPIN_WAIT")) ctx->spin_wait = atoi(sw) != 0;
  }
  if (dev_alloc(ctx, ctx->d_pssm, 2 * PSSM_WORDS) || dev_alloc(ctx, ctx->d_ctrl, 2 * CTRL_WORDS) ||
      dev_alloc(ctx, ctx->d_total, 1) || dev_alloc(ctx, ctx->d_ins_total, 1) ||
      dev_alloc(ctx, ctx->d_bx_sub, 2 * BX_SUB_WORDS) || dev_alloc(ctx, ctx->d_bx_mrow, 2 * 31 * 4) || dev_alloc(ctx, ctx->d_bx_loss, BX_LOSS_WORDS) ||
      dev_alloc(ctx, ctx->d_bx_dl, BX_DL_WORDS) ||
      dev_alloc(ctx, ctx->d_cut_buf, 2)) {
    delete ctx;
    return MIA_HIP_ERR_NOMEM;
  }
  ctrl_bind(ctx, 0);
  if (hipMemset(ctx->d_ctrl, 0, 2 * CTRL_WORDS * 4) != hipSuccess) { delete ctx; return MIA_HIP_ERR_DEVICE; }
  {
    const int32_t one = 1;
    if (dev_alloc(ctx, ctx->d_one, 1) || hipMemcpy(ctx->d_one, &one, 4, hipMemcpyHostToDevice) != hipSuccess) { delete ctx; return MIA_HIP_ERR_DEVICE; }
    if (dev_alloc(ctx, ctx->d_prep_bar, 1) || hipMemset(ctx->d_prep_bar, 0, 4) != hipSuccess) { delete ctx; return MIA_HIP_ERR_DEVICE; }
  }
  if (hipHostMalloc((void**)&ctx->h_pin, mia_hip_ctx::PIN_BYTES, hipHostMallocDefault) != hipSuccess) ctx->h_pin = nullptr;   // optional
  if (ctx->h_pin) memset(ctx->h_pin, 0, mia_hip_ctx::PIN_MISC);
  else ctx->no_prep_fuse = true;            // (k_ref_prep reports a barrier it gave up on through a pinned word: without one, six plain launches)
  *out = ctx;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_comm_destroy(mia_hip_ctx* ctx);
extern "C" void mia_hip_destroy(mia_hip_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  (void)mia_hip_comm_destroy(ctx);
  if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
  if (ctx->h_pin2) (void)hipHostFree(ctx->h_pin2);
  for (auto& e : ctx->ev_free) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (auto& t : ctx->stg) for (auto& e : t.pending) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  (void)hipStreamDestroy(ctx->stream);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
  if (ctx->ev_join3) (void)hipEventDestroy(ctx->ev_join3);
  if (ctx->ev_cons) (void)hipEventDestroy(ctx->ev_cons);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  delete ctx;                               // its DevBuf members free every device block, the pool's included
}

extern "C" int mia_hip_sync(mia_hip_ctx* ctx) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

extern "C" int mia_hip_set_pssm(mia_hip_ctx* ctx, const int32_t* fwd, const int32_t* rc) {
  if (!ctx || !fwd || !rc) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  int m = 0;
  for (int i = 0; i < PSSM_WORDS; i++) {
    int a = fwd[i] < 0 ? -fwd[i] : fwd[i], b = rc[i] < 0 ? -rc[i] : rc[i];
    if (a > m) m = a;
    if (b > m) m = b;
  }
  if (m > 32000) { ctx->err = "PSSM entries beyond +-32000 do not fit the int16 substitution table"; return MIA_HIP_ERR_RANGE; }
  ctx->max_abs = m;
  {
    int lo = 0, hi = 0;
    for (int k = 0; k < PSSM_WORDS; k++) { lo = std::min(lo, std::min((int)fwd[k], (int)rc[k])); hi = std::max(hi, std::max((int)fwd[k], (int)rc[k])); }
    ctx->tally_pk_bias = -lo + hi <= 2047 ? -lo : -1;
  }
  ctx->max_pos = 0;
  for (int i = 0; i < PSSM_WORDS; i++) { if (fwd[i] > ctx->max_pos) ctx->max_pos = fwd[i]; if (rc[i] > ctx->max_pos) ctx->max_pos = rc[i]; }
  const int cpls[N_CPL] = {4, 8, 12};
  for (int c = 0; c < N_CPL; c++) ctx->packs.ok[c] = make_pack_params(64 * cpls[c], m, &ctx->packs.p[c]) ? 1 : 0;
  HIPCHK(hipMemcpyAsync(ctx->d_pssm, fwd, PSSM_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_pssm + PSSM_WORDS, rc, PSSM_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->have_pssm = true;
  ctx->flat = pssm_is_flat(fwd, rc);
  // the score words of a column are linear in its base counts iff sm[d][X][b] (X = A,C,G,T; src/map_align.c:258-261)
  // depends neither on the depth nor on the strand: k_tally_binned then counts only and derives the scores
  ctx->tally_linear = true;
  for (int d = 0; d < 2 * PSSM_DEPTH + 1; d++)
    for (int x = 0; x < 4; x++)
      for (int b = 0; b < 5; b++)
        if (fwd[(d * 5 + x) * 5 + b] != fwd[x * 5 + b] || rc[(d * 5 + x) * 5 + b] != fwd[x * 5 + b]) ctx->tally_linear = false;
  if (ctx->no_linear_tally) ctx->tally_linear = false;
  // tables of the band pipeline (bandx_body.h): substitution scores by (strand, depth, read base, reference code), the best
  // score of every row kind, and what a non-identical base costs at least
  {
    std::vector<int32_t> sub(2 * BX_SUB_WORDS, 0), mrow(2 * 31 * 4, 0);
    std::vector<int16_t> loss(BX_LOSS_WORDS, 0), dl(BX_DL_WORDS, 0);
    ctx->bx_ok = bx_make_tables(fwd, rc, sub.data(), mrow.data(), loss.data(), dl.data(), &ctx->bx_min_m, &ctx->bx_max_m);
    if (ctx->bx_ok) {
      for (int k = 0; k < BX_SUB_WORDS; k++) sub[(size_t)BX_SUB_WORDS + k] = sub[(size_t)k] * 256;
      HIPCHK(hipMemcpyAsync(ctx->d_bx_sub, sub.data(), sub.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(ctx->d_bx_mrow, mrow.data(), mrow.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(ctx->d_bx_loss, loss.data(), loss.size() * 2, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(ctx->d_bx_dl, dl.data(), dl.size() * 2, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->umax_valid = false;
    if (ctx->bx_ok && ctx->d_umax && ctx->rs.n > 0) {
      hipLaunchKernelGGL(k_bx_umax, dim3((unsigned)((ctx->rs.n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rs, ctx->d_bx_mrow, ctx->d_umax);
      HIPCHK(hipGetLastError());
      ctx->umax_valid = true;
    }
  }
  return MIA_HIP_OK;
}

static inline uint8_t base_code(char b) {   // src/map_align.c:16-29: only upper-case ACGT are bases
  switch (b) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; }
}

// 4-bit base codes, two per byte, each read starting on a 4-byte boundary of `packed` (zero-filled by the caller)
// (on the host's threads: a million reads are 100 MB of characters, 0.1 s on one core -- as long as thirty iterations)
static void pack_reads(int64_t n, const char* bases, const int64_t* offsets, const uint32_t* roff, const uint16_t* len, uint8_t* packed) {
  uint8_t lut[256];
  for (int c = 0; c < 256; c++) lut[c] = base_code((char)c);
  auto range = [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; i++) {
      const unsigned char* s = reinterpret_cast<const unsigned char*>(bases) + offsets[i];
      uint8_t* d = packed + roff[i];
      const int l = len[i];
      int k = 0;
      for (; k + 1 < l; k += 2) d[k >> 1] = (uint8_t)(lut[s[k]] | (lut[s[k + 1]] << 4));
      if (k < l) d[k >> 1] = lut[s[k]];
    }
  };
  int T = (int)std::thread::hardware_concurrency();
  if (const char* e = getenv("MIA_HIP_THREADS")) T = atoi(e);
  T = std::max(1, std::min(std::min(T, 32), (int)(n / 16384) + 1));
  if (T == 1) { range(0, n); return; }
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back(range, n * t / T, n * (t + 1) / T);
  range(0, n / T);
  for (auto& x : th) x.join();
}

extern "C" int mia_hip_upload_reads(mia_hip_ctx* ctx, int64_t n, const char* bases, const int64_t* offsets, const uint8_t* rc,
                                    const uint8_t* strand_known, const int32_t* as, const int32_t* ae) {
  if (!ctx || n < 0 || (n > 0 && (!bases || !offsets || !rc || !strand_known || !as || !ae))) return MIA_HIP_ERR_ARG;
  if (n >= (int64_t)1 << 31) { ctx->err = "more than 2^31 reads per context"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<uint32_t> roff((size_t)n);
  std::vector<uint16_t> len((size_t)n);
  uint64_t total = 0;
  int max_len = 1;
  for (int64_t i = 0; i < n; i++) {
    int64_t l = offsets[i + 1] - offsets[i];
    if (l < 1 || l > MIA_HIP_MAX_READ) { ctx->err = "read length outside 1..256 (INIT_ALN_SEQ_LEN)"; return MIA_HIP_ERR_ARG; }
    roff[i] = (uint32_t)total;
    len[i] = (uint16_t)l;
    if (l > max_len) max_len = (int)l;
    total += (uint64_t)(((l + 1) / 2 + 3) & ~3);
    if (total >= ((uint64_t)1 << 32)) { ctx->err = "packed read store exceeds 4 GiB per context"; return MIA_HIP_ERR_ARG; }
  }
  std::vector<uint8_t> packed((size_t)total + 8, 0);
  pack_reads(n, bases, offsets, roff.data(), len.data(), packed.data());
  ctx->max_len = max_len;
  ctx->min_len = max_len;
  ctx->h_len.assign(len.begin(), len.end());
  for (int64_t i = 0; i < n; i++) if ((int)len[(size_t)i] < ctx->min_len) ctx->min_len = len[(size_t)i];
  const int stride = (max_len + 3) & ~3;
  int nomem = 0;
  nomem |= dev_alloc(ctx, ctx->d_packed, packed.size());
  nomem |= dev_alloc(ctx, ctx->d_roff, n);
  nomem |= dev_alloc(ctx, ctx->d_len, n);
  nomem |= dev_alloc(ctx, ctx->d_rc, n);
  nomem |= dev_alloc(ctx, ctx->d_sk, n);
  nomem |= dev_alloc(ctx, ctx->d_as, n);
  nomem |= dev_alloc(ctx, ctx->d_ae, n);
  nomem |= dev_alloc(ctx, ctx->d_score, n);
  nomem |= dev_alloc(ctx, ctx->d_refstart, n);
  nomem |= dev_alloc(ctx, ctx->d_abr, n);
  nomem |= dev_alloc(ctx, ctx->d_status, n);
  nomem |= dev_alloc(ctx, ctx->d_cols, n * stride);
  nomem |= dev_alloc(ctx, ctx->d_bin_of, n);
  nomem |= dev_alloc(ctx, ctx->d_umax, n);
  ctx->rplane_words = (max_len + 63) >> 6;
  nomem |= dev_alloc(ctx, ctx->d_rplanes, n * 2 * ctx->rplane_words + 2);      // (+ 2: k_tally_binned asks for a second word of every plane)
  nomem |= dev_alloc(ctx, ctx->d_list, n + 4 * N_BINS);   // quad bins are padded to multiples of four
  nomem |= dev_alloc(ctx, ctx->d_wide_list, n);
  nomem |= dev_alloc(ctx, ctx->d_retry_list, n);
  nomem |= dev_alloc(ctx, ctx->d_slot, n);
  nomem |= dev_alloc(ctx, ctx->d_partial, (size_t)cull_partial_words(n));      // per 256 reads, and behind them twice per 4 096 (k_slot_count, cull_body.h)
  nomem |= dev_alloc(ctx, ctx->d_drop_f, n);
  nomem |= dev_alloc(ctx, ctx->d_drop_b, n);
  nomem |= dev_alloc(ctx, ctx->d_slot_dropped, 2 * n + 16);
  ctx->n_slots = ctx->d_slot_dropped.cap;
  nomem |= dev_alloc(ctx, ctx->d_back_slot, n) | dev_alloc(ctx, ctx->d_front_slot0, n) | dev_alloc(ctx, ctx->d_link_mark, n);
  nomem |= dev_alloc(ctx, ctx->d_ri_flen, n) | dev_alloc(ctx, ctx->d_ri_blen, n) | dev_alloc(ctx, ctx->d_ri_actf, n) |
         dev_alloc(ctx, ctx->d_ri_trec, n * 16);
  const int64_t slot_cap = 2 * n + 16;
  nomem |= dev_alloc(ctx, ctx->d_si_reclen, slot_cap) | dev_alloc(ctx, ctx->d_si_recact, slot_cap) | dev_alloc(ctx, ctx->d_si_writer, slot_cap) |
         dev_alloc(ctx, ctx->d_si_mult, slot_cap);
  ctx->lk.cap = (int32_t)std::min<int64_t>(n + 16, (int64_t)1 << 20);     // link index field of SlotInfo::writer: 20 bits
  if (ctx->lk.cap > (int32_t)LINK_NONE - 1) ctx->lk.cap = (int32_t)LINK_NONE - 1;
  nomem |= dev_alloc(ctx, ctx->d_lk_rec, (size_t)ctx->lk.cap * 4);
  ctx->ri.flen = ctx->d_ri_flen; ctx->ri.blen = ctx->d_ri_blen; ctx->ri.actf = ctx->d_ri_actf; ctx->ri.trec = ctx->d_ri_trec;
  ctx->si.reclen = ctx->d_si_reclen; ctx->si.recact = ctx->d_si_recact; ctx->si.writer = ctx->d_si_writer; ctx->si.mult = ctx->d_si_mult;
  ctx->lk.rec = ctx->d_lk_rec;
  if (nomem) return MIA_HIP_ERR_NOMEM;
  HIPCHK(hipMemcpyAsync(ctx->d_packed, packed.data(), packed.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_roff, roff.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_len, len.data(), (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_rc, rc, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_sk, strand_known, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_as, as, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_ae, ae, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_score, 0, (size_t)n * 4, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_status, 0, (size_t)n * 4, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_abr, 0, (size_t)n * 2, ctx->stream));   // no soft clip known after pass 1
  HIPCHK(hipMemsetAsync(ctx->d_slot_dropped, 0, (size_t)ctx->n_slots, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_back_slot, 0xFF, (size_t)n * 8, ctx->stream));   // -1: never split
  HIPCHK(hipMemsetAsync(ctx->d_front_slot0, 0xFF, (size_t)n * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_link_mark, 0, (size_t)n, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_drop_f, 0, (size_t)n, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_drop_b, 0, (size_t)n, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ReadSet& r = ctx->rs;
  r.n = n; r.packed = ctx->d_packed; r.roff = ctx->d_roff; r.len = ctx->d_len; r.rc = ctx->d_rc; r.sk = ctx->d_sk;
  r.as = ctx->d_as; r.ae = ctx->d_ae; r.score = ctx->d_score; r.refstart = ctx->d_refstart; r.abr = ctx->d_abr;
  r.status = ctx->d_status; r.cols = ctx->d_cols; r.stride = stride;
  ctx->d_order.release(); ctx->d_order2.release(); ctx->d_okey.release();      // sized by n: made again by the next tally
  ctx->umax_valid = false;
  if (n > 0) hipLaunchKernelGGL(k_read_planes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rs, ctx->rplane_words, ctx->d_rplanes);
  if (ctx->have_pssm && ctx->bx_ok && n > 0) {
    hipLaunchKernelGGL(k_bx_umax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rs, ctx->d_bx_mrow, ctx->d_umax);
    HIPCHK(hipGetLastError());
    ctx->umax_valid = true;
  }
  ctx->aligned = false;
  ctx->tallied = false;
  ctx->culled = false;
  return MIA_HIP_OK;
}

// A launch that signals `stop` with its own completion (hipExtLaunchKernelGGL), or a plain launch if stop is null.  An event
// recorded BEHIND a launch is a marker packet of its own: the next kernel of that stream starts 15-20 us later (measured
// between the plan and the values DP), and a stream waiting for the event sees it as late.
template <typename... KArgs, typename... Args>
static void launch_k(void (*kernel)(KArgs...), dim3 g, dim3 b, size_t shm, hipStream_t s, hipEvent_t stop, Args&&... args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "every kernel argument, defaults included");
  if (stop) hipExtLaunchKernelGGL(kernel, g, b, (uint32_t)shm, s, nullptr, stop, 0, static_cast<KArgs>(args)...);
  else hipLaunchKernelGGL(kernel, g, b, shm, s, static_cast<KArgs>(args)...);
}

// an event pair for one launch of stage `st`; the start event is recorded here, the end event by stage_end
static int stage_begin(mia_hip_ctx* ctx, int st, hipStream_t on = nullptr) {
  if (!ctx->stage_timed(st)) return 0;
  if (ctx->ev_free.empty()) {
    hipEvent_t x, y;
    if (hipEventCreate(&x) != hipSuccess || hipEventCreate(&y) != hipSuccess) return -1;
    ctx->ev_free.push_back({x, y});
  }
  auto p = ctx->ev_free.back();
  ctx->ev_free.pop_back();
  ctx->stg[st].pending.push_back(p);
  (void)hipEventRecord(p.first, on ? on : ctx->stream);
  return 0;
}
static void stage_end(mia_hip_ctx* ctx, int st, hipStream_t on = nullptr) {
  if (ctx->stage_timed(st) && !ctx->stg[st].pending.empty()) (void)hipEventRecord(ctx->stg[st].pending.back().second, on ? on : ctx->stream);
}

// One launch of a timed stage whose kernel carries no event for another stream: the event pair rides on the launch itself
// (start and end of that dispatch, no marker packets in front of and behind the kernel -- on the critical path those cost
// the step 10-20 us each, and the timed region of bench.py times the dominant stage in every step); an untimed stage: the
// launch as it is, between stage_begin / stage_end.
template <typename... KArgs, typename... Args>
static int stage_launch(mia_hip_ctx* ctx, int st, void (*kernel)(KArgs...), dim3 g, dim3 b, size_t shm, hipStream_t s, Args&&... args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "every kernel argument, defaults included");
  if (!ctx->stage_timed(st)) {
    if (stage_begin(ctx, st, s)) return -1;
    hipLaunchKernelGGL(kernel, g, b, shm, s, static_cast<KArgs>(args)...);
    stage_end(ctx, st, s);
    return 0;
  }
  if (ctx->ev_free.empty()) {
    hipEvent_t x, y;
    if (hipEventCreate(&x) != hipSuccess || hipEventCreate(&y) != hipSuccess) return -1;
    ctx->ev_free.push_back({x, y});
  }
  auto p = ctx->ev_free.back();
  ctx->ev_free.pop_back();
  ctx->stg[st].pending.push_back(p);
  hipExtLaunchKernelGGL(kernel, g, b, (uint32_t)shm, s, p.first, p.second, 0, static_cast<KArgs>(args)...);
  return 0;
}

// what the recorded event pairs measured goes into their stages' sums; `except`: one stage whose pairs stay pending (its end is not recorded yet)
static void drain_events(mia_hip_ctx* ctx, int except = -1) {
  for (int k = 0; k < STG_ALL; k++) {
    if (k == except) continue;
    auto& t = ctx->stg[k];
    for (auto& e : t.pending) {
      float ms = 0;
      if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) {
        t.ms += ms;
        t.launches++;
      }
      ctx->ev_free.push_back(e);
    }
    t.pending.clear();
  }
}

extern "C" int mia_hip_set_stage_mask(mia_hip_ctx* ctx, uint32_t mask) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  drain_events(ctx);
  ctx->stage_mask = mask;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_stage_stats(mia_hip_ctx* ctx, int reset, int32_t cap, const char** names, double* ms, int64_t* launches, int32_t* n_stages) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  drain_events(ctx);
  if (n_stages) *n_stages = STG_ALL;
  for (int k = 0; k < STG_ALL && k < cap; k++) {
    if (names) names[k] = stage_name(k);
    if (ms) ms[k] = ctx->stg[k].ms;
    if (launches) launches[k] = ctx->stg[k].launches;
  }
  if (reset) for (auto& t : ctx->stg) { t.ms = 0; t.launches = 0; }
  return MIA_HIP_OK;
}

extern "C" int mia_hip_kernel_time(mia_hip_ctx* ctx, int reset, double* align_ms, int64_t* launches) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  drain_events(ctx);
  if (align_ms) *align_ms = ctx->stg[STG_TRACE].ms;
  if (launches) *launches = ctx->stg[STG_TRACE].launches;
  if (reset) { ctx->stg[STG_TRACE].ms = 0; ctx->stg[STG_TRACE].launches = 0; }
  return MIA_HIP_OK;
}

extern "C" int mia_hip_filter_stats(mia_hip_ctx* ctx, int reset, int64_t* reads_seen, int64_t* reads_finished, double* kernel_ms, int64_t* launches) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  drain_events(ctx);
  if (reads_seen) *reads_seen = ctx->filter_seen;
  if (reads_finished) *reads_finished = ctx->filter_proven;
  if (kernel_ms) *kernel_ms = ctx->stg[STG_FILTER].ms;
  if (launches) *launches = ctx->stg[STG_FILTER].launches;
  if (reset) { ctx->filter_seen = 0; ctx->filter_proven = 0; ctx->stg[STG_FILTER].ms = 0; ctx->stg[STG_FILTER].launches = 0; }
  return MIA_HIP_OK;
}

extern "C" int mia_hip_band_stats(mia_hip_ctx* ctx, int reset, int64_t* reads_finished, double* kernel_ms, int64_t* launches) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  drain_events(ctx);
  if (reads_finished) *reads_finished = ctx->band_done;
  if (kernel_ms) *kernel_ms = ctx->stg[STG_BAND].ms;
  if (launches) *launches = ctx->stg[STG_BAND].launches;
  if (reset) { ctx->band_done = 0; ctx->stg[STG_BAND].ms = 0; ctx->stg[STG_BAND].launches = 0; }
  return MIA_HIP_OK;
}

extern "C" int mia_hip_bx_stats(mia_hip_ctx* ctx, int reset, int64_t* reads4, double* kernel_ms3, int64_t* launches) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  drain_events(ctx);
  if (reads4) { reads4[0] = ctx->bx_seen; reads4[1] = ctx->bx_done[0]; reads4[2] = ctx->bx_done[1]; reads4[3] = ctx->bx_done[2]; }
  if (kernel_ms3) for (int k = 0; k < 3; k++) kernel_ms3[k] = ctx->stg[STG_BX_PLAN + k].ms;
  if (launches) *launches = ctx->bx_launches;
  if (reset) { ctx->bx_seen = 0; for (int k = 0; k < 3; k++) { ctx->bx_done[k] = 0; ctx->stg[STG_BX_PLAN + k].ms = 0; ctx->stg[STG_BX_PLAN + k].launches = 0; } ctx->bx_launches = 0; }
  return MIA_HIP_OK;
}

#ifdef MIA_HIP_ALT_PATHS
// (alt build only, not in include/mia_hip.h: the counts MIA_HIP_DEBUG_SKIP & 65536 collects in k_tally_binned, and their reset)
extern "C" int mia_hip_debug_tally_kinds(mia_hip_ctx* ctx, uint64_t* out8) {
  if (!ctx || !out8) return MIA_HIP_ERR_ARG;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_tally_kinds), 8 * sizeof(uint64_t)));
  uint64_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_tally_kinds), z, sizeof z));
  HIPCHK(hipMemcpyFromSymbol(out8 + 8, HIP_SYMBOL(g_tally_clk), 8 * sizeof(uint64_t)));      // (out8: 16 words)
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_tally_clk), z, sizeof z));
  return MIA_HIP_OK;
}
// (alt build only: the clocks MIA_HIP_BX_DEBUG & 512 collects in k_bx_plan's first launch, and their reset)
extern "C" int mia_hip_debug_plan_clk(mia_hip_ctx* ctx, uint64_t* out12) {
  if (!ctx || !out12) return MIA_HIP_ERR_ARG;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  static uint64_t all[64 * 16], z[64 * 16];
  HIPCHK(hipMemcpyFromSymbol(all, HIP_SYMBOL(g_plan_clk), sizeof all));
  for (int k = 0; k < 12; k++) { out12[k] = 0; for (int st = 0; st < 64; st++) out12[k] += all[st * 16 + k]; }
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_plan_clk), z, sizeof z));
  return MIA_HIP_OK;
}
#endif
extern "C" int mia_hip_bx_counters(mia_hip_ctx* ctx, uint32_t* out32) {
  if (!ctx || !out32) return MIA_HIP_ERR_ARG;
  for (int k = 0; k < 32; k++) out32[k] = ctx->bx_last[k];
  return MIA_HIP_OK;
}

extern "C" int mia_hip_plain_stats(mia_hip_ctx* ctx, int reset, double* plain_ms, int64_t* plain_launches, int64_t* reads_in, int64_t* reads_retried) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  drain_events(ctx);
  if (plain_ms) *plain_ms = ctx->stg[STG_PLAIN].ms;
  if (plain_launches) *plain_launches = ctx->stg[STG_PLAIN].launches;
  if (reads_in) *reads_in = ctx->plain_total;
  if (reads_retried) *reads_retried = ctx->plain_retried;
  if (reset) { ctx->stg[STG_PLAIN].ms = 0; ctx->stg[STG_PLAIN].launches = 0; ctx->plain_total = 0; ctx->plain_retried = 0; }
  return MIA_HIP_OK;
}

template <int CPL>
// own_slabs: the launch gets trace slabs of its own (ctx->d_slabs_retry) and a grid of at most 1 024 workgroups -- it may run
// beside another launch of the same class on another stream (the band kernels' retry list beside the planner's kernels)
static hipError_t launch_window(mia_hip_ctx* ctx, int ci, const int32_t* list, int count, const int32_t* dev_range = nullptr, hipStream_t on = nullptr,
                                bool own_slabs = false, hipEvent_t stop = nullptr) {
  // slab = the largest trace of this class: 256 rows x 64*CPL columns, one byte per cell
  const int64_t slab = (int64_t)MAX_READ * 64 * CPL;
  // persistent grid: never more workgroups than are resident at once (a late starter would work through its whole
  // share of the list on a drained GPU)
  if (!ctx->window_wgs[ci]) {
    int occ = 0;
    const int cus = ctx->cus;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)k_align_window<CPL>, 64, 0) != hipSuccess || occ < 1) occ = 1;
    const int per_cu = ctx->grid_wgs / cus;      // the persistent grid's ceiling
    ctx->window_wgs[ci] = cus * (occ < per_cu ? occ : per_cu);
  }
  int grid = (dev_range || count >= ctx->window_wgs[ci]) ? ctx->window_wgs[ci] : count;   // (a count on the device: the whole persistent grid)
  unsigned char* slabs = nullptr;
  if (own_slabs) {
    grid = std::min(grid, 1024);
    if (!ctx->d_slabs_retry[ci] && dev_alloc(ctx, ctx->d_slabs_retry[ci], slab * 1024)) return hipErrorOutOfMemory;
    slabs = ctx->d_slabs_retry[ci];
  } else {
    if (!ctx->d_slabs[ci] && dev_alloc(ctx, ctx->d_slabs[ci], slab * ctx->grid_wgs)) return hipErrorOutOfMemory;
    slabs = ctx->d_slabs[ci];
  }
  RefInfo ref{ctx->d_ref, ctx->L, ctx->wrap, ctx->explicit_win};
  if (stage_begin(ctx, STG_TRACE, on)) return hipErrorOutOfMemory;
  launch_k(k_align_window<CPL>, dim3(grid), dim3(64), 0, on ? on : ctx->stream, stop, ctx->rs, ref, ctx->d_pssm, ctx->packs.p[ci], list,
           count, slabs, slab, ctx->d_wide_list, ctx->d_bins + 3 * N_BINS, ctx->dbg, dev_range);
  stage_end(ctx, STG_TRACE, on);
  return hipGetLastError();
}

// the window kernel of class ci: 64 * {4, 8, 12} columns
static hipError_t launch_window_class(mia_hip_ctx* ctx, int ci, const int32_t* list, int count, const int32_t* dev_range = nullptr, hipStream_t on = nullptr,
                                      bool own_slabs = false, hipEvent_t stop = nullptr) {
  return ci == 0 ? launch_window<4>(ctx, ci, list, count, dev_range, on, own_slabs, stop)
       : ci == 1 ? launch_window<8>(ctx, ci, list, count, dev_range, on, own_slabs, stop)
                 : launch_window<12>(ctx, ci, list, count, dev_range, on, own_slabs, stop);
}

static int align_all(mia_hip_ctx* ctx);
static bool tally_is_binned(const mia_hip_ctx* ctx);
static int comm_pre_cull_enqueue(mia_hip_ctx* ctx, const int32_t* d_wide_count);
static bool comm_pre_cull_collect(mia_hip_ctx* ctx);

extern "C" int mia_hip_realign(mia_hip_ctx* ctx, const char* new_ref, int32_t ref_len, int circular) {
  if (!ctx || !new_ref || ref_len <= 0) return MIA_HIP_ERR_ARG;
  if (!ctx->have_pssm || !ctx->d_packed) { ctx->err = "set_pssm and upload_reads must precede realign"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  // add_ref_wrap (src/mia.c:657-689): first min(L,256) bases appended when circular
  const int L = ref_len, wl = circular ? (L < MAX_READ ? L : MAX_READ) : 0, wrap = L + wl;
  std::vector<uint8_t> codes((size_t)wrap + 64, 4);
  int64_t n_other = 0;
  for (int i = 0; i < L; i++) { codes[i] = base_code(new_ref[i]); n_other += codes[i] > 3; }
  for (int i = 0; i < wl; i++) codes[L + i] = codes[i];
  // a reference full of ambiguity codes (mt311 itself: every other column) leaves the diagonal filter nothing to decide
  ctx->ref_mostly_bases = n_other * 50 <= L;
  ctx->ref_few_n = n_other * 500 <= L;
  ctx->kh_entries = 0;
  if (n_other) {
    ctx->kh_entries = kh_wild_entries(codes.data(), wrap, BX_WILD);
    if (ctx->kh_entries > ((int64_t)1 << 24)) ctx->kh_entries = 0;
  }
  if (dev_ensure(ctx, ctx->d_ref, (int64_t)codes.size(), (int64_t)codes.size() * 2)) return MIA_HIP_ERR_NOMEM;
  if (ctx->h_pin && codes.size() <= mia_hip_ctx::PIN_BYTES - mia_hip_ctx::PIN_MISC) {
    HIPCHK(hipStreamSynchronize(ctx->stream));             // the staging area may still feed an earlier copy
    memcpy(ctx->h_pin + mia_hip_ctx::PIN_MISC, codes.data(), codes.size());
    HIPCHK(hipMemcpyAsync(ctx->d_ref, ctx->h_pin + mia_hip_ctx::PIN_MISC, codes.size(), hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIPCHK(hipMemcpyAsync(ctx->d_ref, codes.data(), codes.size(), hipMemcpyHostToDevice, ctx->stream));
  }
  ctx->L = L; ctx->wrap = wrap; ctx->have_ref = true; ctx->explicit_win = 0;
  return align_all(ctx);
}

// exact kernel for whole-reference windows and escaped reads (rare): one read per thread, int32 scores and trace in scratch
static int run_wide(mia_hip_ctx* ctx, const RefInfo& ref, int32_t n_wide) {
    if (ctx->wide_to_caller) {
      // pass 1's windows: a read the trace kernels could not finish (a gap of 63 or more on the path -- a window around a
      // stray cluster, where the read does not belong) goes to the whole-strand DP with everything else that is left over;
      // one read per thread here would take longer than that whole kernel
      hipLaunchKernelGGL(k_mark_status, dim3((n_wide + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_wide_list, n_wide, ctx->rs.status, ST_ESCAPE);
      HIPCHK(hipGetLastError());
      return MIA_HIP_OK;
    }
    std::vector<int32_t> wl((size_t)n_wide), as((size_t)n_wide), ae((size_t)n_wide);
    std::vector<uint16_t> ln((size_t)n_wide);
    HIPCHK(hipMemcpy(wl.data(), ctx->d_wide_list, (size_t)n_wide * 4, hipMemcpyDeviceToHost));
    std::vector<int64_t> soff((size_t)n_wide);
    int64_t total = 0;
    for (int t = 0; t < n_wide; t++) {
      HIPCHK(hipMemcpy(&as[t], ctx->rs.as + wl[t], 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(&ae[t], ctx->rs.ae + wl[t], 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(&ln[t], ctx->rs.len + wl[t], 2, hipMemcpyDeviceToHost));
      int s, n1;
      read_window(ref, as[t], ae[t], ln[t], &s, &n1);
      soff[t] = total;
      total += (int64_t)ln[t] * n1 + 5 * (int64_t)n1 + 16;
    }
    if (dev_ensure(ctx, ctx->d_scratch, total) || dev_ensure(ctx, ctx->d_scratch_off, n_wide)) return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemcpyAsync(ctx->d_scratch_off, soff.data(), (size_t)n_wide * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_align_wide, dim3((n_wide + 63) / 64), dim3(64), 0, ctx->stream, ctx->rs, ref, ctx->d_pssm, ctx->d_wide_list,
                       n_wide, ctx->d_scratch_off, ctx->d_scratch);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

// mia_hip_iterate left the new reference as ASCII in d_ascii: its codes, if no k_ref_prep makes them
static void encode_now(mia_hip_ctx* ctx) {
  if (!ctx->pend_encode) return;
  ctx->pend_encode = false;
  hipLaunchKernelGGL(k_ref_encode, dim3((unsigned)((ctx->pend_total + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ascii_src, ctx->pend_L, ctx->pend_wl,
                     ctx->d_ref, ctx->pend_total);
}

// the counters of a deferred alignment, once its control block has reached the host (hb: the words from CTRL_BINS + 3 N_BINS on)
static void align_counters_collect(mia_hip_ctx* ctx, const int32_t* hb, bool filtered, bool bx, bool plain) {
  constexpr int C0 = CTRL_C0;
  const int32_t* h_hdr = hb + (CTRL_HDR - C0);
  const uint32_t* h_filter = reinterpret_cast<const uint32_t*>(hb + (CTRL_FILTER - C0));
  const uint32_t* h_bxc = reinterpret_cast<const uint32_t*>(hb + (CTRL_BXC - C0));
  ctx->filter_seen += ctx->rs.n;
  if (filtered) {
    ctx->filter_proven += h_filter[0];
    ctx->band_done += h_filter[2];
    if (bx) {
      ctx->filter_proven += h_bxc[BXC_DONE_PLAN * BXC_STRIDE];
      for (int k = 0; k < 3; k++) ctx->bx_done[k] += h_bxc[(BXC_DONE_PLAN + k) * BXC_STRIDE];
      ctx->bx_seen += h_bxc[BXC_SEEN * BXC_STRIDE];
    }
  }
  for (int k = 0; k < BXC_COUNTERS; k++) ctx->bx_last[k] = bx ? h_bxc[k * BXC_STRIDE] : 0;
  if (bx) ctx->bx_last[BXC_CUR_VALUES] = h_filter[1];      // (statistics: reads the quick plan left to the full plan -- the lanes kernels have no use for this slot)
  if (plain) ctx->plain_retried += h_hdr[PH_RETRIED_PLAIN];
}

// ---- align_all: the route is decided in ONE place (align_route.h: align_route), the stages below follow it --------------------------
static_assert(ROUTE_QCH == BX_QCH && ROUTE_MAXW == BX_MAXW, "align_route.h carries copies of the two");
static_assert(P1_ROUTE_WILD == BX_WILD, "pass1_route.h carries a copy");

// What the stages of one alignment hand each other.  Nothing of it outlives the call: the context keeps align_end_signalled and spec_*.
struct AlignCall {
  AlignRoute r;
  RefInfo ref; RefPlanes rp{nullptr, nullptr, nullptr}; KmerOcc ko{nullptr, nullptr}; KmerHash kh{};
  uint32_t kslots = 0; int64_t nib_words = 0;
  BxDev bd; int64_t slab_words = 0;        // the band DPs' tables and lists; words of one trace slab (band pipeline, or round 1's k_band_align)
  int gb = 0;                              // the planner's grid: 256 threads, PLAN_PER reads each
  int32_t *d_count, *d_off, *d_cursor, *d_wide_count;
  hipStream_t ps = nullptr;                // the planner's stream: stream2 beside the band DPs of a deferred call, else the context's
  bool pending_join = false;               // band kernels are still running on stream2 / stream3
  bool planner_end_signalled = false;      // the planner chain's last launch has signalled ev_join itself
  bool dbg_steps = false;                  // MIA_HIP_ITER_DEBUG: wait and report after every stage of the deferred chain
};

static AlignRouteIn align_route_in(const mia_hip_ctx* ctx) {
  AlignRouteIn in;
  in.n = ctx->rs.n; in.max_len = ctx->max_len; in.wrap = ctx->wrap; in.L = ctx->L; in.kh_entries = ctx->kh_entries;
  in.plane_words = plane_words((int64_t)ctx->wrap + 64);
  in.flat = ctx->flat; in.ref_mostly_bases = ctx->ref_mostly_bases; in.ref_few_n = ctx->ref_few_n; in.bx_ok = ctx->bx_ok;
  in.explicit_win = ctx->explicit_win != 0; in.deferred = ctx->deferred; in.pend_encode = ctx->pend_encode; in.ref_ready = ctx->ref_ready;
  in.own_umax = ctx->umax_valid && ctx->rs.roff == ctx->d_roff;
  for (int k = 1; k < BXF_KINDS; k++) in.rejects += ctx->bx_last[BXC_FAIL0 + k];
  in.use_filter = ctx->use_filter; in.use_banddp = ctx->use_banddp; in.use_bx = ctx->use_bx; in.use_lanes = ctx->use_lanes;
  in.use_fine = ctx->use_fine; in.use_quick = ctx->use_quick; in.bx_serial = ctx->bx_serial; in.plan_split = ctx->plan_split;
  in.use_direct_open = ctx->use_direct_open; in.no_prep_fuse = ctx->no_prep_fuse;
  in.ext_events = ctx->ext_events; in.dbg = ctx->dbg; in.bx_dbg = ctx->bx_dbg;
  return in;
}

static void align_ck(mia_hip_ctx* ctx, const AlignCall& c, const char* what) {
  if (!c.dbg_steps) return;
  hipError_t e = hipStreamSynchronize(c.ps);
  fprintf(stderr, "[align_all deferred] %s: %s\n", what, hipGetErrorString(e)); fflush(stderr);
}

// BUFFERS: everything the route's kernels write to, grown to this alignment's sizes (the full-window kernels' trace slabs are made
// where those are launched: launch_window)
static int align_ensure_buffers(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  const int64_t n = ctx->rs.n;
  const int wrap = ctx->wrap;
  if (!r.filtered) return MIA_HIP_OK;
  if (dev_ensure(ctx, ctx->d_planes, r.plane_words * 3)) return MIA_HIP_ERR_NOMEM;
  if (r.kocc && !ctx->d_kocc_cnt && (dev_alloc(ctx, ctx->d_kocc_cnt, DF_KTAB) || dev_alloc(ctx, ctx->d_kocc_pos, (int64_t)DF_KTAB * DF_KCAP)))
    return MIA_HIP_ERR_NOMEM;
  if (((r.run_filter && r.banded) || r.quick) && dev_ensure(ctx, ctx->d_left_list, n)) return MIA_HIP_ERR_NOMEM;
  if (!r.bx) {
    // round 1's banded DP: a persistent grid of wavefronts (three per SIMD), each with its own trace slab
    c.slab_words = (int64_t)ctx->max_len * BAND_ROW_WORDS;
    const int64_t words = c.slab_words * std::min<int64_t>((n + 63) / 64, 3072);
    return r.banded ? dev_ensure(ctx, ctx->d_band_slabs, words) : MIA_HIP_OK;
  }
  // the reference as 4-bit codes, the lists, one slab per wavefront of the trace kernel's persistent grid
  c.nib_words = bx_nib_words((int64_t)wrap + 64);
  if (dev_ensure(ctx, ctx->d_refnib, c.nib_words, c.nib_words * 2)) return MIA_HIP_ERR_NOMEM;
  c.kslots = kh_slots_for_entries(wrap, ctx->kh_entries);
  if (dev_ensure(ctx, ctx->d_khash, (int64_t)c.kslots * 4) || dev_ensure(ctx, ctx->d_khash_ovf, (int64_t)c.kslots * 2)) return MIA_HIP_ERR_NOMEM;
  if (r.want_bits && !ctx->d_kbits && dev_alloc(ctx, ctx->d_kbits, KB_WORDS)) return MIA_HIP_ERR_NOMEM;
  if (dev_ensure(ctx, ctx->d_bx_plan, n) || dev_ensure(ctx, ctx->d_bx_expect, n) || dev_ensure(ctx, ctx->d_bx_lists, n * 4 * BX_NCLS)) return MIA_HIP_ERR_NOMEM;
  if (!ctx->bx_values_wgs) {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ctx->use_lanes ? (const void*)k_bxl_values : ALT_KERNEL(k_bx_values), 256, 0) != hipSuccess || occ < 1) occ = 1;
    ctx->bx_values_wgs = ctx->cus * std::min(occ, 4);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ctx->use_lanes ? (const void*)k_bxl_trace : ALT_KERNEL(k_bx_trace), 256, 0) != hipSuccess || occ < 1) occ = 1;
    ctx->bx_trace_wgs = ctx->cus * std::min(occ, 4);      // (every wavefront of the trace grid owns a slab)
  }
  // (the lanes kernels store four rows per word: whole blocks of four rows)
  c.slab_words = ctx->use_lanes ? (int64_t)((ctx->max_len + 3) & ~3) * BXL_SLAB_ROW_WORDS : (int64_t)ctx->max_len * BX_SLAB_ROW_WORDS;
  const int64_t trace_words = c.slab_words * ctx->bx_trace_wgs * 4;
  if (dev_ensure(ctx, ctx->d_bx_slabs, trace_words)) return MIA_HIP_ERR_NOMEM;
  if (r.new_flow) {
    if (dev_ensure(ctx, ctx->d_retry2, n)) return MIA_HIP_ERR_NOMEM;
    if (!ctx->bx_late_wgs) ctx->bx_late_wgs = ctx->cus;        // the values DP's left-overs are few: one workgroup per CU
    const int64_t late_words = (int64_t)((ctx->max_len + 3) & ~3) * BXL_SLAB_ROW_WORDS * ctx->bx_late_wgs * 4;
    if (dev_ensure(ctx, ctx->d_bx_slabs_late, late_words) || dev_ensure(ctx, ctx->d_bx_slabs_late2, late_words)) return MIA_HIP_ERR_NOMEM;
  }
  if (r.split && dev_ensure(ctx, ctx->d_bx_cand, n)) return MIA_HIP_ERR_NOMEM;
  // (the third launch's list only where that launch runs: a record is 72 bytes -- 0.7 GB at 10 M reads)
  if (r.fine && dev_ensure(ctx, ctx->d_bx_cand2, n)) return MIA_HIP_ERR_NOMEM;
  if (r.direct_open) {
    if (dev_ensure(ctx, ctx->d_open_list, n)) return MIA_HIP_ERR_NOMEM;
    if (!ctx->d_slabs_open && dev_alloc(ctx, ctx->d_slabs_open, OPEN_SLAB_BYTES * OPEN_WGS)) return MIA_HIP_ERR_NOMEM;
  }
  return MIA_HIP_OK;
}

// k_ref_prep over one set of buffers: the call's own (align_ref_prep), or the set prepared ahead with the idle half of the control
// block (ref_ahead_queue).  Both go to the context's stream and share the barrier's counter and the `stuck` word.
struct RefPrepSet { uint8_t* codes; int32_t* ctrl; uint32_t* khash; int32_t* kovf; uint64_t* planes; int64_t pstride; uint32_t* nib; KbPair* kbits; };
static int launch_ref_prep(mia_hip_ctx* ctx, const RefPrepSet& s, const char* ascii, int32_t L, int32_t wl, int32_t total, uint32_t kslots, int kwild,
                           int64_t words, int64_t nw) {
  const int wrap = total - 64;
  RefPrep rp2;
  rp2.ascii = ascii; rp2.L = L; rp2.wl = wl; rp2.total = total; rp2.codes = s.codes;
  rp2.ctrl = s.ctrl; rp2.ctrl_words = CTRL_WORDS;
  rp2.kslot = s.khash; rp2.kovf = s.kovf; rp2.kslots = kslots; rp2.kmask = kslots - 1; rp2.kshift = kh_shift_for(kslots); rp2.kwild = kwild;
  rp2.plane_words = words; rp2.plo = s.planes; rp2.phi = s.planes + s.pstride; rp2.pok = s.planes + 2 * s.pstride;
  rp2.nib_words = nw; rp2.nib = s.nib;
  const int64_t want = ((int64_t)wrap + (kwild > 0 ? 63 : 255)) / (kwild > 0 ? 64 : 256);       // (N columns spelled out: 64 positions per workgroup, see kmer_hash_insert_block)
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, ctx->cus));      // one workgroup per compute unit at most: all resident
  // the grid barrier's target: what the counter reaches when this launch's workgroups have all arrived.  The host's count only
  // moves once the launch is known to be queued (a refused launch adds nothing on the device either), the wait inside the
  // kernel is bounded, and a barrier given up on is reported through a pinned word the step's one wait looks at.
  rp2.bar = ctx->d_prep_bar; rp2.bar_target = ctx->prep_bar_count + grid;
  rp2.stuck = ctx->h_pin ? reinterpret_cast<uint32_t*>(ctx->h_pin + (62 << 10)) : nullptr;
  rp2.kbits = s.kbits;
  hipLaunchKernelGGL(k_ref_prep, dim3(grid), dim3(256), 0, ctx->stream, rp2);
  HIPCHK(hipGetLastError());
  ctx->prep_bar_count += grid;
  return MIA_HIP_OK;
}

// REFERENCE PREPARATION: codes, control block, bit planes, and the table of the route -- round 1's 10-mer occurrences, or nibbles, hash
// table and bitmaps of the band pipeline; mia_hip_iterate with the band pipeline: all of it in ONE launch (k_ref_prep)
static int align_ref_prep(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  const int wrap = ctx->wrap;
  const int64_t words = r.plane_words, pstride = ctx->d_planes.cap / 3;      // the block holds three planes
  if (r.prep_none) {
    // everything below was made behind the last consensus, and the control block's current half was cleared with it (ref_ahead_adopt)
    c.rp = RefPlanes{ctx->d_planes, ctx->d_planes + pstride, ctx->d_planes + 2 * pstride};
    c.kh = KmerHash{ctx->d_khash, ctx->d_khash_ovf, c.kslots - 1, kh_shift_for(c.kslots), ctx->kh_entries > 0 ? BX_WILD : 0};
    return MIA_HIP_OK;
  }
  if (!r.fused_prep) {
    encode_now(ctx);
    HIPCHK(hipMemsetAsync(ctx->ctrl, 0, (size_t)CTRL_WORDS * 4, ctx->stream));     // every counter of the iteration at once
  }
  if (!r.filtered) return MIA_HIP_OK;
  c.rp = RefPlanes{ctx->d_planes, ctx->d_planes + pstride, ctx->d_planes + 2 * pstride};
  if (!r.fused_prep)
    hipLaunchKernelGGL(k_ref_planes, dim3((unsigned)((words + 3) / 4 < 4096 ? (words + 3) / 4 : 4096)), dim3(256), 0, ctx->stream, ctx->d_ref, (int64_t)wrap + 64, words,
                       ctx->d_planes, ctx->d_planes + pstride, ctx->d_planes + 2 * pstride);
  if (r.kocc) {
    HIPCHK(hipMemsetAsync(ctx->d_kocc_cnt, 0, (size_t)DF_KTAB * 4, ctx->stream));
    hipLaunchKernelGGL(k_kmer_occ, dim3((unsigned)((wrap + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_ref, (int64_t)wrap, ctx->d_kocc_cnt, ctx->d_kocc_pos, 0);
    c.ko.cnt = ctx->d_kocc_cnt; c.ko.pos = ctx->d_kocc_pos;
  }
  if (!r.bx) return MIA_HIP_OK;
  const int64_t nw = c.nib_words;
  const uint32_t kslots = c.kslots;
  if (!r.fused_prep)
    hipLaunchKernelGGL(k_ref_nibbles, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_ref, (int64_t)wrap, nw, ctx->d_refnib);
  c.kh = KmerHash{ctx->d_khash, ctx->d_khash_ovf, kslots - 1, kh_shift_for(kslots), ctx->kh_entries > 0 ? BX_WILD : 0};
  const KmerHash& kh = c.kh;
  if (!r.fused_prep) {
    HIPCHK(hipMemsetAsync(ctx->d_khash, 0xFF, (size_t)kslots * 16, ctx->stream));
    hipLaunchKernelGGL(k_kmer_hash, dim3((unsigned)((wrap + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_ref, (int64_t)wrap, ctx->d_khash, ctx->d_khash_ovf,
                       kh.mask, kh.shift, kh.wild);
    if (r.want_bits) {
      HIPCHK(hipMemsetAsync(ctx->d_kbits, 0, (size_t)KB_WORDS * sizeof(KbPair), ctx->stream));
      hipLaunchKernelGGL(k_kmer_bits, dim3((unsigned)((ctx->L + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_ref, (int64_t)wrap, (int64_t)ctx->L, ctx->d_kbits);
    }
    return MIA_HIP_OK;
  }
  const RefPrepSet own{ctx->d_ref, ctx->ctrl, ctx->d_khash, ctx->d_khash_ovf, ctx->d_planes, pstride, ctx->d_refnib, r.want_bits ? ctx->d_kbits.p : nullptr};
  if (int rc = launch_ref_prep(ctx, own, ctx->ascii_src, ctx->pend_L, ctx->pend_wl, ctx->pend_total, kslots, kh.wild, words, nw)) return rc;
  ctx->pend_encode = false;
  return MIA_HIP_OK;
}

// what the band pipeline's kernels are handed: tables, lists and counters as the route wants them
static void align_bx_dev(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  BxDev& bd = c.bd;
  bd.tab.sub = ctx->d_bx_sub; bd.tab.mrow = ctx->d_bx_mrow; bd.tab.loss = ctx->d_bx_loss; bd.tab.dl = ctx->d_bx_dl;
  bd.dbg = ctx->bx_dbg & (3u | 32u | 64u | 128u | 512u);
  bd.retry = ctx->d_retry2; bd.retry_n = ctx->d_plan_hdr + PH_RETRY2 + 1;
  bd.listed_mark = r.new_flow ? -5 : 0;
  bd.tab.min_m = ctx->bx_min_m; bd.tab.max_m = ctx->bx_max_m;
  bd.tab.maxw = r.maxw;
  bd.sub256 = ctx->d_bx_sub + BX_SUB_WORDS;
  bd.refnib = ctx->d_refnib;
  bd.umax = (ctx->umax_valid && ctx->rs.roff == ctx->d_roff) ? ctx->d_umax : nullptr;    // (a borrowed read set has none)
  bd.rplanes = bd.umax ? ctx->d_rplanes : nullptr;
  bd.rplane_words = ctx->rplane_words;
  bd.plan = ctx->d_bx_plan; bd.expect = ctx->d_bx_expect; bd.lists = ctx->d_bx_lists; bd.list_stride = ctx->d_bx_lists.cap / (4 * BX_NCLS); bd.ctr = ctx->d_bx_ctr;
  bd.cand = r.split ? ctx->d_bx_cand : nullptr; bd.cand_n = ctx->d_bx_ctr + (size_t)BXC_CAND * BXC_STRIDE;
  bd.cand2 = r.fine ? ctx->d_bx_cand2 : nullptr; bd.cand2_n = ctx->d_bx_ctr + (size_t)BXC_CAND2 * BXC_STRIDE;
  bd.open = r.direct_open ? ctx->d_open_list : nullptr; bd.open_n = ctx->d_bx_ctr + (size_t)BXC_OPEN * BXC_STRIDE;
  bd.qlist = r.quick ? ctx->d_left_list : nullptr; bd.qlist_n = ctx->d_filter_n + 1; bd.mark_all = 0; bd.to_late = 0; bd.qch = r.qch;
  bd.kb = KmerBits{r.quick ? ctx->d_kbits : nullptr, ctx->L};
  bd.plane_words = (int32_t)(r.quick_lds ? r.plane_words : 0);
}

// k_bx_plan<NW, PH> for the 64-row words of the longest read and a phase of the route
using PlanKernel = decltype(&k_bx_plan<1, 0>);
template <int PH>
static PlanKernel plan_kernel_nw(int nwords) {
  switch (nwords) { case 1: return k_bx_plan<1, PH>; case 2: return k_bx_plan<2, PH>; case 3: return k_bx_plan<3, PH>; default: return k_bx_plan<4, PH>; }
}
static PlanKernel plan_kernel(int nwords, int phase) {
  switch (phase) {
    case 0: return plan_kernel_nw<0>(nwords); case 1: return plan_kernel_nw<1>(nwords); case 2: return plan_kernel_nw<2>(nwords); case 3: return plan_kernel_nw<3>(nwords);
    case 4: return plan_kernel_nw<4>(nwords); case 5: return plan_kernel_nw<5>(nwords); default: return plan_kernel_nw<6>(nwords);
  }
}

// PLAN LAUNCHES: the quick plan over all reads, the full plan over what it left (or over all reads), and -- where the plan gives up on
// many reads -- the planner's three head kernels in front of the fork (align_route.h: planner_head_first)
static int align_plan_launches(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  const int64_t n = ctx->rs.n, wrap = ctx->wrap;
  BxDev& bd = c.bd;
  const dim3 pb(256);
  const uint32_t* in_n = (const uint32_t*)(ctx->d_filter_n + 1);
  ctx->diag_scripts_missing = true;         // (the scripts of reads finished as pure diagonals: k_diag_scripts makes them when asked for)
  if (r.direct_open) ctx->direct_open_steps++;
  if (r.quick) ctx->quick_steps++;
  if (stage_begin(ctx, STG_BX_PLAN)) return MIA_HIP_ERR_NOMEM;
  if (r.quick) {
    const dim3 pg((unsigned)((n + 256 * bd.qch - 1) / (256 * bd.qch)));
    const size_t lds = (size_t)(bx_quick_lds_words(bd.qch) * 8 + (r.quick_phase == 5 ? r.plane_words * 24 : 0));
    // (this launch walks all n reads: no in_list)
    launch_k(plan_kernel(r.nwords, r.quick_phase), pg, pb, lds, ctx->stream, (r.fork_at_quick && r.fork_by_launch) ? ctx->ev_fork : nullptr, ctx->rs, c.ref, c.rp, c.kh, wrap, bd,
             (const int32_t*)nullptr, in_n, n, ctx->d_bin_of);
    bd.mark_all = 1;
    if (r.fork_at_quick) {
      if (!r.fork_by_launch) HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
      bd.to_late = 1;
    }
  }
  const int32_t* in_list = r.quick ? ctx->d_left_list : nullptr;
  for (int phase = r.full_first; phase <= r.full_last; phase++) {
    // (the fork event rides on the last launch's own completion signal: no marker between the plan and the values DP)
    hipEvent_t done = (r.fork_by_launch && phase == r.full_last && !r.planner_head_first && !r.fork_at_quick) ? ctx->ev_fork : nullptr;
    launch_k(plan_kernel(r.nwords, phase), dim3(align_route_plan_grid(r, phase, n)), pb, 0, ctx->stream, done, ctx->rs, c.ref, c.rp, c.kh, wrap, bd, in_list, in_n, n, ctx->d_bin_of);
  }
  bd.to_late = 0;
  stage_end(ctx, STG_BX_PLAN);
  HIPCHK(hipGetLastError());
  if (r.planner_head_first) {
    // (banded, many rejects: the values-only quad pass is on)
    hipLaunchKernelGGL(k_plan_count, dim3(c.gb), dim3(256), 0, ctx->stream, ctx->rs, c.ref, ctx->packs, /*use_quad=*/1, 1, 1, ctx->d_bin_of, c.d_count, ctx->d_filter_n);
    hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(512), 0, ctx->stream, c.d_count, c.d_off, ctx->d_plan_hdr, 0, ctx->d_list);
    launch_k(k_plan_fill, dim3(c.gb), dim3(256), 0, ctx->stream, r.fork_by_launch ? ctx->ev_fork : nullptr, n, (const int32_t*)ctx->d_bin_of, (const int32_t*)c.d_off, c.d_cursor, ctx->d_list);
    HIPCHK(hipGetLastError());
  }
  return MIA_HIP_OK;
}

// BAND DPs, THREE STREAMS (align_route.h: BAND DPs): trace DP on stream3, values DP and late trace on stream2 or on the context's
static int align_band_dps(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  const BxDev& bd = c.bd;
  hipStream_t vs = r.values_aside ? ctx->stream2 : ctx->stream;
  if (r.fork_at_quick) {
    if (stage_launch(ctx, STG_BX_VALUES, k_bxl_trace_late2, dim3((unsigned)ctx->bx_late_wgs), dim3(256), 0, ctx->stream, ctx->rs, c.ref, bd, ctx->d_bx_slabs_late2, c.slab_words, ctx->d_bin_of))
      return MIA_HIP_ERR_NOMEM;
  }
  if (!r.fork_by_launch && !r.fork_at_quick) HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
  HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
  HIPCHK(hipStreamWaitEvent(ctx->stream3, ctx->ev_fork, 0));
  if (stage_begin(ctx, STG_BX_TRACE, ctx->stream3)) return MIA_HIP_ERR_NOMEM;
  if (!(ctx->bx_dbg & 8u))
    launch_k(k_bxl_trace, dim3((unsigned)ctx->bx_trace_wgs), dim3(256), 0, ctx->stream3, r.trace_signals ? ctx->ev_join3 : nullptr, ctx->rs, c.ref, bd, ctx->d_bx_slabs, c.slab_words, ctx->d_bin_of);
  stage_end(ctx, STG_BX_TRACE, ctx->stream3);
  if (!r.trace_signals) HIPCHK(hipEventRecord(ctx->ev_join3, ctx->stream3));
  if (!(ctx->bx_dbg & 4u)) {
    if (stage_launch(ctx, STG_BX_VALUES, k_bxl_values, dim3((unsigned)ctx->bx_values_wgs), dim3(256), 0, vs, ctx->rs, c.ref, bd, ctx->d_bin_of)) return MIA_HIP_ERR_NOMEM;
    if (stage_launch(ctx, STG_BX_VALUES, k_bxl_trace_late, dim3((unsigned)ctx->bx_late_wgs), dim3(256), 0, vs, ctx->rs, c.ref, bd, ctx->d_bx_slabs_late, c.slab_words, ctx->d_bin_of))
      return MIA_HIP_ERR_NOMEM;
  }
  if (r.values_aside) HIPCHK(hipEventRecord(ctx->ev_join, ctx->stream2));
  HIPCHK(hipGetLastError());
  c.pending_join = true;
  return MIA_HIP_OK;
}

// BAND DPs, TWO STREAMS (MIA_HIP_BX_SERIAL, MIA_HIP_NO_LANES, caller-supplied windows): round 2's order, the planner behind them.
// The two band DPs do not depend on each other (a read the values DP cannot finish stays open for the full-window
// kernels): they run side by side on two streams -- both are persistent grids whose wavefronts leave as soon as the
// chunks run out, so each fills what the other leaves idle, and the step pays the longer of the two tails, not both.
static int align_band_dps_serial(mia_hip_ctx* ctx, AlignCall& c) {
  const BxDev& bd = c.bd;
  HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
  HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
  if (stage_begin(ctx, STG_BX_TRACE, ctx->stream2)) return MIA_HIP_ERR_NOMEM;
  if (ctx->bx_dbg & 8u) {}
  else if (ctx->use_lanes) hipLaunchKernelGGL(k_bxl_trace, dim3((unsigned)ctx->bx_trace_wgs), dim3(256), 0, ctx->stream2, ctx->rs, c.ref, bd, ctx->d_bx_slabs, c.slab_words, ctx->d_bin_of);
#ifdef MIA_HIP_ALT_PATHS
  else hipLaunchKernelGGL(k_bx_trace, dim3((unsigned)ctx->bx_trace_wgs), dim3(256), 0, ctx->stream2, ctx->rs, c.ref, bd, ctx->d_bx_slabs, c.slab_words, ctx->d_bin_of);
#endif
  stage_end(ctx, STG_BX_TRACE, ctx->stream2);
  HIPCHK(hipEventRecord(ctx->ev_join, ctx->stream2));
  if (stage_begin(ctx, STG_BX_VALUES)) return MIA_HIP_ERR_NOMEM;
  if (ctx->bx_dbg & 4u) {}
  else if (ctx->use_lanes) hipLaunchKernelGGL(k_bxl_values, dim3((unsigned)ctx->bx_values_wgs), dim3(256), 0, ctx->stream, ctx->rs, c.ref, bd, ctx->d_bin_of);
#ifdef MIA_HIP_ALT_PATHS
  else hipLaunchKernelGGL(k_bx_values, dim3((unsigned)ctx->bx_values_wgs), dim3(256), 0, ctx->stream, ctx->rs, c.ref, bd, ctx->d_bin_of);
#endif
  stage_end(ctx, STG_BX_VALUES);
  HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  HIPCHK(hipGetLastError());
  return MIA_HIP_OK;
}

// ROUND 1 (flat matrix, MIA_HIP_NO_BANDX): reads whose alignment is provably one gap-free diagonal never reach the DP kernels
// (diag_filter.h); what the filter leaves over goes through k_band_align, a persistent grid of wavefronts, each with its own trace slab
// (the number of left-over reads stays on the device)
static int align_round1(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  const int64_t n = ctx->rs.n, wrap = ctx->wrap;
  if (r.run_filter) {
    if (stage_begin(ctx, STG_FILTER)) return MIA_HIP_ERR_NOMEM;
    hipLaunchKernelGGL(k_diag_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rs, c.ref, c.rp, c.ko, wrap, ctx->d_bin_of, ctx->dbg,
                       r.banded ? ctx->d_left_list : nullptr, ctx->d_filter_n + 1);
    stage_end(ctx, STG_FILTER);
    HIPCHK(hipGetLastError());
  }
  if (!r.banded) return MIA_HIP_OK;
  const int grid = (int)std::min<int64_t>((n + 63) / 64, 3072);          // three wavefronts per SIMD
  if (stage_begin(ctx, STG_BAND)) return MIA_HIP_ERR_NOMEM;
  hipLaunchKernelGGL(k_band_align, dim3(grid), dim3(64), 0, ctx->stream, ctx->rs, c.ref, c.rp, c.ko, wrap, ctx->d_left_list, ctx->d_filter_n + 1,
                     ctx->d_band_slabs, c.slab_words, ctx->d_bin_of, ctx->d_filter_n + 2, ctx->d_filter_n + 3, ctx->dbg);
  stage_end(ctx, STG_BAND);
  HIPCHK(hipGetLastError());
  return MIA_HIP_OK;
}

// The band kernels of the three-stream order are still running beside the context's stream: wait for them
// there, then let a window kernel take what they put on the retry list (its length stays on the device).
static int bx_join_and_retry(mia_hip_ctx* ctx, AlignCall& c) {
  if (!c.pending_join) return MIA_HIP_OK;
  c.pending_join = false;
  const int32_t* range = ctx->d_plan_hdr + PH_RETRY2;
  const int cols = ctx->max_len + 2 * REALIGN_BUFFER + 2;
  const bool aside = c.r.planner_aside;
  // mia_hip_iterate: the retry list is the band kernels' alone, so its window kernel only waits for THEM (the trace DP on
  // stream3; values and late trace are ahead of it on this stream) and runs beside the tail of the planner's chain on
  // stream2, with trace slabs of its own; the planner is waited for behind it
  if (c.r.values_aside) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));      // (values DP and late trace on stream2)
  HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join3, 0));
  // (this launch is the last of the alignment on the context's stream: with ext_events it signals ev_fork, which
  // mia_hip_iterate's counting sort on stream2 waits for -- see queue_cull)
  hipEvent_t stop = (aside && (ctx->ext_events & 8u)) ? ctx->ev_fork : nullptr;
  ctx->align_end_signalled = stop != nullptr;
  if (c.r.direct_open) {
    // the plan's own open list and the band DPs' retry list in ONE launch, a read of either per wavefront (k_align_open): the planner's
    // stream has had nothing to do in this alignment -- no kernel beside the DPs for the open reads, no wait for that stream here
    if (stage_begin(ctx, STG_TRACE)) return MIA_HIP_ERR_NOMEM;
    launch_k(k_align_open, dim3(OPEN_WGS), dim3(64), 0, ctx->stream, stop, ctx->rs, c.ref, (const int32_t*)ctx->d_pssm, ctx->packs, (const int32_t*)ctx->d_open_list,
             (const uint32_t*)(ctx->d_bx_ctr + (size_t)BXC_OPEN * BXC_STRIDE), ctx->d_slabs_open, (int64_t)OPEN_SLAB_BYTES, ctx->d_wide_list, c.d_wide_count, ctx->dbg,
             (const int32_t*)ctx->d_retry2, (const uint32_t*)(range + 1));
    stage_end(ctx, STG_TRACE);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ctx->err = std::string("k_align_open launch: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
    return MIA_HIP_OK;
  }
  hipError_t e = launch_window_class(ctx, cols <= 64 * 4 ? 0 : cols <= 64 * 8 ? 1 : 2, ctx->d_retry2, 0, range, nullptr, aside, stop);
  if (e != hipSuccess) { ctx->err = std::string("k_align_window (band retry list) launch: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  if (aside) {
    if (!c.planner_end_signalled) HIPCHK(hipEventRecord(ctx->ev_join, ctx->stream2));      // (the planner's chain ends here)
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  }
  return MIA_HIP_OK;
}

// every window class reads its own range from the header (the list is rewritten by the re-plan, so they all go
// before it; a class without reads costs an empty launch -- a few microseconds -- and three of them in front of the quad
// kernel delayed it by ~50 us of launch gaps on a chain that ends about when the band DPs' does: they go behind its first launch)
static int align_window_classes(mia_hip_ctx* ctx, AlignCall& c) {
  for (int ci = 0; ci < N_CPL; ci++) {
    hipError_t e = launch_window_class(ctx, ci, ctx->d_list, 0, ctx->d_plan_hdr + PH_WIN + 2 * ci, c.ps);
    if (e != hipSuccess) { ctx->err = std::string("k_align_window launch: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  }
  align_ck(ctx, c, "window classes");
  return MIA_HIP_OK;
}

// PLANNER CHAIN, DEFERRED FORM (mia_hip_iterate): the same plan, but its numbers stay on the device (k_plan_scan) and every DP kernel
// reads its own range; the host looks at the counters once, when everything has been queued (align_finish_deferred)
static int align_planner_deferred(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  const int64_t n = ctx->rs.n;
  hipStream_t ps = c.ps;
  int32_t* hdr = ctx->d_plan_hdr;
  align_ck(ctx, c, "plan_count");
  // (the plan's open list is taken by the alignment's LAST launch, together with the band DPs' retry list: bx_join_and_retry)
  if (r.direct_open) return MIA_HIP_OK;
  if (!r.planner_head_first) {
    hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(512), 0, ps, c.d_count, c.d_off, hdr, 0, ctx->d_list);      // (writes the quad bins' padding itself: -1 = empty slot)
    hipLaunchKernelGGL(k_plan_fill, dim3(c.gb), dim3(256), 0, ps, n, ctx->d_bin_of, c.d_off, c.d_cursor, ctx->d_list);
  }
  align_ck(ctx, c, "memsets");
  hipLaunchKernelGGL(k_wide_seed, dim3(1), dim3(256), 0, ps, ctx->d_list, hdr, ctx->d_wide_list, c.d_wide_count,
                     r.use_plain ? c.d_count : (int32_t*)nullptr, c.d_cursor);      // (cleared for the re-plan below)
  align_ck(ctx, c, "scan fill seed");
  const size_t quad_lds = (size_t)Q_G * q_sub_bytes(ctx->max_len) + 16;
  if (r.use_plain) {
    if (stage_begin(ctx, STG_PLAIN, ps)) return MIA_HIP_ERR_NOMEM;
    hipLaunchKernelGGL(k_align_quad_plain, dim3(ctx->quad_wgs), dim3(64), quad_lds, ps, ctx->rs, c.ref, ctx->d_pssm, ctx->d_list, 0, ctx->d_bin_of,
                       (const int32_t*)(hdr + PH_QUAD));
    stage_end(ctx, STG_PLAIN, ps);
    align_ck(ctx, c, "quad plain");
    if (int rcw = align_window_classes(ctx, c)) return rcw;
    // what it could not finish (and what the filter's gap hint kept out of it), re-planned into quads
    // (d_count / d_cursor: cleared by k_wide_seed)
    hipLaunchKernelGGL(k_plan_recount, dim3(c.gb), dim3(256), 0, ps, n, ctx->d_bin_of, c.d_count);
    hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(512), 0, ps, c.d_count, c.d_off, hdr, 1, ctx->d_list);
    hipLaunchKernelGGL(k_plan_fill, dim3(c.gb), dim3(256), 0, ps, n, ctx->d_bin_of, c.d_off, c.d_cursor, ctx->d_list);
    align_ck(ctx, c, "replan");
  }
  const int64_t slab = (int64_t)Q_G * MAX_READ * Q_TRACE_STRIDE;
  if (!ctx->d_quad_slabs && dev_alloc(ctx, ctx->d_quad_slabs, slab * ctx->quad_wgs)) return MIA_HIP_ERR_NOMEM;
  if (c.dbg_steps) {
    int32_t hh[PH_WORDS];
    (void)hipMemcpy(hh, hdr, sizeof hh, hipMemcpyDeviceToHost);
    fprintf(stderr, "[align_all deferred] hdr:");
    for (int k = 0; k < PH_WORDS; k++) fprintf(stderr, " %d", hh[k]);
    fprintf(stderr, "  n=%lld max_len=%d quad_lds=%zu\n", (long long)n, ctx->max_len, quad_lds);
  }
  if (stage_begin(ctx, STG_TRACE, ps)) return MIA_HIP_ERR_NOMEM;
  hipLaunchKernelGGL(k_align_quad, dim3(ctx->quad_wgs), dim3(64), quad_lds, ps, ctx->rs, c.ref, ctx->d_pssm, ctx->packs.p[0], ctx->d_list, 0,
                     ctx->d_quad_slabs, slab, ctx->d_wide_list, c.d_wide_count, ctx->d_retry_list, hdr + PH_RETRY + 1, /*band=*/1, ctx->dbg,
                     (const int32_t*)(hdr + PH_QUAD));
  stage_end(ctx, STG_TRACE, ps);
  HIPCHK(hipGetLastError());
  align_ck(ctx, c, "quad trace");
  if (!r.use_plain) { if (int rcw = align_window_classes(ctx, c)) return rcw; }
  // (the last launch of the planner's chain: on stream2 it signals ev_join itself, see bx_join_and_retry)
  const bool sig = r.planner_aside && c.pending_join && (ctx->ext_events & 4u);
  hipError_t e = launch_window_class(ctx, 0, ctx->d_retry_list, 0, hdr + PH_RETRY, ps, false, sig ? ctx->ev_join : nullptr);
  c.planner_end_signalled = sig && e == hipSuccess;
  if (e != hipSuccess) { ctx->err = std::string("k_align_window retry launch: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  return MIA_HIP_OK;
}

// CLOSING STATE: an alignment stands, whatever was derived from the one before does not
static int align_close(mia_hip_ctx* ctx) {
  ctx->aligned = true; ctx->culled = false; ctx->tallied = false; ctx->pre_cull_valid = false;
  return MIA_HIP_OK;
}

// ... the join and the deferred call's one look at the counters: wide / retry counts, the planner's header, filter and band-pipeline
// counters lie side by side in the control block
static int align_finish_deferred(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  align_ck(ctx, c, "retry");
  if (int rcj = bx_join_and_retry(ctx, c)) return rcj;
  align_ck(ctx, c, "band join");
  constexpr int CN = CTRL_CN;
  std::vector<int32_t> pageable;
  int32_t* hb;
  if (ctx->h_pin) hb = reinterpret_cast<int32_t*>(ctx->h_pin);
  else { pageable.resize(CN); hb = pageable.data(); }
  const bool pre_cull = ctx->in_iterate && ctx->comm;
  if (pre_cull) { if (int rcp = comm_pre_cull_enqueue(ctx, c.d_wide_count)) return rcp; }
  const bool spec = ctx->spec_ok && ctx->h_pin && !pre_cull && !c.dbg_steps;
  // (a copy in the middle of the step holds the stream up for 20 us: with zero_copy the step's last kernel, k_cons_scatter,
  // writes these words into h_pin itself, whether or not the speculation held)
  if (!(spec && ctx->zero_copy)) HIPCHK(hipMemcpyAsync(hb, ctx->d_ctr0, (size_t)CN * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (spec) {
    // mia_hip_iterate, one context, a cut line that needs no scores on the host: no wait here.  The caller queues cull,
    // tally and consensus behind this copy; their kernels look at the exact-kernel count themselves (abort_if) and
    // iterate_body reads these counters when it waits for the consensus (align_counters_collect).
    ctx->spec_pending = true; ctx->spec_filtered = r.filtered; ctx->spec_bx = r.bx; ctx->spec_plain = r.use_plain;
    ctx->abort_if = ctx->spec_force ? ctx->d_one : c.d_wide_count;      // (MIA_HIP_SPEC_TEST=1: every iteration takes the second round)
    return align_close(ctx);
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  align_counters_collect(ctx, hb, r.filtered, r.bx, r.use_plain);
  const int32_t n_wide = hb[0];
  if (n_wide > 0) { if (int rcw = run_wide(ctx, c.ref, n_wide)) return rcw; }
  if (pre_cull && comm_pre_cull_collect(ctx)) {
    // some rank had reads for the exact kernel: its sums were taken before their scores were final.  Every rank saw the
    // same eight words per rank, so every rank comes here and the all-gather is repeated with the final numbers.
    if (int rcp = comm_pre_cull_enqueue(ctx, nullptr)) return rcp;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    (void)comm_pre_cull_collect(ctx);
  }
  return align_close(ctx);
}

// PLANNER CHAIN, HOST-ROUND-TRIP FORM (mia_hip_realign, mia_hip_align_windows, pass 1): the bins' counts come to the host, which sizes
// every launch.  Host copies of the counters live in pinned memory when there is some: a copy to or from pageable memory makes the
// host wait for the stream even when it is called "async"
struct HostPlan {
  int32_t local_buf[4 * N_BINS + 16];
  int32_t *h_count, *h_off, *h_count2, *h_off2, *h_misc;
  std::vector<uint32_t> bxc_pageable;
  uint32_t* h_bxc;                                  // all counters of the band pipeline (8 KB), read once the stream is waited for anyway
  bool bx_counters_later = false;                   // (with the band kernels still running beside this stream their counters are read behind the join)
  int n_quads = 0, quad_begin = 0;
  bool wide_known = false;
};

static void host_take_bx_counters(mia_hip_ctx* ctx, const HostPlan& h) {
  ctx->filter_proven += h.h_bxc[BXC_DONE_PLAN * BXC_STRIDE];          // finished without any DP: by the diagonal filter or by the band plan
  for (int k = 0; k < 3; k++) ctx->bx_done[k] += h.h_bxc[(BXC_DONE_PLAN + k) * BXC_STRIDE];
  ctx->bx_seen += h.h_bxc[BXC_SEEN * BXC_STRIDE];
  for (int k = 0; k < BXC_COUNTERS; k++) ctx->bx_last[k] = h.h_bxc[k * BXC_STRIDE];
}

// ... its first round: counters to the host, the lists filled, the window classes launched
static int align_planner_host_fill(mia_hip_ctx* ctx, AlignCall& c, HostPlan& h) {
  const AlignRoute& r = c.r;
  const int64_t n = ctx->rs.n;
  int32_t* hb = ctx->h_pin ? reinterpret_cast<int32_t*>(ctx->h_pin) : h.local_buf;
  h.h_count = hb; h.h_off = hb + N_BINS; h.h_count2 = hb + 2 * N_BINS; h.h_off2 = hb + 3 * N_BINS; h.h_misc = hb + 4 * N_BINS;
  int32_t *h_count = h.h_count, *h_off = h.h_off, *h_misc = h.h_misc;
  h_misc[0] = 0;
  h_misc[6] = 0;
  if (ctx->h_pin) h.h_bxc = reinterpret_cast<uint32_t*>(ctx->h_pin + (24 << 10));
  else { h.bxc_pageable.resize(BXC_WORDS); h.h_bxc = h.bxc_pageable.data(); }
  for (int k = 0; k < BXC_COUNTERS; k++) h.h_bxc[k * BXC_STRIDE] = 0;
  if (r.filtered) {
    HIPCHK(hipMemcpyAsync(&h_misc[0], ctx->d_filter_n, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&h_misc[6], ctx->d_filter_n + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (r.bx) HIPCHK(hipMemcpyAsync(h.h_bxc, ctx->d_bx_ctr, BXC_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipMemcpyAsync(h_count, c.d_count, (size_t)N_BINS * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->filter_proven += (uint32_t)h_misc[0];
  ctx->band_done += (uint32_t)h_misc[6];
  ctx->filter_seen += n;
  h.bx_counters_later = c.pending_join;
  if (!h.bx_counters_later) host_take_bx_counters(ctx, h);
  int run = 0;
  for (int b = 0; b < N_BINS; b++) {
    h_off[b] = run;
    run += b >= BIN_QUAD0 ? ((h_count[b] + 3) & ~3) : h_count[b];   // quad bins: every read length padded to whole quads
  }
  h.quad_begin = h_off[BIN_QUAD0]; h.n_quads = (run - h.quad_begin) / 4;
  if (h.n_quads > 0) HIPCHK(hipMemsetAsync(ctx->d_list + h.quad_begin, 0xFF, (size_t)(run - h.quad_begin) * 4, ctx->stream));   // -1 = empty slot
  HIPCHK(hipMemcpyAsync(c.d_off, h_off, (size_t)N_BINS * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_plan_fill, dim3(c.gb), dim3(256), 0, ctx->stream, n, ctx->d_bin_of, c.d_off, c.d_cursor, ctx->d_list);
  // reads that need the exact kernel from the start: copy their list to the head of wide_list
  const int n_wide0 = h_count[BIN_WIDE];
  if (n_wide0 > 0) {
    HIPCHK(hipMemcpyAsync(ctx->d_wide_list, ctx->d_list + h_off[BIN_WIDE], (size_t)n_wide0 * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(c.d_wide_count, &h_count[BIN_WIDE], 4, hipMemcpyHostToDevice, ctx->stream));
  }
  for (int ci = 0; ci < N_CPL; ci++) {
    if (h_count[ci] == 0) continue;
    hipError_t e = launch_window_class(ctx, ci, ctx->d_list + h_off[ci], h_count[ci]);
    if (e != hipSuccess) { ctx->err = std::string("k_align_window launch: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  }
  return MIA_HIP_OK;
}

// ... first pass over the quads: values only; reads whose alignment is provably the pure diagonal are finished there; what is left
// (and what the filter's gap hint kept out of the first pass) is re-planned into quads of equal read length
static int align_planner_host_plain(mia_hip_ctx* ctx, AlignCall& c, HostPlan& h) {
  const int64_t n = ctx->rs.n;
  if (h.n_quads > 0) {
    const int grid = h.n_quads < ctx->quad_wgs ? h.n_quads : ctx->quad_wgs;
    const size_t quad_lds = (size_t)Q_G * q_sub_bytes(ctx->max_len) + 16;
    if (stage_begin(ctx, STG_PLAIN)) return MIA_HIP_ERR_NOMEM;
    hipLaunchKernelGGL(k_align_quad_plain, dim3(grid), dim3(64), quad_lds, ctx->stream, ctx->rs, c.ref, ctx->d_pssm, ctx->d_list + h.quad_begin,
                       h.n_quads, ctx->d_bin_of, (const int32_t*)nullptr);
    stage_end(ctx, STG_PLAIN);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemsetAsync(c.d_count, 0, (size_t)N_BINS * 4, ctx->stream));
  HIPCHK(hipMemsetAsync(c.d_cursor, 0, (size_t)N_BINS * 4, ctx->stream));
  hipLaunchKernelGGL(k_plan_recount, dim3(c.gb), dim3(256), 0, ctx->stream, n, ctx->d_bin_of, c.d_count);
  HIPCHK(hipMemcpyAsync(h.h_count2, c.d_count, (size_t)N_BINS * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int run2 = 0;
  for (int b = 0; b < N_BINS; b++) { h.h_off2[b] = run2; run2 += b >= BIN_QUAD0 ? ((h.h_count2[b] + 3) & ~3) : 0; }
  ctx->plain_total += (int64_t)h.n_quads * 4;
  for (int b = BIN_QUAD0; b < N_BINS; b++) ctx->plain_retried += h.h_count2[b];
  h.n_quads = run2 / 4;
  h.quad_begin = 0;
  if (h.n_quads > 0) {
    HIPCHK(hipMemsetAsync(ctx->d_list, 0xFF, (size_t)run2 * 4, ctx->stream));
    HIPCHK(hipMemcpyAsync(c.d_off, h.h_off2, (size_t)N_BINS * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_plan_fill, dim3(c.gb), dim3(256), 0, ctx->stream, n, ctx->d_bin_of, c.d_off, c.d_cursor, ctx->d_list);
  }
  return MIA_HIP_OK;
}

// ... the trace pass over the quads, and the reads whose path left the stored trace band: one-read kernel with the full trace
// (windows <= 208 fit class 0)
static int align_planner_host_trace(mia_hip_ctx* ctx, AlignCall& c, HostPlan& h) {
  const int64_t slab = (int64_t)Q_G * MAX_READ * Q_TRACE_STRIDE;
  const int grid = h.n_quads < ctx->quad_wgs ? h.n_quads : ctx->quad_wgs;
  if (!ctx->d_quad_slabs && dev_alloc(ctx, ctx->d_quad_slabs, slab * ctx->quad_wgs)) return MIA_HIP_ERR_NOMEM;
  const size_t quad_lds = (size_t)Q_G * q_sub_bytes(ctx->max_len) + 16;
  if (stage_begin(ctx, STG_TRACE)) return MIA_HIP_ERR_NOMEM;
  hipLaunchKernelGGL(k_align_quad, dim3(grid), dim3(64), quad_lds, ctx->stream, ctx->rs, c.ref, ctx->d_pssm, ctx->packs.p[0], ctx->d_list + h.quad_begin,
                     h.n_quads, ctx->d_quad_slabs, slab, ctx->d_wide_list, c.d_wide_count, ctx->d_retry_list, c.d_wide_count + 1, /*band=*/1,
                     ctx->dbg, (const int32_t*)nullptr);
  stage_end(ctx, STG_TRACE);
  HIPCHK(hipGetLastError());
  // (the two counters sit side by side: one copy, one wait; the wide count is final unless the retry kernel runs)
  HIPCHK(hipMemcpyAsync(&h.h_misc[2], c.d_wide_count, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int32_t n_retry = h.h_misc[3];
  if (n_retry > 0) {
    hipError_t e = launch_window_class(ctx, 0, ctx->d_retry_list, n_retry);
    if (e != hipSuccess) { ctx->err = std::string("k_align_window retry launch: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  } else {
    h.wide_known = true;
  }
  return MIA_HIP_OK;
}

static int align_planner_host(mia_hip_ctx* ctx, AlignCall& c) {
  const AlignRoute& r = c.r;
  HostPlan h;
  if (int rc = align_planner_host_fill(ctx, c, h)) return rc;
  if ((h.n_quads > 0 || r.filtered) && r.use_plain) { if (int rc = align_planner_host_plain(ctx, c, h)) return rc; }
  if (h.n_quads > 0) { if (int rc = align_planner_host_trace(ctx, c, h)) return rc; }
  if (c.pending_join) { if (int rcj = bx_join_and_retry(ctx, c)) return rcj; h.wide_known = false; }
  // exact kernel for whole-reference windows and escaped reads
  if (!h.wide_known) {
    HIPCHK(hipMemcpyAsync(&h.h_misc[2], c.d_wide_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (h.bx_counters_later) HIPCHK(hipMemcpyAsync(h.h_bxc, ctx->d_bx_ctr, BXC_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (h.bx_counters_later) host_take_bx_counters(ctx, h);
  }
  const int32_t n_wide = h.h_misc[2];
  if (n_wide > 0) { if (int rcw = run_wide(ctx, c.ref, n_wide)) return rcw; }
  return align_close(ctx);
}

// every strand_known read against its window of ctx->d_ref: plan, values-only pass, trace kernels, exact kernel
static int align_all(mia_hip_ctx* ctx) {
  const int64_t n = ctx->rs.n;
  if (!ctx->spec_ok) { ctx->spec_pending = false; ctx->abort_if = nullptr; }
  ctx->align_end_signalled = false;
  ctx->buckets_queued = 0;                  // (a counting sort queued for an earlier alignment is void)
  if (n == 0) { ctx->aligned = true; return MIA_HIP_OK; }
  AlignCall c;
  c.r = align_route(align_route_in(ctx));
  const AlignRoute& r = c.r;
  ctx->last_route_bx = r.bx;
  c.ref = RefInfo{ctx->d_ref, ctx->L, ctx->wrap, ctx->explicit_win};
  c.d_count = ctx->d_bins; c.d_off = ctx->d_bins + N_BINS; c.d_cursor = ctx->d_bins + 2 * N_BINS; c.d_wide_count = ctx->d_bins + 3 * N_BINS;
  c.gb = (int)((n + (int64_t)256 * PLAN_PER - 1) / ((int64_t)256 * PLAN_PER));
  c.dbg_steps = ctx->deferred && alt_env("MIA_HIP_ITER_DEBUG") != nullptr;
  if (int rc = align_ensure_buffers(ctx, c)) return rc;
  if (int rc = align_ref_prep(ctx, c)) return rc;
  if (r.bx) {
    align_bx_dev(ctx, c);
    if (int rc = align_plan_launches(ctx, c)) return rc;
    if (r.three_streams) { if (int rc = align_band_dps(ctx, c)) return rc; }
    else if (r.two_streams) { if (int rc = align_band_dps_serial(ctx, c)) return rc; }
    ctx->bx_launches++;
  } else if (r.filtered) {
    if (int rc = align_round1(ctx, c)) return rc;
  }
  c.ps = r.planner_aside ? ctx->stream2 : ctx->stream;
  if (r.plan_count_late)
    hipLaunchKernelGGL(k_plan_count, dim3(c.gb), dim3(256), 0, c.ps, ctx->rs, c.ref, ctx->packs, /*use_quad=*/1, (int)r.filtered, (int)(r.filtered && r.use_plain), ctx->d_bin_of,
                       c.d_count, ctx->d_filter_n);
  if (!ctx->deferred) return align_planner_host(ctx, c);
  if (int rc = align_planner_deferred(ctx, c)) return rc;
  return align_finish_deferred(ctx, c);
}

extern "C" int mia_hip_align_windows(mia_hip_ctx* ctx, const char* ref, int64_t ref_len, const int64_t* win_start, const int32_t* win_len) {
  if (!ctx || !ref || !win_start || !win_len || ref_len <= 0) return MIA_HIP_ERR_ARG;
  if (!ctx->have_pssm || !ctx->d_packed) { ctx->err = "set_pssm and upload_reads must precede align_windows"; return MIA_HIP_ERR_STATE; }
  if (ref_len > INT32_MAX - 128) { ctx->err = "align_windows: the reference string must stay below 2^31 characters"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->rs.n;
  std::vector<int32_t> as((size_t)n), ae((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    if (win_len[i] <= 0 || win_start[i] < 0 || win_start[i] + win_len[i] > ref_len) {
      ctx->err = "align_windows: window " + std::to_string(i) + " is empty or leaves the reference string";
      return MIA_HIP_ERR_ARG;
    }
    as[(size_t)i] = (int32_t)win_start[i];
    ae[(size_t)i] = (int32_t)(win_start[i] + win_len[i] - 1);
  }
  std::vector<uint8_t> codes((size_t)ref_len + 64, 4);
  for (int64_t i = 0; i < ref_len; i++) codes[(size_t)i] = base_code(ref[i]);
  if (dev_ensure(ctx, ctx->d_ref, (int64_t)codes.size())) return MIA_HIP_ERR_NOMEM;
  HIPCHK(hipMemcpyAsync(ctx->d_ref, codes.data(), codes.size(), hipMemcpyHostToDevice, ctx->stream));
  if (n) {
    HIPCHK(hipMemcpyAsync(ctx->d_as, as.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_ae, ae.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  // not a reference the consensus path can use: cull / tally need a realign first
  ctx->L = (int)ref_len; ctx->wrap = (int)ref_len; ctx->have_ref = false; ctx->explicit_win = 1; ctx->ref_mostly_bases = true; ctx->kh_entries = 0;
  const int rcode = align_all(ctx);
  HIPCHK(hipStreamSynchronize(ctx->stream));   // as / ae / codes are host buffers of this call
  return rcode;
}

extern "C" int mia_hip_get_alignments(mia_hip_ctx* ctx, int32_t* score, int32_t* as, int32_t* ae) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->aligned) { ctx->err = "realign first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->rs.n;
  if (score) HIPCHK(hipMemcpyAsync(score, ctx->d_score, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (as) HIPCHK(hipMemcpyAsync(as, ctx->d_as, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (ae) HIPCHK(hipMemcpyAsync(ae, ctx->d_ae, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_scripts(mia_hip_ctx* ctx, int16_t* cols, int32_t stride, int32_t* ref_start) {
  if (!ctx || (cols && stride < ctx->max_len)) return MIA_HIP_ERR_ARG;
  if (!ctx->aligned) { ctx->err = "realign first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->rs.n;
  if (cols) {
    if (ctx->diag_scripts_missing && n > 0) {
      hipLaunchKernelGGL(k_diag_scripts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rs);
      HIPCHK(hipGetLastError());
      ctx->diag_scripts_missing = false;
    }
    HIPCHK(hipMemcpy2DAsync(cols, (size_t)stride * 2, ctx->d_cols, (size_t)ctx->rs.stride * 2, (size_t)ctx->max_len * 2, n,
                            hipMemcpyDeviceToHost, ctx->stream));
  }
  if (ref_start) HIPCHK(hipMemcpyAsync(ref_start, ctx->d_refstart, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

// ---- cull ----------------------------------------------------------------------
static int finish_params(mia_hip_ctx* ctx);
// second half of the cull: every link (own or gathered) acts on the slot it points at, then each read's dropped bits,
// depth-code parameters and multiplicities are final.  Runs at the end of mia_hip_cull and again after mia_hip_set_links.
static int finish_cull(mia_hip_ctx* ctx) {
  const int64_t nl = ctx->links_cap_all;
  if (dev_ensure(ctx, ctx->d_link_len, nl, nl + 64) || dev_ensure(ctx, ctx->d_link_act, nl, nl + 64)) return MIA_HIP_ERR_NOMEM;
  // (the context's own links behind a cull that took the ticket: k_cull_records' last workgroup has applied them)
  if (!(ctx->cull_applied && ctx->d_links_all == ctx->lk.rec))
    hipLaunchKernelGGL(k_links_apply, dim3(32), dim3(256), 0, ctx->stream, ctx->d_links_all, ctx->d_n_links_all, (int32_t)ctx->links_cap_all, ctx->si,
                       ctx->d_slot_dropped, ctx->n_slots, ctx->d_link_len, ctx->d_link_act, ctx->d_cull_flags, ctx->abort_if);
  ctx->links_applied = true;
  return finish_params(ctx);
}

static int finish_params(mia_hip_ctx* ctx) {
  const int64_t n = ctx->rs.n;
  hipLaunchKernelGGL(k_rec_params, dim3((int)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rs, ctx->L, ctx->d_slot, ctx->d_slot_dropped,
                     ctx->n_slots, ctx->d_back_slot, ctx->ri, ctx->si, ctx->d_links_all, ctx->d_link_len, ctx->d_link_act, ctx->d_n_links_all,
                     (int32_t)ctx->links_cap_all, ctx->read_base, ctx->d_drop_f, ctx->d_drop_b, ctx->d_cull_flags, ctx->abort_if,
                     (ctx->umax_valid && ctx->rs.roff == ctx->d_roff && ctx->d_rplanes && ctx->d_umax) ? ctx->d_umax : (const int32_t*)nullptr,
                     (ctx->cull_with_records && ctx->d_n_links_all == ctx->lk.n) ? 1 : 0);
  HIPCHK(hipGetLastError());
  return MIA_HIP_OK;
}

// the error flags of the cull kernels, checked where the stream is synchronised anyway
static int check_cull_flags(mia_hip_ctx* ctx, uint32_t fl) {
  if (fl & 8u) { ctx->err = "more formerly split reads than the link list holds"; return MIA_HIP_ERR_RANGE; }
  if (fl & 4u) {
    ctx->err = "a formerly split read points at an AlnSeq slot that holds no record of this iteration (the reference would show "
               "the slot's content from an earlier iteration); not reproduced";
    return MIA_HIP_ERR_RANGE;
  }
  return MIA_HIP_OK;
}

extern "C" int mia_hip_cull(mia_hip_ctx* ctx, int32_t hard_cut, double slope, double intercept, int64_t slot_base) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->aligned) { ctx->err = "realign first"; return MIA_HIP_ERR_STATE; }
  if (ctx->explicit_win) { ctx->err = "the last alignment ran on caller-supplied windows (align_windows): realign first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->rs.n;
  if (n == 0) return MIA_HIP_OK;
  // (two launches: record counts per block of 256 reads, scanned by the block that finishes last; then slots, record
  // geometry, dropped marks and links of every read in one kernel -- k_slot_count / k_cull_records)
  const int nb = (int)((n + 255) / 256);
  if (!ctx->d_cull_sync) {
    if (dev_alloc(ctx, ctx->d_cull_sync, 4)) return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemsetAsync(ctx->d_cull_sync, 0, 16, ctx->stream));
  }
  if (!ctx->d_cull_stats) {
    if (dev_alloc(ctx, ctx->d_cull_stats, 4)) return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemsetAsync(ctx->d_cull_stats, 0, 16, ctx->stream));
  }
  hipLaunchKernelGGL(k_slot_count, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, ctx->stream, ctx->rs, ctx->L, ctx->d_partial, nb, slot_base, ctx->d_total, (uint32_t*)nullptr, ctx->abort_if,
                     (const uint8_t*)ctx->d_link_mark);
  // (MIA_HIP_CULL_SCAN=1: the counts scanned by a single-workgroup launch in between, as before)
  if (ctx->cull_scan) hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, ctx->stream, ctx->d_partial, nb, slot_base, ctx->d_total, ctx->abort_if);
  if (slot_base + 2 * n + 16 > ctx->n_slots) {   // sharded runs: slots are global indices
    DevBuf<uint8_t> nd;
    const int64_t ns = slot_base + 2 * n + 16;
    if (dev_alloc(ctx, nd, ns)) return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemsetAsync(nd, 0, (size_t)ns, ctx->stream));
    HIPCHK(hipMemcpyAsync(nd, ctx->d_slot_dropped, (size_t)ctx->n_slots, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->d_slot_dropped = std::move(nd);
    ctx->n_slots = ns;
  }
  // records per read and per slot, the reads' own dropped marks, and the links of formerly split reads -- all without a
  // host round trip: the record total and the link count stay on the device, the error flags are read by mia_hip_tally
  ctx->slot_base = slot_base;
  ctx->si.base = slot_base;
  ctx->si.n_local_p = ctx->d_total;
  if (!ctx->in_iterate) HIPCHK(hipMemsetAsync(ctx->lk.n, 0, 8, ctx->stream));                     // link count, cull flags (neighbours in the control block)
  // lean: only where nothing but this call's own finish_cull can want the side arrays -- a sharded iteration applies gathered links
  // (k_rec_geom, k_links_apply on the full list), a step-wise caller may go on with mia_hip_set_links
  const bool lean_ok = ctx->in_iterate && !ctx->comm && ctx->cull_with_records && !ctx->cull_scan && !ctx->no_cull_lean;
  const bool apply = lean_ok && !ctx->no_cull_apply;
  if (apply && (dev_ensure(ctx, ctx->d_link_len, (int64_t)ctx->lk.cap, (int64_t)ctx->lk.cap + 64) || dev_ensure(ctx, ctx->d_link_act, (int64_t)ctx->lk.cap, (int64_t)ctx->lk.cap + 64)))
    return MIA_HIP_ERR_NOMEM;
  hipLaunchKernelGGL(k_cull_records, dim3((unsigned)nb), dim3(256), 0, ctx->stream, ctx->rs, ctx->L, (const int64_t*)ctx->d_partial, ctx->d_slot, ctx->ri, ctx->si,
                     ctx->read_base, ctx->d_cull_flags, ctx->d_slot_dropped, ctx->n_slots, hard_cut, slope, intercept, ctx->d_back_slot,
                     (const int64_t*)ctx->d_front_slot0, ctx->lk, ctx->dev_cut, ctx->abort_if, ctx->cull_scan ? 0 : nb, slot_base, ctx->d_total,
                     ctx->cull_with_records ? 1 : 0, ctx->d_drop_f, ctx->d_drop_b,
                     (ctx->umax_valid && ctx->rs.roff == ctx->d_roff && ctx->d_rplanes && ctx->d_umax) ? ctx->d_umax : (const int32_t*)nullptr,
                     lean_ok ? 1 : 0, (int32_t*)ctx->d_cull_stats,
                     apply ? (uint32_t*)ctx->d_cull_sync : (uint32_t*)nullptr, (int32_t*)ctx->d_link_len, (int32_t*)ctx->d_link_act,
                     (uint8_t*)ctx->d_link_mark);
  HIPCHK(hipGetLastError());
  ctx->cull_lean_ok = lean_ok;
  ctx->cull_applied = apply;
  // by default the links to apply are this context's own; a sharded run replaces them with the gathered list (mia_hip_set_links)
  ctx->d_links_all = ctx->lk.rec;
  ctx->d_n_links_all = ctx->lk.n;
  ctx->links_cap_all = ctx->lk.cap;
  ctx->culled = true;
  ctx->links_applied = false;
  return finish_cull(ctx);
}

// the reads' mark bytes again, behind a copy into d_back_slot or d_front_slot0
static int link_marks_launch(mia_hip_ctx* ctx) {
  const int64_t n = ctx->rs.n;
  if (n == 0) return MIA_HIP_OK;
  hipLaunchKernelGGL(k_link_marks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, (const int64_t*)ctx->d_back_slot, (const int64_t*)ctx->d_front_slot0,
                     (uint8_t*)ctx->d_link_mark);
  HIPCHK(hipGetLastError());
  return MIA_HIP_OK;
}
// {links counted before the last cull (-1: not counted, MIA_HIP_CULL_SCAN), 1 if that cull ran in its lean form}
static int cull_stats_read(mia_hip_ctx* ctx, int32_t* st) {
  st[0] = -1; st[1] = 0;
  if (!ctx->d_cull_stats) return MIA_HIP_OK;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(st, ctx->d_cull_stats, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}
extern "C" int mia_hip_cull_stats(mia_hip_ctx* ctx, int64_t* links_before, int32_t* lean) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->culled) { ctx->err = "cull first"; return MIA_HIP_ERR_STATE; }
  int32_t st[2];
  if (int rc = cull_stats_read(ctx, st)) return rc;
  if (links_before) *links_before = st[0];
  if (lean) *lean = st[1];
  return MIA_HIP_OK;
}
// The step-wise calls that go on from a cull's d_slot and side arrays: after a lean cull those hold an earlier iteration's values
static int refuse_after_lean_cull(mia_hip_ctx* ctx) {
  if (!ctx->cull_lean_ok) return MIA_HIP_OK;
  int32_t st[2];
  if (int rc = cull_stats_read(ctx, st)) return rc;
  if (!st[1]) return MIA_HIP_OK;
  ctx->err = "the last cull ran inside mia_hip_iterate without a link and left the slot and link side arrays unwritten: call mia_hip_cull first";
  return MIA_HIP_ERR_STATE;
}

extern "C" int mia_hip_set_back_slots(mia_hip_ctx* ctx, const int64_t* back_slot) {
  if (ctx) ctx->pre_cull_valid = false;
  if (!ctx || !back_slot) return MIA_HIP_ERR_ARG;
  if (!ctx->d_back_slot) { ctx->err = "upload_reads first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(ctx->d_back_slot, back_slot, (size_t)ctx->rs.n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (int rcm = link_marks_launch(ctx)) return rcm;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

extern "C" int mia_hip_set_pass1_state(mia_hip_ctx* ctx, const int64_t* front_slot, const int64_t* back_slot, const int32_t* score) {
  if (ctx) ctx->pre_cull_valid = false;
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->d_back_slot) { ctx->err = "upload_reads first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->rs.n;
  if (front_slot) HIPCHK(hipMemcpyAsync(ctx->d_front_slot0, front_slot, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (back_slot) HIPCHK(hipMemcpyAsync(ctx->d_back_slot, back_slot, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (score) HIPCHK(hipMemcpyAsync(ctx->d_score, score, n * 4, hipMemcpyHostToDevice, ctx->stream));
  if (int rcm = link_marks_launch(ctx)) return rcm;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

extern "C" int mia_hip_set_read_base(mia_hip_ctx* ctx, int64_t read_base) {
  if (!ctx || read_base < 0) return MIA_HIP_ERR_ARG;
  ctx->read_base = read_base;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_links(mia_hip_ctx* ctx, int64_t** d_links, int64_t* n_links) {
  if (!ctx || !ctx->culled) return MIA_HIP_ERR_STATE;
  int32_t nl = 0;
  HIPCHK(hipSetDevice(ctx->device));
  // on the context's own (non-blocking) stream, behind the k_cull_mark that counts the links; once it has been waited for,
  // the list itself is complete too and the caller's collective may read it from any stream
  HIPCHK(hipMemcpyAsync(&nl, ctx->lk.n, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (d_links) *d_links = ctx->lk.rec;
  if (n_links) *n_links = nl;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_set_links(mia_hip_ctx* ctx, const int64_t* d_links_all, int64_t n_all) {
  if (!ctx || n_all < 0 || (n_all > 0 && !d_links_all)) return MIA_HIP_ERR_ARG;
  if (!ctx->culled) { ctx->err = "cull first"; return MIA_HIP_ERR_STATE; }
  if (n_all >= (int64_t)LINK_NONE) { ctx->err = "too many links"; return MIA_HIP_ERR_RANGE; }
  if (int rcl = refuse_after_lean_cull(ctx)) return rcl;
  HIPCHK(hipSetDevice(ctx->device));
  // own copy of the gathered list (the caller's buffer may be a temporary of the collective)
  if (n_all * 4 > (ctx->owned_links.empty() ? 0 : ctx->owned_links.back().cap)) {      // (a link is four words)
    DevBuf<int64_t> nb;
    if (dev_alloc(ctx, nb, (n_all + 64) * 4)) return MIA_HIP_ERR_NOMEM;
    ctx->owned_links.push_back(std::move(nb));      // (the previous gathered buffer, if any, is released with the context)
  }
  if (!ctx->owned_links.empty()) ctx->d_links_all = ctx->owned_links.back();
  if (n_all > 0) HIPCHK(hipMemcpyAsync(ctx->d_links_all, d_links_all, (size_t)n_all * 32, hipMemcpyDeviceToDevice, ctx->stream));
  ctx->n_links_all = (int32_t)n_all;
  if (!ctx->d_n_links_gathered && dev_alloc(ctx, ctx->d_n_links_gathered, 1)) return MIA_HIP_ERR_NOMEM;
  const int32_t n32 = (int32_t)n_all;
  HIPCHK(hipMemcpyAsync(ctx->d_n_links_gathered, &n32, 4, hipMemcpyHostToDevice, ctx->stream));
  ctx->d_n_links_all = ctx->d_n_links_gathered;
  ctx->links_cap_all = n_all;
  // slot state back to "owners only", then every link once
  const int64_t n = ctx->rs.n;
  HIPCHK(hipMemsetAsync(ctx->d_cull_flags, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_rec_geom, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rs, ctx->L, ctx->d_slot, ctx->ri, ctx->si,
                     ctx->read_base, ctx->d_cull_flags);
  HIPCHK(hipGetLastError());
  const int rc_fc = finish_cull(ctx);
  HIPCHK(hipStreamSynchronize(ctx->stream));   // n32 above is a stack local; the caller's buffer may be a temporary
  return rc_fc;
}

extern "C" int mia_hip_link_lengths(mia_hip_ctx* ctx, int32_t** d_len, int32_t** d_act, int64_t* n) {
  if (!ctx || !ctx->links_applied) return MIA_HIP_ERR_STATE;
  if (int rcl = refuse_after_lean_cull(ctx)) return rcl;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // k_links_apply fills both buffers; the caller reduces them on a stream of its own
  if (d_len) *d_len = ctx->d_link_len;
  if (d_act) *d_act = ctx->d_link_act;
  if (n) *n = ctx->n_links_all;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_finish_links(mia_hip_ctx* ctx) {
  if (!ctx || !ctx->links_applied) return MIA_HIP_ERR_STATE;
  if (int rcl = refuse_after_lean_cull(ctx)) return rcl;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemsetAsync(ctx->d_cull_flags, 0, 4, ctx->stream));
  return finish_params(ctx);
}

extern "C" int mia_hip_get_record_params(mia_hip_ctx* ctx, int32_t* params, int64_t* back_slot) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->culled) { ctx->err = "cull first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->rs.n;
  if (params) HIPCHK(hipMemcpy2DAsync(params, 32, ctx->ri.trec + TREC_PARAMS, 64, 32, n, hipMemcpyDeviceToHost, ctx->stream));   // words 8..15 of each record
  if (back_slot) HIPCHK(hipMemcpyAsync(back_slot, ctx->d_back_slot, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_dropped(mia_hip_ctx* ctx, uint8_t* front, uint8_t* back) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->rs.n;
  if (front) HIPCHK(hipMemcpyAsync(front, ctx->d_drop_f, n, hipMemcpyDeviceToHost, ctx->stream));
  if (back) HIPCHK(hipMemcpyAsync(back, ctx->d_drop_b, n, hipMemcpyDeviceToHost, ctx->stream));
  uint32_t cflags = 0;
  if (ctx->culled) HIPCHK(hipMemcpyAsync(&cflags, ctx->d_cull_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return check_cull_flags(ctx, cflags);
}

extern "C" int mia_hip_set_slot_dropped(mia_hip_ctx* ctx, const uint8_t* flags, int64_t n_flags) {
  if (!ctx || !flags || n_flags < 0) return MIA_HIP_ERR_ARG;
  if (!ctx->d_slot_dropped) { ctx->err = "upload_reads first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  if (n_flags > ctx->n_slots) {            // a shard is handed the marks of ALL slots: its own lie behind the other ranks'
    const int rca = dev_alloc(ctx, ctx->d_slot_dropped, n_flags + 16);
    ctx->n_slots = ctx->d_slot_dropped.cap;      // (0 with the block gone)
    if (rca) return rca;
  }
  HIPCHK(hipMemsetAsync(ctx->d_slot_dropped, 0, (size_t)ctx->n_slots, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_slot_dropped, flags, (size_t)n_flags, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

// find_fsdb_score_cut (src/fsdb.c:269-383): host-side IEEE double (built with -ffp-contract=off).
// Bit-exactness argument per pass:
//   1. xbar/ybar: every partial sum is an integer below 2^53, so each double addition is exact and
//      the result does not depend on the order -> accumulate in int64.
//   2. ssxy/ssxx: sums of inexact products, order dependent -> sequential, in fsdb order, exactly as
//      the reference.  If all reads have the same length every (len - xbar) is exactly 0, both sums
//      are exactly 0 and slope_bf = 0/0 = NaN: that case is answered without the pass.
//   3. max slope delta: a maximum is order independent (NaN deltas never win, as in the reference).
extern "C" void mia_hip_score_cut(const int32_t* score, const int32_t* seq_len, const uint8_t* unique_best, int64_t n,
                                  double* slope, double* intercept) {
  int64_t sx = 0, sy = 0, j = 0;
  int32_t lmin = INT32_MAX, lmax = INT32_MIN;
  for (int64_t i = 0; i < n; i++) {
    const bool u = (!unique_best || unique_best[i]) && score[i] >= 2000;
    sx += u ? seq_len[i] : 0;
    sy += u ? score[i] : 0;
    j += u;
    if (u) { lmin = seq_len[i] < lmin ? seq_len[i] : lmin; lmax = seq_len[i] > lmax ? seq_len[i] : lmax; }
  }
  double xbar = (double)sx, ybar = (double)sy;
  xbar /= (double)(size_t)j;
  ybar /= (double)(size_t)j;
  double slope_bf, intercept_bf, max_delta = 0;
  if (j > 0 && lmin == lmax) {
    const double zero = 0.0;
    slope_bf = zero / zero;                      // ssxy / ssxx with both sums exactly 0
    intercept_bf = ybar - slope_bf * xbar;
  } else {
    double ssxy = 0, ssxx = 0;
    auto used = [&](int64_t i) { return (!unique_best || unique_best[i]) && score[i] >= 2000; };
    for (int64_t i = 0; i < n; i++) if (used(i)) {
      ssxy += (seq_len[i] - xbar) * (score[i] - ybar);
      ssxx += (seq_len[i] - xbar) * (seq_len[i] - xbar);
    }
    slope_bf = ssxy / ssxx;
    intercept_bf = ybar - slope_bf * xbar;
    double m4[4] = {0, 0, 0, 0};
    for (int64_t i = 0; i < n; i++) if (used(i)) {
      double d = (score[i] - ((slope_bf * seq_len[i]) + intercept_bf)) / seq_len[i];
      if (d > m4[i & 3]) m4[i & 3] = d;
    }
    for (int k = 0; k < 4; k++) if (m4[k] > max_delta) max_delta = m4[k];
  }
  *intercept = intercept_bf;
  if ((slope_bf - max_delta) > 0) *slope = slope_bf - (max_delta * 2.0);
  else *slope = (double)(slope_bf * (80 / 100.0));
}

extern "C" int mia_hip_score_sums(mia_hip_ctx* ctx, int64_t* sums5) {
  if (!ctx || !sums5) return MIA_HIP_ERR_ARG;
  if (!ctx->aligned) { ctx->err = "realign first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->d_sums && dev_alloc(ctx, ctx->d_sums, 8)) return MIA_HIP_ERR_NOMEM;
  ctx->pre_cull_valid = false;
  hipLaunchKernelGGL(k_score_sums_init, dim3(1), dim3(64), 0, ctx->stream, ctx->d_sums, (const int32_t*)nullptr);
  const int64_t n = ctx->rs.n;
  if (n > 0) {
    int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cus);   // few blocks: five same-address atomics per block
    hipLaunchKernelGGL(k_score_sums, dim3(grid), dim3(256), 0, ctx->stream, ctx->rs, ctx->d_sums, ctx->L, ctx->d_back_slot, ctx->d_front_slot0);
    HIPCHK(hipGetLastError());
  }
  int64_t local7[7];
  int64_t* stage = ctx->h_pin ? reinterpret_cast<int64_t*>(ctx->h_pin + (16 << 10)) : local7;   // pinned: the copy does not block by itself
  HIPCHK(hipMemcpyAsync(stage, ctx->d_sums, 56, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  memcpy(sums5, stage, 40);
  ctx->pre_cull_records = stage[5];
  ctx->pre_cull_links = stage[6];
  ctx->pre_cull_valid = true;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_pre_cull_counts(mia_hip_ctx* ctx, int64_t* n_records, int64_t* n_links) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->pre_cull_valid) { ctx->err = "score_sums (after the last realign) first"; return MIA_HIP_ERR_STATE; }
  if (n_records) *n_records = ctx->pre_cull_records;
  if (n_links) *n_links = ctx->pre_cull_links;
  return MIA_HIP_OK;
}

// HOST helper: what find_fsdb_score_cut returns when every used read has the same length -- both regression sums
// are exactly 0, slope_bf = 0/0 -- from the (possibly all-reduced) sums alone.  Returns 1 if the lengths differ: the
// order-dependent double sums of passes 2 and 3 then need the scores on the host (mia_hip_score_cut).
extern "C" int mia_hip_score_cut_from_sums(const int64_t* sums5, double* slope, double* intercept) {
  const int64_t sx = sums5[0], sy = sums5[1], j = sums5[2];
  if (!(j > 0 && sums5[3] == sums5[4])) return 1;
  double xbar = (double)sx, ybar = (double)sy;
  xbar /= (double)(size_t)j;
  ybar /= (double)(size_t)j;
  const double zero = 0.0;
  const double slope_bf = zero / zero;
  const double intercept_bf = ybar - slope_bf * xbar;
  const double max_delta = 0;
  *intercept = intercept_bf;
  if ((slope_bf - max_delta) > 0) *slope = slope_bf - (max_delta * 2.0);
  else *slope = (double)(slope_bf * (80 / 100.0));
  return 0;
}

extern "C" int mia_hip_num_records(mia_hip_ctx* ctx, int64_t* n_records) {
  if (!ctx || !n_records) return MIA_HIP_ERR_ARG;
  if (!ctx->aligned) { ctx->err = "realign first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->rs.n;
  *n_records = 0;
  if (n == 0) return MIA_HIP_OK;
  const int nb = (int)((n + 4095) / 4096);
  hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(256), 0, ctx->stream, ctx->rs, ctx->L, ctx->d_partial);
  hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, ctx->stream, ctx->d_partial, nb, (int64_t)0, ctx->d_total);
  HIPCHK(hipMemcpyAsync(n_records, ctx->d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

// ---- tally + consensus -------------------------------------------------------------
// The insert-event list: exactly `elems` entries, and the kernels' view of it (tb.events, tb.cap_events: an int32) set with it.
// Every caller decides for itself when the list is too short.
static int ensure_events(mia_hip_ctx* ctx, int64_t elems) {
  const int rc = dev_alloc(ctx, ctx->d_tb_events, elems);
  ctx->tb.events = ctx->d_tb_events;
  ctx->tb.cap_events = (int32_t)std::min<int64_t>(ctx->d_tb_events.cap, INT32_MAX);
  return rc;
}

static int ensure_tally(mia_hip_ctx* ctx) {
  const int Lp = ctx->L + 1;
  // tally[12][Lp], then gaps[Lp] (+ one slot per rank of a sharded run): one memset clears all
  int rc = dev_ensure(ctx, ctx->d_tb_tally, (int64_t)(TALLY_WORDS + 1) * Lp + 256);
  rc |= dev_ensure(ctx, ctx->d_ins_off, Lp);
  rc |= dev_ensure(ctx, ctx->d_calls, Lp);
  if (rc) return MIA_HIP_ERR_NOMEM;
  // every inserted read base is one event; 1/8 of all bases is far beyond any real data, overflow is detected and reported
  if (!ctx->tb.events && ensure_events(ctx, std::min<int64_t>(ctx->rs.n * 32 + 4096, (int64_t)1 << 30))) return MIA_HIP_ERR_NOMEM;
  ctx->tb.tally = ctx->d_tb_tally;
  ctx->tb.Lp = Lp;
  ctx->tb.gaps = ctx->tb.tally + (size_t)TALLY_WORDS * Lp;      // right behind the tally of THIS reference length
  return MIA_HIP_OK;
}

// everything of mia_hip_tally that is queued on the stream; the event count and the error flags are read afterwards
// the binned tally's layout for this reference: buckets of TALLY_BUCKET columns, one workgroup per TALLY_CHUNK reads of a bucket
// the position-specific matrices' tally sorts by strand as well (bucket_of, mia_consensus_kernels.h): twice the buckets
// (reads of more than 128 bases -- configs[4]'s 150 -- take the RALL instance of k_tally_binned: every row through the runs; the vertical
// counters and the end-row runs work on two 64-row plane words.  With the split but neither -- a first attempt -- such reads paid for the
// part-filled workgroups and got nothing for it: 2.18 against round 4's 1.51 ms per 5 M reads of 150 bases.)
static bool tally_rall(const mia_hip_ctx* ctx) { return ctx->max_len > 128 && ctx->max_len <= 256 && ctx->tally_runs && ctx->tally_rall; }
static int tally_split(const mia_hip_ctx* ctx) {
  return (!ctx->tally_linear && ctx->tally_strand_split && (ctx->max_len <= 128 || tally_rall(ctx))) ? 1 : 0;
}
static int tally_nb(const mia_hip_ctx* ctx) { return (ctx->wrap / TALLY_BUCKET + 1) << tally_split(ctx); }
static bool tally_is_binned(const mia_hip_ctx* ctx) {
  const int nb = ctx->wrap / TALLY_BUCKET + 1;
  return ctx->rs.n > 0 && ctx->use_binned_tally && nb <= 4096 && ctx->max_abs <= 32767;   // (the LDS copy of the matrices is int16)
}
// Counting sort of the reads by alignment start (k_bucket_count / _scan / _fill) on stream `on`.  It reads nothing but the
// alignment starts, so mia_hip_iterate queues it on stream2 BESIDE the cull kernels (it also clears the tally buffers:
// nothing adds to them before the tally kernel).  tally_launch waits for ev_join if `on` is not the context's stream.
// reads per workgroup of the binned tally (the linear matrix: one read per lane -- measured, mia_consensus_kernels.h)
static int tally_chunk(const mia_hip_ctx* ctx) { return ctx->tally_linear ? TALLY_CHUNK_LINEAR : TALLY_CHUNK; }
static int bucket_launch(mia_hip_ctx* ctx, hipStream_t on) {
  int rc = ensure_tally(ctx);
  if (rc) return rc;
  const int Lp = ctx->tb.Lp;
  const int64_t tally_words = (int64_t)(TALLY_WORDS + 1) * Lp + 256;                               // tally, gaps, the ranks' event counts
  const int64_t n = ctx->rs.n;
  const int nb = tally_nb(ctx), split = tally_split(ctx);
  const int chunk = tally_chunk(ctx);
  const int grid = (int)(n / chunk) + nb + 1;
  if (4 * (nb + 1) + 4 * grid > ctx->d_bucket.cap) {
    if (dev_alloc(ctx, ctx->d_bucket, (int64_t)(4 * (nb + 1) + 4 * grid) * 2)) return MIA_HIP_ERR_NOMEM;
    ctx->bucket_clean_nb = -1;
  }
  if (!ctx->d_order && dev_alloc(ctx, ctx->d_order, n)) return MIA_HIP_ERR_NOMEM;
  int32_t *d_cnt = ctx->d_bucket, *d_off = d_cnt + (nb + 1), *d_wgoff = d_off + (nb + 1), *d_cur = d_wgoff + (nb + 1), *d_wgb = d_cur + (nb + 1);
  // the bucket counts are left at zero by k_bucket_scan; only a fresh (or differently laid out) buffer is cleared here
  if (ctx->bucket_clean_nb != nb) { HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)(nb + 1) * 4, on)); ctx->bucket_clean_nb = nb; }
  const int gb = (int)((n + 256 * BUCKET_PER - 1) / (256 * BUCKET_PER));
  hipLaunchKernelGGL(k_bucket_count, dim3(gb), dim3(256), (size_t)nb * 4, on, ctx->rs, nb, d_cnt, ctx->tb.tally, tally_words, ctx->abort_if, split);
  hipLaunchKernelGGL(k_bucket_scan, dim3(1), dim3(256), 0, on, d_cnt, nb, d_off, d_wgoff, d_cur, d_wgb, ctx->abort_if, chunk);
  const bool sigb = on != ctx->stream && (ctx->ext_events & 16u);
  if (!split) launch_k(k_bucket_fill, dim3(gb), dim3(256), (size_t)nb * 8, on, sigb ? ctx->ev_join : nullptr, ctx->rs, nb, d_off, d_cur, ctx->d_order, ctx->abort_if, split, (uint8_t*)nullptr, 0);
  else {
    // ... and every bucket by alignment start (k_sort2_count / k_sort2_fill: the tally's runs of equal starts)
    const int64_t words2 = (int64_t)nb * SORT2_KEYS * 2;
    if (dev_ensure(ctx, ctx->d_sort2, words2)) return MIA_HIP_ERR_NOMEM;
    // (each on its own: a failure of the second must not leave the first behind as "both are there" -- ADVICE r05)
    if (!ctx->d_order2 && dev_alloc(ctx, ctx->d_order2, n)) return MIA_HIP_ERR_NOMEM;
    if (!ctx->d_okey && dev_alloc(ctx, ctx->d_okey, n + 64)) return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemsetAsync(ctx->d_sort2, 0, (size_t)words2 * 4, on));
    const int32_t packed = (n < (1 << 24) && !ctx->sort2_unpacked) ? 1 : 0;      // (the key in the entry's top byte, or -- 2^24 reads and more -- in a byte array beside it)
    hipLaunchKernelGGL(k_bucket_fill, dim3(gb), dim3(256), (size_t)nb * 8, on, ctx->rs, nb, (const int32_t*)d_off, d_cur, ctx->d_order, ctx->abort_if, split, ctx->d_okey, packed);
    hipLaunchKernelGGL(k_sort2_count, dim3(grid), dim3(256), 0, on, nb, (const int32_t*)d_wgoff, (const int32_t*)d_wgb, (const int32_t*)ctx->d_order, (const uint8_t*)ctx->d_okey, packed,
                       ctx->d_sort2, ctx->abort_if);
    launch_k(k_sort2_fill, dim3(grid), dim3(256), 0, on, sigb ? ctx->ev_join : nullptr, nb, (const int32_t*)d_off, (const int32_t*)d_wgoff, (const int32_t*)d_wgb,
             (const int32_t*)ctx->d_order, (const uint8_t*)ctx->d_okey, packed, (const int32_t*)ctx->d_sort2, ctx->d_sort2 + (int64_t)nb * SORT2_KEYS, ctx->d_order2, ctx->abort_if);
  }
  HIPCHK(hipGetLastError());
  if (on != ctx->stream && !sigb) HIPCHK(hipEventRecord(ctx->ev_join, on));
  ctx->buckets_queued = on != ctx->stream ? 2 : 1;
  return MIA_HIP_OK;
}

static int tally_launch(mia_hip_ctx* ctx) {
  if (!ctx->aligned) { ctx->err = "realign first"; return MIA_HIP_ERR_STATE; }
  if (!ctx->culled) { ctx->err = "cull first (the dropped bits and record parameters are its output)"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  int rc = ensure_tally(ctx);
  if (rc) return rc;
  const int Lp = ctx->tb.Lp;
  const int64_t tally_words = (int64_t)(TALLY_WORDS + 1) * Lp + 256;                               // tally, gaps, the ranks' event counts
  if (!ctx->in_iterate) HIPCHK(hipMemsetAsync(ctx->tb.n_events, 0, 8, ctx->stream));              // event count, flags (neighbours in the control block)
  const int64_t n = ctx->rs.n;
  const bool binned = tally_is_binned(ctx);
  if (!binned) HIPCHK(hipMemsetAsync(ctx->tb.tally, 0, (size_t)tally_words * 4, ctx->stream));     // (the binned path clears it inside k_bucket_count)
  if (n > 0) {
    RefInfo ref{ctx->d_ref, ctx->L, ctx->wrap};
    const int nb = tally_nb(ctx), split = tally_split(ctx);
    if (binned) {
      // counting sort of the reads by alignment start, then one LDS tally window per workgroup
      if (!ctx->buckets_queued) { if (int rcb = bucket_launch(ctx, ctx->stream)) return rcb; }
      if (ctx->buckets_queued == 2) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
      ctx->buckets_queued = 0;
      const int chunk = tally_chunk(ctx);
      const int grid = (int)(n / chunk) + nb + 1;
      int32_t *d_cnt = ctx->d_bucket, *d_off = d_cnt + (nb + 1), *d_wgoff = d_off + (nb + 1), *d_cur = d_wgoff + (nb + 1), *d_wgb = d_cur + (nb + 1);
      const int64_t slab_words = (int64_t)grid * (TALLY_WORDS - 1) * TALLY_WIN;
      if (dev_ensure(ctx, ctx->d_tally_slabs, slab_words)) return MIA_HIP_ERR_NOMEM;
      // (the bit planes and the N marks of the context's own reads: k_read_planes / k_bx_umax at upload)
      const bool planes_ok = ctx->umax_valid && ctx->rs.roff == ctx->d_roff && ctx->d_rplanes && ctx->d_umax;
      const bool defer = ctx->tally_defer;
      if (defer && dev_ensure(ctx, ctx->d_gen_list, n)) return MIA_HIP_ERR_NOMEM;
      int32_t* n_gen = ctx->d_genn;
      if (defer && !ctx->in_iterate) HIPCHK(hipMemsetAsync(n_gen, 0, 4, ctx->stream));     // (mia_hip_iterate clears the whole control block)
#define MIA_TALLY_ARGS(PL, RW, UM, BIAS)                                                                                                              \
  dim3(grid), dim3(256), 0, ctx->stream, ctx->rs, ref, ctx->d_pssm, ctx->d_drop_f, ctx->d_drop_b, ctx->tb, nb, d_off, d_wgoff, split ? ctx->d_order2 : ctx->d_order, ctx->ri.trec, \
      ctx->ri.actf, ctx->d_tally_slabs, ctx->dbg, PL, RW, UM, d_wgb, BIAS, ctx->abort_if, chunk, defer ? ctx->d_gen_list : (int32_t*)nullptr, n_gen, split | ((split && ctx->tally_runs) ? 2 : 0)
      const uint64_t* pl_arg = planes_ok ? ctx->d_rplanes : nullptr;
      const int32_t* um_arg = planes_ok ? ctx->d_umax : nullptr;
      int rct;
      if (ctx->tally_linear)
        rct = defer ? stage_launch(ctx, STG_TALLY, k_tally_binned<true, true>, MIA_TALLY_ARGS(pl_arg, ctx->rplane_words, um_arg, -1))
                    : stage_launch(ctx, STG_TALLY, k_tally_binned<true, false>, MIA_TALLY_ARGS(pl_arg, ctx->rplane_words, um_arg, -1));
      else if (split && tally_rall(ctx))
        rct = defer ? stage_launch(ctx, STG_TALLY, k_tally_binned<false, true, true>, MIA_TALLY_ARGS(pl_arg, ctx->rplane_words, um_arg, ctx->tally_pk_bias))
                    : stage_launch(ctx, STG_TALLY, k_tally_binned<false, false, true>, MIA_TALLY_ARGS(pl_arg, ctx->rplane_words, um_arg, ctx->tally_pk_bias));
      else
        rct = defer ? stage_launch(ctx, STG_TALLY, k_tally_binned<false, true>, MIA_TALLY_ARGS(split ? pl_arg : nullptr, ctx->rplane_words, split ? um_arg : nullptr, ctx->tally_pk_bias))
                    : stage_launch(ctx, STG_TALLY, k_tally_binned<false, false>, MIA_TALLY_ARGS(split ? pl_arg : nullptr, ctx->rplane_words, split ? um_arg : nullptr, ctx->tally_pk_bias));
#undef MIA_TALLY_ARGS
      if (rct) return MIA_HIP_ERR_NOMEM;
      GenReads gen{ctx->rs, ref, ctx->d_pssm, ctx->d_drop_f, ctx->d_drop_b, ctx->ri.trec, ctx->ri.actf, defer ? ctx->d_gen_list : nullptr, n_gen};
      hipLaunchKernelGGL(k_tally_reduce, dim3((Lp + 255) / 256 + (defer ? TALLY_GEN_BLOCKS : 0), TALLY_WORDS - 1, TALLY_REDUCE_SHARES), dim3(256), 0, ctx->stream, ctx->tb, nb, d_wgoff,
                         ctx->d_tally_slabs, ctx->abort_if, gen, split);
    } else {
      hipLaunchKernelGGL(k_tally, dim3((int)((n + 3) / 4)), dim3(256), 0, ctx->stream, ctx->rs, ref, ctx->d_pssm, ctx->d_drop_f,
                         ctx->d_drop_b, ctx->tb, ctx->ri.trec, ctx->ri.actf);
    }
    HIPCHK(hipGetLastError());
  }
  return MIA_HIP_OK;
}

// what the tally kernels left in their counters (event count, overflow and geometry flags, the cull's flags)
static int tally_finish(mia_hip_ctx* ctx, uint32_t n_events, uint32_t flags, uint32_t cflags) {
  ctx->n_events_host = (int32_t)n_events;
  if (int rcf = check_cull_flags(ctx, cflags)) return rcf;
  if (flags & 1u) { ctx->err = "insert event list overflow"; return MIA_HIP_ERR_NOMEM; }
  if (ctx->n_events_host > ctx->tb.cap_events) ctx->n_events_host = ctx->tb.cap_events;
  ctx->tallied = true;
  ctx->consensus_done = false;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_tally(mia_hip_ctx* ctx) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (int rc = tally_launch(ctx)) return rc;
  uint32_t local3[3] = {0, 0, 0};
  uint32_t* h3 = ctx->h_pin ? reinterpret_cast<uint32_t*>(ctx->h_pin + (17 << 10)) : local3;   // pinned: three copies, one wait
  HIPCHK(hipMemcpyAsync(&h3[0], ctx->tb.n_events, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(&h3[1], ctx->tb.flags, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(&h3[2], ctx->d_cull_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return tally_finish(ctx, h3[0], h3[1], h3[2]);
}

extern "C" int mia_hip_tally_buffers(mia_hip_ctx* ctx, int32_t** d_tally, int64_t* n_tally_words, int32_t** d_gaps,
                                     int64_t* n_gaps_words) {
  if (!ctx || !ctx->tallied) return MIA_HIP_ERR_STATE;
  if (d_tally) *d_tally = ctx->tb.tally;
  if (n_tally_words) *n_tally_words = (int64_t)TALLY_WORDS * ctx->tb.Lp;
  if (d_gaps) *d_gaps = ctx->tb.gaps;
  if (n_gaps_words) *n_gaps_words = ctx->tb.Lp;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_ins_events(mia_hip_ctx* ctx, uint64_t** d_events, int64_t* n_events) {
  if (!ctx || !ctx->tallied) return MIA_HIP_ERR_STATE;
  if (d_events) *d_events = ctx->tb.events;
  if (n_events) *n_events = ctx->n_events_host;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_set_ins_events(mia_hip_ctx* ctx, const uint64_t* d_events, int64_t n_events) {
  if (!ctx || !ctx->tallied || n_events < 0) return MIA_HIP_ERR_STATE;
  HIPCHK(hipSetDevice(ctx->device));
  if (n_events > ctx->tb.cap_events && ensure_events(ctx, n_events)) return MIA_HIP_ERR_NOMEM;
  if (n_events > 0 && d_events != ctx->tb.events)
    HIPCHK(hipMemcpyAsync(ctx->tb.events, d_events, (size_t)n_events * 8, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->n_events_host = (int32_t)n_events;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_tally(mia_hip_ctx* ctx, int32_t* tally, int32_t* gaps) {
  if (!ctx || !ctx->tallied) return MIA_HIP_ERR_STATE;
  HIPCHK(hipSetDevice(ctx->device));
  const int Lp = ctx->tb.Lp;
  if (tally) HIPCHK(hipMemcpyAsync(tally, ctx->tb.tally, (size_t)TALLY_WORDS * Lp * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (gaps) HIPCHK(hipMemcpyAsync(gaps, ctx->tb.gaps, (size_t)Lp * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

extern "C" int mia_hip_set_tally(mia_hip_ctx* ctx, int32_t ref_len, const int32_t* tally, const int32_t* gaps) {
  if (!ctx || ref_len <= 0 || !tally) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (ref_len != ctx->L) {
    // tallies of another reference than the one the reads were aligned to: the alignment state (windows, wrap, cull marks)
    // no longer belongs to them -- whatever needs it must realign first
    ctx->aligned = false; ctx->culled = false; ctx->have_ref = false; ctx->links_applied = false;
  }
  ctx->L = ref_len;
  int rc = ensure_tally(ctx);
  if (rc) return rc;
  const int Lp = ctx->tb.Lp;
  HIPCHK(hipMemcpyAsync(ctx->tb.tally, tally, (size_t)TALLY_WORDS * Lp * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->tb.gaps, 0, ((size_t)Lp + 256) * 4, ctx->stream));      // gaps and the ranks' event-count slots behind them
  if (gaps) HIPCHK(hipMemcpyAsync(ctx->tb.gaps, gaps, (size_t)Lp * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->tb.n_events, 0, 4, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->n_events_host = 0;
  ctx->tallied = true;
  ctx->consensus_done = false;
  return MIA_HIP_OK;
}

// the kernels of mia_hip_consensus: column calls, then the insert columns tallied and called into buffers of `cap` slots.
// events_on_device: the insert-event count is read by k_ins_tally itself (mia_hip_iterate has not seen it yet)
static int consensus_launch(mia_hip_ctx* ctx, int cons_code, int64_t cap, bool columns, bool events_on_device) {
  const int L = ctx->L, Lp = ctx->tb.Lp;
  if (columns) {
    hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t*)ctx->tb.gaps, Lp, 1, L, ctx->d_ins_off, ctx->d_ins_total);   // ins_off[p] = gaps[1] + .. + gaps[p-1]
    hipLaunchKernelGGL(k_call_columns, dim3((L + 255) / 256), dim3(256), 0, ctx->stream, ctx->tb.tally, Lp, L, cons_code, ctx->d_calls);
  }
  if (cap <= 0) return MIA_HIP_OK;
  HIPCHK(hipMemsetAsync(ctx->d_ins_tally, 0, (size_t)ins_words(cap) * 4, ctx->stream));
  const int ne = ctx->n_events_host;
  if (events_on_device)
    hipLaunchKernelGGL(k_ins_tally, dim3(256), dim3(256), 0, ctx->stream, ctx->tb.events, 0, ctx->d_pssm, ctx->d_ins_off, ctx->tb.gaps, L, ctx->d_ins_tally,
                       (int32_t)cap, (const int32_t*)ctx->tb.n_events, ctx->tb.cap_events);
  else if (ne > 0)
    hipLaunchKernelGGL(k_ins_tally, dim3((ne + 255) / 256), dim3(256), 0, ctx->stream, ctx->tb.events, ne, ctx->d_pssm, ctx->d_ins_off,
                       ctx->tb.gaps, L, ctx->d_ins_tally, (int32_t)cap, (const int32_t*)nullptr, 0);
  hipLaunchKernelGGL(k_call_inserts, dim3((L + 255) / 256), dim3(256), 0, ctx->stream, ctx->tb.tally, Lp, L, ctx->tb.gaps,
                     ctx->d_ins_off, ctx->d_ins_tally, cons_code, ctx->d_ins_calls, (int32_t)cap);
  return MIA_HIP_OK;
}

extern "C" int mia_hip_consensus(mia_hip_ctx* ctx, int cons_code, char* out, int64_t out_cap, int64_t* out_len) {
  if (!ctx || !out) return MIA_HIP_ERR_ARG;
  if (!ctx->tallied) { ctx->err = "tally first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  const int L = ctx->L, Lp = ctx->tb.Lp;
  // The insert columns are tallied and called into buffers of the capacity the last call left behind, and their total
  // comes back with the results: one wait for the stream instead of two.  Only when the total has outgrown the buffers
  // are they enlarged and the insert part run again.
  auto insert_part = [&](int64_t cap) -> int { return consensus_launch(ctx, cons_code, cap, false, false); };
  if (int rcc = consensus_launch(ctx, cons_code, 0, true, false)) return rcc;
  int rc0 = insert_part(ctx->ins_tally_cap);
  if (rc0) return rc0;
  HIPCHK(hipGetLastError());
  // results through the pinned staging area when they fit (copies into pageable memory make the host wait one by one)
  const size_t need = 16 + (size_t)L + 2 * (size_t)Lp * 4 + (size_t)ctx->ins_tally_cap + 64;
  std::vector<unsigned char> pageable;
  unsigned char* base;
  if (ctx->h_pin && need <= mia_hip_ctx::PIN_BYTES - mia_hip_ctx::PIN_MISC) base = ctx->h_pin + mia_hip_ctx::PIN_MISC;
  else { pageable.resize(need); base = pageable.data(); }
  int32_t* h_total = reinterpret_cast<int32_t*>(base);
  int32_t* gaps = reinterpret_cast<int32_t*>(base + 16);
  int32_t* off = gaps + Lp;
  char* calls = reinterpret_cast<char*>(off + Lp);
  char* ins = calls + L;
  HIPCHK(hipMemcpyAsync(h_total, ctx->d_ins_total, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(calls, ctx->d_calls, (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(gaps, ctx->tb.gaps, (size_t)Lp * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(off, ctx->d_ins_off, (size_t)Lp * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (ctx->ins_tally_cap > 0) HIPCHK(hipMemcpyAsync(ins, ctx->d_ins_calls, (size_t)ctx->ins_tally_cap, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int32_t total = *h_total;
  std::vector<char> ins_big;
  if (total > ctx->ins_tally_cap) {
    const int64_t cap = (int64_t)total + total / 4 + 1024;
    ctx->ins_tally_cap = 0;
    if (dev_alloc(ctx, ctx->d_ins_tally, ins_words(cap)) || dev_alloc(ctx, ctx->d_ins_calls, cap)) return MIA_HIP_ERR_NOMEM;
    ctx->ins_tally_cap = cap;
    rc0 = insert_part(cap);
    if (rc0) return rc0;
    HIPCHK(hipGetLastError());
    ins_big.resize((size_t)total + 1);
    HIPCHK(hipMemcpyAsync(ins_big.data(), ctx->d_ins_calls, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ins = ins_big.data();
  }
  // string assembly of consensus_assembly_string (src/mia.c:551-600): insert calls, then the column call; '-' is skipped
  int64_t o = 0;
  for (int p = 0; p < L; p++) {
    if (p > 0)
      for (int j = 0; j < gaps[p]; j++) {
        char c = ins[off[p] + j];
        if (c != '-' && c != ' ') { if (o + 1 >= out_cap) { ctx->err = "consensus buffer too small"; return MIA_HIP_ERR_ARG; } out[o++] = c; }
      }
    char c = calls[p];
    if (c != '-' && c != ' ') { if (o + 1 >= out_cap) { ctx->err = "consensus buffer too small"; return MIA_HIP_ERR_ARG; } out[o++] = c; }
  }
  out[o] = 0;
  if (out_len) *out_len = o;
  ctx->consensus_done = true;
  ctx->ins_total_host = total;
  return MIA_HIP_OK;
}

// (the communicator entry points and mia_hip_iterate: mia_hip_iterate.inc; trimming, ma, pass 1, Myers, ceilings: mia_hip_tools.inc)
#include "mia_hip_iterate.inc"
#include "mia_hip_tools.inc"
