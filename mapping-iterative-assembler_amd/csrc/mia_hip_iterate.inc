// mia_hip_iterate.inc -- part of mia_hip.hip (one translation unit): the communicator entry points (RCCL / loopback / a table
// of the host program's own) and mia_hip_iterate, the loop body of /root/reference/src/mia_main.c:931-963 as one call --
// alignment, score cut, cull, tally, the exchanges of a sharded run, consensus (DESIGN.md 3.5, 5; HISTORY.md 3.11).

// ---- several GPUs (SURVEY 8e: reads shard, tallies all-reduce) ------------------------------------------
// The exchanges of a sharded iteration go through ctx->coll, a table of two collectives (include/mia_hip.h); the
// transports themselves -- RCCL over xGMI, the in-process loopback -- live in mia_comm.hip.
constexpr int PRE_WORDS = 8;         // per rank before the cull: five score sums, AlnSeq records, links, reads waiting for the exact kernel
#define COLLCHK(call)                                                                                  \
  do {                                                                                                 \
    const int r_ = (call);                                                                             \
    if (r_ != MIA_HIP_OK) {                                                                            \
      const char* t_ = ctx->coll.error ? ctx->coll.error(ctx->coll.user) : nullptr;                    \
      ctx->err = std::string(#call) + ": " + (t_ && *t_ ? t_ : "collective failed");                   \
      return r_;                                                                                       \
    }                                                                                                  \
  } while (0)

static int comm_attach_table(mia_hip_ctx* ctx, const mia_hip_collectives& t) {
  if (dev_alloc(ctx, ctx->d_gather, (int64_t)PRE_WORDS * t.n_ranks)) return MIA_HIP_ERR_NOMEM;
  ctx->coll = t;
  ctx->coll_name = t.name ? t.name : "";                  // (the table is copied, its name included: the caller's string may go away)
  ctx->coll.name = t.name ? ctx->coll_name.c_str() : nullptr;
  ctx->comm = true; ctx->comm_ranks = t.n_ranks; ctx->comm_rank = t.rank;
  ctx->h_gather.assign((size_t)PRE_WORDS * t.n_ranks, 0);
  ctx->ev_pad = 0;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_comm_init(mia_hip_ctx* ctx, const void* id128, int32_t n_ranks, int32_t rank) {
  if (!ctx || !id128 || n_ranks < 1 || n_ranks > 256 || rank < 0 || rank >= n_ranks) return MIA_HIP_ERR_ARG;
  if (ctx->comm) { ctx->err = "this context already has a communicator"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  mia_hip_collectives t;
  if (int rc = mia_comm_rccl_table(id128, n_ranks, rank, &t, &ctx->err)) return rc;
  if (int rc = comm_attach_table(ctx, t)) { if (t.destroy) t.destroy(t.user); return rc; }     // (no half-made communicator stays behind)
  return MIA_HIP_OK;
}

extern "C" int mia_hip_comm_attach(mia_hip_ctx* ctx, const mia_hip_collectives* table) {
  if (!ctx || !table || !table->all_gather || !table->all_reduce_i32 || table->n_ranks < 1 || table->n_ranks > 256 || table->rank < 0 ||
      table->rank >= table->n_ranks)
    return MIA_HIP_ERR_ARG;
  if (ctx->comm) { ctx->err = "this context already has a communicator"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  return comm_attach_table(ctx, *table);
}

extern "C" int mia_hip_comm_info(mia_hip_ctx* ctx, int32_t* n_ranks, int32_t* rank, const char** transport) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  int32_t nr = 1, rk = 0;
  if (ctx->comm) {
    nr = ctx->comm_ranks; rk = ctx->comm_rank;
    if (ctx->coll.query) { if (int rc = ctx->coll.query(ctx->coll.user, &nr, &rk)) { ctx->err = "the transport could not say how many ranks it has"; return rc; } }
  }
  if (n_ranks) *n_ranks = nr;
  if (rank) *rank = rk;
  if (transport) *transport = ctx->comm ? (ctx->coll.name ? ctx->coll.name : "caller") : "none";
  return MIA_HIP_OK;
}

extern "C" int mia_hip_comm_destroy(mia_hip_ctx* ctx) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->comm) return MIA_HIP_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->coll.destroy) ctx->coll.destroy(ctx->coll.user);
  ctx->coll = mia_hip_collectives{};
  ctx->comm = false; ctx->comm_ranks = 1; ctx->comm_rank = 0;
  return MIA_HIP_OK;
}

// all-gather of ragged 8-byte records (links: 4 words each; insert events: 1): every rank contributes counts[rank] * words
// words from `mine`; the concatenation in rank order lands in ctx->d_lall.  counts are known on every rank.
static int comm_gather_ragged(mia_hip_ctx* ctx, const int64_t* mine, const std::vector<int64_t>& counts, int words, int64_t* total_out) {
  const int W = ctx->comm_ranks;
  int64_t mx = 0, total = 0;
  for (int r = 0; r < W; r++) { mx = std::max(mx, counts[(size_t)r]); total += counts[(size_t)r]; }
  *total_out = total;
  if (total == 0) return MIA_HIP_OK;
  const int64_t pad = mx * words;
  if (dev_ensure(ctx, ctx->d_lmine, pad, pad * 2) || dev_ensure(ctx, ctx->d_lstage, pad * W, pad * W * 2) || dev_ensure(ctx, ctx->d_lall, total * words, total * words * 2))
    return MIA_HIP_ERR_NOMEM;
  HIPCHK(hipMemsetAsync(ctx->d_lmine, 0, (size_t)pad * 8, ctx->stream));
  const int64_t nm = counts[(size_t)ctx->comm_rank] * words;
  if (nm > 0) HIPCHK(hipMemcpyAsync(ctx->d_lmine, mine, (size_t)nm * 8, hipMemcpyDeviceToDevice, ctx->stream));
  COLLCHK(ctx->coll.all_gather(ctx->coll.user, ctx->d_lmine, ctx->d_lstage, (size_t)pad * 8, ctx->stream));
  int64_t o = 0;
  for (int r = 0; r < W; r++) {
    const int64_t c = counts[(size_t)r] * words;
    if (c > 0) HIPCHK(hipMemcpyAsync(ctx->d_lall + o, ctx->d_lstage + (int64_t)r * pad, (size_t)c * 8, hipMemcpyDeviceToDevice, ctx->stream));
    o += c;
  }
  return MIA_HIP_OK;
}

// What the cull needs from the other ranks -- their score sums (find_fsdb_score_cut's first pass), how many AlnSeq records
// precede this rank's, how many links each cull will emit, and whether some rank still has reads for the exact kernel --
// in ONE small all-gather, queued BEHIND the alignment kernels and in front of the alignment's one host wait: a sharded
// iteration waits for the host as often as a single context does.
static int comm_pre_cull_enqueue(mia_hip_ctx* ctx, const int32_t* d_wide_count) {
  const int64_t n = ctx->rs.n;
  const int W = ctx->comm_ranks;
  if (!ctx->d_sums && dev_alloc(ctx, ctx->d_sums, 8)) return MIA_HIP_ERR_NOMEM;
  hipLaunchKernelGGL(k_score_sums_init, dim3(1), dim3(64), 0, ctx->stream, ctx->d_sums, d_wide_count);
  const int grid = (int)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cus);
  hipLaunchKernelGGL(k_score_sums, dim3(grid), dim3(256), 0, ctx->stream, ctx->rs, ctx->d_sums, ctx->L, ctx->d_back_slot, ctx->d_front_slot0);
  HIPCHK(hipGetLastError());
  COLLCHK(ctx->coll.all_gather(ctx->coll.user, ctx->d_sums, ctx->d_gather, (size_t)PRE_WORDS * 8, ctx->stream));
  int64_t* stage = ctx->h_pin ? reinterpret_cast<int64_t*>(ctx->h_pin + (40 << 10)) : ctx->h_gather.data();
  HIPCHK(hipMemcpyAsync(stage, ctx->d_gather, (size_t)PRE_WORDS * W * 8, hipMemcpyDeviceToHost, ctx->stream));
  return MIA_HIP_OK;
}
// ... and once the stream has been waited for
static bool comm_pre_cull_collect(mia_hip_ctx* ctx) {
  const int W = ctx->comm_ranks;
  if (ctx->h_pin) memcpy(ctx->h_gather.data(), ctx->h_pin + (40 << 10), (size_t)PRE_WORDS * W * 8);
  bool any_wide = false;
  for (int r = 0; r < W; r++) any_wide = any_wide || ctx->h_gather[(size_t)PRE_WORDS * r + 7] != 0;
  return any_wide;
}

// What a rank puts behind ref->gaps before the max-reduce: its insert-event count in slot `rank` of W, and in the three slots behind
// those "my event list overflowed", "my cull met a link it cannot reproduce", "my link list overflowed" (tally flag 1, cull flags 4, 8)
constexpr int COMM_FLAG_SLOTS = 3;
__global__ void k_or_u32(uint32_t* dst, uint32_t bits) { if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(dst, bits); }
__global__ void k_put_rank_words(int32_t* slots, int32_t rank, int32_t W, const int32_t* n_events, int32_t clamp, const uint32_t* tally_flags, const uint32_t* cull_flags) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  slots[rank] = min(*n_events, clamp);
  const uint32_t tf = tally_flags ? *tally_flags : 0u, cf = cull_flags ? *cull_flags : 0u;
  slots[W] = (tf & 1u) ? 1 : 0;
  slots[W + 1] = (cf & 4u) ? 1 : 0;
  slots[W + 2] = (cf & 8u) ? 1 : 0;
}

// The insert events of all ranks, gathered in blocks of `pad` (stage[r * pad + i], i < counts[r]), packed into one list in
// rank order; *n_out = their number.  counts[] are the W slots behind ref->gaps that rode on its max-reduce.  If some rank
// had more than `pad` events nothing is touched and bit 8 of the tally flags says so (the host repeats the exchange with
// the counts in hand).  One workgroup per rank in y.
__global__ __launch_bounds__(256) void k_events_compact(const uint64_t* __restrict__ stage, int64_t pad, const int32_t* __restrict__ counts, int W,
                                                          uint64_t* __restrict__ out, int32_t cap, int32_t* n_out, uint32_t* flags) {
  const int r = blockIdx.y;
  int64_t before = 0, total = 0;
  bool over = false;
  for (int k = 0; k < W; k++) {
    const int64_t c = counts[k];
    over = over || c > pad;
    if (k < r) before += c;
    total += c;
  }
  over = over || total > cap;
  if (over) { if (r == 0 && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(flags, 8u); return; }
  const int64_t mine = counts[r];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < mine; i += (int64_t)gridDim.x * 256) out[before + i] = stage[(int64_t)r * pad + i];
  if (r == 0 && blockIdx.x == 0 && threadIdx.x == 0) *n_out = (int32_t)total;
}

// ---- reference ahead (ref_ahead.h, DESIGN.md 3.5) -------------------------------------------------------------------------
// characters of the string that are no base, and the entries their spellings add to the 10-mer table of the wrapped string
// (kh_wild_entries, without making the codes)
static void ref_count_other(const char* ref, int L, int wrap, int64_t* n_other_out, int64_t* kh_entries_out) {
  // (base_code: only upper-case ACGT are bases.  Four compares per character, no table: the loop is one the compiler turns into
  // vector instructions -- the shadow launch waits for this count, with the device idle)
  uint32_t cnt = 0;
  for (int i = 0; i < L; i++) { const char c = ref[i]; cnt += (uint32_t)((c != 'A') & (c != 'C') & (c != 'G') & (c != 'T')); }
  int64_t n_other = cnt, e = 0;
  if (n_other) {
    int k = 0;
    auto other = [&](int j) { return base_code(ref[j < L ? j : j - L]) > 3 ? 1 : 0; };
    for (int pq = 0; pq < wrap; pq++) {
      k += other(pq);
      if (pq >= DF_K) k -= other(pq - DF_K);
      if (pq >= DF_K - 1 && k <= BX_WILD) e += (int64_t)1 << (2 * k);
    }
    if (e > ((int64_t)1 << 24)) e = 0;
  }
  *n_other_out = n_other; *kh_entries_out = e;
}

// What k_ref_prep's arguments would be for a call of mia_hip_iterate on a reference of L characters with these counts -- by the
// functions such a call uses itself (align_route, align_ensure_buffers) -- and whether the call would take the band pipeline,
// the only route whose tables are prepared ahead.  Asked twice: behind a consensus (the shadow launch's key) and at the top of the
// next call (the key it wants).
static bool ref_ahead_want(const mia_hip_ctx* ctx, int L, int circular, int64_t n_other, int64_t kh_entries, RefAheadKey* key) {
  const int wl = circular ? (L < MAX_READ ? L : MAX_READ) : 0, wrap = L + wl;
  AlignRouteIn in = align_route_in(ctx);
  in.L = L; in.wrap = wrap; in.plane_words = plane_words((int64_t)wrap + 64); in.kh_entries = kh_entries;
  in.ref_mostly_bases = n_other * 50 <= L; in.ref_few_n = n_other * 500 <= L;
  in.explicit_win = false; in.deferred = true; in.pend_encode = true; in.ref_ready = false;
  const AlignRoute r = align_route(in);
  key->L = L; key->circular = circular ? 1 : 0; key->n_other = n_other; key->kh_entries = kh_entries;
  key->kslots = kh_slots_for_entries(wrap, kh_entries); key->kwild = kh_entries > 0 ? BX_WILD : 0;
  key->plane_words = r.plane_words; key->nib_words = bx_nib_words((int64_t)wrap + 64); key->bits = r.want_bits;
  return r.bx && r.fused_prep;
}

// THE SHADOW LAUNCH: k_ref_prep for the consensus a call returns, into the second set of buffers and the idle half of the control
// block.  Nothing the call returns depends on it: whatever goes wrong here leaves no shadow behind, and the next call prepares its
// reference as it always did.
//   WHEN.  Behind the step's wait the host has the string and could derive every argument from it -- but the device then idles while
//   the host notices the end, counts and launches (measured: a step as long as without the shadow launch, and a caller that waits
//   for the context behind the call pays for the launch in full).  So the launch is SPECULATIVE and nothing else: queued right
//   behind k_cons_scatter, with the key this call's own reference has (ref_ahead_speculate) -- at steady state the consensus is as
//   long as its reference and holds no N either -- and the host waits for k_cons_scatter's own event, not for the stream.  Behind the
//   wait the key is made from the string as returned (ref_ahead_settle): equal keys -- the launch that is already running read the
//   right string with the right arguments, and the next call may adopt it; else it is dropped and the next call is a miss.
//   A speculative launch reads key.L characters of the result block, which holds at least this call's L: in bounds whatever the
//   consensus turns out to be.  It is only made with kwild = 0: no 10-mer is spelled out then, the table (four slots per column) cannot
//   fill up whatever the characters are, and the insert's probe loop ends.
static bool ref_ahead_allowed(const mia_hip_ctx* ctx) {
  return !ctx->no_ref_ahead && !ctx->no_prep_fuse && ctx->h_pin && ctx->last_route_bx && ctx->rs.n > 0;
}
// src: the string, for the device -- the pinned result block (with zero_copy k_cons_scatter writes no device copy)
static bool ref_ahead_queue(mia_hip_ctx* ctx, const RefAheadKey& key, const char* src) {
  mia_hip_ctx::RefAhead& ah = ctx->ahead;
  const int L = key.L, wl = key.circular ? (L < MAX_READ ? L : MAX_READ) : 0, total = L + wl + 64;
  // the twins grow as their originals do (iterate_body, align_ensure_buffers)
  if (dev_ensure(ctx, ah.d_ref, total, (int64_t)total * 2) || dev_ensure(ctx, ah.d_planes, key.plane_words * 3) ||
      dev_ensure(ctx, ah.d_refnib, key.nib_words, key.nib_words * 2) || dev_ensure(ctx, ah.d_khash, (int64_t)key.kslots * 4) ||
      dev_ensure(ctx, ah.d_khash_ovf, (int64_t)key.kslots * 2) || (key.bits && !ah.d_kbits && dev_alloc(ctx, ah.d_kbits, KB_WORDS)))
    return false;
  const RefPrepSet twin{ah.d_ref, ctx->d_ctrl + (size_t)(1 - ctx->ctrl_half) * CTRL_WORDS, ah.d_khash, ah.d_khash_ovf, ah.d_planes, ah.d_planes.cap / 3,
                        ah.d_refnib, key.bits ? ah.d_kbits.p : nullptr};
  if (launch_ref_prep(ctx, twin, src, L, wl, total, key.kslots, key.kwild, key.plane_words, key.nib_words)) return false;
  ah.key = key;
  return true;
}
static void ref_ahead_speculate(mia_hip_ctx* ctx, const RefAheadKey& key, const char* src) {
  ctx->ahead.valid = false;
  ctx->ahead.queued = key.kwild == 0 && ref_ahead_queue(ctx, key, src);
}
// h_str: the string in the pinned result block, len characters
static void ref_ahead_settle(mia_hip_ctx* ctx, const char* h_str, int64_t len, int circular) {
  mia_hip_ctx::RefAhead& ah = ctx->ahead;
  const bool queued = ah.queued;
  ah.valid = false; ah.queued = false;
  if (!queued || !ref_ahead_allowed(ctx) || len <= 0 || len > (1 << 22)) return;
  const int L = (int)len, wl = circular ? (L < MAX_READ ? L : MAX_READ) : 0, wrap = L + wl;
  int64_t n_other = 0, kh_entries = 0;
  ref_count_other(h_str, L, wrap, &n_other, &kh_entries);            // (counted here instead of at the top of the call that adopts this)
  RefAheadKey key;
  if (!ref_ahead_want(ctx, L, circular, n_other, kh_entries, &key) || !ref_ahead_same_key(ah.key, key)) return;
  ah.str.assign(h_str, (size_t)L);
  ah.valid = true;
}

// ADOPTION (a hit, ref_ahead_hit): the second set becomes the context's, the half of the control block that was cleared with it the
// current one.  Only ever from iterate_body, never while an AlignBorrow lends d_ref.p out (mia_hip_tools.inc).
static void ref_ahead_adopt(mia_hip_ctx* ctx) {
  mia_hip_ctx::RefAhead& ah = ctx->ahead;
  std::swap(ctx->d_ref, ah.d_ref); std::swap(ctx->d_planes, ah.d_planes); std::swap(ctx->d_refnib, ah.d_refnib);
  std::swap(ctx->d_khash, ah.d_khash); std::swap(ctx->d_khash_ovf, ah.d_khash_ovf);
  if (ah.key.bits) std::swap(ctx->d_kbits, ah.d_kbits);
  ctrl_bind(ctx, 1 - ctx->ctrl_half);
}

// ---- one whole iteration -------------------------------------------------------------------------
// reiterate_assembly + pop_smp_from_FSDB + cull_maln_from_fsdb + consensus_assembly_string (src/mia_main.c:931-963) as
// one call: the same kernels as mia_hip_realign / _cull / _tally / _consensus, but what those entry points hand back to
// the host between the kernels -- the planner's bin sizes, the cut line, the insert-event count, five result arrays --
// stays on the device.  The host waits twice: once behind the alignment (reads that need the exact scalar kernel must be
// known before anything is culled) and once for the consensus string -- with or without a communicator.
static int iterate_body(mia_hip_ctx* ctx, const char* new_ref, int32_t ref_len, int circular, int32_t hard_cut, const double* slope_intercept,
                        int cons_code, char* out, int64_t out_cap, int64_t* out_len);

extern "C" int mia_hip_iterate(mia_hip_ctx* ctx, const char* new_ref, int32_t ref_len, int circular, int32_t hard_cut, const double* slope_intercept,
                               int cons_code, char* out, int64_t out_cap, int64_t* out_len) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  int rc;
  if (!new_ref || ref_len <= 0 || !out || out_cap < 1) { ctx->err = "iterate: bad argument"; rc = MIA_HIP_ERR_ARG; }
  else if (!ctx->have_pssm || !ctx->d_packed) { ctx->err = "set_pssm and upload_reads must precede iterate"; rc = MIA_HIP_ERR_STATE; }
  else rc = iterate_body(ctx, new_ref, ref_len, circular, hard_cut, slope_intercept, cons_code, out, out_cap, out_len);
  ctx->in_iterate = false; ctx->deferred = false; ctx->ref_ready = false;
  // a rank that fails here will not come to the collectives the others are about to enter: tell the transport, so that
  // they return an error as well instead of waiting for ever
  if (rc != MIA_HIP_OK && ctx->comm && ctx->coll.abort) ctx->coll.abort(ctx->coll.user);
  return rc;
}

static int iterate_body(mia_hip_ctx* ctx, const char* new_ref, int32_t ref_len, int circular, int32_t hard_cut, const double* slope_intercept,
                        int cons_code, char* out, int64_t out_cap, int64_t* out_len) {
  HIPCHK(hipSetDevice(ctx->device));
  // -- the new reference: ASCII up, codes and wrap made on the device (make_ref_upper / add_ref_wrap, src/mia.c:642-689)
  const int L = ref_len, wl = circular ? (L < MAX_READ ? L : MAX_READ) : 0, wrap = L + wl, total = wrap + 64;
  // REFERENCE AHEAD: the last call prepared the string it returned (ref_ahead_speculate, ref_ahead_settle).  If this is that string, what was counted on it
  // holds, and if the call wants what was prepared (ref_ahead_hit) it adopts it.
  mia_hip_ctx::RefAhead& ah = ctx->ahead;
  const bool had_shadow = ah.valid;
  ah.queued = false;
  const bool same_string = had_shadow && ref_ahead_same_string(ah.key, ah.str.data(), new_ref, L, circular);
  int64_t n_other = 0, kh_entries = 0;
  if (same_string) { n_other = ah.key.n_other; kh_entries = ah.key.kh_entries; }
  else ref_count_other(new_ref, L, wrap, &n_other, &kh_entries);
  ctx->ref_mostly_bases = n_other * 50 <= L;
  ctx->ref_few_n = n_other * 500 <= L;
  ctx->kh_entries = kh_entries;
  const bool staged = ctx->h_pin && (size_t)L <= mia_hip_ctx::PIN_BYTES - mia_hip_ctx::PIN_MISC;
  bool hit = false;
  if (had_shadow) {
    ah.valid = false;                        // (adopted or dropped: either way it is not there for the call after this one)
    RefAheadKey want;
    hit = ref_ahead_want(ctx, L, circular, n_other, kh_entries, &want) && ref_ahead_hit(ah.key, want, ah.str.data(), new_ref);
  }
  // A MISS waits for the stream as the call always did (the staging area may still feed an earlier copy), and with that for the
  // shadow launch; if that gave its barrier up, the word is cleared here: a call that uses nothing of it must not fail for it.
  // A HIT does not wait.  Everything that reads the adopted tables is queued behind the shadow launch on this stream, or behind an
  // event of this stream; the caller is usually back before the launch has ended (it is queued some 30 us before the call returns and
  // runs for 20), and a wait here put the plan's launch latency behind it -- measured: with the wait the step was as long as without
  // the shadow launch.  The stream is ASKED once: if the launch has ended and gave up, the call is a miss; if it has not ended,
  // the check behind the step's own wait finds the word, as it does for the call's own k_ref_prep (the iteration is void then).
  uint32_t* stuck = ctx->h_pin ? reinterpret_cast<uint32_t*>(ctx->h_pin + (62 << 10)) : nullptr;
  bool shadow_ended = !hit;
  if (hit) {
    const hipError_t eq = hipStreamQuery(ctx->stream);
    if (eq != hipErrorNotReady) { HIPCHK(eq); shadow_ended = true; }
  } else if (staged || had_shadow) HIPCHK(hipStreamSynchronize(ctx->stream));
  if (had_shadow && shadow_ended && stuck && *stuck) {
    *stuck = 0;
    ctx->no_prep_fuse = true;                // (from now on: six plain launches, and no shadow launch)
    hit = false;
  }
  if (hit) {
    ref_ahead_adopt(ctx);
  } else {
    if (dev_ensure(ctx, ctx->d_ref, total, (int64_t)total * 2) || dev_ensure(ctx, ctx->d_ascii, L, (int64_t)L * 2)) return MIA_HIP_ERR_NOMEM;
    if (staged) {
      memcpy(ctx->h_pin + mia_hip_ctx::PIN_MISC, new_ref, (size_t)L);
      // (zero_copy: the step's first kernel reads the sixteen thousand characters from the pinned area itself -- a copy in
      // front of it is a second engine and a wait between the two before anything runs)
      if (ctx->zero_copy) ctx->ascii_src = reinterpret_cast<const char*>(ctx->h_pin + mia_hip_ctx::PIN_MISC);
      else { HIPCHK(hipMemcpyAsync(ctx->d_ascii, ctx->h_pin + mia_hip_ctx::PIN_MISC, (size_t)L, hipMemcpyHostToDevice, ctx->stream)); ctx->ascii_src = ctx->d_ascii; }
    } else {
      HIPCHK(hipMemcpyAsync(ctx->d_ascii, new_ref, (size_t)L, hipMemcpyHostToDevice, ctx->stream));
      ctx->ascii_src = ctx->d_ascii;
    }
    // (the codes are made by align_all's first launch: k_ref_prep with everything else that is derived from the reference, or k_ref_encode)
    ctx->pend_encode = true; ctx->pend_L = L; ctx->pend_wl = wl; ctx->pend_total = total;
  }
  ctx->ref_ready = hit;
  if (ctx->rs.n == 0) { encode_now(ctx); HIPCHK(hipGetLastError()); }
  const bool dbg_steps = alt_env("MIA_HIP_ITER_DEBUG") != nullptr;      // diagnostic: wait and report after every stage
  // MIA_HIP_TIMING=1 (release builds too): host time at every stage boundary, no waits added -- where the HOST is held up (allocations, copies)
  static const bool host_laps = getenv("MIA_HIP_TIMING") != nullptr;
  const auto lap_t0 = std::chrono::steady_clock::now();
  auto checkpoint = [&](const char* what) {
    if (dbg_steps) { hipError_t e = hipStreamSynchronize(ctx->stream); fprintf(stderr, "[mia_hip_iterate] %s: %s\n", what, hipGetErrorString(e)); fflush(stderr); }
    if (host_laps) fprintf(stderr, "[mia_hip_iterate host] %-20s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - lap_t0).count());
  };
  checkpoint(hit ? "reference (ahead)" : "reference");
  ctx->L = L; ctx->wrap = wrap; ctx->have_ref = true; ctx->explicit_win = 0;
  const int64_t n = ctx->rs.n;
  const int W = ctx->comm_ranks;
  if (ctx->comm && n == 0) { ctx->err = "iterate: every rank of a sharded run needs reads"; return MIA_HIP_ERR_ARG; }
  if (ctx->comm && W > 256 - COMM_FLAG_SLOTS) { ctx->err = "iterate: more than 253 ranks"; return MIA_HIP_ERR_ARG; }
  // -- re-alignment (one wait, at its end; a sharded run's pre-cull all-gather rides in front of that wait)
  ctx->in_iterate = true;
  ctx->deferred = true;
  // no host wait behind the alignment when nothing on the host depends on it: one context, and a cut line that is given,
  // hard, or NaN by construction (reads of one length) -- see align_all / abort_if
  ctx->spec_pending = false; ctx->abort_if = nullptr;
  ctx->spec_ok = !ctx->comm && n > 0 && !ctx->no_spec && (hard_cut > 0 || slope_intercept || ctx->min_len == ctx->max_len);
  const int rca = align_all(ctx);
  ctx->deferred = false;
  ctx->spec_ok = false;
  ctx->pend_encode = false; ctx->ref_ready = false;      // (never outlive the call)
  if (rca) { ctx->spec_pending = false; ctx->abort_if = nullptr; return rca; }
  checkpoint("realign");
  int64_t slot_base = 0, g_sums[5] = {0, 0, 0, 0, 0};
  std::vector<int64_t> link_counts((size_t)W, 0), n_of((size_t)W, n);
  if (ctx->comm) {
    g_sums[3] = INT32_MAX; g_sums[4] = INT32_MIN;
    for (int r = 0; r < W; r++) {
      const int64_t* q = ctx->h_gather.data() + (size_t)PRE_WORDS * r;
      g_sums[0] += q[0]; g_sums[1] += q[1]; g_sums[2] += q[2];
      g_sums[3] = std::min(g_sums[3], q[3]); g_sums[4] = std::max(g_sums[4], q[4]);
      if (r < ctx->comm_rank) slot_base += q[5];
      link_counts[(size_t)r] = q[6];
    }
  }
  // -- the cut line of find_fsdb_score_cut (src/fsdb.c:269-383)
  double slope = 0, intercept = 0;
  const bool one_length = ctx->comm ? (g_sums[2] == 0 || g_sums[3] == g_sums[4]) : (ctx->min_len == ctx->max_len || n == 0);
  if (hard_cut > 0) {
  } else if (slope_intercept) {
    slope = slope_intercept[0]; intercept = slope_intercept[1];
  } else if (one_length) {
    // reads of one length: both regression sums are exactly 0, slope_bf = 0/0, and every derived quantity is that NaN
    // whatever the scores (mia_hip_score_cut_from_sums spells the arithmetic out) -- nothing to compute
    const double zero = 0.0;
    slope = intercept = zero / zero;
  } else if (!ctx->comm) {
    // sums of products in IEEE double are order dependent: the reference's sequential order over the scores, on the host
    std::vector<int32_t> score((size_t)n);
    HIPCHK(hipMemcpyAsync(score.data(), ctx->d_score, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    mia_hip_score_cut(score.data(), ctx->h_len.data(), nullptr, n, &slope, &intercept);
  } else {
    // the same over the reads of ALL ranks in fsdb order (= rank order): scores and lengths gathered, the regression on
    // every rank's host (identical inputs, identical arithmetic)
    DevBuf<int32_t> d_nl;                                  // {score..., len...} of this rank, padded to the longest
    std::vector<int64_t> cnt1((size_t)W, 1);
    int64_t tot = 0;
    int64_t n64 = n;
    DevBuf<int64_t> d_n;
    if (dev_alloc(ctx, d_n, 1)) return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemcpyAsync(d_n, &n64, 8, hipMemcpyHostToDevice, ctx->stream));
    if (int rcg = comm_gather_ragged(ctx, d_n, cnt1, 1, &tot)) return rcg;
    HIPCHK(hipMemcpyAsync(n_of.data(), ctx->d_lall, (size_t)W * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int64_t nmax = 0, ntot = 0;
    for (int r = 0; r < W; r++) { nmax = std::max(nmax, n_of[(size_t)r]); ntot += n_of[(size_t)r]; }
    if (dev_alloc(ctx, d_nl, nmax * 2) || dev_ensure(ctx, ctx->d_scores_all, (int64_t)W * nmax * 2)) return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemsetAsync(d_nl, 0, (size_t)nmax * 2 * 4, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_nl, ctx->d_score, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_nl + nmax, ctx->h_len.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    COLLCHK(ctx->coll.all_gather(ctx->coll.user, d_nl, ctx->d_scores_all, (size_t)nmax * 2 * 4, ctx->stream));
    std::vector<int32_t> all((size_t)W * nmax * 2), score((size_t)ntot), lens((size_t)ntot);
    HIPCHK(hipMemcpyAsync(all.data(), ctx->d_scores_all, all.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int64_t o = 0;
    for (int r = 0; r < W; r++) {
      memcpy(score.data() + o, all.data() + (size_t)r * nmax * 2, (size_t)n_of[(size_t)r] * 4);
      memcpy(lens.data() + o, all.data() + (size_t)r * nmax * 2 + nmax, (size_t)n_of[(size_t)r] * 4);
      o += n_of[(size_t)r];
    }
    mia_hip_score_cut(score.data(), lens.data(), nullptr, ntot, &slope, &intercept);
  }
  if (!(hard_cut > 0) && slope <= 0) slope = 100.0;         // src/mia.c:440-442
  auto queue_cull = [&]() -> int {
    ctx->buckets_queued = 0;
    const bool side = tally_is_binned(ctx) && !ctx->no_side_buckets;
    // (nothing has been waited for: stream2 must stay behind the alignment -- but not behind the cull)
    // (... unless the alignment's last launch on this stream has signalled ev_fork itself: bx_join_and_retry)
    if (side && ctx->spec_pending && !ctx->align_end_signalled) HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
    if (int rcc = mia_hip_cull(ctx, hard_cut, slope, intercept, slot_base)) return rcc;
    // the tally's counting sort reads nothing the cull writes: on stream2, beside the cull kernels (queued behind them on the
    // host side -- the GPU is waiting for the first cull kernel at this point, not for these)
    if (side) {
      if (ctx->spec_pending) HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
      if (int rcb = bucket_launch(ctx, ctx->stream2)) return rcb;
    }
    return MIA_HIP_OK;
  };
  if (int rcq = queue_cull()) return rcq;
  if (ctx->comm) {
    // links of formerly split reads (stale fs->back_asp, include/mia_hip.h) may point at slots of another rank: every rank
    // gets all links, applies those that hit its own slots, the record lengths the readers need come back by a max-reduce
    int64_t any = 0;
    for (int r = 0; r < W; r++) any += link_counts[(size_t)r];
    if (any > 0) {
      int64_t* dl = nullptr; int64_t nl = 0, total_l = 0;
      if (int rcl = mia_hip_links(ctx, &dl, &nl)) return rcl;
      if (nl != link_counts[(size_t)ctx->comm_rank]) { ctx->err = "iterate: the cull emitted another number of links than the score sweep announced"; return MIA_HIP_ERR_STATE; }
      if (int rcg = comm_gather_ragged(ctx, dl, link_counts, 4, &total_l)) return rcg;
      if (int rcs = mia_hip_set_links(ctx, ctx->d_lall, total_l)) return rcs;
      int32_t *dlen = nullptr, *dact = nullptr; int64_t nn = 0;
      if (int rcl = mia_hip_link_lengths(ctx, &dlen, &dact, &nn)) return rcl;
      COLLCHK(ctx->coll.all_reduce_i32(ctx->coll.user, dlen, (size_t)nn, MIA_HIP_OP_MAX, ctx->stream));
      COLLCHK(ctx->coll.all_reduce_i32(ctx->coll.user, dact, (size_t)nn, MIA_HIP_OP_MAX, ctx->stream));
      if (int rcf = mia_hip_finish_links(ctx)) return rcf;
    }
  }
  checkpoint("cull");
  if (n == 0) { out[0] = 0; if (out_len) *out_len = 0; return MIA_HIP_OK; }
  // -- tally and consensus, queued back to back
  if (ctx->comm && ctx->ev_pad > 0) {
    if (const char* e = alt_env("MIA_HIP_EV_PAD")) { const long long v = atoll(e); if (v > 0) ctx->ev_pad = v; }   // (tests: force the overflow path; every rank reads the same value)
    // the gathered events land in this context's list: room for every rank's block before anything is tallied into it
    if (int rct = ensure_tally(ctx)) return rct;
    if (ctx->ev_pad * W > ctx->tb.cap_events && ensure_events(ctx, std::min<int64_t>(ctx->ev_pad * W + 4096, (int64_t)1 << 30))) return MIA_HIP_ERR_NOMEM;
  }
  if (int rct = tally_launch(ctx)) return rct;
  checkpoint("tally");
  const int Lp = ctx->tb.Lp;
  ctx->n_events_host = 0;
  int32_t* h_evc = ctx->h_pin ? reinterpret_cast<int32_t*>(ctx->h_pin + (56 << 10)) : nullptr;      // the ranks' event counts, read with the results
  std::vector<int32_t> evc_pageable;
  if (ctx->comm && !h_evc) { evc_pageable.resize((size_t)W); h_evc = evc_pageable.data(); }
  // the events of all ranks with the counts in hand (one more wait for the host): the first sharded iteration, and whenever
  // a rank had more events than the blocks of the other way were sized for
  auto exchange_events_counted = [&]() -> int {
    HIPCHK(hipMemcpyAsync(h_evc, ctx->tb.gaps + Lp, (size_t)W * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> ev_counts((size_t)W);
    for (int r = 0; r < W; r++) ev_counts[(size_t)r] = h_evc[r];
    int64_t total_ev = 0;
    if (int rcg = comm_gather_ragged(ctx, reinterpret_cast<const int64_t*>(ctx->tb.events), ev_counts, 1, &total_ev)) return rcg;
    if (total_ev > ctx->tb.cap_events && ensure_events(ctx, total_ev + 4096)) return MIA_HIP_ERR_NOMEM;
    if (total_ev > 0) HIPCHK(hipMemcpyAsync(ctx->tb.events, ctx->d_lall, (size_t)total_ev * 8, hipMemcpyDeviceToDevice, ctx->stream));
    int32_t* te = ctx->h_pin ? reinterpret_cast<int32_t*>(ctx->h_pin + (60 << 10)) : nullptr;
    int32_t te_local = (int32_t)total_ev;
    if (te) { *te = te_local; HIPCHK(hipMemcpyAsync(ctx->tb.n_events, te, 4, hipMemcpyHostToDevice, ctx->stream)); }
    else { HIPCHK(hipMemcpyAsync(ctx->tb.n_events, &te_local, 4, hipMemcpyHostToDevice, ctx->stream)); HIPCHK(hipStreamSynchronize(ctx->stream)); }
    return MIA_HIP_OK;
  };
  // ... and without: every rank contributes a block of ev_pad events (sized from the counts of the iteration before, the
  // same on every rank), the counts that rode on the gaps reduce tell k_events_compact how much of each block is real
  auto exchange_events_padded = [&]() -> int {
    const int64_t pad = ctx->ev_pad;
    if (dev_ensure(ctx, ctx->d_lstage, pad * W, pad * W * 2)) return MIA_HIP_ERR_NOMEM;
    COLLCHK(ctx->coll.all_gather(ctx->coll.user, ctx->tb.events, ctx->d_lstage, (size_t)pad * 8, ctx->stream));
    const unsigned gx = (unsigned)std::min<int64_t>((pad + 255) / 256, 64);
    hipLaunchKernelGGL(k_events_compact, dim3(gx, (unsigned)W), dim3(256), 0, ctx->stream, (const uint64_t*)ctx->d_lstage.p, pad, (const int32_t*)(ctx->tb.gaps + Lp), W,
                       ctx->tb.events, ctx->tb.cap_events, ctx->tb.n_events, ctx->tb.flags);
    HIPCHK(hipGetLastError());
    return MIA_HIP_OK;
  };
  bool counted = false;
  if (ctx->comm) {
    // integer column tallies add up, ref->gaps is a maximum (src/mia.c:486-504); every rank's insert-event count rides on
    // the max-reduce in W extra slots behind gaps; then the events themselves are gathered
    if (ctx->fake_event_overflow)      // (alt build, MIA_HIP_FAKE_EVENT_OVERFLOW=1 when the context was made -- tests: this rank pretends its event list overflowed)
      hipLaunchKernelGGL(k_or_u32, dim3(1), dim3(1), 0, ctx->stream, ctx->tb.flags, 1u);
    hipLaunchKernelGGL(k_put_rank_words, dim3(1), dim3(1), 0, ctx->stream, ctx->tb.gaps + Lp, (int32_t)ctx->comm_rank, (int32_t)W, (const int32_t*)ctx->tb.n_events,
                       ctx->tb.cap_events, (const uint32_t*)ctx->tb.flags, (const uint32_t*)ctx->d_cull_flags);
    COLLCHK(ctx->coll.all_reduce_i32(ctx->coll.user, ctx->tb.tally, (size_t)TALLY_WORDS * Lp, MIA_HIP_OP_SUM, ctx->stream));
    COLLCHK(ctx->coll.all_reduce_i32(ctx->coll.user, ctx->tb.gaps, (size_t)Lp + W + COMM_FLAG_SLOTS, MIA_HIP_OP_MAX, ctx->stream));
    counted = ctx->ev_pad <= 0;
    if (int rce = counted ? exchange_events_counted() : exchange_events_padded()) return rce;
  }
  const int64_t cons_cap = (int64_t)L + ctx->ins_tally_cap + 64;          // string bytes
  const int64_t res_bytes = (int64_t)CH_WORDS * 4 + cons_cap;
  const size_t need = (size_t)res_bytes;
  // (the result blocks are about to move: a shadow launch that this call adopted without waiting may still be reading the last string)
  if (res_bytes > ctx->d_cons.cap || need > ctx->pin2_bytes) HIPCHK(hipStreamSynchronize(ctx->stream));
  if (dev_ensure(ctx, ctx->d_cons, res_bytes, res_bytes * 2) || dev_ensure(ctx, ctx->d_cons_pos, Lp, (int64_t)Lp * 2)) return MIA_HIP_ERR_NOMEM;
  if (need > ctx->pin2_bytes) {
    if (ctx->h_pin2) (void)hipHostFree(ctx->h_pin2);
    ctx->h_pin2 = nullptr; ctx->pin2_bytes = 0;
    if (hipHostMalloc((void**)&ctx->h_pin2, need * 2, hipHostMallocDefault) != hipSuccess) { ctx->err = "hipHostMalloc"; return MIA_HIP_ERR_NOMEM; }
    ctx->pin2_bytes = need * 2;
  }
  int32_t* h_hdr = reinterpret_cast<int32_t*>(ctx->h_pin2);
  char* h_str = reinterpret_cast<char*>(ctx->h_pin2) + CH_WORDS * 4;
  // REFERENCE AHEAD, speculatively (ref_ahead_speculate): one context, the string written to the host by k_cons_scatter itself, a
  // reference of plain bases -- the key of a consensus as long as its reference and as free of N
  RefAheadKey spec_key;
  bool spec_ahead = !ctx->comm && ctx->zero_copy && n_other == 0 && ref_ahead_allowed(ctx) && ref_ahead_want(ctx, L, circular, 0, 0, &spec_key);
  // consensus calls, the string consensus_assembly_string returns put together on the device (characters per column, their
  // prefix sums, a scatter), header and string back in one copy, the second and last wait
  auto consensus_tail = [&]() -> int {
    // (a workgroup alone on sixteen thousand columns is slower than a launch costs -- 44 + 111 us for two single-workgroup
    // kernels against 5 us each for these: the launches that remain are the ones with a chip-wide dependence between them)
    const int64_t cap = ctx->ins_tally_cap;
    int32_t* d_res = reinterpret_cast<int32_t*>(ctx->d_cons.p);
    const unsigned gl = (unsigned)((L + 255) / 256);
    const bool zc = ctx->zero_copy;        // header, string and the alignment's counters written to the host by k_cons_scatter itself
    // the two prefix sums of the tail (insert columns before a column, characters before a column) are worked out by the blocks
    // of their consumers while the sequence is short enough for that (MIA_HIP_TAIL_SCANS=1: single-workgroup launches, as for long references)
    const bool fused_scans = Lp <= (1 << 17) && !ctx->tail_scans;      // (100 kb: ~20 us inside the consumers against 60 us per single-workgroup scan)
    const unsigned glp = (unsigned)((Lp + 255) / 256);
    if (!fused_scans) {
      hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t*)ctx->tb.gaps, Lp, 1, L, ctx->d_ins_off, ctx->d_ins_total, ctx->abort_if);   // ins_off[p] = gaps[1] + .. + gaps[p-1]
      hipLaunchKernelGGL(k_call_columns_z, dim3(gl), dim3(256), 0, ctx->stream, (const int32_t*)ctx->tb.tally, Lp, L, cons_code, ctx->d_calls, ctx->d_ins_tally, ins_words(cap), ctx->abort_if,
                         (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    } else
      hipLaunchKernelGGL(k_call_columns_z, dim3(glp > gl ? glp : gl), dim3(256), 0, ctx->stream, (const int32_t*)ctx->tb.tally, Lp, L, cons_code, ctx->d_calls, ctx->d_ins_tally, ins_words(cap), ctx->abort_if,
                         (const int32_t*)ctx->tb.gaps, ctx->d_ins_off, ctx->d_ins_total);
    if (cap > 0)
      hipLaunchKernelGGL(k_ins_tally, dim3(256), dim3(256), 0, ctx->stream, ctx->tb.events, 0, ctx->d_pssm, ctx->d_ins_off, ctx->tb.gaps, L, ctx->d_ins_tally,
                         (int32_t)cap, (const int32_t*)ctx->tb.n_events, ctx->tb.cap_events, ctx->abort_if);
    checkpoint("consensus kernels");
    hipLaunchKernelGGL(k_call_inserts_count, dim3(gl), dim3(256), 0, ctx->stream, (const int32_t*)ctx->tb.tally, Lp, L, (const int32_t*)ctx->tb.gaps,
                       (const int32_t*)ctx->d_ins_off, ctx->d_ins_tally, cons_code, (const char*)ctx->d_calls, ctx->d_ins_calls, (int32_t)cap,
                       (const int32_t*)ctx->d_ins_total, ctx->d_cons_pos, ctx->abort_if);
    if (!fused_scans) hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t*)ctx->d_cons_pos, L, 0, L, ctx->d_cons_pos, d_res + CH_LEN, ctx->abort_if);
    // (with a shadow launch behind it the kernel signals ev_cons itself: the host waits for that, the stream goes on)
    launch_k(k_cons_scatter, dim3(gl), dim3(256), 0, ctx->stream, spec_ahead ? ctx->ev_cons : (hipEvent_t) nullptr, (const char*)ctx->d_calls, (const char*)ctx->d_ins_calls,
                       (const int32_t*)ctx->tb.gaps, (const int32_t*)ctx->d_ins_off, L, (int32_t)cap, (const int32_t*)ctx->d_ins_total,
                       (const int32_t*)ctx->d_cons_pos, d_res, (int32_t)cons_cap, (const int32_t*)ctx->tb.n_events, (const uint32_t*)ctx->tb.flags,
                       (const uint32_t*)ctx->d_cull_flags, ctx->abort_if, zc ? reinterpret_cast<int32_t*>(ctx->h_pin2) : (int32_t*)nullptr,
                       ctx->d_ctr0, (int32_t)CTRL_CN, (zc && ctx->spec_pending) ? reinterpret_cast<int32_t*>(ctx->h_pin) : (int32_t*)nullptr,
                       fused_scans ? 1 : 0, ctx->comm ? (const int32_t*)(ctx->tb.gaps + Lp + W) : (const int32_t*)nullptr);
    HIPCHK(hipGetLastError());
    if (spec_ahead) ref_ahead_speculate(ctx, spec_key, h_str);
    checkpoint("assemble");
    if (!zc) HIPCHK(hipMemcpyAsync(ctx->h_pin2, ctx->d_cons, need, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->comm && !counted) HIPCHK(hipMemcpyAsync(h_evc, ctx->tb.gaps + Lp, (size_t)W * 4, hipMemcpyDeviceToHost, ctx->stream));
    // the step's one wait.  The host has nothing else to do for this millisecond: it asks until the stream is done instead of
    // sleeping on an interrupt (MIA_HIP_SPIN_WAIT=0: hipStreamSynchronize)
    if (ctx->spin_wait) {
      hipError_t eq;
      while ((eq = spec_ahead ? hipEventQuery(ctx->ev_cons) : hipStreamQuery(ctx->stream)) == hipErrorNotReady) {}
      HIPCHK(eq);
    } else if (spec_ahead) HIPCHK(hipEventSynchronize(ctx->ev_cons));
    else HIPCHK(hipStreamSynchronize(ctx->stream));
    return MIA_HIP_OK;
  };
  if (int rct = consensus_tail()) return rct;
  if (ctx->h_pin) {
    // k_ref_prep's grid barrier is bounded (mia_iter_kernels.h): a grid that never became wholly resident ends here, as an error
    uint32_t* stuck = reinterpret_cast<uint32_t*>(ctx->h_pin + (62 << 10));
    if (*stuck) {
      *stuck = 0;
      ctx->no_prep_fuse = true;              // (from now on: six plain launches)
      ctx->err = "k_ref_prep: part of the launch never reached the grid barrier (device partitioned or compute units masked?); the iteration's results are void";
      return MIA_HIP_ERR_DEVICE;
    }
  }
  if (ctx->spec_pending) {
    // the alignment's counters arrived with the consensus.  Reads waiting for the exact kernel (next to never): every kernel
    // queued behind the alignment has returned without touching anything; the exact kernel runs, and cull, tally and consensus
    // are queued again -- this time unconditionally
    ctx->spec_pending = false;
    ctx->abort_if = nullptr;
    const int32_t* hb = reinterpret_cast<const int32_t*>(ctx->h_pin);
    align_counters_collect(ctx, hb, ctx->spec_filtered, ctx->spec_bx, ctx->spec_plain);
    const int32_t n_wide = hb[0];
    if (n_wide > 0 || ctx->spec_force) {
      ctx->spec_redone++;
      RefInfo rinfo{ctx->d_ref, ctx->L, ctx->wrap, ctx->explicit_win};
      if (n_wide > 0) { if (int rcw = run_wide(ctx, rinfo, n_wide)) return rcw; }
      if (int rcq = queue_cull()) return rcq;
      if (int rct = tally_launch(ctx)) return rct;
      // (the speculative shadow launch read a string the aborted tail never wrote: it is dropped, and none rides on the second round)
      spec_ahead = false; ctx->ahead.queued = false;
      if (int rct = consensus_tail()) return rct;
    }
  }
  uint32_t tflags = (uint32_t)h_hdr[CH_TALLY_FLAGS];
  if (ctx->comm && !counted && (tflags & 8u)) {
    // some rank had more insert events than the blocks held (every rank sees the same counts, so every rank is here):
    // the lists and counts are untouched -- exchange them with the counts in hand and call the consensus again
    counted = true;
    if (int rce = exchange_events_counted()) return rce;
    if (int rct = consensus_tail()) return rct;
    tflags = (uint32_t)h_hdr[CH_TALLY_FLAGS];
  }
  tflags &= ~8u;
  if (ctx->comm) {
    // the block size of the next iteration's event exchange, from counts every rank has seen: half as much again as the
    // largest, re-sized only when that leaves the band [pad/4, 0.8 pad] (identical arithmetic on identical numbers)
    int64_t mx = 0;
    for (int r = 0; r < W; r++) mx = std::max<int64_t>(mx, h_evc[r]);
    if (ctx->ev_pad <= 0 || mx * 5 > ctx->ev_pad * 4 || mx * 4 < ctx->ev_pad) ctx->ev_pad = mx + mx / 2 + 1024;
  }
  ctx->in_iterate = false;
  if (int rcf = tally_finish(ctx, (uint32_t)h_hdr[CH_N_EVENTS], tflags, (uint32_t)h_hdr[CH_CULL_FLAGS])) return rcf;
  if (h_hdr[CH_OVERFLOW]) {
    // more insert columns than the buffers of the last call hold: the step-wise entry point enlarges them and calls again
    ctx->iter_fallbacks++;
    return mia_hip_consensus(ctx, cons_code, out, out_cap, out_len);
  }
  const int64_t len = h_hdr[CH_LEN];
  if (len + 1 > out_cap) { ctx->err = "consensus buffer too small"; return MIA_HIP_ERR_ARG; }
  ref_ahead_settle(ctx, h_str, len, circular);       // (in front of the copy: the device works while the host copies and returns)
  memcpy(out, h_str, (size_t)len);
  out[len] = 0;
  if (out_len) *out_len = len;
  ctx->consensus_done = true;
  ctx->ins_total_host = h_hdr[CH_INS_TOTAL];
  return MIA_HIP_OK;
}

