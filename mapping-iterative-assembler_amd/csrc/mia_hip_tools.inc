// mia_hip_tools.inc -- part of mia_hip.hip (one translation unit): the entry points beside the per-iteration path -- adapter
// trimming (trim_frag), ma's tallies, pass 1 (new_kmer_filter + sg_align), Myers distances, the measured ceilings of bench.py.

// ---- adapter trimming ---------------------------------------------------------------------------
extern "C" int mia_hip_trim(mia_hip_ctx* ctx, const char* adapter, int64_t n, const char* bases, const int64_t* offsets,
                            uint8_t* trimmed, int32_t* trim_point) {
  if (!ctx || !adapter || n < 0 || (n > 0 && (!bases || !offsets || !trimmed || !trim_point))) return MIA_HIP_ERR_ARG;
  const int len2 = (int)strlen(adapter);
  if (len2 < 1 || len2 > MAX_ADAPTER) { ctx->err = "adapter length outside 1..127"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  if (n == 0) { ctx->trim_escapes = ctx->trim_launches = ctx->trim_scratch_bytes = 0; return MIA_HIP_OK; }
  for (int64_t i = 0; i < n; i++) {
    const int64_t l = offsets[i + 1] - offsets[i];
    if (l < 1 || l > MIA_HIP_MAX_READ) { ctx->err = "read length outside 1..256"; return MIA_HIP_ERR_ARG; }
  }
  // init_flatsubmat (src/pssm.c:96-126)
  std::vector<int32_t> flat((size_t)PSSM_WORDS);
  for (int d = 0; d < 31; d++)
    for (int i = 0; i < 5; i++)
      for (int j = 0; j < 5; j++)
        flat[(size_t)(d * 5 + i) * 5 + j] = i == 4 ? -10 : (j == 4 ? -100 : (i == j ? 200 : -600));
  PackParams pk;
  if (!make_pack_params(256, 600, &pk)) return MIA_HIP_ERR_RANGE;
  const int64_t chars = offsets[n] - offsets[0];
  std::vector<uint8_t> codes((size_t)chars), acodes((size_t)len2), apacked((size_t)(len2 + 1) / 2 + 4, 0);
  for (int64_t k = 0; k < chars; k++) codes[(size_t)k] = base_code(bases[offsets[0] + k]);
  for (int k = 0; k < len2; k++) { acodes[(size_t)k] = base_code(adapter[k]); apacked[(size_t)k >> 1] |= (uint8_t)(acodes[(size_t)k] << ((k & 1) * 4)); }
  std::vector<int64_t> off0((size_t)n + 1);
  for (int64_t i = 0; i <= n; i++) off0[(size_t)i] = offsets[i] - offsets[0];
  int occ = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)k_trim, 64, 0));
  if (occ < 1) occ = 1;
  if (occ > 32) occ = 32;
  if (occ > 4) occ &= ~3;
  int64_t grid = (int64_t)ctx->cus * occ;
  if (grid > n) grid = n;
  const int64_t slab = (int64_t)(MAX_ADAPTER + 1) * MAX_READ;
  DevBuf<uint8_t> d_codes, d_ap, d_ac, d_trimmed;   // every temporary is released on any return
  DevBuf<int64_t> d_off;
  DevBuf<int32_t> d_flat, d_tp, d_list, d_scratch;
  DevBuf<uint32_t> d_status;
  DevBuf<unsigned char> d_slabs;
  DevBuf<int16_t> d_cols;
  int nomem = dev_alloc(ctx, d_codes, chars + 8) | dev_alloc(ctx, d_ap, (int64_t)apacked.size()) | dev_alloc(ctx, d_ac, len2) |
            dev_alloc(ctx, d_trimmed, n) | dev_alloc(ctx, d_off, n + 1) | dev_alloc(ctx, d_flat, PSSM_WORDS) |
            dev_alloc(ctx, d_tp, n) | dev_alloc(ctx, d_status, n) | dev_alloc(ctx, d_slabs, slab * grid) |
            dev_alloc(ctx, d_cols, grid * MAX_READ);
  if (nomem) return MIA_HIP_ERR_NOMEM;
  hipError_t e = hipSuccess;
  auto up = [&](void* d, const void* h, size_t b) { if (e == hipSuccess && b) e = hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, ctx->stream); };
  up(d_codes, codes.data(), (size_t)chars); up(d_ap, apacked.data(), apacked.size()); up(d_ac, acodes.data(), (size_t)len2);
  up(d_off, off0.data(), (size_t)(n + 1) * 8); up(d_flat, flat.data(), (size_t)PSSM_WORDS * 4);
  TrimReads tr{n, d_codes, d_off, d_trimmed, d_tp, d_status};
  std::vector<uint32_t> status((size_t)n);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_trim, dim3((unsigned)grid), dim3(64), 0, ctx->stream, tr, d_ap, len2, d_flat, pk, d_slabs, slab, d_cols);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(status.data(), d_status, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  // gaps of 63 or more on the optimal path: exact scalar re-run of those reads (MIA_HIP_TRIM_EXACT of the alt build: of every read),
  // TRIM_EXACT_PIECE reads per launch on one scratch, so that a batch full of such reads needs 0.55 GB at 127 adapter bases and no more
  std::vector<int32_t> esc;
  int64_t launches = 0, scratch_bytes = 0;
  if (e == hipSuccess)
    for (int64_t i = 0; i < n; i++) if (status[(size_t)i] != ST_OK || ctx->trim_exact) esc.push_back((int32_t)i);
  if (e == hipSuccess && !esc.empty()) {
    const int64_t words = (int64_t)len2 * MAX_READ + 5 * (int64_t)MAX_READ, total = (int64_t)esc.size();
    const int64_t piece = total < TRIM_EXACT_PIECE ? total : TRIM_EXACT_PIECE;
    if (dev_alloc(ctx, d_list, total) || dev_alloc(ctx, d_scratch, words * piece)) return MIA_HIP_ERR_NOMEM;
    scratch_bytes = words * piece * (int64_t)sizeof(int32_t);
    up(d_list, esc.data(), esc.size() * 4);
    for (int64_t lo = 0; lo < total && e == hipSuccess; lo += piece) {     // (one stream: a piece starts when the one before it is done)
      const int64_t cnt = total - lo < piece ? total - lo : piece;
      hipLaunchKernelGGL(k_trim_wide, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, ctx->stream, tr, d_ac, len2, d_flat, d_list + lo,
                         (int32_t)cnt, d_scratch, words);
      e = hipGetLastError();
      launches++;
    }
  }
  if (e == hipSuccess) e = hipMemcpyAsync(trimmed, d_trimmed, (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(trim_point, d_tp, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { ctx->err = std::string("trim: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  ctx->trim_escapes = (int64_t)esc.size();
  ctx->trim_launches = launches;
  ctx->trim_scratch_bytes = scratch_bytes;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_trim_stats(mia_hip_ctx* ctx, int64_t* exact_reruns) {
  if (!ctx || !exact_reruns) return MIA_HIP_ERR_ARG;
  *exact_reruns = ctx->trim_escapes;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_trim_rerun_stats(mia_hip_ctx* ctx, int64_t* launches, int64_t* scratch_bytes) {
  if (!ctx || !launches || !scratch_bytes) return MIA_HIP_ERR_ARG;
  *launches = ctx->trim_launches;
  *scratch_bytes = ctx->trim_scratch_bytes;
  return MIA_HIP_OK;
}

// ---- ma -------------------------------------------------------------------------------------
// The records the last mia_hip_ma_tally left on the device (ma_records.h): every view of an export is built on this.
static MaRecords ma_records(const mia_hip_ctx* ctx) {
  return MaRecords{ctx->ma_n, ctx->ma_L, ctx->d_ma_start, ctx->d_ma_rev, ctx->d_ma_coff, ctx->d_ma_seq, ctx->d_ma_rec_ins, ctx->d_ma_ins_list, ctx->d_ma_ipos,
                   ctx->d_ma_ioff, ctx->d_ma_ib, ctx->d_ma_smp};
}

// What the statistics calls (profile, ends, cols) share: the segment characters and the selection `use` go up into the context's
// buffers (NULL stays NULL: every record is whole, every record counts); used = the records that count.
struct MaSelection { const uint8_t *segment, *use; int64_t used; };
static int ma_selection(mia_hip_ctx* ctx, const uint8_t* segment, const uint8_t* use, MaSelection* sel) {
  const int64_t n = ctx->ma_n;
  if (dev_ensure(ctx, ctx->d_ends_seg, n + 1) || dev_ensure(ctx, ctx->d_prof_use, n + 1)) return MIA_HIP_ERR_NOMEM;
  if (segment && n > 0) HIPCHK(hipMemcpyAsync(ctx->d_ends_seg, segment, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  if (use && n > 0) HIPCHK(hipMemcpyAsync(ctx->d_prof_use, use, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  *sel = MaSelection{segment ? (const uint8_t*)ctx->d_ends_seg : nullptr, use ? (const uint8_t*)ctx->d_prof_use : nullptr, 0};
  for (int64_t r = 0; r < n; r++) sel->used += !use || use[r] ? 1 : 0;
  return MIA_HIP_OK;
}

// A persistent grid: the workgroups that are resident at once (per_cu on every compute unit), or `wgs`, one per chunk of the work,
// when there are fewer -- and one workgroup that finds no chunk where there is no work (records that all lack columns).
static dim3 ma_grid(const mia_hip_ctx* ctx, int64_t wgs, int per_cu) {
  const int64_t wide = (int64_t)ctx->cus * per_cu;
  return dim3((unsigned)(wgs < 1 ? 1 : wgs < wide ? wgs : wide));
}

// A result's way down, queued on the context's stream: nothing for a caller who passed no buffer and for an empty result.
static hipError_t ma_down(mia_hip_ctx* ctx, void* host, const void* dev, size_t bytes) {
  return host && bytes ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
}

// What the two filters by molecule (damage, score) share in front of their launches.  The checks, in the order the callers always
// had them: the records are resident, there is a reference, the caller's own arguments are right (own_error: what is wrong with
// them, or NULL), col_off starts at 0, mate pairs the records.  Then, with records: the reference, the selection and the pairing go
// up (mate into the caller's own buffer), and the view of the flat columns and the two grids -- over col_wgs chunks of columns and
// rec_wgs chunks of records -- are made.
struct MaMolFrame { MaFlatView v{MaRecords{}, 0, nullptr, nullptr}; const int64_t* mate = nullptr; dim3 col_grid, rec_grid; };
static int ma_mol_frame(mia_hip_ctx* ctx, const char* who, const char* ref_seq, const uint8_t* use, const int64_t* mate, const char* own_error,
                        DevBuf<int64_t>& d_mate, int64_t col_wgs, int64_t rec_wgs, int per_cu, MaMolFrame* f) {
  const std::string name = who;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede " + name; return MIA_HIP_ERR_STATE; }
  if (!ref_seq) { ctx->err = name + ": no reference sequence"; return MIA_HIP_ERR_ARG; }
  if (own_error) { ctx->err = name + ": " + own_error; return MIA_HIP_ERR_ARG; }
  if (ctx->ma_n > 0 && ctx->ma_cols < 0) { ctx->err = name + ": col_off[0] of the tallied records is not 0"; return MIA_HIP_ERR_ARG; }
  const int64_t n = ctx->ma_n;
  if (!ma_mate_ok(mate, n)) { ctx->err = name + ": mate is out of range, the record itself or not mutual"; return MIA_HIP_ERR_ARG; }
  if (n == 0) return MIA_HIP_OK;
  HIPCHK(hipSetDevice(ctx->device));
  MaSelection sel;
  if (dev_ensure(ctx, ctx->d_prof_ref, (int64_t)ctx->ma_L) || (mate && dev_ensure(ctx, d_mate, n))) return MIA_HIP_ERR_NOMEM;
  if (const int rc = ma_selection(ctx, nullptr, use, &sel)) return rc;
  HIPCHK(hipMemcpyAsync(ctx->d_prof_ref, ref_seq, (size_t)ctx->ma_L, hipMemcpyHostToDevice, ctx->stream));
  if (mate) HIPCHK(hipMemcpyAsync(d_mate, mate, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  f->v = MaFlatView{ma_records(ctx), ctx->ma_cols, ctx->d_prof_ref, sel.use};
  f->mate = mate ? (const int64_t*)d_mate : nullptr;
  f->col_grid = ma_grid(ctx, col_wgs, per_cu);
  f->rec_grid = ma_grid(ctx, rec_wgs, per_cu);
  return MIA_HIP_OK;
}

extern "C" int mia_hip_ma_tally(mia_hip_ctx* ctx, int32_t ref_len, const int32_t* gaps, int64_t n, const int32_t* start,
                                const uint8_t* revcom, const int64_t* col_off, const char* seq, const char* smp, int64_t n_ins,
                                const int32_t* ins_record, const int32_t* ins_pos, const int64_t* ins_off, const char* ins_bases) {
  if (!ctx || ref_len <= 0 || !gaps || n < 0 || n_ins < 0 || (n > 0 && (!start || !revcom || !col_off || !seq || !smp)) ||
      (n_ins > 0 && (!ins_record || !ins_pos || !ins_off || !ins_bases)))
    return MIA_HIP_ERR_ARG;
  if (!ctx->have_pssm) { ctx->err = "set_pssm must precede ma_tally"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  bool cols_ok = true;                             // (a record past the reference is the tally's to refuse; one of no columns it never sees)
  for (int64_t r = 0; r < n; r++) {
    if (col_off[r + 1] < col_off[r] || start[r] < 0) { ctx->err = "malformed record geometry"; return MIA_HIP_ERR_ARG; }
    cols_ok = cols_ok && (int64_t)start[r] + (col_off[r + 1] - col_off[r]) <= (int64_t)ref_len + 1;   // (a circular assembly's record may end on column L)
  }
  for (int64_t e = 0; e < n_ins; e++)
    if (ins_record[e] < 0 || ins_record[e] >= n || ins_off[e + 1] < ins_off[e]) { ctx->err = "malformed insert list"; return MIA_HIP_ERR_ARG; }
  ctx->L = ref_len;
  ctx->wrap = ref_len;
  const int64_t ins_chars = n_ins ? ins_off[n_ins] : 0;
  // no list yet (cap_events 0), or one that was sized for another job
  if (ctx->tb.cap_events < ins_chars + 16 && ensure_events(ctx, ins_chars + 4096)) return MIA_HIP_ERR_NOMEM;
  int rc = ensure_tally(ctx);
  if (rc) return rc;
  const int Lp = ctx->tb.Lp;
  const int64_t chars = n ? col_off[n] : 0;
  // the INS_POS pairs by record (the exports fetch a record's own range, and its pair of a position by bisection)
  if (n > INT32_MAX - 1 || n_ins > INT32_MAX - 1) { ctx->err = "ma_tally: more than 2^31 records or INS_POS pairs"; return MIA_HIP_ERR_ARG; }
  std::vector<int32_t> rec_ins, ins_list;
  ma_list_pairs(n, n_ins, ins_record, ins_pos, &rec_ins, &ins_list);
  // The records stay on the device behind this call (mia_hip_ma_region reads them): buffers of the context, made here, before anything
  // is queued.  Strand and depth codes stay for mia_hip_ma_profile; the pairs' record numbers are needed by the tally alone.  SEQ and
  // SMP are readable up to the next multiple of MA_REC_LANE behind their last character (k_ma_profile loads them in words of that size),
  // and so are the pairs' characters (k_ma_ends counts their '-' in such words too).
  ctx->ma_resident = false;
  ctx->ma_out = {};
  ctx->collapse.done = false;
  ctx->ma_ace_gaps_ok = ma_ace_gaps_ok(gaps, ref_len);
  ctx->ma_ace_cols_ok = cols_ok;
  ctx->ma_sam_gaps_ok = ma_sam_gaps_ok(gaps, ref_len);
  DevBuf<int32_t> d_irec;   // every temporary is released on any return
  int nomem = dev_alloc(ctx, ctx->d_ma_start, n + 1) | dev_alloc(ctx, ctx->d_ma_rev, n + 1) | dev_alloc(ctx, ctx->d_ma_coff, n + 1) |
            dev_alloc(ctx, ctx->d_ma_seq, chars + MA_REC_LANE) | dev_alloc(ctx, ctx->d_ma_smp, chars + MA_REC_LANE) | dev_alloc(ctx, d_irec, n_ins + 1) |
            dev_alloc(ctx, ctx->d_ma_ipos, n_ins + 1) | dev_alloc(ctx, ctx->d_ma_ioff, n_ins + 1) |
            dev_alloc(ctx, ctx->d_ma_ib, ins_chars + MA_REC_LANE) | dev_alloc(ctx, ctx->d_ma_gaps, ref_len) |
            dev_alloc(ctx, ctx->d_ma_rec_ins, n + 1) | dev_alloc(ctx, ctx->d_ma_ins_list, n_ins + 1) |
            dev_alloc(ctx, ctx->d_ma_colmap, (int64_t)ref_len + 1) | dev_alloc(ctx, ctx->d_ma_rows, n + 1) |
            dev_alloc(ctx, ctx->d_ma_ctl, (int64_t)MAR_STATE + n / MAR_PER_WG + 2);
  if (nomem) return MIA_HIP_ERR_NOMEM;
  ctx->ma_n = n;                                   // (nothing reads them before ma_resident is set again)
  ctx->ma_n_ins = n_ins;
  ctx->ma_L = ref_len;
  hipError_t e = hipSuccess;
  auto up = [&](void* d, const void* h, size_t b) { if (e == hipSuccess && b) e = hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, ctx->stream); };
  auto zero = [&](void* d, size_t b) { if (e == hipSuccess) e = hipMemsetAsync(d, 0, b, ctx->stream); };
  zero(ctx->tb.tally, (size_t)TALLY_WORDS * Lp * 4);
  zero(ctx->tb.gaps, (size_t)Lp * 4);
  zero(ctx->tb.n_events, 4);
  zero(ctx->tb.flags, 4);
  up(ctx->tb.gaps, gaps, (size_t)ref_len * 4);
  up(ctx->d_ma_start, start, (size_t)n * 4); up(ctx->d_ma_rev, revcom, (size_t)n); up(ctx->d_ma_coff, col_off, (size_t)(n + 1) * 8);
  up(ctx->d_ma_seq, seq, (size_t)chars); up(ctx->d_ma_smp, smp, (size_t)chars);
  if (n_ins) {
    up(d_irec, ins_record, (size_t)n_ins * 4); up(ctx->d_ma_ipos, ins_pos, (size_t)n_ins * 4); up(ctx->d_ma_ioff, ins_off, (size_t)(n_ins + 1) * 8);
    up(ctx->d_ma_ib, ins_bases, (size_t)ins_chars);
  }
  up(ctx->d_ma_gaps, gaps, (size_t)ref_len * 4);
  up(ctx->d_ma_rec_ins, rec_ins.data(), (size_t)(n + 1) * 4);
  up(ctx->d_ma_ins_list, ins_list.data(), (size_t)n_ins * 4);
  if (e == hipSuccess && n > 0) {
    const MaRecords mr = ma_records(ctx);
    if (stage_launch(ctx, STG_MA_TALLY, k_ma_tally, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, mr, (const int32_t*)ctx->d_pssm, ctx->tb))
      return MIA_HIP_ERR_NOMEM;
    if (n_ins > 0)
      hipLaunchKernelGGL(k_ma_ins_events, dim3((unsigned)((n_ins + 255) / 256)), dim3(256), 0, ctx->stream, mr, n_ins, d_irec, mr.ins_pos, mr.ins_off,
                         mr.ins_bases, ctx->tb);
    e = hipGetLastError();
  }
  uint32_t flags = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&ctx->n_events_host, ctx->tb.n_events, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&flags, ctx->tb.flags, 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { ctx->err = std::string("ma_tally: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  if (flags & 1u) { ctx->err = "insert event list overflow"; return MIA_HIP_ERR_NOMEM; }
  if (flags & 2u) { ctx->err = "a record reaches past the reference or carries a depth code outside A.._"; return MIA_HIP_ERR_ARG; }
  if (ctx->n_events_host > ctx->tb.cap_events) ctx->n_events_host = ctx->tb.cap_events;
  ctx->tallied = true;
  ctx->consensus_done = false;
  ctx->ma_resident = true;
  ctx->ma_tally_no++;
  ctx->ma_cols = n == 0 ? 0 : col_off[0] == 0 ? chars : -1;         // (mia_hip_ma_profile takes flat position 0 as record 0's first column)
  return MIA_HIP_OK;
}

// print_region's rows (src/map_align.c:660-750) for the records of the last mia_hip_ma_tally: see mia_ma_region_kernels.h
extern "C" int mia_hip_ma_region(mia_hip_ctx* ctx, int32_t first, int32_t last, int64_t* n_rows, int64_t* width) {
  if (!ctx || !n_rows || !width) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede ma_region"; return MIA_HIP_ERR_STATE; }
  if (first <= last && (first < 0 || last >= ctx->ma_L)) { ctx->err = "ma_region: the region reaches outside the reference"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ma_out.region_done = false;
  const int64_t n = ctx->ma_n;
  const int32_t n_wgs = (int32_t)((n + MAR_PER_WG - 1) / MAR_PER_WG);
  MaRegionView v{ma_records(ctx), ctx->d_ma_gaps, first, last, ctx->d_ma_colmap};
  HIPCHK(hipMemsetAsync(ctx->d_ma_ctl, 0, ((size_t)MAR_STATE + (size_t)n_wgs) * 8, ctx->stream));
  if (stage_launch(ctx, STG_MA_SELECT, k_ma_region_select, dim3((unsigned)n_wgs + 1), dim3(MAR_THREADS), 0, ctx->stream, v, n_wgs, ctx->d_ma_ctl,
                   ctx->d_ma_colmap, ctx->d_ma_rows))
    return MIA_HIP_ERR_NOMEM;
  HIPCHK(hipGetLastError());
  unsigned long long hdr[MAR_STATE] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(hdr, ctx->d_ma_ctl, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int64_t rows = (int64_t)hdr[MAR_ROWS], w = (int64_t)hdr[MAR_WIDTH];
  if (rows < 0 || rows > n || w < 0) { ctx->err = "ma_region: the selection came back inconsistent"; return MIA_HIP_ERR_DEVICE; }
  if (rows > 0 && w > 0) {
    if (w > INT64_MAX / rows) { ctx->err = "ma_region: the text does not fit"; return MIA_HIP_ERR_NOMEM; }
    if (dev_ensure(ctx, ctx->d_ma_text, rows * w)) return MIA_HIP_ERR_NOMEM;
    if (stage_launch(ctx, STG_MA_RENDER, k_ma_region_render, dim3((unsigned)((rows + MAR_THREADS / 64 - 1) / (MAR_THREADS / 64))), dim3(MAR_THREADS), 0,
                     ctx->stream, v, ctx->d_ma_rows, rows, w, ctx->d_ma_text))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  ctx->ma_out.first = first; ctx->ma_out.last = last; ctx->ma_out.rows = rows; ctx->ma_out.width = w;
  ctx->ma_out.region_done = true;
  *n_rows = rows;
  *width = w;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_region(mia_hip_ctx* ctx, int64_t* rows, char* text, int64_t cap_rows) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.region_done) { ctx->err = "ma_region first"; return MIA_HIP_ERR_STATE; }
  if (cap_rows < ctx->ma_out.rows) { ctx->err = "get_ma_region: buffers too small"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ma_down(ctx, rows, ctx->d_ma_rows, (size_t)ctx->ma_out.rows * 8));
  HIPCHK(ma_down(ctx, text, ctx->d_ma_text, (size_t)(ctx->ma_out.rows * ctx->ma_out.width)));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

// The read blocks of ace_output (src/io.c:807-889) for the records of the last mia_hip_ma_tally: see mia_ma_ace_kernels.h
extern "C" int mia_hip_ma_ace(mia_hip_ctx* ctx, int64_t* n_records, int64_t* body_bytes) {
  if (!ctx || !n_records || !body_bytes) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede ma_ace"; return MIA_HIP_ERR_STATE; }
  if (!ctx->ma_ace_gaps_ok) { ctx->err = "ma_ace: GAPS opens insert columns in front of column 0, or holds a negative value: no ACE export"; return MIA_HIP_ERR_ARG; }
  if (!ctx->ma_ace_cols_ok) { ctx->err = "ma_ace: a record reaches past the reference"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ma_out.ace_done = false;
  const int64_t n = ctx->ma_n;
  const int32_t L = ctx->ma_L, n_wgs = (int32_t)((n + MAR_PER_WG - 1) / MAR_PER_WG);
  if (dev_ensure(ctx, ctx->d_ace_g, (int64_t)L + 2) || dev_ensure(ctx, ctx->d_ace_af, n + 1) || dev_ensure(ctx, ctx->d_ace_len, n + 1) || dev_ensure(ctx, ctx->d_ace_off, n + 1))
    return MIA_HIP_ERR_NOMEM;
  MaAceView v{ma_records(ctx), ctx->d_ace_g};
  hipLaunchKernelGGL(k_ma_ace_gaps, dim3(1), dim3(MAA_SCAN_THREADS), 0, ctx->stream, (const int32_t*)ctx->d_ma_gaps, L, ctx->d_ace_g);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(ctx->d_ma_ctl, 0, ((size_t)MAR_STATE + (size_t)n_wgs) * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_ace_off, 0, 8, ctx->stream));         // (no records: the one offset there is)
  if (n_wgs > 0) {
    if (stage_launch(ctx, STG_MA_ACE_LAYOUT, k_ma_ace_layout, dim3((unsigned)n_wgs), dim3(MAR_THREADS), 0, ctx->stream, v, n_wgs, ctx->d_ma_ctl, ctx->d_ace_af,
                     ctx->d_ace_len, ctx->d_ace_off))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
  }
  unsigned long long hdr[MAR_STATE] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(hdr, ctx->d_ma_ctl, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int64_t bytes = (int64_t)hdr[MAR_ROWS];
  if (bytes < n) { ctx->err = "ma_ace: the layout came back inconsistent"; return MIA_HIP_ERR_DEVICE; }   // (a record's text holds a newline at least)
  if (n > 0) {
    if (dev_ensure(ctx, ctx->d_ace_body, bytes)) return MIA_HIP_ERR_NOMEM;
    if (stage_launch(ctx, STG_MA_ACE_RENDER, k_ma_ace_render, dim3((unsigned)((n + MAR_THREADS / 64 - 1) / (MAR_THREADS / 64))), dim3(MAR_THREADS), 0, ctx->stream, v,
                     (const int64_t*)ctx->d_ace_off, ctx->d_ace_body))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  ctx->ma_out.ace_bytes = bytes;
  ctx->ma_out.ace_done = true;
  *n_records = n;
  *body_bytes = bytes;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_ace(mia_hip_ctx* ctx, int64_t* af_pos, int64_t* padded_len, int64_t* body_off, char* body, int64_t cap_bytes) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.ace_done) { ctx->err = "ma_ace first"; return MIA_HIP_ERR_STATE; }
  if (body && cap_bytes < ctx->ma_out.ace_bytes) { ctx->err = "get_ma_ace: buffer too small"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->ma_n;
  HIPCHK(ma_down(ctx, af_pos, ctx->d_ace_af, (size_t)n * 8));
  HIPCHK(ma_down(ctx, padded_len, ctx->d_ace_len, (size_t)n * 8));
  HIPCHK(ma_down(ctx, body_off, ctx->d_ace_off, (size_t)(n + 1) * 8));
  HIPCHK(ma_down(ctx, body, ctx->d_ace_body, (size_t)ctx->ma_out.ace_bytes));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

// CIGAR, SEQ and NM of the SAM export (ma_hip -f 8) for the records of the last mia_hip_ma_tally: see mia_ma_sam_kernels.h
extern "C" int mia_hip_ma_sam(mia_hip_ctx* ctx, const char* ref_seq, int64_t* n_records, int64_t* body_bytes) {
  if (!ctx || !n_records || !body_bytes) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede ma_sam"; return MIA_HIP_ERR_STATE; }
  if (!ref_seq) { ctx->err = "ma_sam: no reference sequence"; return MIA_HIP_ERR_ARG; }
  if (!ctx->ma_sam_gaps_ok) { ctx->err = "ma_sam: GAPS holds a negative value"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ma_out.sam_done = false;
  const int64_t n = ctx->ma_n;
  const int32_t L = ctx->ma_L, n_wgs = (int32_t)((n + MAS_PER_WG - 1) / MAS_PER_WG);
  if (dev_ensure(ctx, ctx->d_sam_ref, (int64_t)L) || dev_ensure(ctx, ctx->d_sam_cum, ctx->ma_n_ins + n + 1) || dev_ensure(ctx, ctx->d_sam_nm, n + 1) ||
      dev_ensure(ctx, ctx->d_sam_cig, n + 1) || dev_ensure(ctx, ctx->d_sam_off, n + 1) || dev_ensure(ctx, ctx->d_sam_ctl, (int64_t)MAR_STATE + n_wgs + 1))
    return MIA_HIP_ERR_NOMEM;
  HIPCHK(hipMemcpyAsync(ctx->d_sam_ref, ref_seq, (size_t)L, hipMemcpyHostToDevice, ctx->stream));
  MaSamView v{ma_records(ctx), ctx->d_sam_ref, ctx->d_sam_cum};
  HIPCHK(hipMemsetAsync(ctx->d_sam_ctl, 0, ((size_t)MAR_STATE + (size_t)n_wgs) * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_sam_off, 0, 8, ctx->stream));         // (no records: the one offset there is)
  if (n_wgs > 0) {
    if (stage_launch(ctx, STG_MA_SAM_LAYOUT, k_ma_sam_layout, dim3((unsigned)n_wgs), dim3(MAS_THREADS), 0, ctx->stream, v, n_wgs, ctx->d_sam_ctl, ctx->d_sam_nm,
                     ctx->d_sam_cig, ctx->d_sam_off))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
  }
  unsigned long long hdr[MAR_STATE] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(hdr, ctx->d_sam_ctl, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int64_t bytes = (int64_t)hdr[MAR_ROWS];
  if (bytes < n * MA_SAM_EMPTY_BYTES) { ctx->err = "ma_sam: the layout came back inconsistent"; return MIA_HIP_ERR_DEVICE; }   // (no body is shorter than that of a record without SEQ)
  if (n > 0) {
    if (dev_ensure(ctx, ctx->d_sam_body, bytes)) return MIA_HIP_ERR_NOMEM;
    if (stage_launch(ctx, STG_MA_SAM_RENDER, k_ma_sam_render, dim3((unsigned)((n + MAS_WAVES - 1) / MAS_WAVES)), dim3(MAS_THREADS), 0, ctx->stream, v,
                     (const int64_t*)ctx->d_sam_cig, (const int64_t*)ctx->d_sam_off, ctx->d_sam_body))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  ctx->ma_out.sam_bytes = bytes;
  ctx->ma_out.sam_done = true;
  *n_records = n;
  *body_bytes = bytes;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_sam(mia_hip_ctx* ctx, int32_t* nm, int64_t* body_off, char* body, int64_t cap_bytes) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.sam_done) { ctx->err = "ma_sam first"; return MIA_HIP_ERR_STATE; }
  if (body && cap_bytes < ctx->ma_out.sam_bytes) { ctx->err = "get_ma_sam: buffer too small"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->ma_n;
  HIPCHK(ma_down(ctx, nm, ctx->d_sam_nm, (size_t)n * 4));
  HIPCHK(ma_down(ctx, body_off, ctx->d_sam_off, (size_t)(n + 1) * 8));
  HIPCHK(ma_down(ctx, body, ctx->d_sam_body, (size_t)ctx->ma_out.sam_bytes));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

// The substitution profile (ma_hip -f 9, -f 91) of the records of the last mia_hip_ma_tally: see mia_ma_profile_kernels.h
extern "C" int mia_hip_ma_profile(mia_hip_ctx* ctx, const char* ref_seq, const uint8_t* use, int64_t* n_used, int64_t* n_events) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede ma_profile"; return MIA_HIP_ERR_STATE; }
  if (!ref_seq) { ctx->err = "ma_profile: no reference sequence"; return MIA_HIP_ERR_ARG; }
  if (ctx->ma_n > 0 && ctx->ma_cols < 0) { ctx->err = "ma_profile: col_off[0] of the tallied records is not 0"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ma_out.prof_done = false;
  const int64_t n = ctx->ma_n, T = ctx->ma_cols;
  const int32_t L = ctx->ma_L;
  MaSelection sel;
  if (dev_ensure(ctx, ctx->d_prof_ref, (int64_t)L) || dev_ensure(ctx, ctx->d_prof_bins, MA_PROF_BINS)) return MIA_HIP_ERR_NOMEM;
  if (const int rc = ma_selection(ctx, nullptr, use, &sel)) return rc;
  HIPCHK(hipMemcpyAsync(ctx->d_prof_ref, ref_seq, (size_t)L, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_prof_bins, 0, (size_t)MA_PROF_BINS * 8, ctx->stream));
  if (n > 0) {                                              // (records that all lack columns: one workgroup that finds no chunk)
    MaFlatView v{ma_records(ctx), T, ctx->d_prof_ref, sel.use};
    if (stage_launch(ctx, STG_MA_PROFILE, k_ma_profile, ma_grid(ctx, ma_prof_chunks(T), MAP_WGS_PER_CU), dim3(MAP_THREADS), 0, ctx->stream, v, (unsigned long long*)ctx->d_prof_bins))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(ctx->ma_prof_bins, ctx->d_prof_bins, (size_t)MA_PROF_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int64_t events = 0;
  for (int b = 0; b < MA_PROF_BINS; b++) events += ctx->ma_prof_bins[b];
  ctx->ma_out.prof_done = true;
  if (n_used) *n_used = sel.used;
  if (n_events) *n_events = events;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_profile(mia_hip_ctx* ctx, int64_t* count, int64_t* del, int64_t* bad_code, int64_t* beyond) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.prof_done) { ctx->err = "ma_profile first"; return MIA_HIP_ERR_STATE; }
  if (count) memcpy(count, ctx->ma_prof_bins, sizeof(int64_t) * MA_PROF_COUNTS);
  if (del) memcpy(del, ctx->ma_prof_bins + MA_PROF_DEL, sizeof(int64_t) * MA_PROF_DEPTHS);
  if (bad_code) *bad_code = ctx->ma_prof_bins[MA_PROF_BAD];
  if (beyond) *beyond = ctx->ma_prof_bins[MA_PROF_BEYOND];
  return MIA_HIP_OK;
}

// Fragment-end context and read lengths (ma_hip -f 92, -f 93) of the records of the last mia_hip_ma_tally: see mia_ma_ends_kernels.h.
// Columns, strands and the INS_POS pairs by record are on the device already; the reference, the segments and the selection go up.
extern "C" int mia_hip_ma_ends(mia_hip_ctx* ctx, const char* ref_seq, const uint8_t* segment, const uint8_t* use, int64_t* n_used,
                               int64_t* n_ends5, int64_t* n_ends3) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede ma_ends"; return MIA_HIP_ERR_STATE; }
  if (!ref_seq) { ctx->err = "ma_ends: no reference sequence"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ma_out.ends_done = false;
  const int64_t n = ctx->ma_n;
  const int32_t L = ctx->ma_L;
  MaSelection sel;
  if (dev_ensure(ctx, ctx->d_prof_ref, (int64_t)L) || dev_ensure(ctx, ctx->d_ends_bins, MA_ENDS_BINS)) return MIA_HIP_ERR_NOMEM;
  if (const int rc = ma_selection(ctx, segment, use, &sel)) return rc;
  HIPCHK(hipMemcpyAsync(ctx->d_prof_ref, ref_seq, (size_t)L, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->d_ends_bins, 0, (size_t)MA_ENDS_BINS * 8, ctx->stream));
  if (n > 0) {
    MaEndsView v{ma_records(ctx), ctx->d_prof_ref, sel.segment, sel.use};
    if (stage_launch(ctx, STG_MA_ENDS, k_ma_ends, ma_grid(ctx, ma_ends_chunks(n), MAE_WGS_PER_CU), dim3(MAE_THREADS), 0, ctx->stream, v, (unsigned long long*)ctx->d_ends_bins))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(ctx->ma_ends_bins, ctx->d_ends_bins, (size_t)MA_ENDS_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int64_t ends[2] = {0, 0};
  for (int end = 0; end < 2; end++)                          // every end adds one event to each of its 20 positions: count position 0
    for (int c = 0; c < MA_ENDS_CLASSES; c++) ends[end] += ctx->ma_ends_bins[ma_ends_ctx_bin(end, 0, c)];
  ctx->ma_out.ends_done = true;
  if (n_used) *n_used = sel.used;
  if (n_ends5) *n_ends5 = ends[0];
  if (n_ends3) *n_ends3 = ends[1];
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_ends(mia_hip_ctx* ctx, int64_t* ctx_count, int64_t* len_count, int64_t* halves) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.ends_done) { ctx->err = "ma_ends first"; return MIA_HIP_ERR_STATE; }
  if (ctx_count) memcpy(ctx_count, ctx->ma_ends_bins, sizeof(int64_t) * MA_ENDS_CTX);
  if (len_count) memcpy(len_count, ctx->ma_ends_bins + MA_ENDS_LEN, sizeof(int64_t) * 2 * MA_ENDS_LENS);
  if (halves) *halves = ctx->ma_ends_bins[MA_ENDS_HALVES];
  return MIA_HIP_OK;
}

// The strand-split column table (ma_hip -f 42) of the records of the last mia_hip_ma_tally: see mia_ma_cols_kernels.h.  Columns and
// strands are on the device already; only the segments and the selection go up (no reference characters: the pass does not need them).
extern "C" int mia_hip_ma_cols(mia_hip_ctx* ctx, const uint8_t* segment, const uint8_t* use, int64_t* n_used, int64_t* n_events, int64_t* beyond,
                               int64_t* ends_outside) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede ma_cols"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->ma_out.cols_done = false;
  const int64_t n = ctx->ma_n, words = (int64_t)MA_COLS_WORDS * ctx->ma_L;
  const int32_t L = ctx->ma_L;
  unsigned long long out[2] = {0, 0};
  ctx->ma_cols_tab.assign((size_t)words, 0);
  MaSelection sel;
  if (const int rc = ma_selection(ctx, segment, use, &sel)) return rc;
  if (n > 0) {                                               // without records there is no launch and the table is zero
    if (dev_ensure(ctx, ctx->d_cols_tab, words) || dev_ensure(ctx, ctx->d_cols_out, 2)) return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemsetAsync(ctx->d_cols_tab, 0, (size_t)words * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_cols_out, 0, sizeof out, ctx->stream));
    MaColsView v{ma_records(ctx), sel.segment, sel.use};
    // persistent grid over (tile, slice) jobs: the workgroups that are resident at once, or one per job when there are fewer
    const int64_t wgs = (int64_t)ctx->cus * MAC_WGS_PER_CU, slices = ma_cols_slices(n, L, wgs), per_slice = (n + slices - 1) / slices;
    if (stage_launch(ctx, STG_MA_COLS, k_ma_cols, ma_grid(ctx, ma_cols_tiles(L) * slices, MAC_WGS_PER_CU), dim3(MAC_THREADS), 0, ctx->stream, v, slices, per_slice, (uint32_t*)ctx->d_cols_tab,
                     (unsigned long long*)ctx->d_cols_out))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctx->ma_cols_tab.data(), ctx->d_cols_tab, (size_t)words * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(out, ctx->d_cols_out, sizeof out, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  int64_t events = (int64_t)out[0];
  for (int64_t i = 0; i < (int64_t)MA_COLS_STARTS * L; i++) events += ctx->ma_cols_tab[(size_t)i];       // words 0 .. 11 of every column
  ctx->ma_out.cols_done = true;
  if (n_used) *n_used = sel.used;
  if (n_events) *n_events = events;
  if (beyond) *beyond = (int64_t)out[0];
  if (ends_outside) *ends_outside = (int64_t)out[1];
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_cols(mia_hip_ctx* ctx, int32_t* cols) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.cols_done) { ctx->err = "ma_cols first"; return MIA_HIP_ERR_STATE; }
  if (cols) memcpy(cols, ctx->ma_cols_tab.data(), ctx->ma_cols_tab.size() * sizeof(int32_t));
  return MIA_HIP_OK;
}

// The duplicate filter (ma_hip -u, -t): see mia_ma_dedup_kernels.h.  Independent of mia_hip_ma_tally: it takes the records'
// coordinates, strands, scores and the pairing of the halves, and leaves keep, rep and the size histogram in buffers of its own.
extern "C" int mia_hip_ma_dedup(mia_hip_ctx* ctx, int32_t ref_len, int64_t n_records, const int32_t* start, const int32_t* end, const uint8_t* revcom,
                                const int32_t* score, const int64_t* mate, int32_t tolerance, int64_t* n_molecules, int64_t* n_clusters) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  auto& dd = ctx->dedup;
  dd.done = false;
  ctx->collapse.done = false;
  if (tolerance < 0 || tolerance > MA_DEDUP_MAX_TOL) { ctx->err = "ma_dedup: the tolerance must lie in 0 .. 100"; return MIA_HIP_ERR_ARG; }
  if (ref_len < 1 || ref_len > MA_DEDUP_MAX_L) { ctx->err = "ma_dedup: reference length out of range"; return MIA_HIP_ERR_ARG; }
  if (n_records < 0 || n_records >= ((int64_t)1 << 31)) { ctx->err = "ma_dedup: record count out of range"; return MIA_HIP_ERR_ARG; }
  const int64_t n = n_records;
  const int32_t L = ref_len;
  if (n > 0 && (!start || !end || !revcom || !score)) { ctx->err = "ma_dedup: null array"; return MIA_HIP_ERR_ARG; }
  int64_t M = 0, orphans = 0;
  for (int64_t r = 0; r < n; r++) {
    if (start[r] < 0 || (int64_t)end[r] < (int64_t)start[r] - 1 || (int64_t)end[r] >= 2ll * L) { ctx->err = "ma_dedup: a record's START or END is out of range"; return MIA_HIP_ERR_ARG; }
    if (!ma_mate_record_ok(mate, n, r)) { ctx->err = "ma_dedup: mate is out of range, the record itself or not mutual"; return MIA_HIP_ERR_ARG; }
    const int64_t m = mate ? mate[r] : MA_MOL_NONE;
    if (m == MA_MOL_ORPHAN) { orphans++; continue; }
    if (m == MA_MOL_NONE || ma_dedup_front(start, r, m)) { M++; continue; }
    if (end[r] >= L) { ctx->err = "ma_dedup: the back half of a pair ends behind the reference"; return MIA_HIP_ERR_ARG; }
  }
  dd.n = n; dd.molecules = M; dd.orphans = orphans; dd.clusters = 0;
  dd.sorted_side = 0; dd.runs = 0; dd.has_mate = mate != nullptr; dd.L = L; dd.tally_no = ctx->ma_resident ? ctx->ma_tally_no : 0;
  memset(dd.hist, 0, sizeof dd.hist);
  if (n > 0) {
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ma_dedup_width(L), passes = ma_dedup_passes(L);
    const int64_t sort_wgs = ma_dedup_sort_wgs(n), scan_wgs = ma_dedup_wgs(n);
    int rc = dev_ensure(ctx, dd.d_start, n) | dev_ensure(ctx, dd.d_end, n) | dev_ensure(ctx, dd.d_score, n) | dev_ensure(ctx, dd.d_rc, n);
    rc |= dev_ensure(ctx, dd.d_keep, n) | dev_ensure(ctx, dd.d_rep, n) | dev_ensure(ctx, dd.d_hist, MA_DEDUP_HIST);
    if (mate) rc |= dev_ensure(ctx, dd.d_mate, n);
    for (int b = 0; b < 2; b++) rc |= dev_ensure(ctx, dd.d_key[b], n) | dev_ensure(ctx, dd.d_val[b], n) | dev_ensure(ctx, dd.d_jump[b], n + 1);
    rc |= dev_ensure(ctx, dd.d_counts, MAD_RADIX * sort_wgs) | dev_ensure(ctx, dd.d_ctl, MAR_STATE + scan_wgs);
    rc |= dev_ensure(ctx, dd.d_runid, n) | dev_ensure(ctx, dd.d_first, n + 1) | dev_ensure(ctx, dd.d_runkey, n) | dev_ensure(ctx, dd.d_best, n);
    rc |= dev_ensure(ctx, dd.d_mark, n) | dev_ensure(ctx, dd.d_cluster, n) | dev_ensure(ctx, dd.d_anchor, n + 1);
    if (rc) return MIA_HIP_ERR_NOMEM;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dd.d_start, start, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dd.d_end, end, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dd.d_score, score, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dd.d_rc, revcom, (size_t)n, hipMemcpyHostToDevice, s));
    if (mate) HIPCHK(hipMemcpyAsync(dd.d_mate, mate, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dd.d_hist, 0, (size_t)MA_DEDUP_HIST * 8, s));
    const int64_t* d_mate = mate ? (const int64_t*)dd.d_mate : nullptr;
    auto grid_for = [&](int64_t items) { return ma_grid(ctx, ma_dedup_wgs(items), MAD_WGS_PER_CU); };
    if (stage_launch(ctx, STG_MA_DEDUP_KEYS, k_ma_dedup_keys, grid_for(n), dim3(MAD_THREADS), 0, s, n, L, W, (const int32_t*)dd.d_start, (const int32_t*)dd.d_end,
                     (const uint8_t*)dd.d_rc, d_mate, (unsigned long long*)dd.d_key[0], (uint32_t*)dd.d_val[0], (uint8_t*)dd.d_keep, (int64_t*)dd.d_rep))
      return MIA_HIP_ERR_NOMEM;
    int cur = 0;
    for (int p = 0; p < passes; p++, cur ^= 1) {
      if (stage_launch(ctx, STG_MA_DEDUP_SORT, k_ma_dedup_sort_count, dim3((unsigned)sort_wgs), dim3(MAD_THREADS), 0, s, (const unsigned long long*)dd.d_key[cur], n,
                       8 * p, (uint32_t*)dd.d_counts, sort_wgs) ||
          stage_launch(ctx, STG_MA_DEDUP_SORT, k_ma_dedup_sort_scan, dim3(1), dim3(MAD_THREADS), 0, s, (uint32_t*)dd.d_counts, (int64_t)MAD_RADIX * sort_wgs) ||
          stage_launch(ctx, STG_MA_DEDUP_SORT, k_ma_dedup_sort_scatter, dim3((unsigned)sort_wgs), dim3(MAD_THREADS), 0, s, (const unsigned long long*)dd.d_key[cur],
                       (const uint32_t*)dd.d_val[cur], (unsigned long long*)dd.d_key[cur ^ 1], (uint32_t*)dd.d_val[cur ^ 1], n, 8 * p,
                       (const uint32_t*)dd.d_counts, sort_wgs))
        return MIA_HIP_ERR_NOMEM;
    }
    HIPCHK(hipGetLastError());
    const unsigned long long* sk = dd.d_key[cur];
    const uint32_t* sm = dd.d_val[cur];
    dd.sorted_side = cur;
    if (M > 0) {
      const int64_t run_wgs = ma_dedup_wgs(M);
      HIPCHK(hipMemsetAsync(dd.d_ctl, 0, (size_t)(MAR_STATE + run_wgs) * 8, s));
      HIPCHK(hipMemsetAsync(dd.d_best, 0, (size_t)M * 8, s));
      if (stage_launch(ctx, STG_MA_DEDUP_RUNS, k_ma_dedup_runs, dim3((unsigned)run_wgs), dim3(MAD_THREADS), 0, s, sk, sm, M, (const int32_t*)dd.d_score, d_mate,
                       (unsigned long long*)dd.d_ctl, (int32_t)run_wgs, (uint32_t*)dd.d_runid, (uint32_t*)dd.d_first, (unsigned long long*)dd.d_runkey,
                       (unsigned long long*)dd.d_best))
        return MIA_HIP_ERR_NOMEM;
      unsigned long long runs = 0;
      HIPCHK(hipMemcpyAsync(&runs, dd.d_ctl + MAR_ROWS, 8, hipMemcpyDeviceToHost, s));     // the one read-back: the round count hangs on it
      HIPCHK(hipStreamSynchronize(s));
      const int64_t R = (int64_t)runs;
      if (R < 1 || R > M) { ctx->err = "ma_dedup: the run count came back inconsistent"; return MIA_HIP_ERR_DEVICE; }
      dd.runs = R;
      if (stage_launch(ctx, STG_MA_DEDUP_NEXT, k_ma_dedup_next, grid_for(R + 1), dim3(MAD_THREADS), 0, s, (const unsigned long long*)dd.d_runkey, R, W, tolerance,
                       (uint32_t*)dd.d_jump[0], (uint32_t*)dd.d_mark))
        return MIA_HIP_ERR_NOMEM;
      int jc = 0;
      for (int round = 0; round < ma_dedup_rounds(R); round++, jc ^= 1)
        if (stage_launch(ctx, STG_MA_DEDUP_ANCHORS, k_ma_dedup_double, grid_for(R + 1), dim3(MAD_THREADS), 0, s, (const uint32_t*)dd.d_jump[jc],
                         (uint32_t*)dd.d_jump[jc ^ 1], (uint32_t*)dd.d_mark, R))
          return MIA_HIP_ERR_NOMEM;
      const int64_t cl_wgs = ma_dedup_wgs(R);
      HIPCHK(hipMemsetAsync(dd.d_ctl, 0, (size_t)(MAR_STATE + cl_wgs) * 8, s));
      if (stage_launch(ctx, STG_MA_DEDUP_CLUSTERS, k_ma_dedup_cluster_scan, dim3((unsigned)cl_wgs), dim3(MAD_THREADS), 0, s, (const uint32_t*)dd.d_mark, R,
                       (unsigned long long*)dd.d_ctl, (int32_t)cl_wgs, (uint32_t*)dd.d_cluster, (uint32_t*)dd.d_anchor) ||
          stage_launch(ctx, STG_MA_DEDUP_CLUSTERS, k_ma_dedup_hist, grid_for(R), dim3(MAD_THREADS), 0, s, (const uint32_t*)dd.d_anchor,
                       (const unsigned long long*)dd.d_ctl, (const uint32_t*)dd.d_first, (const unsigned long long*)dd.d_runkey, W, (unsigned long long*)dd.d_hist) ||
          stage_launch(ctx, STG_MA_DEDUP_CLUSTERS, k_ma_dedup_scatter, grid_for(M), dim3(MAD_THREADS), 0, s, sm, M, (const uint32_t*)dd.d_runid,
                       (const uint32_t*)dd.d_cluster, (const uint32_t*)dd.d_anchor, (const unsigned long long*)dd.d_best, d_mate, (uint8_t*)dd.d_keep,
                       (int64_t*)dd.d_rep))
        return MIA_HIP_ERR_NOMEM;
      HIPCHK(hipGetLastError());
      unsigned long long clusters = 0;
      HIPCHK(hipMemcpyAsync(&clusters, dd.d_ctl + MAR_ROWS, 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(dd.hist, dd.d_hist, sizeof dd.hist, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      dd.clusters = (int64_t)clusters;
    } else {
      HIPCHK(hipStreamSynchronize(s));
    }
    drain_events(ctx);                      // (some forty launches a call: their event pairs go back to the free list now)
  }
  dd.done = true;
  if (n_molecules) *n_molecules = dd.molecules;
  if (n_clusters) *n_clusters = dd.clusters;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_dedup(mia_hip_ctx* ctx, uint8_t* keep, int64_t* rep, int64_t* size_hist, int64_t* orphans) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  auto& dd = ctx->dedup;
  if (!dd.done) { ctx->err = "ma_dedup first"; return MIA_HIP_ERR_STATE; }
  if (dd.n > 0 && (keep || rep)) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ma_down(ctx, keep, dd.d_keep, (size_t)dd.n));
    HIPCHK(ma_down(ctx, rep, dd.d_rep, (size_t)dd.n * 8));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  if (size_hist) memcpy(size_hist, dd.hist, sizeof dd.hist);
  if (orphans) *orphans = dd.orphans;
  return MIA_HIP_OK;
}

// The duplicate consensus (ma_hip -u -j, -f 98): see mia_ma_collapse_kernels.h.  Everything it reads is on the device already -- the
// tallied records and what mia_hip_ma_dedup left --; rec_of and vote go up, SEQ' and members stay there until mia_hip_get_ma_collapse.
extern "C" int mia_hip_ma_collapse(mia_hip_ctx* ctx, const int64_t* rec_of, const uint8_t* vote, int64_t* n_collapsed, int64_t* n_changed) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  auto& cc = ctx->collapse;
  auto& dd = ctx->dedup;
  cc.done = false;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede ma_collapse"; return MIA_HIP_ERR_STATE; }
  if (!dd.done) { ctx->err = "ma_dedup must precede ma_collapse"; return MIA_HIP_ERR_STATE; }
  if (dd.tally_no != ctx->ma_tally_no) { ctx->err = "ma_collapse: the last ma_dedup is older than the last ma_tally"; return MIA_HIP_ERR_STATE; }
  if (dd.n != ctx->ma_n) { ctx->err = "ma_collapse: ma_dedup and ma_tally were given different numbers of records"; return MIA_HIP_ERR_ARG; }
  if (ctx->ma_n > 0 && ctx->ma_cols < 0) { ctx->err = "ma_collapse: col_off[0] of the tallied records is not 0"; return MIA_HIP_ERR_ARG; }
  const int64_t n = ctx->ma_n, T = ctx->ma_cols, M = dd.molecules, C = dd.clusters;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  std::vector<int32_t> rec32;
  if (n > 0) {
    // rec_of is a permutation, and every record of the filter has the coordinates of the tallied record it names
    std::vector<int32_t> d_start((size_t)n), d_end((size_t)n), t_start((size_t)n);
    std::vector<int64_t> t_off((size_t)n + 1);
    HIPCHK(hipMemcpyAsync(d_start.data(), dd.d_start, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(d_end.data(), dd.d_end, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(t_start.data(), ctx->d_ma_start, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(t_off.data(), ctx->d_ma_coff, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<uint8_t> seen(rec_of ? (size_t)n : 0, 0);
    if (rec_of) rec32.resize((size_t)n);
    for (int64_t f = 0; f < n; f++) {
      const int64_t r = rec_of ? rec_of[f] : f;
      if (r < 0 || r >= n || (rec_of && seen[(size_t)r])) { ctx->err = "ma_collapse: rec_of is no permutation of the tallied records"; return MIA_HIP_ERR_ARG; }
      if (rec_of) { seen[(size_t)r] = 1; rec32[(size_t)f] = (int32_t)r; }
      if (d_start[(size_t)f] != t_start[(size_t)r] || (int64_t)d_end[(size_t)f] != (int64_t)t_start[(size_t)r] + (t_off[(size_t)r + 1] - t_off[(size_t)r]) - 1) {
        ctx->err = "ma_collapse: a record's START or END as ma_dedup was given it disagrees with the tallied record's start + columns - 1";
        return MIA_HIP_ERR_ARG;
      }
    }
  }
  cc.n = n; cc.cols = T; cc.collapsed = cc.changed = 0; cc.launched = false;
  memset(cc.hist, 0, sizeof cc.hist);
  const int64_t lone = dd.hist[ma_dedup_size_bin(true, 1)] + dd.hist[ma_dedup_size_bin(false, 1)];
  if (n > 0 && M > 0 && C > lone) {                          // without a cluster of two or more nothing is launched and SEQ' is SEQ
    const int32_t n_wgs = (int32_t)ma_collapse_wgs(C);
    const int64_t words = (T + MA_REC_LANE - 1) / MA_REC_LANE;
    if (dev_ensure(ctx, cc.d_rep_f, C) || dev_ensure(ctx, cc.d_rep_b, C) || dev_ensure(ctx, cc.d_cnt_off, C + 1) || dev_ensure(ctx, cc.d_members, n) ||
        dev_ensure(ctx, cc.d_seq, (words + 1) * MA_REC_LANE) || dev_ensure(ctx, cc.d_ctl, (int64_t)MAR_STATE + n_wgs) || dev_ensure(ctx, cc.d_hist, MA_COL_HIST) ||
        (rec_of && dev_ensure(ctx, cc.d_rec_of, n)) || (vote && dev_ensure(ctx, cc.d_vote, n)))
      return MIA_HIP_ERR_NOMEM;
    if (rec_of) HIPCHK(hipMemcpyAsync(cc.d_rec_of, rec32.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (vote) HIPCHK(hipMemcpyAsync(cc.d_vote, vote, (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(cc.d_members, 0, (size_t)n * 4, s));
    HIPCHK(hipMemsetAsync(cc.d_hist, 0, (size_t)MA_COL_HIST * 8, s));
    HIPCHK(hipMemsetAsync(cc.d_ctl, 0, (size_t)(MAR_STATE + n_wgs) * 8, s));
    const MaRecords v = ma_records(ctx);
    const MaColDedup d{M, C, dd.d_val[dd.sorted_side], dd.d_runid, dd.d_first, dd.d_cluster, dd.d_anchor, dd.d_best, dd.has_mate ? (const int64_t*)dd.d_mate : nullptr,
                       dd.d_start, rec_of ? (const int32_t*)cc.d_rec_of : nullptr, vote ? (const uint8_t*)cc.d_vote : nullptr};
    auto grid_for = [&](int64_t wgs) { return ma_grid(ctx, wgs, MAJ_WGS_PER_CU); };
    if (stage_launch(ctx, STG_MA_COLLAPSE_PLAN, k_ma_collapse_copy, grid_for(ma_collapse_wgs(words)), dim3(MAJ_THREADS), 0, s, v.seq, (char*)cc.d_seq, words) ||
        stage_launch(ctx, STG_MA_COLLAPSE_PLAN, k_ma_collapse_plan, dim3((unsigned)n_wgs), dim3(MAJ_THREADS), 0, s, v, d, (unsigned long long*)cc.d_ctl, n_wgs,
                     (int32_t*)cc.d_rep_f, (int32_t*)cc.d_rep_b, (int64_t*)cc.d_cnt_off, (int32_t*)cc.d_members, (unsigned long long*)cc.d_hist))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    unsigned long long total = 0;
    HIPCHK(hipMemcpyAsync(&total, cc.d_ctl + MAR_ROWS, 8, hipMemcpyDeviceToHost, s));      // the one read-back: the count array's size hangs on it
    HIPCHK(hipStreamSynchronize(s));
    const int64_t Q = (int64_t)total;
    if (Q < 0 || Q > T) { ctx->err = "ma_collapse: the plan came back inconsistent"; return MIA_HIP_ERR_DEVICE; }
    if (dev_ensure(ctx, cc.d_cnt, Q * MA_COL_CLASSES + 1)) return MIA_HIP_ERR_NOMEM;
    if (Q > 0) HIPCHK(hipMemsetAsync(cc.d_cnt, 0, (size_t)Q * MA_COL_CLASSES * 4, s));
    if (stage_launch(ctx, STG_MA_COLLAPSE_COUNT, k_ma_collapse_count, grid_for((ma_col_chunks(M) + MAJ_WAVES - 1) / MAJ_WAVES), dim3(MAJ_THREADS), 0, s, v, d,
                     (const int32_t*)cc.d_rep_f, (const int32_t*)cc.d_rep_b, (const int64_t*)cc.d_cnt_off, (uint32_t*)cc.d_cnt, (char*)cc.d_seq,
                     (unsigned long long*)cc.d_hist))
      return MIA_HIP_ERR_NOMEM;
    if (Q > 0 && stage_launch(ctx, STG_MA_COLLAPSE_DECIDE, k_ma_collapse_decide, grid_for(ma_collapse_wgs(Q)), dim3(MAJ_THREADS), 0, s, v, d, (const int32_t*)cc.d_rep_f,
                              (const int32_t*)cc.d_rep_b, (const int64_t*)cc.d_cnt_off, (const uint32_t*)cc.d_cnt, Q, (char*)cc.d_seq, (unsigned long long*)cc.d_hist))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cc.hist, cc.d_hist, sizeof cc.hist, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    drain_events(ctx);
    cc.launched = true;
    for (int b = 0; b < 2 * MA_COL_SIZE_BINS; b++) {
      const int64_t* row = cc.hist + b * MA_COL_COUNTS;
      for (int k = 0; k < MA_COL_COUNTS; k++) if (row[k] < 0) { ctx->err = "ma_collapse: the counts came back inconsistent"; return MIA_HIP_ERR_DEVICE; }
      cc.collapsed += row[MA_COL_CLUSTERS];
      cc.changed += row[MA_COL_TO_BASE] + row[MA_COL_TO_GAP] + row[MA_COL_TO_N];
    }
  }
  cc.done = true;
  if (n_collapsed) *n_collapsed = cc.collapsed;
  if (n_changed) *n_changed = cc.changed;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_collapse(mia_hip_ctx* ctx, char* seq, int64_t cap_bytes, int32_t* members, int64_t* hist) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  auto& cc = ctx->collapse;
  if (!ctx->ma_resident || !ctx->dedup.done || !cc.done) { ctx->err = "ma_collapse first"; return MIA_HIP_ERR_STATE; }
  if (seq && cap_bytes < cc.cols) { ctx->err = "get_ma_collapse: buffer too small"; return MIA_HIP_ERR_ARG; }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(ma_down(ctx, seq, cc.launched ? (const char*)cc.d_seq : (const char*)ctx->d_ma_seq, (size_t)cc.cols));
  if (cc.launched) HIPCHK(ma_down(ctx, members, cc.d_members, (size_t)cc.n * 4));
  else if (members && cc.n > 0) memset(members, 0, (size_t)cc.n * 4);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (hist) memcpy(hist, cc.hist, sizeof cc.hist);
  return MIA_HIP_OK;
}

// The deaminated-fragment filter (ma_hip -D, -e, -S, -f 95) of the records of the last mia_hip_ma_tally: see mia_ma_damage_kernels.h.
// Columns, depth codes and strands are on the device already; the reference, the selection and the pairing go up.
extern "C" int mia_hip_ma_damage(mia_hip_ctx* ctx, const char* ref_seq, const uint8_t* use, const int64_t* mate, int32_t n_pos, int32_t single_stranded,
                                 int32_t ends_mode, int64_t* n_molecules, int64_t* n_kept) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  ctx->ma_out.damage_done = false;
  auto& dg = ctx->damage;
  const char* const own_error = !ma_dmg_pos_ok(n_pos)      ? "the number of positions must lie in 1 .. 15"
                                : !ma_dmg_mode_ok(ends_mode) ? "the ends mode must be 0 (any), 1 (5'), 2 (3') or 3 (both)"
                                                             : nullptr;
  MaMolFrame f;
  if (const int rc = ma_mol_frame(ctx, "ma_damage", ref_seq, use, mate, own_error, dg.d_mate, ma_dmg_chunks(ctx->ma_cols), ma_dmg_record_wgs(ctx->ma_n),
                                  MAG_WGS_PER_CU, &f))
    return rc;
  const int64_t n = ctx->ma_n;
  memset(dg.bins, 0, sizeof dg.bins);
  if (n > 0) {                                               // without records there is no launch and every result is zero
    if (dev_ensure(ctx, dg.d_hit, 2 * n) || dev_ensure(ctx, dg.d_pos, 2 * n) || dev_ensure(ctx, dg.d_keep, n) || dev_ensure(ctx, dg.d_bins, MA_DMG_BINS))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemsetAsync(dg.d_hit, 0, (size_t)n * 2 * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(dg.d_keep, 0, (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(dg.d_bins, 0, (size_t)MA_DMG_BINS * 8, ctx->stream));
    if (stage_launch(ctx, STG_MA_DAMAGE_HITS, k_ma_damage_hits, f.col_grid, dim3(MAG_THREADS), 0, ctx->stream, f.v, single_stranded ? 1 : 0, (uint32_t*)dg.d_hit,
                     (uint32_t*)dg.d_hit + n))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    MaDmgMolView mv{n, f.v.revcom, f.v.use, f.mate, (const uint32_t*)dg.d_hit, (const uint32_t*)dg.d_hit + n, n_pos, ends_mode,
                    (uint8_t*)dg.d_pos, (uint8_t*)dg.d_pos + n, (uint8_t*)dg.d_keep};
    if (stage_launch(ctx, STG_MA_DAMAGE_MOLECULES, k_ma_damage_molecules, f.rec_grid, dim3(MAG_THREADS), 0, ctx->stream, mv, (unsigned long long*)dg.d_bins))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dg.bins, dg.d_bins, (size_t)MA_DMG_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  int64_t molecules = 0;
  for (int b = 0; b < MA_DMG_HIST; b++) molecules += dg.bins[b];
  ctx->ma_out.damage_done = true;
  if (n_molecules) *n_molecules = molecules;
  if (n_kept) *n_kept = dg.bins[MA_DMG_KEPT];
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_damage(mia_hip_ctx* ctx, uint8_t* pos5, uint8_t* pos3, uint8_t* keep, int64_t* hist, int64_t* orphans) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.damage_done) { ctx->err = "ma_damage first"; return MIA_HIP_ERR_STATE; }
  const int64_t n = ctx->ma_n;
  auto& dg = ctx->damage;
  if (n > 0 && (pos5 || pos3 || keep)) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ma_down(ctx, pos5, dg.d_pos, (size_t)n));
    HIPCHK(ma_down(ctx, pos3, dg.d_pos + n, (size_t)n));
    HIPCHK(ma_down(ctx, keep, dg.d_keep, (size_t)n));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  if (hist) memcpy(hist, dg.bins, sizeof(int64_t) * MA_DMG_HIST);
  if (orphans) *orphans = dg.bins[MA_DMG_ORPHANS];
  return MIA_HIP_OK;
}

// The end mask (ma_hip -E, -x, -f 96) of the records of the last mia_hip_ma_tally: see mia_ma_mask_kernels.h.  Everything it reads is on
// the device already; the new record view stays there until mia_hip_get_ma_mask.
extern "C" int mia_hip_ma_mask(mia_hip_ctx* ctx, int32_t n5, int32_t n3, int32_t mode, int32_t single_stranded, int64_t* n_kept, int64_t* cols_kept) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  ctx->ma_out.mask_done = false;
  if (!ctx->ma_resident) { ctx->err = "ma_tally must precede ma_mask"; return MIA_HIP_ERR_STATE; }
  if (!ma_mask_args_ok(n5, n3, mode, single_stranded)) {
    ctx->err = "ma_mask: n5 and n3 must lie in 0 .. 15 and not both be 0, the mode be 0 (trim) or 1 (N), and single_stranded go with mode 1";
    return MIA_HIP_ERR_ARG;
  }
  if (ctx->ma_n > 0 && ctx->ma_cols < 0) { ctx->err = "ma_mask: col_off[0] of the tallied records is not 0"; return MIA_HIP_ERR_ARG; }
  const int64_t n = ctx->ma_n, T = ctx->ma_cols, n_ins = ctx->ma_n_ins;
  auto& mk = ctx->mask;
  memset(mk.bins, 0, sizeof mk.bins);
  mk.cols_kept = 0;
  mk.mode = mode;
  if (n > 0) {                                               // without records there is no launch and every result is zero
    HIPCHK(hipSetDevice(ctx->device));
    const int32_t n_wgs = (int32_t)ma_mask_layout_wgs(n);
    // (the new strings are no longer than the old ones: sized before the layout is known, padded as the old ones are)
    if (dev_ensure(ctx, mk.d_lohi, 2 * n) || dev_ensure(ctx, mk.d_rec, 3 * n) || dev_ensure(ctx, mk.d_off, n + 1) || dev_ensure(ctx, mk.d_seq, T + MA_REC_LANE) ||
        dev_ensure(ctx, mk.d_smp, T + MA_REC_LANE) || dev_ensure(ctx, mk.d_pair_keep, n_ins + 1) || dev_ensure(ctx, mk.d_ipos, n_ins + 1) ||
        dev_ensure(ctx, mk.d_ctl, (int64_t)MAR_STATE + n_wgs + 1) || dev_ensure(ctx, mk.d_bins, MA_MASK_BINS))
      return MIA_HIP_ERR_NOMEM;
    uint32_t *lo = (uint32_t*)mk.d_lohi, *hi = (uint32_t*)mk.d_lohi + n;
    int32_t *first = (int32_t*)mk.d_rec, *count = (int32_t*)mk.d_rec + n, *start = (int32_t*)mk.d_rec + 2 * n;
    HIPCHK(hipMemsetAsync(lo, 0xff, (size_t)n * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(hi, 0, (size_t)n * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(mk.d_bins, 0, (size_t)MA_MASK_BINS * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(mk.d_ctl, 0, ((size_t)MAR_STATE + (size_t)n_wgs) * 8, ctx->stream));
    const MaFlatView v{ma_records(ctx), T, nullptr, nullptr};
    if (stage_launch(ctx, STG_MA_MASK_BOUNDS, k_ma_mask_bounds, ma_grid(ctx, ma_mask_chunks(T), MAM_WGS_PER_CU), dim3(MAM_THREADS), 0, ctx->stream, v, n5, n3, mode, single_stranded ? 1 : 0,
                     lo, hi, (unsigned long long*)mk.d_bins))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    const MaMaskRecView rv{v, n5, n3, mode, lo, hi, first, count, start};
    if (stage_launch(ctx, STG_MA_MASK_LAYOUT, k_ma_mask_layout, dim3((unsigned)n_wgs), dim3(MAM_THREADS), 0, ctx->stream, rv, n_wgs,
                     (unsigned long long*)mk.d_ctl, (int64_t*)mk.d_off, (unsigned long long*)mk.d_bins))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    unsigned long long hdr[MAR_STATE] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(hdr, mk.d_ctl, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int64_t new_T = (int64_t)hdr[MAR_ROWS];
    if (new_T < 0 || new_T > T) { ctx->err = "ma_mask: the layout came back inconsistent"; return MIA_HIP_ERR_DEVICE; }
    const MaMaskApplyView av{v, n5, n3, mode, single_stranded ? 1 : 0, first, (const int64_t*)mk.d_off, new_T};
    const int64_t pieces = ma_mask_chunks(ma_mask_padded(new_T)), pair_wgs = (n_ins + MAM_THREADS - 1) / MAM_THREADS;
    if (stage_launch(ctx, STG_MA_MASK_APPLY, k_ma_mask_apply, ma_grid(ctx, std::max(pieces, pair_wgs), MAM_WGS_PER_CU), dim3(MAM_THREADS), 0, ctx->stream, av, (const int32_t*)count, n_ins,
                     (char*)mk.d_seq, (char*)mk.d_smp, (uint8_t*)mk.d_pair_keep, (int32_t*)mk.d_ipos, (unsigned long long*)mk.d_bins))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mk.bins, mk.d_bins, (size_t)MA_MASK_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < MA_MASK_HIST; b++) {                 // trim mode: the zone columns that left = all of them - those that stayed
      mk.bins[b] -= mk.bins[MA_MASK_STAY + b];
      if (mk.bins[b] < 0) { ctx->err = "ma_mask: the counts came back inconsistent"; return MIA_HIP_ERR_DEVICE; }
    }
    mk.cols_kept = new_T;
  }
  ctx->ma_out.mask_done = true;
  if (n_kept) *n_kept = mk.bins[MA_MASK_KEPT];
  if (cols_kept) *cols_kept = mk.cols_kept;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_mask(mia_hip_ctx* ctx, int32_t* first, int32_t* count, int32_t* start, int64_t* col_off, char* seq, char* smp, int64_t cap_bytes,
                                   uint8_t* pair_keep, int32_t* ins_pos, int64_t* hist, int64_t* scalars) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.mask_done) { ctx->err = "ma_mask first"; return MIA_HIP_ERR_STATE; }
  auto& mk = ctx->mask;
  if ((seq || smp) && cap_bytes < mk.cols_kept) { ctx->err = "get_ma_mask: buffer too small"; return MIA_HIP_ERR_ARG; }
  const int64_t n = ctx->ma_n, n_ins = ctx->ma_n_ins;
  if (n > 0) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ma_down(ctx, first, mk.d_rec, (size_t)n * 4));
    HIPCHK(ma_down(ctx, count, (int32_t*)mk.d_rec + n, (size_t)n * 4));
    HIPCHK(ma_down(ctx, start, (int32_t*)mk.d_rec + 2 * n, (size_t)n * 4));
    HIPCHK(ma_down(ctx, col_off, mk.d_off, (size_t)(n + 1) * 8));
    HIPCHK(ma_down(ctx, seq, mk.d_seq, (size_t)mk.cols_kept));
    HIPCHK(ma_down(ctx, smp, mk.d_smp, (size_t)mk.cols_kept));
    HIPCHK(ma_down(ctx, pair_keep, mk.d_pair_keep, (size_t)n_ins));
    HIPCHK(ma_down(ctx, ins_pos, mk.d_ipos, (size_t)n_ins * 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  } else if (col_off) {
    col_off[0] = 0;
  }
  if (hist) memcpy(hist, mk.bins, sizeof(int64_t) * MA_MASK_HIST);
  if (scalars) {
    scalars[0] = mk.bins[MA_MASK_EMPTIED]; scalars[1] = mk.bins[MA_MASK_EMPTIED + 1]; scalars[2] = mk.bins[MA_MASK_STRIPPED];
    scalars[3] = mk.bins[MA_MASK_PAIRS]; scalars[4] = mk.bins[MA_MASK_KEPT]; scalars[5] = mk.cols_kept;
  }
  return MIA_HIP_OK;
}

// The table of the damage model (ma_hip -K, ma_pmd_body.h): host arithmetic alone, no context and no device.
extern "C" int mia_hip_ma_pmd_table(double p, double c0, double pi, double eps, int32_t single_stranded, int32_t* w) {
  if (!w) return MIA_HIP_ERR_ARG;
  return ma_pmd_model(p, c0, pi, eps, single_stranded != 0, w) ? MIA_HIP_OK : MIA_HIP_ERR_ARG;
}

// The damage score (ma_hip -L, -K, -S, -f 97) of the records of the last mia_hip_ma_tally: see mia_ma_pmd_kernels.h.  Columns, depth
// codes and strands are on the device already; the reference, the selection, the pairing and the weights go up.
extern "C" int mia_hip_ma_score(mia_hip_ctx* ctx, const char* ref_seq, const uint8_t* use, const int64_t* mate, const int32_t* w, int64_t threshold,
                                int64_t* n_molecules, int64_t* n_kept) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  ctx->ma_out.score_done = false;
  auto& sc = ctx->score;
  const char* const own_error = !w ? "no weight table" : !ma_pmd_weights_ok(w) ? "a weight lies outside -2^20 .. 2^20" : nullptr;
  MaMolFrame f;
  if (const int rc = ma_mol_frame(ctx, "ma_score", ref_seq, use, mate, own_error, sc.d_mate, ma_pmd_chunks(ctx->ma_cols), ma_pmd_record_wgs(ctx->ma_n),
                                  MAQ_WGS_PER_CU, &f))
    return rc;
  const int64_t n = ctx->ma_n;
  memset(sc.bins, 0, sizeof sc.bins);
  if (n > 0) {                                               // without records there is no launch and every result is zero
    if (dev_ensure(ctx, sc.d_w, MA_PMD_WEIGHTS) || dev_ensure(ctx, sc.d_rec, n) || dev_ensure(ctx, sc.d_mol, n) || dev_ensure(ctx, sc.d_keep, n) ||
        dev_ensure(ctx, sc.d_bins, MA_PMD_BINS))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipMemcpyAsync(sc.d_w, w, (size_t)MA_PMD_WEIGHTS * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(sc.d_rec, 0, (size_t)n * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(sc.d_mol, 0, (size_t)n * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(sc.d_keep, 0, (size_t)n, ctx->stream));
    HIPCHK(hipMemsetAsync(sc.d_bins, 0, (size_t)MA_PMD_BINS * 8, ctx->stream));
    if (stage_launch(ctx, STG_MA_SCORE_COLS, k_ma_score_cols, f.col_grid, dim3(MAQ_THREADS), 0, ctx->stream, f.v, (const int32_t*)sc.d_w,
                     (unsigned long long*)sc.d_rec))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    MaPmdMolView mv{n, f.v.revcom, f.v.use, f.mate, (const int64_t*)sc.d_rec.p, threshold, (int64_t*)sc.d_mol, (uint8_t*)sc.d_keep};
    if (stage_launch(ctx, STG_MA_SCORE_MOLECULES, k_ma_score_molecules, f.rec_grid, dim3(MAQ_THREADS), 0, ctx->stream, mv, (unsigned long long*)sc.d_bins))
      return MIA_HIP_ERR_NOMEM;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sc.bins, sc.d_bins, (size_t)MA_PMD_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  int64_t molecules = 0;
  for (int b = 0; b < MA_PMD_HIST; b++) molecules += sc.bins[b];
  ctx->ma_out.score_done = true;
  if (n_molecules) *n_molecules = molecules;
  if (n_kept) *n_kept = sc.bins[MA_PMD_KEPT];
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ma_score(mia_hip_ctx* ctx, int64_t* rec_score, int64_t* mol_score, uint8_t* keep, int64_t* hist, int64_t* orphans) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->ma_resident || !ctx->ma_out.score_done) { ctx->err = "ma_score first"; return MIA_HIP_ERR_STATE; }
  const int64_t n = ctx->ma_n;
  auto& sc = ctx->score;
  if (n > 0 && (rec_score || mol_score || keep)) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ma_down(ctx, rec_score, sc.d_rec, (size_t)n * 8));
    HIPCHK(ma_down(ctx, mol_score, sc.d_mol, (size_t)n * 8));
    HIPCHK(ma_down(ctx, keep, sc.d_keep, (size_t)n));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  if (hist) memcpy(hist, sc.bins, sizeof(int64_t) * MA_PMD_HIST);
  if (orphans) *orphans = sc.bins[MA_PMD_ORPHANS];
  return MIA_HIP_OK;
}

extern "C" int mia_hip_get_ins_tally(mia_hip_ctx* ctx, int32_t* ins_off, int32_t* ins_tally, int64_t cap_slots, int64_t* n_slots) {
  if (!ctx) return MIA_HIP_ERR_ARG;
  if (!ctx->tallied || !ctx->consensus_done) { ctx->err = "consensus first"; return MIA_HIP_ERR_STATE; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t total = ctx->ins_total_host;
  if (n_slots) *n_slots = total;
  if (ins_off) HIPCHK(hipMemcpyAsync(ins_off, ctx->d_ins_off, (size_t)ctx->tb.Lp * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (ins_tally && total > 0) {
    if (cap_slots < total) { ctx->err = "ins_tally buffer too small"; return MIA_HIP_ERR_ARG; }
    HIPCHK(hipMemcpyAsync(ins_tally, ctx->d_ins_tally, (size_t)total * 9 * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return MIA_HIP_OK;
}

// ---- pass 1 ----------------------------------------------------------------------------
// populate_kpa + add_kmer (src/kmer.c:65-107,153-168): the k-mers that occur in `seq`, each with its ascending
// positions (at most 128; further ones are silently dropped, :75-77).  Only the occurring k-mers are listed -- the
// dense 4^k table is zeroed and filled on the device.
static void build_kmer_lists(const std::string& seq, int k, int soft_mask, std::vector<uint32_t>& kmer, std::vector<uint32_t>& entry,
                             std::vector<int32_t>& pos) {
  const int n = (int)seq.size();
  std::vector<uint64_t> kp;   // (k-mer << 32) | position: sorting keeps positions ascending inside a k-mer
  kp.reserve((size_t)(n > 0 ? n : 1));
  for (int i = 0; i + k <= n; i++) {
    bool ok = true;
    uint64_t v = 0;
    for (int t = 0; t < k && ok; t++) {
      char c = seq[i + t];
      if (soft_mask && (c >= 'a' && c <= 'z')) ok = false;
      switch (c & ~32) { case 'A': v = v << 2; break; case 'C': v = (v << 2) | 1; break; case 'G': v = (v << 2) | 2; break;
                         case 'T': v = (v << 2) | 3; break; default: ok = false; }
    }
    if (ok) kp.push_back((v << 32) | (uint32_t)i);
  }
  std::sort(kp.begin(), kp.end());
  kmer.clear(); entry.clear(); pos.clear();
  for (size_t i = 0; i < kp.size();) {
    size_t j = i;
    while (j < kp.size() && (kp[j] >> 32) == (kp[i] >> 32)) j++;
    const size_t cnt = (j - i) < (size_t)MAX_KMER_POS ? (j - i) : (size_t)MAX_KMER_POS;
    kmer.push_back((uint32_t)(kp[i] >> 32));
    entry.push_back((uint32_t)(pos.size() << 8) | (uint32_t)cnt);
    for (size_t t = 0; t < cnt; t++) pos.push_back((int32_t)(uint32_t)kp[i + t]);
    i = j;
  }
  pos.push_back(0);
}

// What align_all reads, overwrites or counts in the context while it runs on a borrowed read set and reference (the anchored part of
// pass 1): each field is named ONCE, here; AlignBorrow copies these out and assigns them back.
//   RESTORED: the read set and its longest read; the four lists and the reference (lent through their owners' .p: the blocks come
//   from the pool, the owners' own blocks are put back -- align_all only reads these five, nothing allocates them while they are
//   lent); L, wrap, explicit_win, use_filter; what the context knows of its own alignment (aligned, culled, tallied, pre_cull_valid,
//   diag_scripts_missing); ref_mostly_bases and kh_entries; the read counts of mia_hip_plain_stats, _filter_stats and _bx_stats; and,
//   beside this list, every stage timer's sum and launch count but pass 1's (AlignBorrow itself).
//   LEFT BEHIND by the borrowed run: bx_last, the band pipeline's counters of the last alignment -- the job's next alignment reads its
//   rejects from them (AlignRouteIn::rejects), which moves reads between exact kernels and changes no result; bx_launches, band_done,
//   direct_open_steps and quick_steps, which are statistics; align_end_signalled, which every alignment sets anew before anything
//   reads it; and the buffers the borrowed run grows (trace slabs, the open list and the like), which every alignment sizes for itself.
//   REFERENCE AHEAD: d_ref is lent by its raw pointer, and ref_ahead_adopt swaps d_ref's block for its twin's.  The two never meet: adoption
//   happens at the top of iterate_body alone, a borrow lives inside one mia_hip_pass1 call, and neither calls the other.  ref_mostly_bases
//   and kh_entries, restored here, are the context's; what the shadow launch counted lives in ctx->ahead.key and is not lent.
static auto align_lent_fields(mia_hip_ctx* c) {
  return std::tie(c->rs, c->d_bin_of.p, c->d_list.p, c->d_wide_list.p, c->d_retry_list.p, c->max_len, c->d_ref.p, c->L, c->wrap, c->explicit_win,
                  c->use_filter, c->aligned, c->culled, c->tallied, c->pre_cull_valid, c->ref_mostly_bases, c->diag_scripts_missing, c->kh_entries,
                  c->plain_total, c->plain_retried, c->filter_seen, c->filter_proven, c->bx_seen, c->bx_done[0], c->bx_done[1], c->bx_done[2]);
}
template <class... T>
static std::tuple<T...> tuple_values(const std::tuple<T&...>& refs) { return std::tuple<T...>(refs); }

// Lets align_all run on a borrowed read set and reference and puts the context back as it was (align_lent_fields).  The stage
// timers of the iteration path must not see what the borrowed run adds (bench.py's roofline reads them): what is pending goes into
// their sums first, and what the borrowed run leaves pending is dropped with the sums put back.  Pass 1's own pair, whose end is not
// recorded yet, stays pending.
struct AlignBorrow {
  mia_hip_ctx* c;
  decltype(tuple_values(align_lent_fields(nullptr))) saved;
  double stg_ms[STG_COUNT];
  int64_t stg_launches[STG_COUNT];
  explicit AlignBorrow(mia_hip_ctx* ctx) : c(ctx), saved(tuple_values(align_lent_fields(ctx))) {
    drain_events(c, STG_PASS1);
    for (int k = 0; k < STG_COUNT; k++) { stg_ms[k] = c->stg[k].ms; stg_launches[k] = c->stg[k].launches; }
  }
  ~AlignBorrow() {
    drain_events(c, STG_PASS1);
    for (int k = 0; k < STG_COUNT; k++)
      if (k != STG_PASS1) { c->stg[k].ms = stg_ms[k]; c->stg[k].launches = stg_launches[k]; }
    align_lent_fields(c) = saved;
  }
};

// One mia_hip_pass1 call: its arguments, the route (pass1_route.h), what the host prepares and the device temporaries, which go back
// to the context's pool when the call ends, whichever way.  The stages below run in the order they are written in.
struct Pass1Call {
  mia_hip_ctx* ctx;
  const char* ref; int L, circular, kmer_len, soft_mask;
  int64_t n; const char* bases; const int64_t* offsets;
  int32_t* score; uint8_t* rc; int32_t *as, *ae; uint8_t* flags;
  PackParams pk;
  Pass1Route r;
  // host side
  std::string fw, rcs;                           // both strands, wrapped: make_reverse_complement, add_ref_wrap -- src/mia_main.c:637-676
  std::vector<uint8_t> cf, cr, packed;           // their codes; the reads' 4-bit codes
  std::vector<uint32_t> roff; std::vector<uint16_t> len;
  uint64_t total = 0; int max_len = 1;
  int64_t p1_other = 0;                          // N columns of the forward strand
  // device side
  PoolLease<uint8_t> d_cf, d_cr, d_packed, d_rc, d_flags;
  PoolLease<uint32_t> d_tab[2], d_kl[2], d_el[2], d_roff, d_status, d_ckpt, d_ntodo;
  PoolLease<int32_t> d_pos[2], d_score, d_as, d_ae, d_todo, d_p1kcnt, d_p1kpos;
  PoolLease<uint16_t> d_len;
  PoolLease<unsigned char> d_trace;
  PoolLease<uint64_t> d_p1planes;
  KmerIndex kx{};
  Pass1Reads pr{};
  int64_t n_dp = 0;                              // reads no stage has decided yet
  bool p1_timed = false;
  // MIA_HIP_P1_TIMING: the tools read these lines
  bool timing = false;
  std::chrono::steady_clock::time_point t_start;
  void lap(const char* what) {
    if (!timing) return;
    auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[mia_hip_pass1] %-12s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_start).count());
    t_start = t;
  }
  KmerOcc kocc(int strand) const { return KmerOcc{d_p1kcnt + strand * DF_KTAB, d_p1kpos + strand * DF_KTAB * DF_KCAP}; }
};

static void pass1_host_reference(Pass1Call& p) {
  const int L = p.L, wl = p.circular ? (L < MAX_READ ? L : MAX_READ) : 0, wrap = L + wl;
  p.fw.assign(p.ref, p.ref + L);
  p.rcs.assign((size_t)L, 'N');
  for (int i = 0; i < L; i++) p.rcs[i] = revcom_char_host(p.ref[L - 1 - i]);
  p.fw += p.fw.substr(0, wl);
  p.rcs += p.rcs.substr(0, wl);
  p.cf.assign((size_t)wrap + 64, 4);
  p.cr.assign((size_t)wrap + 64, 4);
  for (int i = 0; i < wrap; i++) {
    p.cf[i] = base_code((char)toupper((unsigned char)p.fw[i]));
    p.cr[i] = base_code((char)toupper((unsigned char)p.rcs[i]));
  }
  for (int i = 0; i < L; i++) p.p1_other += p.cf[(size_t)i] > 3;
}

// reads (as sequenced); validated before anything is allocated on the device
static int pass1_index_reads(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  p.roff.resize((size_t)p.n);
  p.len.resize((size_t)p.n);
  for (int64_t i = 0; i < p.n; i++) {
    int64_t l = p.offsets[i + 1] - p.offsets[i];
    if (l < 1 || l > MIA_HIP_MAX_READ) { ctx->err = "read length outside 1..256"; return MIA_HIP_ERR_ARG; }
    p.roff[i] = (uint32_t)p.total; p.len[i] = (uint16_t)l;
    if (l > p.max_len) p.max_len = (int)l;
    p.total += (uint64_t)(((l + 1) / 2 + 3) & ~3);
    if (p.total >= ((uint64_t)1 << 32)) { ctx->err = "packed read store exceeds 4 GiB per call"; return MIA_HIP_ERR_ARG; }
  }
  return MIA_HIP_OK;
}

static auto pass1_kernel(const Pass1Route& r) { return r.cpl == P1_CPL_WIDE ? k_pass1<P1_CPL_WIDE> : k_pass1<P1_CPL_NARROW>; }

// everything pass1_route() reads; the walk over both strands for the N columns' spellings only where the route will use its answer
static Pass1RouteIn pass1_route_input(const Pass1Call& p) {
  const mia_hip_ctx* ctx = p.ctx;
  Pass1RouteIn in;
  in.n = p.n; in.max_len = p.max_len; in.L = p.L; in.circular = p.circular != 0; in.kmer_len = p.kmer_len;
  in.max_pos = ctx->max_pos; in.flat = ctx->flat; in.bx_ok = ctx->bx_ok; in.use_bx = ctx->use_bx; in.use_filter = ctx->use_filter;
  in.p1_other = p.p1_other;
  in.alt_cpl = alt_int("MIA_HIP_P1_CPL"); in.alt_plain = alt_int("MIA_HIP_P1_PLAIN");
  in.cus = ctx->cus;
  if (pass1_wants_wild(in)) {
    const int len1 = pass1_len1(in);
    std::vector<uint8_t> both(p.cf.begin(), p.cf.begin() + len1);
    both.insert(both.end(), p.cr.begin(), p.cr.begin() + len1);
    in.wild_entries = kh_wild_entries(both.data(), (int64_t)both.size(), BX_WILD);
  }
  return in;
}

// the route, its refusals, and the persistent grid: the workgroups of k_pass1<cpl> that are resident at once with this call's LDS
static int pass1_decide(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  p.r = pass1_route(pass1_route_input(p));
  if (p.r.refusal != P1_REFUSE_NONE) { ctx->err = pass1_refusal_message(p.r.refusal); return pass1_refusal_code(p.r.refusal); }
  HIPCHK(hipFuncSetAttribute((const void*)pass1_kernel(p.r), hipFuncAttributeMaxDynamicSharedMemorySize, P1_LDS_LIMIT));
  int waves_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&waves_cu, (const void*)pass1_kernel(p.r), 64, (size_t)p.r.lds));
  if (waves_cu < 1) { ctx->err = "pass-1 kernel does not fit a compute unit"; return MIA_HIP_ERR_RANGE; }
  pass1_set_grid(p.r, waves_cu, ctx->cus, p.n);
  return MIA_HIP_OK;
}

// mia -k: the dense 4^k tables of both strands, filled on the device from the lists of the k-mers that occur
static int pass1_kmer_tables(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  if (pool_take(ctx, p.d_cf, p.cf.size()) || pool_take(ctx, p.d_cr, p.cr.size())) return MIA_HIP_ERR_NOMEM;
  p.kx.k = p.kmer_len > 0 ? p.kmer_len : -1;
  if (p.kx.k <= 0) return MIA_HIP_OK;
  const size_t nk = (size_t)1 << (2 * p.kx.k);
  for (int s = 0; s < 2; s++) {
    std::vector<uint32_t> kmer, entry;
    std::vector<int32_t> pos;
    build_kmer_lists(s ? p.rcs : p.fw, p.kx.k, p.soft_mask, kmer, entry, pos);
    const size_t ne = kmer.size();
    if (pool_take(ctx, p.d_tab[s], nk) || pool_take(ctx, p.d_pos[s], pos.size()) || pool_take(ctx, p.d_kl[s], ne + 1) || pool_take(ctx, p.d_el[s], ne + 1))
      return MIA_HIP_ERR_NOMEM;
    hipError_t ke = hipMemsetAsync(p.d_tab[s], 0, nk * 4, ctx->stream);
    if (ke == hipSuccess) ke = hipMemcpy(p.d_pos[s], pos.data(), pos.size() * 4, hipMemcpyHostToDevice);
    if (ke == hipSuccess && ne) ke = hipMemcpy(p.d_kl[s], kmer.data(), ne * 4, hipMemcpyHostToDevice);
    if (ke == hipSuccess && ne) ke = hipMemcpy(p.d_el[s], entry.data(), ne * 4, hipMemcpyHostToDevice);
    if (ke == hipSuccess && ne) {
      hipLaunchKernelGGL(k_kmer_fill, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, ctx->stream, (int32_t)ne, p.d_kl[s], p.d_el[s], p.d_tab[s]);
      ke = hipGetLastError();
    }
    if (ke != hipSuccess) { ctx->err = std::string("pass1 k-mer table: ") + hipGetErrorString(ke); return MIA_HIP_ERR_DEVICE; }
    p.kx.tab[s] = p.d_tab[s];
    p.kx.pos[s] = p.d_pos[s];
  }
  return MIA_HIP_OK;
}

// (every allocation first: an early return leaves no copy in flight from the host vectors)
static int pass1_allocate(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  const Pass1Route& r = p.r;
  const size_t n = (size_t)p.n;
  p.packed.assign((size_t)p.total + 8, 0);
  pack_reads(p.n, p.bases, p.offsets, p.roff.data(), p.len.data(), p.packed.data());
  if (p.timing) fprintf(stderr, "[mia_hip_pass1] cpl %d plain %d waves/CU %d lds %d\n", r.cpl, r.plain, r.waves_cu, r.lds);
  if (pool_take(ctx, p.d_packed, p.packed.size()) || pool_take(ctx, p.d_roff, n) || pool_take(ctx, p.d_len, n) || pool_take(ctx, p.d_rc, n) ||
      pool_take(ctx, p.d_flags, n) || pool_take(ctx, p.d_status, n) || pool_take(ctx, p.d_score, n) || pool_take(ctx, p.d_as, n) ||
      pool_take(ctx, p.d_ae, n) || pool_take(ctx, p.d_trace, (size_t)(r.trace_bytes * r.grid)) || pool_take(ctx, p.d_ckpt, (size_t)(r.ckpt_words * r.grid)))
    return MIA_HIP_ERR_NOMEM;
  if (r.need_todo && (pool_take(ctx, p.d_todo, n) || pool_take(ctx, p.d_ntodo, 1))) return MIA_HIP_ERR_NOMEM;
  if (r.need_ktab && (pool_take(ctx, p.d_p1kcnt, (size_t)DF_KTAB * 2) || pool_take(ctx, p.d_p1kpos, (size_t)DF_KTAB * DF_KCAP * 2))) return MIA_HIP_ERR_NOMEM;
  if (r.filtered && pool_take(ctx, p.d_p1planes, (size_t)plane_words(r.len1) * 6)) return MIA_HIP_ERR_NOMEM;
  p.pr = Pass1Reads{p.n, p.d_packed, p.d_roff, p.d_len, p.d_score, p.d_as, p.d_ae, p.d_rc, p.d_flags, p.d_status};
  return MIA_HIP_OK;
}

// reference codes and reads go up; the call's device time (filter, anchored windows and DP) is measured from behind them
static int pass1_upload(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  auto up = [&](void* d, const void* h, size_t b) { return hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, ctx->stream); };
  HIPCHK(up(p.d_cf, p.cf.data(), p.cf.size()));
  HIPCHK(up(p.d_cr, p.cr.data(), p.cr.size()));
  HIPCHK(up(p.d_packed, p.packed.data(), p.packed.size()));
  HIPCHK(up(p.d_roff, p.roff.data(), (size_t)p.n * 4));
  HIPCHK(up(p.d_len, p.len.data(), (size_t)p.n * 2));
  p.n_dp = p.n;
  ctx->pass1_filtered = 0;
  ctx->pass1_anchored = 0;
  drain_events(ctx);                       // (nothing of an earlier call may sit in the pass-1 timer)
  p.p1_timed = ((ctx->stage_mask >> STG_PASS1) & 1u) && stage_begin(ctx, STG_PASS1) == 0;
  return MIA_HIP_OK;
}

static void pass1_kmer_occ(Pass1Call& p, int wild) {
  const int len1 = p.r.len1;
  hipStream_t s = p.ctx->stream;
  hipLaunchKernelGGL(k_kmer_occ, dim3((unsigned)((len1 + 255) / 256)), dim3(256), 0, s, p.d_cf, (int64_t)len1, p.d_p1kcnt, p.d_p1kpos, wild);
  hipLaunchKernelGGL(k_kmer_occ, dim3((unsigned)((len1 + 255) / 256)), dim3(256), 0, s, p.d_cr, (int64_t)len1, p.d_p1kcnt + DF_KTAB,
                     p.d_p1kpos + DF_KTAB * DF_KCAP, wild);
}

// The diagonal filter (diag_filter.h) decides most reads by bit-parallel comparison against every diagonal of both strands; the
// list of the reads it leaves goes to the stages behind it.
static int pass1_filter_stage(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  const int len1 = p.r.len1;
  const int64_t n = p.n, words = plane_words(len1);
  uint64_t* pl = p.d_p1planes;
  const unsigned planes_grid = (unsigned)((words + 3) / 4 < 4096 ? (words + 3) / 4 : 4096);
  hipLaunchKernelGGL(k_ref_planes, dim3(planes_grid), dim3(256), 0, ctx->stream, p.d_cf, (int64_t)len1, words, pl, pl + words, pl + 2 * words);
  hipLaunchKernelGGL(k_ref_planes, dim3(planes_grid), dim3(256), 0, ctx->stream, p.d_cr, (int64_t)len1, words, pl + 3 * words, pl + 4 * words, pl + 5 * words);
  HIPCHK(hipMemsetAsync(p.d_ntodo, 0, 4, ctx->stream));
  RefPlanes pf{pl, pl + words, pl + 2 * words}, prc{pl + 3 * words, pl + 4 * words, pl + 5 * words};
  // 10-mer tables of both strands for rule (c) (diag_filter.h: KmerOcc)
  KmerOcc kf{nullptr, nullptr}, kr{nullptr, nullptr};
  if (p.r.need_ktab) {
    HIPCHK(hipMemsetAsync(p.d_p1kcnt, 0, (size_t)DF_KTAB * 2 * 4, ctx->stream));
    pass1_kmer_occ(p, 0);
    kf = p.kocc(0); kr = p.kocc(1);
  }
  hipLaunchKernelGGL(k_pass1_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p.pr, pf, prc, kf, kr, len1, p.L, p.d_todo, p.d_ntodo);
  HIPCHK(hipGetLastError());
  uint32_t h_ntodo = 0;
  HIPCHK(hipMemcpyAsync(&h_ntodo, p.d_ntodo, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  p.n_dp = h_ntodo;
  ctx->pass1_filtered = n - p.n_dp;
  if (p.timing) fprintf(stderr, "[mia_hip_pass1] diagonal filter: %lld of %lld reads decided\n", (long long)(n - p.n_dp), (long long)n);
  return MIA_HIP_OK;
}

// The anchored stage's temporaries: one allocation for all of them (twenty separate ones cost more than the stage)
struct Pass1Arena {
  PoolLease<unsigned char> block;
  uint32_t *roff, *status, *nrest;
  uint16_t* len;
  uint8_t *rc, *sk, *ref2;
  int32_t *as, *ae, *score, *refstart, *bin, *list, *wide, *retry, *rest, *bound, *budget, *u;
  int16_t *abr, *cols;
  int take(mia_hip_ctx* ctx, int64_t m, int64_t n_dp, int len1, int stride) {
    size_t top = 0;
    auto carve = [&](size_t bytes) { const size_t at = top; top += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_roff = carve((size_t)m * 4), o_status = carve((size_t)m * 4), o_nrest = carve(64), o_len = carve((size_t)m * 2),
                 o_rc = carve((size_t)m), o_sk = carve((size_t)m), o_ref2 = carve((size_t)2 * len1 + 64), o_as = carve((size_t)m * 4),
                 o_ae = carve((size_t)m * 4), o_score = carve((size_t)m * 4), o_refstart = carve((size_t)m * 4), o_bin = carve((size_t)m * 4),
                 o_list = carve(((size_t)m + 4 * N_BINS) * 4), o_wide = carve((size_t)m * 4), o_retry = carve((size_t)m * 4),
                 o_rest = carve((size_t)n_dp * 4), o_abr = carve((size_t)m * 2), o_cols = carve((size_t)m * stride * 2),
                 o_bound = carve((size_t)n_dp * 4), o_budget = carve((size_t)n_dp * 4), o_u = carve((size_t)n_dp * 4);
    if (pool_take(ctx, block, top)) return MIA_HIP_ERR_NOMEM;
    unsigned char* a = block;
    roff = (uint32_t*)(a + o_roff); status = (uint32_t*)(a + o_status); nrest = (uint32_t*)(a + o_nrest);
    len = (uint16_t*)(a + o_len);
    rc = a + o_rc; sk = a + o_sk; ref2 = a + o_ref2;
    as = (int32_t*)(a + o_as); ae = (int32_t*)(a + o_ae); score = (int32_t*)(a + o_score); refstart = (int32_t*)(a + o_refstart);
    bin = (int32_t*)(a + o_bin); list = (int32_t*)(a + o_list); wide = (int32_t*)(a + o_wide); retry = (int32_t*)(a + o_retry);
    rest = (int32_t*)(a + o_rest); bound = (int32_t*)(a + o_bound); budget = (int32_t*)(a + o_budget); u = (int32_t*)(a + o_u);
    abr = (int16_t*)(a + o_abr); cols = (int16_t*)(a + o_cols);
    return MIA_HIP_OK;
  }
};

// align_all on the windows the anchors chose: the context is lent the arena's read set and the two strands as one reference
static int pass1_align_windows(Pass1Call& p, Pass1Arena& w, int64_t m, int stride) {
  mia_hip_ctx* ctx = p.ctx;
  AlignBorrow borrow(ctx);
  ReadSet& r = ctx->rs;
  r.n = m; r.packed = p.d_packed; r.roff = w.roff; r.len = w.len; r.rc = w.rc; r.sk = w.sk; r.as = w.as; r.ae = w.ae; r.score = w.score;
  r.refstart = w.refstart; r.abr = w.abr; r.status = w.status; r.cols = w.cols; r.stride = stride;
  ctx->d_bin_of.p = w.bin; ctx->d_list.p = w.list; ctx->d_wide_list.p = w.wide; ctx->d_retry_list.p = w.retry; ctx->max_len = p.max_len;
  ctx->d_ref.p = w.ref2; ctx->L = 2 * p.r.len1; ctx->wrap = 2 * p.r.len1; ctx->explicit_win = 1; ctx->use_filter = 0;
  ctx->ref_mostly_bases = p.r.ref_mostly_bases; ctx->kh_entries = p.r.wild_entries;
  ctx->wide_to_caller = true;
  const int rc = align_all(ctx);
  ctx->wide_to_caller = false;
  return rc;
}

// Anchored stage (mia_pass1_kernels.h): what the filter left over is aligned in +-50 windows around the places where
// six 10-mers of the read occur -- provably the same result as the whole-strand DP when the budget check of
// k_pass1_select holds; everything else goes on to k_pass1.  Needs both strands free of N (a 10-mer with an N is not
// in the table and an N column costs less than a mismatch), or tables that list the N columns under every spelling.
static int pass1_anchor_stage(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  const int len1 = p.r.len1;
  const int64_t n_dp = p.n_dp, m = n_dp * P1A_SLOTS;
  const int stride = (p.max_len + 3) & ~3;
  const unsigned per_read = (unsigned)((n_dp + 255) / 256);
  if (!p.r.filtered) hipLaunchKernelGGL(k_iota, dim3(per_read), dim3(256), 0, ctx->stream, p.n, p.d_todo);      // no filter made the list: every read
  if (p.r.rebuild_ktab_for_anchors) {
    HIPCHK(hipMemsetAsync(p.d_p1kcnt, 0, (size_t)DF_KTAB * 2 * 4, ctx->stream));
    pass1_kmer_occ(p, p.r.wild);
  }
  Pass1Arena w;
  if (const int rc = w.take(ctx, m, n_dp, len1, stride)) return rc;
  HIPCHK(hipMemsetAsync(w.rc, 0, (size_t)m, ctx->stream));
  HIPCHK(hipMemsetAsync(w.abr, 0, (size_t)m * 2, ctx->stream));
  HIPCHK(hipMemsetAsync(w.status, 0, (size_t)m * 4, ctx->stream));
  HIPCHK(hipMemsetAsync(w.score, 0, (size_t)m * 4, ctx->stream));
  HIPCHK(hipMemsetAsync(w.nrest, 0, 64, ctx->stream));
  HIPCHK(hipMemsetAsync(w.ref2, 4, (size_t)2 * len1 + 64, ctx->stream));
  HIPCHK(hipMemcpyAsync(w.ref2, p.d_cf, (size_t)len1, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(w.ref2 + len1, p.d_cr, (size_t)len1, hipMemcpyDeviceToDevice, ctx->stream));
  BxTab p1tab;
  p1tab.sub = ctx->d_bx_sub; p1tab.mrow = ctx->d_bx_mrow; p1tab.loss = ctx->d_bx_loss; p1tab.dl = ctx->d_bx_dl; p1tab.min_m = ctx->bx_min_m; p1tab.max_m = ctx->bx_max_m; p1tab.maxw = 32;
  auto anchor = ctx->flat ? k_pass1_anchor<false> : k_pass1_anchor<true>;
  hipLaunchKernelGGL(anchor, dim3(per_read), dim3(256), 0, ctx->stream, p.pr, p.d_todo, n_dp, p.kocc(0), p.kocc(1), len1, w.roff, w.len, w.sk, w.as, w.ae,
                     w.bound, w.budget, w.u, p1tab);
  HIPCHK(hipGetLastError());
  if (const int rc = pass1_align_windows(p, w, m, stride)) return rc;
  hipLaunchKernelGGL(k_pass1_select, dim3(per_read), dim3(256), 0, ctx->stream, p.pr, p.d_todo, n_dp, len1, p.L, w.sk, w.score, w.as, w.ae, w.abr, w.status,
                     w.bound, w.budget, w.u, w.rest, w.nrest);
  HIPCHK(hipGetLastError());
  uint32_t h_rest[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h_rest, w.nrest, 64, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint32_t h_nrest = h_rest[0];
  if (p.timing) fprintf(stderr, "[mia_hip_pass1] left to the whole-strand DP: %u no cluster, %u unfinished windows, %u clipped, %u over budget, %u weak clusters\n",
                        h_rest[1], h_rest[2], h_rest[3], h_rest[4], h_rest[5]);
  if (p.timing) fprintf(stderr, "[mia_hip_pass1] no cluster: %u reads with N, %u too few blocks, %u too many clusters, %u too wide, %u too many strong, %u none strong, %u no room\n",
                        h_rest[9], h_rest[10], h_rest[11], h_rest[12], h_rest[13], h_rest[14], h_rest[15]);
  // the survivors' list replaces the filter's (d_todo is at least as long)
  HIPCHK(hipMemcpyAsync(p.d_todo, w.rest, (size_t)h_nrest * 4, hipMemcpyDeviceToDevice, ctx->stream));
  ctx->pass1_anchored = n_dp - h_nrest;
  if (p.timing) fprintf(stderr, "[mia_hip_pass1] anchored windows: %lld of %lld left-over reads decided\n", (long long)(n_dp - h_nrest), (long long)n_dp);
  p.n_dp = h_nrest;
  return MIA_HIP_OK;
}

// the whole-strand DP (k_pass1<CPL>) on what is left: all reads, or the list of the stages in front of it
static int pass1_dp_stage(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  const Pass1Route& r = p.r;
  const int64_t g = r.grid < p.n_dp ? r.grid : p.n_dp;
  auto kfn = pass1_kernel(r);
  hipLaunchKernelGGL(kfn, dim3((unsigned)g), dim3(64), r.lds, ctx->stream, p.pr, p.d_cf, p.d_cr, r.len1, p.L, ctx->d_pssm, p.pk, p.kx, p.d_trace,
                     r.trace_bytes, p.d_ckpt, r.ckpt_words, r.rows_p, r.mask_words, r.plain, p.d_todo, p.n_dp);
  HIPCHK(hipGetLastError());
  return MIA_HIP_OK;
}

static int pass1_download(Pass1Call& p) {
  mia_hip_ctx* ctx = p.ctx;
  const size_t n = (size_t)p.n;
  if (p.p1_timed) stage_end(ctx, STG_PASS1);
  auto back = [&](void* h, const void* d, size_t b) { return hipMemcpyAsync(h, d, b, hipMemcpyDeviceToHost, ctx->stream); };
  HIPCHK(back(p.score, p.d_score, n * 4));
  HIPCHK(back(p.as, p.d_as, n * 4));
  HIPCHK(back(p.ae, p.d_ae, n * 4));
  HIPCHK(back(p.rc, p.d_rc, n));
  HIPCHK(back(p.flags, p.d_flags, n));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  p.lap("h2d+kernel+d2h");
  if (p.p1_timed && !ctx->stg[STG_PASS1].pending.empty()) {
    // the whole call's device time (filter, anchored windows and DP), measured on the pair taken behind the upload
    const auto pair = ctx->stg[STG_PASS1].pending.back();
    float ms = 0;
    if (hipEventElapsedTime(&ms, pair.first, pair.second) == hipSuccess) ctx->pass1_ms = ms;
  }
  p.lap("done");
  return MIA_HIP_OK;
}

extern "C" int mia_hip_pass1(mia_hip_ctx* ctx, const char* ref, int32_t ref_len, int circular, int kmer_len, int soft_mask,
                             int64_t n, const char* bases, const int64_t* offsets, int32_t* score, uint8_t* rc, int32_t* as,
                             int32_t* ae, uint8_t* flags) {
  if (!ctx || !ref || ref_len <= 0 || n < 0 || (n > 0 && (!bases || !offsets || !score || !rc || !as || !ae || !flags))) return MIA_HIP_ERR_ARG;
  if (!ctx->have_pssm) { ctx->err = "set_pssm must precede pass1"; return MIA_HIP_ERR_STATE; }
  if (kmer_len > 14) { ctx->err = "Cannot use kmer length greater than 14"; return MIA_HIP_ERR_ARG; }   // MAX_KMER_LEN
  HIPCHK(hipSetDevice(ctx->device));
  if (n == 0) return MIA_HIP_OK;
  Pass1Call p{ctx, ref, ref_len, circular, kmer_len, soft_mask, n, bases, offsets, score, rc, as, ae, flags};
  p.timing = alt_env("MIA_HIP_P1_TIMING") != nullptr;
  p.t_start = std::chrono::steady_clock::now();
  if (!make_pack_params(1024, ctx->max_abs, &p.pk)) { ctx->err = "PSSM too large for the packed pass-1 kernel"; return MIA_HIP_ERR_RANGE; }
  int code = MIA_HIP_OK;      // the first stage that fails ends the call: its code, its message in ctx->err
  pass1_host_reference(p);
  if ((code = pass1_index_reads(p)) || (code = pass1_decide(p)) || (code = pass1_kmer_tables(p))) return code;
  p.lap("ref+kmer");
  if ((code = pass1_allocate(p))) return code;
  p.lap("pack+alloc");
  if ((code = pass1_upload(p))) return code;
  if (p.r.filtered && (code = pass1_filter_stage(p))) return code;
  if (p.r.anchored_ok && p.n_dp > 0 && (code = pass1_anchor_stage(p))) return code;
  if (p.n_dp > 0 && (code = pass1_dp_stage(p))) return code;
  return pass1_download(p);
}

// ---- Myers ------------------------------------------------------------------------------
// `walk` (a single long pair only): the rows 0 .. dist of k_myers_ond's table and the diagonal the search ended on, for the
// walk back (mia_hip_myers_align); left empty when the pair went another way.
struct MyersWalk { std::vector<int32_t> table; int end_k = 0; bool have = false; };
static int myers_run(mia_hip_ctx* ctx, int64_t n, const char* const* seq_a, const char* const* seq_b, const int32_t* mode,
                     const int32_t* maxd, uint32_t* dist, MyersWalk* walk) {
  if (!ctx || n < 0 || (n > 0 && (!seq_a || !seq_b || !mode || !maxd || !dist))) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (n == 0) return MIA_HIP_OK;
  // two kinds of pair: seq_a of up to 320 characters -- one pair per lane (k_myers_lanes), sequences packed as 4-bit IUPAC
  // bitmaps -- and longer ones, one pair per wavefront (k_myers), as ASCII
  static const struct Bits { uint8_t t[256]; Bits() { for (int c = 0; c < 256; c++) t[c] = (uint8_t)iupac_bits((char)c); } } bits;
  std::vector<MyersPair> pairs;
  std::vector<MyersLanePair> lp;
  std::vector<int32_t> long_index, lane_index;
  std::vector<uint32_t> codes;
  std::string blob;
  std::vector<size_t> oa, ob;
  int max_blk = 1;
  size_t ond_lds = 0, n_ond = 0, n_beyond = 0;      // k_myers_ond: LDS of its largest pair, pairs it takes, pairs k_myers may have to finish
  // lengths first (on all host threads: a hundred thousand strlen calls and forty million characters to pack are most of
  // this call's time next to a 0.3 ms kernel), then the offsets, then the packing into the places they name
  std::vector<uint32_t> la_of((size_t)n), lb_of((size_t)n);
  int T = (int)std::thread::hardware_concurrency();
  T = std::max(1, std::min(std::min(T, 32), (int)(n / 2048) + 1));
  auto parallel = [&](auto&& fn) {
    if (T == 1) { fn(0); return; }
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (auto& x : th) x.join();
  };
  std::atomic<bool> too_long{false};      // (written by several host threads)
  parallel([&](int t) {
    for (int64_t i = n * t / T, hi = n * (t + 1) / T; i < hi; i++) {
      const size_t la = strlen(seq_a[i]), lb = strlen(seq_b[i]);
      if (la > 64u * 64u * MYERS_MAX_K || lb >= ((size_t)1 << 31)) { too_long.store(true, std::memory_order_relaxed); la_of[(size_t)i] = 0; lb_of[(size_t)i] = 0; continue; }
      la_of[(size_t)i] = (uint32_t)la; lb_of[(size_t)i] = (uint32_t)lb;
    }
  });
  if (too_long.load()) { ctx->err = "seq_a longer than 32768 characters"; return MIA_HIP_ERR_ARG; }
  std::vector<uint32_t> word_off((size_t)n, 0);
  {
    uint64_t words = 0;
    for (int64_t i = 0; i < n; i++) {
      const size_t la = la_of[(size_t)i], lb = lb_of[(size_t)i];
      const uint64_t need = (la + 7) / 8 + 1 + (lb + 7) / 8 + 1;       // (one spare word behind each sequence: the kernel may fetch it)
      if (la <= 64u * MYERS_LANE_K && words + need < ((uint64_t)1 << 31) && !ctx->myers_no_lanes) {
        MyersLanePair q;
        q.a_off = (uint32_t)words; q.b_off = (uint32_t)(words + (la + 7) / 8 + 1);
        q.la = (int32_t)la; q.lb = (int32_t)lb; q.mode = mode[i]; q.maxd = maxd[i];
        word_off[(size_t)i] = (uint32_t)words;
        words += need;
        lp.push_back(q);
        lane_index.push_back((int32_t)i);
      } else {
        MyersPair q;
        blob.resize((blob.size() + 7) & ~(size_t)7); oa.push_back(blob.size()); blob.append(seq_a[i], la);      // (8-byte starts: k_myers_ond packs a word per load)
        blob.resize((blob.size() + 7) & ~(size_t)7); ob.push_back(blob.size()); blob.append(seq_b[i], lb);
        q.a = nullptr; q.b = nullptr;
        q.la = (int32_t)la; q.lb = (int32_t)lb; q.mode = mode[i]; q.maxd = maxd[i];
        // rows of D-paths k_myers_ond may walk for this pair: all of maxd if the two LDS rows fit beside the sequences
        q.cap = 0; q.pad = 0; q.a_off = q.b_off = 0;
        if (!ctx->myers_no_ond && myers_ond_lds((int)la, (int)lb, 16) <= (size_t)MYERS_OND_LDS_BUDGET) {
          int64_t md = std::min<int64_t>(std::max<int32_t>(maxd[i], 0), (int64_t)la + (int64_t)lb);
          int64_t cap = std::min<int64_t>(md, MYERS_OND_MAX_CAP);
          const int64_t room = ((int64_t)MYERS_OND_LDS_BUDGET - (int64_t)myers_ond_lds((int)la, (int)lb, 0)) / 16 - 1;
          cap = std::min(cap, room);
          // (a pair far apart costs cap^2 / 256 cell steps here before the bit-vector kernel gets it, whose sweep takes
          // (len_b + 64) * ceil(blocks / 64) block steps: stop where the two would cost about the same)
          const double sweep = ((double)lb + 64.0) * (double)(((la + 63) / 64 + 63) / 64);
          cap = std::min<int64_t>(cap, std::max<int64_t>(64, (int64_t)std::sqrt(64.0 * sweep)));
          q.cap = (int32_t)std::max<int64_t>(cap, 0);
          const uint64_t need_ond = (la + 7) / 8 + (lb + 7) / 8;
          if (words + need_ond >= ((uint64_t)1 << 31)) q.cap = 0;
          if (q.cap > 0) { q.a_off = (uint32_t)words; q.b_off = (uint32_t)(words + (la + 7) / 8); words += need_ond; }
          if (q.cap > 0) { ond_lds = std::max(ond_lds, myers_ond_lds((int)la, (int)lb, q.cap)); n_ond++; if (q.cap < md) n_beyond++; }
          else n_beyond++;
        } else n_beyond++;
        pairs.push_back(q);
        long_index.push_back((int32_t)i);
        const int nb = (int)((la + 63) / 64);
        if (nb > max_blk) max_blk = nb;
      }
    }
    codes.assign((size_t)words, 0u);
  }
  {
    auto pack = [&](const char* str, size_t len, uint32_t* dst) {
      const unsigned char* s2 = reinterpret_cast<const unsigned char*>(str);
      for (size_t w = 0; w < (len + 7) / 8; w++) {
        uint32_t v = 0;
        const size_t lim = std::min<size_t>(8, len - w * 8);
        for (size_t c = 0; c < lim; c++) v |= (uint32_t)bits.t[s2[w * 8 + c]] << (4 * c);
        dst[w] = v;
      }
    };
    const size_t nlp = lp.size();
    parallel([&](int t) {
      for (size_t k = nlp * (size_t)t / (size_t)T, hi = nlp * (size_t)(t + 1) / (size_t)T; k < hi; k++) {
        const MyersLanePair& q = lp[k];
        const int64_t i = lane_index[k];
        pack(seq_a[i], (size_t)q.la, codes.data() + q.a_off);
        pack(seq_b[i], (size_t)q.lb, codes.data() + q.b_off);
      }
    });
    // the long pairs k_myers_ond takes: the same packing (one pair may be 16.6 kb: the two sequences on two threads when it is alone)
    const size_t npl = pairs.size();
    if (npl == 1 && pairs[0].cap > 0 && pairs[0].la + pairs[0].lb > 8192) {
      const int64_t i = long_index[0];
      std::thread other([&] { pack(seq_b[i], (size_t)pairs[0].lb, codes.data() + pairs[0].b_off); });
      pack(seq_a[i], (size_t)pairs[0].la, codes.data() + pairs[0].a_off);
      other.join();
    } else
      parallel([&](int t) {
        for (size_t k = npl * (size_t)t / (size_t)T, hi = npl * (size_t)(t + 1) / (size_t)T; k < hi; k++) {
          const MyersPair& q = pairs[k];
          if (q.cap <= 0) continue;
          const int64_t i = long_index[k];
          pack(seq_a[i], (size_t)q.la, codes.data() + q.a_off);
          pack(seq_b[i], (size_t)q.lb, codes.data() + q.b_off);
        }
      });
  }
  PoolLease<char> d_blob;
  PoolLease<MyersPair> d_pairs;
  PoolLease<MyersLanePair> d_lp;
  PoolLease<uint32_t> d_out, d_out_long, d_codes;
  PoolLease<int32_t> d_index, d_table, d_endk;
  const size_t nl = lp.size(), ng = pairs.size();
  if (pool_take(ctx, d_out, (size_t)n)) return MIA_HIP_ERR_NOMEM;
  hipError_t e = hipSuccess;
  // (every allocation first: an early return leaves no copy in flight from the host vectors and no event behind)
  if (nl && (pool_take(ctx, d_lp, nl) || pool_take(ctx, d_index, nl))) return MIA_HIP_ERR_NOMEM;
  if ((nl || n_ond) && pool_take(ctx, d_codes, codes.size() + 8)) return MIA_HIP_ERR_NOMEM;
  if (ng && (pool_take(ctx, d_blob, blob.size() + 1) || pool_take(ctx, d_pairs, ng) || pool_take(ctx, d_out_long, ng))) return MIA_HIP_ERR_NOMEM;
  const bool want_walk = walk && ng == 1 && nl == 0 && n_ond == 1;
  if (want_walk) {
    const size_t cells = ((size_t)pairs[0].cap + 1) * ((size_t)pairs[0].cap + 1);
    if (pool_take(ctx, d_table, cells) || pool_take(ctx, d_endk, (size_t)1)) return MIA_HIP_ERR_NOMEM;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  if (nl) {
    e = hipMemcpyAsync(d_lp, lp.data(), nl * sizeof(MyersLanePair), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_index, lane_index.data(), nl * 4, hipMemcpyHostToDevice, ctx->stream);
  }
  if ((nl || n_ond) && e == hipSuccess && !codes.empty()) e = hipMemcpyAsync(d_codes, codes.data(), codes.size() * 4, hipMemcpyHostToDevice, ctx->stream);
  if (ng && e == hipSuccess) {
    for (size_t i = 0; i < ng; i++) { pairs[i].a = d_blob + oa[i]; pairs[i].b = d_blob + ob[i]; }
    if (n_beyond) e = hipMemcpyAsync(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream);      // (the characters: only k_myers reads them)
    if (e == hipSuccess) e = hipMemcpyAsync(d_pairs, pairs.data(), ng * sizeof(MyersPair), hipMemcpyHostToDevice, ctx->stream);
  }
  if (e0) (void)hipEventRecord(e0, ctx->stream);
  if (nl && e == hipSuccess) {
    hipLaunchKernelGGL(k_myers_lanes, dim3((unsigned)((nl + 63) / 64)), dim3(64), 0, ctx->stream, (const MyersLanePair*)d_lp, (const uint32_t*)d_codes, (int32_t)nl,
                       (const int32_t*)d_index, d_out);
    e = hipGetLastError();
  }
  if (n_ond && e == hipSuccess) {
    e = hipFuncSetAttribute((const void*)k_myers_ond, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
    if (e == hipSuccess) {
      const int grid = (int)(ng < 8192 ? ng : 8192);
      hipLaunchKernelGGL(k_myers_ond, dim3(grid), dim3(MYERS_OND_THREADS), ond_lds, ctx->stream, (const MyersPair*)d_pairs, (const uint32_t*)d_codes, (int32_t)ng, d_out_long,
                         d_table, d_endk);
      e = hipGetLastError();
    }
  }
  if (ng && n_beyond && e == hipSuccess) {
    const int lds = 16 * max_blk * 8;
    e = hipFuncSetAttribute((const void*)k_myers, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) {
      const int grid = (int)(ng < 8192 ? ng : 8192);
      hipLaunchKernelGGL(k_myers, dim3(grid), dim3(64), lds, ctx->stream, d_pairs, (int32_t)ng, d_out_long, n_ond ? 1 : 0);
      e = hipGetLastError();
    }
  }
  if (e1) (void)hipEventRecord(e1, ctx->stream);
  std::vector<uint32_t> out_long(ng);
  if (e == hipSuccess && nl) e = hipMemcpyAsync(dist, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);      // (the long pairs' entries are filled in below)
  if (e == hipSuccess && ng) e = hipMemcpyAsync(out_long.data(), d_out_long, ng * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && e0 && e1) { float ms = 0; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->myers_kernel_ms = ms; }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (e != hipSuccess) { ctx->err = std::string("myers: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  for (size_t i = 0; i < ng; i++) dist[long_index[i]] = out_long[i];
  // (only when k_myers_ond ITSELF found the distance: one it gave up on at its cap and k_myers then finished has D >= cap, and rows
  // >= cap of the table were never written nor allocated -- ADVICE r05; the host's ond_backtrace takes that pair)
  if (want_walk && out_long[0] < (uint32_t)pairs[0].cap) {
    // the rows the walk back reads: 0 .. dist of the table (row d starts at d*d), and the diagonal the search ended on
    const size_t cells = ((size_t)out_long[0] + 1) * ((size_t)out_long[0] + 1);
    walk->table.resize(cells);
    e = hipMemcpyAsync(walk->table.data(), d_table, cells * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&walk->end_k, d_endk, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("myers: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
    walk->have = true;
  }
  return MIA_HIP_OK;
}

extern "C" int mia_hip_myers(mia_hip_ctx* ctx, int64_t n, const char* const* seq_a, const char* const* seq_b, const int32_t* mode,
                             const int32_t* maxd, uint32_t* dist) {
  return myers_run(ctx, n, seq_a, seq_b, mode, maxd, dist, nullptr);
}

// The same distances for pairs the caller has packed already (include/mia_hip.h: 4-bit IUPAC bitmaps, eight to a word, a spare
// word behind every sequence): no strlen, no packing, one pair per lane.  seq_a of more than 64 * MYERS_LANE_K characters is
// refused (mia_hip_myers takes those, one pair per wavefront).  VERDICT r03 item 10: the host side of mia_hip_myers was 17 x the
// kernel's time.
extern "C" int mia_hip_myers_packed(mia_hip_ctx* ctx, int64_t n, const uint32_t* codes, int64_t n_words, const uint32_t* a_off, const uint32_t* b_off,
                                    const int32_t* la, const int32_t* lb, const int32_t* mode, const int32_t* maxd, uint32_t* dist) {
  if (!ctx || n < 0 || n >= ((int64_t)1 << 31) || n_words < 0 || n_words >= ((int64_t)1 << 31) ||
      (n > 0 && (!codes || !a_off || !b_off || !la || !lb || !mode || !maxd || !dist))) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (n == 0) return MIA_HIP_OK;
  std::vector<MyersLanePair> lp((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    if (la[i] < 0 || lb[i] < 0 || la[i] > 64 * MYERS_LANE_K || (int64_t)a_off[i] + (la[i] + 7) / 8 + 1 > n_words || (int64_t)b_off[i] + (lb[i] + 7) / 8 + 1 > n_words) {
      ctx->err = "myers_packed: a sequence lies outside the packed buffer, or seq_a is longer than one lane holds (use mia_hip_myers)";
      return MIA_HIP_ERR_ARG;
    }
    MyersLanePair& q = lp[(size_t)i];
    q.a_off = a_off[i]; q.b_off = b_off[i]; q.la = la[i]; q.lb = lb[i]; q.mode = mode[i]; q.maxd = maxd[i];
  }
  PoolLease<MyersLanePair> d_lp;
  PoolLease<uint32_t> d_out, d_codes;
  if (pool_take(ctx, d_out, (size_t)n) || pool_take(ctx, d_lp, (size_t)n) || pool_take(ctx, d_codes, (size_t)n_words + 8)) return MIA_HIP_ERR_NOMEM;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  hipError_t e = hipMemcpyAsync(d_lp, lp.data(), (size_t)n * sizeof(MyersLanePair), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_codes, codes, (size_t)n_words * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e0) (void)hipEventRecord(e0, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_myers_lanes, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, (const MyersLanePair*)d_lp, (const uint32_t*)d_codes, (int32_t)n,
                       (const int32_t*)nullptr, d_out);
    e = hipGetLastError();
  }
  if (e1) (void)hipEventRecord(e1, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dist, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  else (void)hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && e0 && e1) { float ms = 0; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->myers_kernel_ms = ms; }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (e != hipSuccess) { ctx->err = std::string("myers_packed: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  return MIA_HIP_OK;
}

extern "C" int mia_hip_myers_time(mia_hip_ctx* ctx, double* kernel_ms) {
  if (!ctx || !kernel_ms) return MIA_HIP_ERR_ARG;
  *kernel_ms = ctx->myers_kernel_ms;
  return MIA_HIP_OK;
}

// The alignment behind a distance the device has already established: Myers' furthest-reaching D-paths (1986) for
// D = 0 .. dist, then the walk back with the reference's preferences (mismatch, then a seq_b-only column, then a
// seq_a-only column, else one step down the snake; src/myers_align.c:47-83).  Host code: the table has (dist+1)^2
// cells and is walked once; the O(len * dist / 64) search for `dist` itself ran on the GPU.
static bool ond_backtrace(const char* a, int la, const char* b, int lb, int mode, int dist, std::string* row_a, std::string* row_b) {
  auto bits = [](char c) { return (int)iupac_bits(c); };
  std::vector<int32_t> v((size_t)(dist + 1) * (size_t)(dist + 1), OND_NONE);   // row d starts at d*d, diagonal k at index k+d
  int end_k = 0;
  bool found = false;
  for (int d = 0; d <= dist && !found; d++) {
    const int klo = -d > -la ? -d : -la, khi = d < lb ? d : lb;
    auto prev = [&](int kk) -> int32_t { return (kk < -(d - 1) || kk > d - 1) ? OND_NONE : v[ond_at(d - 1, kk)]; };
    for (int k = klo; k <= khi; k++) {
      int x = ond_cell(d, k, prev);
      if (x == OND_NONE) continue;
      int y = x - k;
      while (x < lb && y < la && x >= 0 && y >= 0 && (bits(b[x]) & bits(a[y]))) { x++; y++; }
      v[ond_at(d, k)] = x;
      if (ond_arrived(mode, x, k, la, lb)) {
        if (d != dist) return false;
        end_k = k; found = true;
        break;
      }
    }
  }
  if (!found) return false;
  return ond_walk_back(v.data(), a, la, b, lb, dist, end_k, row_a, row_b);
}

extern "C" int mia_hip_myers_align(mia_hip_ctx* ctx, const char* seq_a, int32_t mode, const char* seq_b, int32_t maxd, uint32_t* dist,
                                   char* bt_a, char* bt_b) {
  if (!ctx || !seq_a || !seq_b || !dist || mode < 0 || mode > 2) return MIA_HIP_ERR_ARG;
  MyersWalk walk;
  const int rc = myers_run(ctx, 1, &seq_a, &seq_b, &mode, &maxd, dist, (bt_a || bt_b) ? &walk : nullptr);
  if (rc != MIA_HIP_OK || *dist == 0xFFFFFFFFu || (!bt_a && !bt_b)) return rc;
  std::string ra, rb;
  // a long pair: the device's own table, walked back here; a short one (or one the bit-vector kernel finished): the D-paths
  // again on the host, O((len_a + len_b) * dist) for a few hundred characters
  const bool ok = walk.have ? ond_walk_back(walk.table.data(), seq_a, (int)strlen(seq_a), seq_b, (int)strlen(seq_b), (int)*dist, walk.end_k, &ra, &rb)
                            : ond_backtrace(seq_a, (int)strlen(seq_a), seq_b, (int)strlen(seq_b), mode, (int)*dist, &ra, &rb);
  if (!ok) {
    ctx->err = "myers_align: the D-path table does not end at the distance the device computed";
    return MIA_HIP_ERR_DEVICE;
  }
  if (bt_a) memcpy(bt_a, ra.c_str(), ra.size() + 1);
  if (bt_b) memcpy(bt_b, rb.c_str(), rb.size() + 1);
  return MIA_HIP_OK;
}

// ---- measured ceilings (bench.py's roofline) -----------------------------------------------
extern "C" int mia_hip_measure_peaks(mia_hip_ctx* ctx, int64_t copy_bytes, double* hbm_copy_gbs, double* valu_ginst_s) {
  if (!ctx || copy_bytes < (1 << 20)) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  DevBuf<uint4> a, b;
  int rc = MIA_HIP_OK;
  if (hbm_copy_gbs) {
    const int64_t n16 = copy_bytes / 16;
    if (dev_alloc(ctx, a, n16) || dev_alloc(ctx, b, n16)) rc = MIA_HIP_ERR_NOMEM;
    else {
      HIPCHK(hipMemsetAsync(a, 1, (size_t)n16 * 16, ctx->stream));
      float best = 1e30f;
      for (int variant = 0; variant < 8; variant++) {
        const int grid = ctx->cus * (variant & 1 ? 32 : 8);
        for (int rep = 0; rep < 4; rep++) {                   // the first repetition warms the TLBs
          (void)hipEventRecord(e0, ctx->stream);
          switch (variant >> 1) {
            case 0: hipLaunchKernelGGL((k_peak_copy<1, false>), dim3(grid * 2), dim3(256), 0, ctx->stream, (const uint4*)a, (uint4*)b, n16); break;
            case 1: hipLaunchKernelGGL((k_peak_copy<4, false>), dim3(grid), dim3(256), 0, ctx->stream, (const uint4*)a, (uint4*)b, n16); break;
            case 2: hipLaunchKernelGGL((k_peak_copy<4, true>), dim3(grid), dim3(256), 0, ctx->stream, (const uint4*)a, (uint4*)b, n16); break;
            default: hipLaunchKernelGGL((k_peak_copy<8, true>), dim3(grid), dim3(256), 0, ctx->stream, (const uint4*)a, (uint4*)b, n16); break;
          }
          (void)hipEventRecord(e1, ctx->stream);
          HIPCHK(hipEventSynchronize(e1));
          float ms = 0;
          HIPCHK(hipEventElapsedTime(&ms, e0, e1));
          if (alt_env("MIA_HIP_PEAK_DEBUG")) fprintf(stderr, "[peak copy] variant %d rep %d: %.1f GB/s\n", variant, rep, 2.0 * (double)n16 * 16 / (ms * 1e-3) / 1e9);
          if (rep > 0 && ms < best) best = ms;
        }
      }
      *hbm_copy_gbs = 2.0 * (double)n16 * 16 / (best * 1e-3) / 1e9;      // bytes read + bytes written
    }
  }
  if (valu_ginst_s && rc == MIA_HIP_OK) {
    DevBuf<int32_t> out;
    const int wgs = ctx->cus * 8, iters = 4096;               // 8 waves per SIMD: enough to cover the issue latency
    if (dev_alloc(ctx, out, (int64_t)wgs * 256)) rc = MIA_HIP_ERR_NOMEM;
    else {
      float best = 1e30f;
      for (int rep = 0; rep < 4; rep++) {
        (void)hipEventRecord(e0, ctx->stream);
        hipLaunchKernelGGL(k_peak_valu, dim3(wgs), dim3(256), 0, ctx->stream, out, iters, 12345 + rep);
        (void)hipEventRecord(e1, ctx->stream);
        if (hipEventSynchronize(e1) != hipSuccess) break;
        float ms = 0;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess && rep > 0 && ms < best) best = ms;
      }
      *valu_ginst_s = (double)wgs * 4 * iters * PEAK_VALU_OPS_PER_ITER / (best * 1e-3) / 1e9;   // wave instructions per second
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}

// the pure issue ceiling and the clock it was reached at (k_peak_issue): independent v_add_u32, 8 waves per SIMD
extern "C" int mia_hip_measure_issue(mia_hip_ctx* ctx, double* add_ginst_s, double* shader_clock_mhz) {
  if (!ctx || (!add_ginst_s && !shader_clock_mhz)) return MIA_HIP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  const int wgs = ctx->cus * 8, iters = 4096;
  DevBuf<int32_t> out;
  DevBuf<unsigned long long> clk;
  if (dev_alloc(ctx, out, (int64_t)wgs * 256) || dev_alloc(ctx, clk, (int64_t)wgs * 2)) return MIA_HIP_ERR_NOMEM;
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  float best = 1e30f;
  hipError_t e = hipSuccess;
  for (int rep = 0; rep < 4 && e == hipSuccess; rep++) {
    (void)hipEventRecord(e0, ctx->stream);
    hipLaunchKernelGGL(k_peak_issue, dim3(wgs), dim3(256), 0, ctx->stream, out, iters, 4321 + rep, clk);
    (void)hipEventRecord(e1, ctx->stream);
    e = hipEventSynchronize(e1);
    float ms = 0;
    if (e == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && rep > 0 && ms < best) best = ms;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess) { ctx->err = std::string("measure_issue: ") + hipGetErrorString(e); return MIA_HIP_ERR_DEVICE; }
  if (add_ginst_s) *add_ginst_s = (double)wgs * 4 * iters * PEAK_ISSUE_OPS_PER_ITER / (best * 1e-3) / 1e9;
  if (shader_clock_mhz) {
    std::vector<unsigned long long> h((size_t)wgs * 2);
    HIPCHK(hipMemcpy(h.data(), clk, h.size() * 8, hipMemcpyDeviceToHost));
    double cs = 0, rs = 0;
    for (int k = 0; k < wgs; k++) { cs += (double)h[2 * (size_t)k]; rs += (double)h[2 * (size_t)k + 1]; }
    *shader_clock_mhz = rs > 0 ? cs / rs * 100.0 : 0.0;           // s_memrealtime ticks at a constant 100 MHz
  }
  return MIA_HIP_OK;
}

extern "C" int mia_hip_pass1_time(mia_hip_ctx* ctx, double* kernel_ms) {
  if (!ctx || !kernel_ms) return MIA_HIP_ERR_ARG;
  *kernel_ms = ctx->pass1_ms;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_pass1_filtered(mia_hip_ctx* ctx, int64_t* reads) {
  if (!ctx || !reads) return MIA_HIP_ERR_ARG;
  *reads = ctx->pass1_filtered;
  return MIA_HIP_OK;
}

extern "C" int mia_hip_pass1_anchored(mia_hip_ctx* ctx, int64_t* reads) {
  if (!ctx || !reads) return MIA_HIP_ERR_ARG;
  *reads = ctx->pass1_anchored;
  return MIA_HIP_OK;
}
