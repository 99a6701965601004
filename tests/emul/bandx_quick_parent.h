// bandx_quick_parent.h -- TEST INFRASTRUCTURE: bx_finish, bx_quick and bx_quick2 as csrc/bandx_body.h had them before the quick plan was made
// leaner (one seek per read, no N credit in the quick forms, block tests by clean-run masks, the bitmaps' answers carried from the first
// form to the second), frozen word for word in a namespace of their own.  tests/test_emul_quick_lean.py asks both versions the same
// questions and wants the same BxPlan, field by field.  Everything these three call (DiagScan, bx_loss_rows, bx_count, bx_rows_loss,
// bx_window_nmin, bx_ones_span, the tables) is the live code: none of it changed.  The one departure from the original text: the two
// calls of bx_finish name this namespace (argument-dependent look-up finds the live one too).  Include behind bandx_body.h.  Do not edit.
#pragma once
namespace mia {
namespace parent {
// B0 (the loss of one valid path) and what follows from it
// PATHS: 0 = whatever the anchors say, 1 = the caller knows d_first == d_last, 2 = the caller knows they differ
template <int NW, int PATHS = 0>
MIA_HD inline void bx_finish(DiagScan<NW>& sc, const RefPlanes& rp, const BxAnchors& an, int s, int len1, int len2, int st, const BxTab& T, BxPlan* out) {
  out->mode = BX_NONE;
  const int R = len2 - 1, d_first = an.d_first, d_last = PATHS == 1 ? an.d_first : an.d_last;
  uint64_t m1[NW];
  sc.seek(rp, (int64_t)s + d_first);
#pragma unroll
  for (int j = 0; j < NW; j++) m1[j] = bx_loss_rows<NW>(sc, j);
  int b0 = 0, nfail = 0;
  if (PATHS == 1 || (PATHS == 0 && d_first == d_last)) {
    b0 = bx_rows_loss<NW>(sc, m1, 0, len2, len2, st, T, 0, &nfail);
  } else {
    // rows [0, t) on d_first, one gap, the rest on d_last: a column gap (d_last > d_first) or `skip` inserted rows
    const int shift = d_last - d_first, skip = shift < 0 ? -shift : 0;            // |shift| < BX_MAXW
    int t_lo = an.t_lo, t_hi = an.t_hi - skip;
    if (t_hi > R - skip) t_hi = R - skip;
    if (t_lo > t_hi) t_lo = t_hi;
    if (t_lo < 1) { out->b0 = BXF_PATH; return; }
    uint64_t m2[NW];
    DiagScan<NW> s2 = sc;
    s2.seek(rp, (int64_t)s + d_last);
#pragma unroll
    for (int j = 0; j < NW; j++) m2[j] = bx_loss_rows<NW>(s2, j);
    // the switch row with the fewest mismatches in [t_lo, t_hi]
    int cur = bx_count<NW>(m1, 0, t_lo) + bx_count<NW>(m2, t_lo + skip, len2), best = cur, tbest = t_lo;
    for (int t = t_lo + 1; t <= t_hi; t++) {
      cur += bx_bit<NW>(m1, t - 1) - bx_bit<NW>(m2, t - 1 + skip);
      if (cur < best) { best = cur; tbest = t; }
    }
    b0 = shift > 0 ? GOP + GEP * shift : GOP + (GEP + T.max_m) * skip;
    b0 = bx_rows_loss<NW>(sc, m1, 0, tbest, len2, st, T, b0, &nfail);
    b0 = bx_rows_loss<NW>(s2, m2, tbest + skip, len2, len2, st, T, b0, &nfail);
  }
  const bool proof = nfail == 0;
  // what bounds the optimum is the value the RECURRENCE reaches along the written-down path, which the new-start quirk
  // can push below the path's own (found by tools/band_campaign.py with the ancient matrix: two heavy substitutions in
  // rows 0 and 1, a start in row 2 that forfeits 214, and a six-column gap that then wins by 30)
  const int b0x = b0 + nfail * T.max_m;
  out->b0 = BXF_BUDGET;
  // the pigeonhole: a path that crosses no block cleanly loses more than B0.  Against a reference full of ambiguity codes B0
  // is mostly N columns (ten of them under a 100-base read, 210 each) -- but so is every other path's loss: the window-wide
  // credit (bx_make_tables, bx_window_nmin) is worked out only for the reads the plain sum turns away
  int ncredit = 0;
  if (b0x > an.budget || (an.l_out >= 0 && an.l_out <= b0x)) {
    if (T.loss[BX_LOSS_NCRED + st * BX_NCRED_K + 1] > 0) {
      const int nm = bx_window_nmin(rp, s, len1, len2, an.fine != 0);
      const int16_t* cum = T.loss + BX_LOSS_NCRED + st * BX_NCRED_K;
      // (beyond the table every further column carries what the last one did: the interior rows' credit)
      if (nm > 0) ncredit = nm < BX_NCRED_K ? cum[nm] : cum[BX_NCRED_K - 1] + (nm - (BX_NCRED_K - 1)) * (cum[BX_NCRED_K - 1] - cum[BX_NCRED_K - 2]);
    }
  }
#ifdef BX_DIAG
  bx_diag[0] = b0x; bx_diag[1] = an.budget; bx_diag[2] = an.l_out; bx_diag[3] = ncredit; bx_diag[4] = an.fine; bx_diag[5] = an.s_un; bx_diag[6] = an.a_hi - an.a_lo;
#endif
  if (b0x > an.budget + ncredit) return;
  // Anchors were set aside (bx_anchors, bx_fine_anchors): a path that crosses none of the kept ones cleanly must lose more than B0.
  // l_out charges it every block that is clean nowhere outside the kept range.  Six-mers are clean somewhere by chance -- against a
  // reference with an N in every tenth column half the blocks are, and l_out collapsed -- but a path does not get to USE them all:
  // it has at most J = B0 / (GOP + GEP) events (each costs that much), so its rows lie on at most J + 1 diagonals, and the blocks it
  // crosses cleanly are clean on one of those: at most the J + 1 largest per-diagonal counts together (fc2 diagonals hold two, fc1
  // hold one or more, none holds three).  Every other block is broken -- by a row that is no match (fdl_b) or by an event, which
  // pays for the blocks it touches (the netting of the stray tables).
  int l_out = an.l_out;
  if (an.fine && l_out >= 0 && an.fc2 >= 0) {
    const int m = b0x / (GOP + GEP) + 1;
    const int two = m < an.fc2 ? m : an.fc2, rest = m - two, ones = an.fc1 - an.fc2;
    const int t = 2 * two + (rest < ones ? rest : ones);
    const int alt = an.budget + 1 - an.fmax * t;
    if (alt > l_out) l_out = alt;
  }
  if (l_out >= 0 && l_out + ncredit <= b0x) { out->b0 = BXF_SPAN; return; }
  // how far a path that loses no more than b0 can stray from the anchors: all of b0 spent on one gap (band_body.h) --
  // or, tighter, what is left of b0 once every block that occurs nowhere in the window has been paid for (an.s_un: such
  // a block costs dl wherever it is crossed, unless a gap of the path itself breaks it -- the stray tables are net of
  // that).  In full: loss(P) >= s_un + sum over P's events of (cost - dl of the unanchored blocks the event touches), every
  // term >= 0; to be n diagonals off an anchor, the events between that place and the anchor add up to n in one direction.
  int g_dn = b0x < GOP + GEP ? 0 : (b0x - GOP) / GEP, g_up = g_dn;
  if (g_dn > 0) {
    const int x = b0x - an.s_un;
    if (x < 0) { out->b0 = BXF_PATH; return; }         // (cannot happen: every path pays for the blocks that occur nowhere)
    const int16_t* dn = T.dl + (an.fine ? bx_stray_off_fine(st, 0) : bx_stray_off(st, len2, 0));
    const int16_t* up = T.dl + (an.fine ? bx_stray_off_fine(st, 1) : bx_stray_off(st, len2, 1));
    if (g_dn > BX_GMAX) g_dn = g_up = BX_GMAX + 1;     // (beyond the tables: the band is too wide anyway)
    else {
      // either side can be reached either way: below the anchors by skipped rows behind them or by a column gap in front
      // of them (the path starts low and comes up), above them the other way round
      while (g_dn > 0 && dn[g_dn] > x && up[g_dn] > x) g_dn--;
      g_up = g_dn;
    }
  }
  // N CREDIT.  A band of [a_lo - G, a_hi + G] is already proven, the written-down path P0 lies in it.  Every N column c
  // with a_hi + G <= c <= R + a_lo - G (window columns) is crossed by EVERY path P of that band that starts in row 0: by a row
  // r = c - d for a diagonal d of the band (cost >= kap of that depth range) or inside a column gap (GEP >= kap).  Take that
  // much (credit = the sum of kap over those columns) out of both sides: P's events must fit into y = B0 - credit, where an
  // event costs, net of the credit it may consume, at least GOP -- a column gap GOP + GEP per column that is NOT one
  // of those, skipped rows GOP + (GEP + min M) each (they cross nothing), a late start of r rows GOP + GEP (r + 1) +
  // r min M (it misses at most r of the columns).  P runs through an anchor somewhere (the pigeonhole), so it never is
  // further from the anchors than its column gaps add up to, or its skipped rows:
  //   y < GOP      no event at all: a pure diagonal through an anchor.
  //   j gaps       hold m_j = (y - j GOP) / GEP columns without credit between them, and each of them at most H(m_j) credited
  //                ones, H(m) = the most credited columns in a stretch with at most m others (bx_ones_span): together no
  //                more than m_j + min(all credited, j H(m_j)) columns;
  //   skipped rows number at most (y - GOP) / (GEP + min M).
  // The band this gives is proven in turn, so the argument can be repeated with it (more columns count, y shrinks).
  // (Against mt311, every tenth column an ambiguity code, B0 is mostly such columns: without the credit the band would
  // be 20-30 diagonals wide.)  sc sits on d_first: bit q of its planes is window column d_first + q.
  if (g_dn + g_up > 0) {
    int G = b0x < GOP + GEP ? 0 : (b0x - GOP) / GEP;
    const int gt = g_dn > g_up ? g_dn : g_up;
    if (gt <= BX_GMAX && gt < G) G = gt;
    for (int pass = 0; pass < 2 && G > 0; pass++) {
      const int q_lo = an.a_hi + G - d_first, q_hi = R + an.a_lo - G - d_first;      // (0 <= q_lo, q_hi <= R)
      int credit = 0, k = 0, dmin = 1 << 14;              // dmin: the least a credited column costs MORE when a row crosses it than the credit it carries
      uint64_t cm[NW];
#pragma unroll
      for (int j = 0; j < NW; j++) {
        uint64_t w = ~sc.cok[j] & sc.rows[j];
        cm[j] = 0;
        while (w) {
          const int t = df_ctz(w), q = j * 64 + t;
          w &= w - 1;
          if (q < q_lo || q > q_hi) continue;
          int r_lo = q + d_first - an.a_hi - G, r_hi = q + d_first - an.a_lo + G;
          if (r_lo < 0) r_lo = 0;
          if (r_hi > R) r_hi = R;
          const int kv = T.loss[BX_LOSS_KAP + (st * 31 + sm_depth(r_lo, len2)) * 31 + sm_depth(r_hi, len2)];
          if (kv <= 0) continue;
          const int kv2 = T.loss[BX_LOSS_KAP2 + (st * 31 + sm_depth(r_lo, len2)) * 31 + sm_depth(r_hi, len2)];
          if (kv2 - kv < dmin) dmin = kv2 - kv;
          credit += kv;
          k++;
          cm[j] |= 1ull << t;
        }
      }
      const int y = b0x - credit;
      if (credit <= 0 || y >= 4 * GOP) break;
      // A credited column under a ROW costs lambda, which may exceed the credit it carries (min(GEP, lambda): 210 against 200 with the
      // flat matrix) by dmin or more; only the columns inside the path's gaps get away with GEP.  A path with j gaps that hold
      // h of the k credited columns therefore needs  j GOP + GEP m + (k - h) dmin <= y  -- with ten N columns under a read that is
      // what tells "one substitution, no room for any gap" (the plan finishes the read) from "one substitution and a gap of one".
      if (dmin < 0 || dmin >= (1 << 14)) dmin = 0;
      int gn = 0;
      if (y >= GOP) {
        const int rows_room = y - GOP - k * dmin;                   // skipped rows cross nothing: every credited column is under a row
        gn = rows_room >= 0 ? rows_room / (GEP + T.min_m) : 0;
        // (H is worked out once, for the one-gap case's m -- the largest: H grows with m, so the same value bounds the cases of two
        // and more gaps from above; walking the bit masks once per case was a third of the planner's time against mt311)
        const int h1 = bx_ones_span<NW>(cm, (y - GOP) / GEP);
        for (int j = 1; j * GOP <= y; j++) {
          const int h = j * h1 < k ? j * h1 : k, room = y - j * GOP - (k - h) * dmin;
          if (room < 0) continue;
          const int tot = room / GEP + h;
          if (tot > gn) gn = tot;
        }
      }
      if (gn >= G) break;
      G = gn;
      if (gn < g_dn) g_dn = gn;
      if (gn < g_up) g_up = gn;
    }
  }
  // (one diagonal more where the window's first column is within reach, as band_body.h)
  if (an.a_lo - g_dn - 1 < 0) { g_dn++; g_up++; }
  const int d0 = an.a_lo - g_dn, w = an.a_hi - an.a_lo + g_dn + g_up + 1;
  out->b0 = BXF_WIDTH;
  if (w > T.maxw) return;
  out->d0 = d0; out->w = w; out->b0 = b0; out->dstar = d_first;
  if (d_first != d_last || !proof) out->mode = BX_TRACE;
  else out->mode = w == 1 ? BX_DONE : BX_VALUES;
  // the widest band of the read's class must not leave the window anywhere for the plain form of the recurrence
  const int wc = bx_class_width(bx_class_of(w));
  out->edge = !(d0 >= 0 && len2 - 1 + d0 + wc <= len1);
}
template <int NW>
MIA_HD inline bool bx_quick(DiagScan<NW>& sc, const RefPlanes& rp, const KmerHash& kh, const KmerBits& kb, int s, int len1, int len2, int st, int d, const BxTab& T,
                            BxPlan* out) {
  constexpr int NB = bx_nb_max<NW>();
  out->mode = BX_NONE; out->b0 = 0;
  if (!kb.w || d < 0 || d > len1 - len2 || len1 > kb.ref_len) return false;
  if (kh.wild > 0 && !all_bases(rp, s, (int64_t)s + len1)) return false;      // (a reference with N columns: only the windows that hold none -- see above)
  const int R = len2 - 1, nb_cut = bx_blocks_of(len2);
  sc.seek(rp, (int64_t)s + d);
  uint64_t m1[NW];
  int nm = 0;
#pragma unroll
  for (int j = 0; j < NW; j++) { m1[j] = bx_loss_rows<NW>(sc, j); nm += df_popc(m1[j]); }
  if (nm > BX_QUICK_MAX) return false;
  const int16_t* dl = T.dl + (st * (MAX_READ + 1) + len2) * BX_BLOCKS;
  uint32_t kidx[NB], w1[NB], w2[NB];
  int32_t dlv[NB];
#pragma unroll
  for (int b = 0; b < NB; b++) {
    kidx[b] = 0; dlv[b] = 0; w1[b] = 0; w2[b] = 0;
    if (b < nb_cut) {
      kidx[b] = bx_kmer_planes<NW>(sc, bx_block_row(b, len2, nb_cut));
      const KbPair pr = kb.w[kidx[b] >> 5];
      w1[b] = pr.present; w2[b] = pr.repeated;
      dlv[b] = dl[b];
    }
  }
  BX_LOADS_ISSUED();
  int budget = -1, nbv = 0, s_un = 0, b_lo = -1, b_hi = -1;
#pragma unroll
  for (int b = 0; b < NB; b++) {
    if (b >= nb_cut) continue;
    const int o = bx_block_row(b, len2, nb_cut);
    const bool clean = bx_count<NW>(m1, o, o + DF_K) == 0;
    const bool present = ((w1[b] >> (kidx[b] & 31u)) & 1u) != 0u, repeated = ((w2[b] >> (kidx[b] & 31u)) & 1u) != 0u;
    if (!present) {                           // occurs nowhere: every path breaks this block
      budget += dlv[b]; s_un += dlv[b]; nbv++;
    } else if (clean && !repeated) {          // the reference's own 10-mer of this place, and its only one: anchored on d
      budget += dlv[b]; nbv++;
      if (b_lo < 0) b_lo = b;
      b_hi = b;
    }
  }
  if (nbv < BX_MIN_BLOCKS || b_lo < 0) return false;
  BxAnchors an;
  an.fail = 0; an.a_lo = d; an.a_hi = d; an.d_first = d; an.d_last = d; an.budget = budget; an.t_lo = 1; an.t_hi = R; an.l_out = -1; an.s_un = s_un;
  an.r_head = bx_block_row(b_lo, len2, nb_cut); an.r_tail = bx_block_row(b_hi, len2, nb_cut) + DF_K; an.rescue = 0; an.fine = 0; an.fc1 = 0; an.fc2 = 0; an.fmax = 0;
  parent::bx_finish<NW, 1>(sc, rp, an, s, len1, len2, st, T, out);
  if (out->mode == BX_NONE) { out->b0 = 0; return false; }
  return true;
}
template <int NW>
MIA_HD inline bool bx_quick2(DiagScan<NW>& sc, const RefPlanes& rp, const KmerHash& kh, const KmerBits& kb, int s, int len1, int len2, int st, int d, const BxTab& T,
                             BxPlan* out) {
  constexpr int NB = bx_nb_max<NW>();
  out->mode = BX_NONE; out->b0 = 0;
  if (!kb.w || d < 0 || d > len1 - len2 || len1 > kb.ref_len) return false;
  if (kh.wild > 0 && !all_bases(rp, s, (int64_t)s + len1)) return false;      // (a reference with N columns: only the windows that hold none -- see above)
  const int R = len2 - 1, nb_cut = bx_blocks_of(len2);
  const int16_t* dl = T.dl + (st * (MAX_READ + 1) + len2) * BX_BLOCKS;
  uint32_t kidx[NB], w1[NB], w2[NB];
  int32_t dlv[NB];
#pragma unroll
  for (int b = 0; b < NB; b++) {
    kidx[b] = 0; dlv[b] = 0; w1[b] = 0; w2[b] = 0;
    if (b < nb_cut) {
      kidx[b] = bx_kmer_planes<NW>(sc, bx_block_row(b, len2, nb_cut));
      const KbPair pr = kb.w[kidx[b] >> 5];
      w1[b] = pr.present; w2[b] = pr.repeated;
      dlv[b] = dl[b];
    }
  }
  BX_LOADS_ISSUED();
  uint32_t uniq = 0, absent = 0;               // bit b: the block's 10-mer occurs once / nowhere in the reference
#pragma unroll
  for (int b = 0; b < NB; b++) {
    if (b >= nb_cut) continue;
    const bool present = ((w1[b] >> (kidx[b] & 31u)) & 1u) != 0u, repeated = ((w2[b] >> (kidx[b] & 31u)) & 1u) != 0u;
    if (!present) absent |= 1u << b; else if (!repeated) uniq |= 1u << b;
  }
  // the unique blocks that are clean on diagonal x (bit b), for x = d - SHIFT .. d + SHIFT: one seek, then a column at a time
  uint32_t on[2 * BX_QUICK_SHIFT + 1];
  sc.seek(rp, (int64_t)s + d - BX_QUICK_SHIFT);
#pragma unroll
  for (int k = 0; k <= 2 * BX_QUICK_SHIFT; k++) {
    if (k) sc.advance(rp, (int64_t)s + d - BX_QUICK_SHIFT + k);
    uint64_t m[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) m[j] = bx_loss_rows<NW>(sc, j);
    uint32_t c = 0;
#pragma unroll
    for (int b = 0; b < NB; b++) {
      if (b >= nb_cut) continue;
      const int o = bx_block_row(b, len2, nb_cut);
      if (bx_count<NW>(m, o, o + DF_K) == 0) c |= 1u << b;
    }
    const int x = d - BX_QUICK_SHIFT + k;
    on[k] = (x >= 0 && x <= len1 - len2) ? (c & uniq) : 0u;       // (the written-down path must stay inside the window: bx_anchors' BXF_PATH)
  }
  const uint32_t cd = on[BX_QUICK_SHIFT];
  if (!cd) return false;                       // no anchor on the read's own diagonal (an indel in its first rows: the full plan's end-indel rescue)
  const int b_first = 31 - df_clz32(cd);       // the last block anchored on d
  int best = -1, best_n = 0;
#pragma unroll
  for (int k = 0; k <= 2 * BX_QUICK_SHIFT; k++) {
    if (k == BX_QUICK_SHIFT) continue;
    const uint32_t c2 = on[k];
    if (!c2 || (c2 & ((2u << b_first) - 1u))) continue;            // nothing there, or a block of it in front of d's last: not "d, one indel, d2"
    const int nn = df_popc32(c2);
    if (nn > best_n) { best_n = nn; best = k; }
  }
  if (best < 0) return false;
  const uint32_t c2 = on[best];
  const int d2 = d - BX_QUICK_SHIFT + best;
  const uint32_t fam = cd | c2 | absent;
  int budget = -1, s_un = 0, nbv = 0;
#pragma unroll
  for (int b = 0; b < NB; b++) {
    if (!((fam >> b) & 1u)) continue;
    budget += dlv[b]; nbv++;
    if ((absent >> b) & 1u) s_un += dlv[b];
  }
  if (nbv < BX_MIN_BLOCKS) return false;
  const int b_lo = df_ctz32(cd), b_last = df_ctz32(c2), b_hi = 31 - df_clz32(c2);
  BxAnchors an;
  an.fail = 0; an.a_lo = d < d2 ? d : d2; an.a_hi = d < d2 ? d2 : d; an.d_first = d; an.d_last = d2; an.budget = budget; an.l_out = -1; an.s_un = s_un;
  an.t_lo = bx_block_row(b_first, len2, nb_cut) + DF_K; an.t_hi = bx_block_row(b_last, len2, nb_cut);
  if (an.t_lo < 1) an.t_lo = 1;
  an.r_head = bx_block_row(b_lo, len2, nb_cut); an.r_tail = bx_block_row(b_hi, len2, nb_cut) + DF_K; an.rescue = 0; an.fine = 0; an.fc1 = 0; an.fc2 = 0; an.fmax = 0;
  (void)R;
  parent::bx_finish<NW, 2>(sc, rp, an, s, len1, len2, st, T, out);
  if (out->mode == BX_NONE) { out->b0 = 0; return false; }
  return true;
}
}  // namespace parent
}  // namespace mia
