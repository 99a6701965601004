// emu_quick_lean.cpp -- TEST INFRASTRUCTURE: the quick plan's two forms (csrc/bandx_body.h: bx_quick, bx_quick2, the lean bx_finish) on the
// CPU beside their frozen predecessors (bandx_quick_parent.h), asked the same questions: every diagonal of a window, every NW the kernel
// could run the read under.  Built by tests/test_emul_quick_lean.py into oracle/_build/.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "diag_filter.h"
#include "band_body.h"
#include "bandx_body.h"
#include "bandx_quick_parent.h"

using namespace mia;

namespace {
struct QlRef {
  std::vector<uint8_t> codes;
  std::vector<uint64_t> lo, hi, ok;
  std::vector<uint32_t> kslot;
  std::vector<int32_t> kovf;
  std::vector<KbPair> bits;
  KmerHash ko;
  KmerBits kb;
  RefPlanes rp;
};
struct QlTab {
  std::vector<int32_t> sub, mrow;
  std::vector<int16_t> loss, dl;
  int32_t min_m = 0, max_m = 0;
  bool ok = false;
};

bool same_plan(bool oka, const BxPlan& a, bool okb, const BxPlan& b) {
  if (oka != okb || a.mode != b.mode || a.b0 != b.b0) return false;
  if (!oka) return true;
  return a.d0 == b.d0 && a.w == b.w && a.dstar == b.dstar && a.edge == b.edge;
}
BxPlan blank() { BxPlan p; p.mode = BX_NONE; p.d0 = 0; p.w = 1; p.dstar = 0; p.b0 = 0; p.edge = 0; return p; }

// counts: 0 queries, 1 one-diagonal form planned, 2 one-indel form planned, 3 the one-indel form planned a read the one-diagonal form had
// looked up in the bitmaps (at most BX_QUICK_MAX lost rows on d) and refused, 4 unused, 5 BX_DONE, 6 BX_VALUES, 7 BX_TRACE (either form).
// diff: kind, NW, d, and the two plans' fields.
template <int NW>
int compare_nw(const QlRef& R, const BxTab& T, int s, int len1, const uint8_t* packed, int len2, int st, int64_t* counts, int32_t* diff) {
  int bad = 0;
  auto report = [&](int kind, int d, bool oka, const BxPlan& a, bool okb, const BxPlan& b) {
    if (bad++) return;
    const int32_t v[16] = {kind, NW, d, oka, a.mode, a.d0, a.w, a.b0, a.dstar, a.edge, okb, b.mode, b.d0, b.w, b.b0, b.dstar};
    memcpy(diff, v, sizeof v);
  };
  // (one diagonal in front of the window and one behind it: both versions must refuse them alike)
  for (int d = -1; d <= len1 - len2 + 1; d++) {
    counts[0]++;
    DiagScan<NW> sa, sb, sc2, sd;
    // (the kernel asks bx_plannable first, then loads the read: a read with an N is no query of the quick plan)
    if (!sa.load_read(packed, len2) || !sb.load_read(packed, len2) || !sc2.load_read(packed, len2) || !sd.load_read(packed, len2)) return -1;
    BxPlan pa = blank(), pb = blank(), pc = blank(), pd = blank(), pe = blank();
    const bool oka = parent::bx_quick<NW>(sa, R.rp, R.ko, R.kb, s, len1, len2, st, d, T, &pa);
    const bool okb = bx_quick<NW>(sb, R.rp, R.ko, R.kb, s, len1, len2, st, d, T, &pb);
    if (!same_plan(oka, pa, okb, pb)) report(1, d, oka, pa, okb, pb);
    if (okb) { counts[1]++; counts[5 + (pb.mode == BX_DONE ? 0 : (pb.mode == BX_VALUES ? 1 : 2))]++; }
    // the one-indel form for EVERY query (the kernel asks it about the reads the first form refused; its answer is defined for all)
    const bool okc = parent::bx_quick2<NW>(sc2, R.rp, R.ko, R.kb, s, len1, len2, st, d, T, &pc);
    const bool okd = bx_quick2<NW>(sd, R.rp, R.ko, R.kb, s, len1, len2, st, d, T, &pd);                    // a fresh scan (the kernel)
    if (!same_plan(okc, pc, okd, pd)) report(2, d, okc, pc, okd, pd);
    const bool oke = bx_quick2<NW>(sb, R.rp, R.ko, R.kb, s, len1, len2, st, d, T, &pe);                    // the scan the first form left behind (bx_plan_quick)
    if (!same_plan(okc, pc, oke, pe)) report(3, d, okc, pc, oke, pe);
    if (okd) { counts[2]++; counts[5 + (pd.mode == BX_DONE ? 0 : (pd.mode == BX_VALUES ? 1 : 2))]++; }
    if (okd && !okb) {
      DiagScan<NW> sm;
      sm.load_read(packed, len2);
      sm.seek(R.rp, (int64_t)s + d);
      if (sm.mismatches() <= BX_QUICK_MAX) counts[3]++;
    }
  }
  return bad;
}
}  // namespace

extern "C" void* ql_tab_new(const int32_t* fwd, const int32_t* rc) {
  QlTab* t = new QlTab;
  t->sub.assign(BX_SUB_WORDS, 0); t->mrow.assign(2 * 31 * 4, 0); t->loss.assign(BX_LOSS_WORDS, 0); t->dl.assign(BX_DL_WORDS, 0);
  t->ok = bx_make_tables(fwd, rc, t->sub.data(), t->mrow.data(), t->loss.data(), t->dl.data(), &t->min_m, &t->max_m);
  return t;
}
extern "C" int ql_tab_ok(void* t) { return ((QlTab*)t)->ok ? 1 : 0; }
extern "C" void ql_tab_free(void* t) { delete (QlTab*)t; }

// wrapped: a circular reference whose last 256 codes are the wrap -- the places the bitmaps count are the ones in front of it
extern "C" void* ql_ref_new(const uint8_t* ref_codes, int64_t n_codes, int wrapped) {
  QlRef* r = new QlRef;
  r->codes.assign(ref_codes, ref_codes + n_codes);
  const int64_t words = plane_words(n_codes);
  r->lo.resize((size_t)words); r->hi.resize((size_t)words); r->ok.resize((size_t)words);
  for (int64_t w = 0; w < words; w++) plane_word(ref_codes, n_codes, w, &r->lo[(size_t)w], &r->hi[(size_t)w], &r->ok[(size_t)w]);
  r->rp = RefPlanes{r->lo.data(), r->hi.data(), r->ok.data()};
  bool has_n = false;
  for (int64_t p = 0; p < n_codes; p++) has_n |= ref_codes[p] > 3;
  const int wild = has_n ? BX_WILD : 0;
  const uint32_t kslots = kh_slots_for_entries(n_codes, wild ? kh_wild_entries(ref_codes, n_codes, wild) : 0);
  r->kslot.assign((size_t)kslots * 4, KH_EMPTY);
  r->kovf.assign((size_t)kslots * 2, 0);
  r->ko = KmerHash{r->kslot.data(), r->kovf.data(), kslots - 1, kh_shift_for(kslots), wild};
  for (int64_t p = 0; p < n_codes; p++) kh_insert_wild_host(r->kslot.data(), r->kovf.data(), kslots - 1, r->ko.shift, ref_codes, n_codes, p, wild);
  const int64_t L = wrapped && n_codes > 2 * 256 ? n_codes - 256 : n_codes;
  r->bits.assign((size_t)KB_WORDS, KbPair{0u, 0u});
  for (int64_t p = 0; p < L; p++) kmer_bits_insert(ref_codes, n_codes, p, r->bits.data());
  r->kb = KmerBits{r->bits.data(), (int32_t)L};
  return r;
}
extern "C" void ql_ref_free(void* r) { delete (QlRef*)r; }

// every diagonal of the window [s, s + len1) for the read, under every NW the kernel could run it with (the longest read of the run
// sets NW); returns the number of queries whose answers differ (diff16: the first of them), -1 for a read with an N; 0 queries for a
// window the plan does not take
extern "C" int ql_compare(void* ref, void* tab, int s, int len1, const uint8_t* read_codes, int len2, int st, int64_t* counts, int32_t* diff16) {
  const QlRef& R = *(QlRef*)ref;
  const QlTab& Q = *(QlTab*)tab;
  if (!Q.ok) return -2;
  std::vector<uint32_t> packed((size_t)(len2 / 8 + 2), 0);
  uint8_t* pb = (uint8_t*)packed.data();
  for (int r = 0; r < len2; r++) pb[r >> 1] |= (uint8_t)((read_codes[r] & 15) << ((r & 1) * 4));
  BxTab T{Q.sub.data(), Q.mrow.data(), Q.loss.data(), Q.dl.data(), Q.min_m, Q.max_m, BX_MAXW};
  if (!bx_plannable(R.rp, R.ko, (int64_t)R.codes.size(), s, len1, len2)) return 0;
  int bad = 0;
  for (int nw = (len2 + 63) >> 6; nw <= 4; nw++) {
    int b;
    switch (nw) {
      case 1: b = compare_nw<1>(R, T, s, len1, pb, len2, st, counts, bad ? diff16 + 16 : diff16); break;
      case 2: b = compare_nw<2>(R, T, s, len1, pb, len2, st, counts, bad ? diff16 + 16 : diff16); break;
      case 3: b = compare_nw<3>(R, T, s, len1, pb, len2, st, counts, bad ? diff16 + 16 : diff16); break;
      default: b = compare_nw<4>(R, T, s, len1, pb, len2, st, counts, bad ? diff16 + 16 : diff16); break;
    }
    if (b < 0) return b;
    bad += b;
  }
  return bad;
}
