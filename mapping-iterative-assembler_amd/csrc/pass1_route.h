// pass1_route.h -- what one mia_hip_pass1 call does with its reads: chunk width, shortcuts in front of the whole-strand DP, sizes and
// refusals.  THE one place where that is decided.  Plain C++17, no HIP: pass1_route() reads its argument and nothing else, so a CPU
// test (tests/test_pass1_route_cpu.py) enumerates it against a restatement of every rule and pins the routes of the benched workloads.
// mia_hip_pass1 (mia_hip_tools.inc) fills Pass1RouteIn, asks once, and its stages only follow the answer.  A rule and its reason live
// here, once.
#pragma once
#include <stdint.h>

#include <optional>

#include "../../include/mia_hip.h"
#include "pass1_body.h"

namespace mia {

constexpr int P1_ROUTE_WILD = 3;                       // = BX_WILD (bandx_body.h; held together by mia_hip.hip)
constexpr int P1_LDS_LIMIT = 160 * 1024;               // LDS of a gfx950 compute unit: what one workgroup of k_pass1 may ask for
constexpr int P1_TABLE_MAX_COLS = 1 << 22;             // longest strand the 10-mer tables of the filter and of the anchors are made for (as align_route.h)
constexpr int64_t P1_WILD_MAX_ENTRIES = (int64_t)1 << 24;      // most entries the N columns' spellings may add to those tables
constexpr int64_t P1_KMER_MAX_COLS = (int64_t)1 << 24;         // the -k table's entries hold a position list's start in 24 bits (build_kmer_lists)

struct Pass1RouteIn {
  int64_t n = 0;                       // reads
  int max_len = 1, L = 0;              // longest read; reference columns
  bool circular = false;
  int kmer_len = -1;                   // mia -k (<= 0: no k-mer masks)
  int max_pos = 0;                     // largest positive PSSM entry
  bool flat = false, bx_ok = false;    // the matrix: flat; the band pipeline has tables for it
  int use_bx = 1, use_filter = 1;      // the alt switches of the context (read_alt_switches)
  int64_t p1_other = 0;                // columns of the forward strand that are no plain base
  int64_t wild_entries = 0;            // kh_wild_entries of both strands, where pass1_wants_wild() asked for it (else 0)
  std::optional<int> alt_cpl, alt_plain;      // MIA_HIP_P1_CPL, MIA_HIP_P1_PLAIN (alt build only)
  int waves_cu = 0, cus = 1;           // resident workgroups of k_pass1<cpl> per compute unit (0: not asked yet), compute units
};

enum Pass1Refusal { P1_REFUSE_NONE = 0, P1_REFUSE_HORIZON, P1_REFUSE_KMER_TABLE, P1_REFUSE_LDS };

struct Pass1Route {
  int wl = 0, wrap = 0, len1 = 0;      // wrapped stretch, columns with it, columns of one strand as the kernels see it
  int cpl = P1_CPL_NARROW, plain = 1, ch = 0, nch = 0, mask_words = 0, lds = 0, rows_p = 0;
  int64_t trace_bytes = 0, ckpt_words = 0;      // per workgroup
  int waves_cu = 0;                    // whole waves per SIMD (pass1_set_grid)
  int64_t grid = 0;                    // persistent grid of k_pass1 (0 until the occupancy is known)
  bool fast_ok = false, gen_ok = false, filtered = false, want_wild = false, anchored_ok = false;
  bool need_todo = false, need_ktab = false, rebuild_ktab_for_anchors = false, ref_mostly_bases = false;
  int wild = 0;                        // k_kmer_occ's `wild` for the anchors' tables
  int64_t wild_entries = 0;            // the caller's, 0 when there are too many (the borrowed alignment's kh_entries)
  Pass1Refusal refusal = P1_REFUSE_NONE;
};

inline const char* pass1_refusal_message(Pass1Refusal r) {
  switch (r) {
    case P1_REFUSE_HORIZON: return "PSSM too large for the pass-1 candidate horizon";
    case P1_REFUSE_KMER_TABLE: return "reference too long for the k-mer table";
    case P1_REFUSE_LDS: return "reference too long for the pass-1 LDS masks";
    default: return "";
  }
}
inline int pass1_refusal_code(Pass1Refusal r) { return r == P1_REFUSE_NONE ? MIA_HIP_OK : MIA_HIP_ERR_RANGE; }

// reference strands: add_ref_wrap (src/mia_main.c:637-676): a circular reference carries its first MAX_READ columns again
inline int pass1_wl(const Pass1RouteIn& in) { return in.circular ? (in.L < MAX_READ ? in.L : MAX_READ) : 0; }
inline int pass1_len1(const Pass1RouteIn& in) { return in.L + pass1_wl(in); }

// The premises of the two shortcuts in front of the whole-strand DP.  fast: the diagonal filter (diag_filter.h) -- flat matrix and no
// k-mer mask (a masked DP is a different recurrence); it decides most reads by bit-parallel comparison against every diagonal of both
// strands.  gen: any other matrix the band pipeline has tables for -- the anchored windows in losses (mia_pass1_kernels.h, GEN); the
// diagonal filter stays the flat matrix's.
struct Pass1Premises { bool fast_ok, gen_ok, table_ok; };
inline Pass1Premises pass1_premises(const Pass1RouteIn& in) {
  const bool common = in.use_filter && in.kmer_len <= 0 && pass1_len1(in) >= in.max_len;
  return {in.flat && common, !in.flat && in.bx_ok && in.use_bx && common, pass1_len1(in) <= P1_TABLE_MAX_COLS};
}

// kh_wild_entries is a host walk over both strands: only where the anchored stage could use its answer (N columns to spell out, a
// matrix it runs with, strands the tables are made for)
inline bool pass1_wants_wild(const Pass1RouteIn& in) {
  const Pass1Premises p = pass1_premises(in);
  return (p.fast_ok || p.gen_ok) && in.p1_other && p.table_ok;
}

// persistent grid = exactly the waves that are resident at once (registers AND LDS): a wave that only starts when another has drained
// would run its whole share of the reads on a nearly idle GPU.  Whole waves per SIMD only: an uneven remainder (13 = 4+3+3+3)
// measured slower than 12, the extra workgroups start late.
inline void pass1_set_grid(Pass1Route& r, int waves_cu, int cus, int64_t n) {
  r.waves_cu = waves_cu > 4 ? waves_cu & ~3 : waves_cu;
  r.grid = (int64_t)cus * r.waves_cu;
  if (r.grid > n) r.grid = n;
}

inline Pass1Route pass1_route(const Pass1RouteIn& in) {
  Pass1Route r;
  r.wl = pass1_wl(in); r.wrap = in.L + r.wl; r.len1 = pass1_len1(in);
  // Chunk width.  Dropping candidates further left than the horizon `rel` is exact only if they can never beat a
  // new start: a score is at most rows * max positive entry, a new start costs P(rows+1), a gap of >= rel-1 columns
  // costs P(rel-1).  Wide chunks (768 columns, horizon 256) for the unmasked sweep when that holds, else narrow
  // ones (256 columns, horizon 768), which also skip masked stretches at a finer grain.
  auto horizon_ok = [&](int cpl) {
    return (int64_t)in.max_len * in.max_pos + (GOP + GEP * (in.max_len + 1)) < (int64_t)(GOP + GEP * (p1_rel(cpl) - 1));
  };
  r.cpl = (in.kmer_len <= 0 && horizon_ok(P1_CPL_WIDE)) ? P1_CPL_WIDE : P1_CPL_NARROW;
  if (in.alt_cpl && ((*in.alt_cpl == P1_CPL_WIDE && horizon_ok(P1_CPL_WIDE)) || *in.alt_cpl == P1_CPL_NARROW)) r.cpl = *in.alt_cpl;
  r.ch = p1_ch(r.cpl);
  // the wide unmasked sweep runs on plain keys (pass1_body.h, run_plain); MIA_HIP_P1_PLAIN=0 keeps the packed sweep
  r.plain = in.alt_plain ? *in.alt_plain != 0 : 1;
  // LDS: sub table + 5 carry arrays + 2 column masks (the column masks are only read when the k-mer filter is on)
  r.nch = (r.len1 + r.ch - 1) / r.ch;
  r.mask_words = in.kmer_len > 0 ? r.nch * (r.ch / 32) + 4 : 0;
  r.lds = MAX_READ * 10 + 5 * MAX_READ * 4 + 2 * r.mask_words * 4;
  r.rows_p = (in.max_len + 3) & ~3;
  r.trace_bytes = (int64_t)r.rows_p * r.ch * 2;
  r.ckpt_words = (int64_t)2 * r.nch * 5 * r.rows_p;
  if (in.waves_cu > 0) pass1_set_grid(r, in.waves_cu, in.cus, in.n);

  const Pass1Premises p = pass1_premises(in);
  r.fast_ok = p.fast_ok; r.gen_ok = p.gen_ok;
  r.ref_mostly_bases = in.p1_other * 50 <= in.L;      // fewer than 2 % of the columns are N (what align_all is told as well)
  r.filtered = r.fast_ok && r.ref_mostly_bases;
  // the anchored stage behind the filter (or in its place: a reference full of ambiguity codes, mt311 itself, leaves the filter
  // nothing to decide): the windows' 10-mer tables list the N columns under every spelling (bandx_body.h, N COLUMNS)
  r.want_wild = pass1_wants_wild(in);
  r.wild_entries = (r.want_wild && in.wild_entries <= P1_WILD_MAX_ENTRIES) ? in.wild_entries : 0;
  r.anchored_ok = (r.fast_ok || r.gen_ok) && (in.p1_other == 0 || r.wild_entries > 0) && p.table_ok;
  r.need_todo = r.filtered || r.anchored_ok;          // the list of the reads that are left, and its count
  r.need_ktab = r.need_todo && p.table_ok;            // the 10-mer tables of both strands: the filter's rule (c) (diag_filter.h: KmerOcc), the anchors
  // the anchors' tables: with the N columns' spellings (the filter's rule (c) wants them without)
  r.rebuild_ktab_for_anchors = r.anchored_ok && r.need_ktab && (in.p1_other || !r.filtered);
  r.wild = (r.rebuild_ktab_for_anchors && in.p1_other) ? P1_ROUTE_WILD : 0;

  if (!horizon_ok(r.cpl)) r.refusal = P1_REFUSE_HORIZON;
  else if (in.kmer_len > 0 && (int64_t)r.wrap >= P1_KMER_MAX_COLS) r.refusal = P1_REFUSE_KMER_TABLE;
  else if (r.lds > P1_LDS_LIMIT) r.refusal = P1_REFUSE_LDS;
  return r;
}

// Complement of one reference character for the reverse strand (src/map_align.c:418-432): IUPAC codes in either case, '-' stays,
// anything that is no letter becomes N.  (A lower-case letter that is no IUPAC code comes out as ' ': the table this replaces added
// 32 to its empty entries, and the strands it makes are compared with the reference's byte by byte.)
inline char revcom_char_host(char b) {
  if (b == '-') return '-';
  const bool lower = b >= 'a' && b <= 'z';
  char r = 0;
  switch (lower ? b - 32 : b) {
    case 'A': r = 'T'; break;  case 'C': r = 'G'; break;  case 'G': r = 'C'; break;  case 'T': r = 'A'; break;  case 'U': r = 'A'; break;
    case 'R': r = 'Y'; break;  case 'Y': r = 'R'; break;  case 'K': r = 'M'; break;  case 'M': r = 'K'; break;
    case 'B': r = 'V'; break;  case 'V': r = 'B'; break;  case 'D': r = 'H'; break;  case 'H': r = 'D'; break;
    case 'S': r = 'S'; break;  case 'W': r = 'W'; break;  case 'N': r = 'N'; break;  case 'X': r = 'X'; break;
    default: break;
  }
  if (lower) return (char)(r + 32);
  return r ? r : 'N';
}

}  // namespace mia
