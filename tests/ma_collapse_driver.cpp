// Host caller of the shared code of the duplicate consensus (csrc/ma_collapse_body.h: what the kernels of mia_ma_collapse_kernels.h run
// per lane), in the kernels' own stages -- plan (a cluster per lane, the offsets of the count array), count (a chunk of MA_COL_K sorted
// entries per wavefront, 64 columns at a time, decided on the spot or added to the count array), decide (a column of the count array
// per lane, its cluster by bisection) -- over arrays of exactly the device's sizes, so that AddressSanitizer sees every index.  The
// duplicate filter's results come from ma_dedup_body.h in the stages of tests/ma_dedup_driver.cpp.  Beside it a serial walk that shares
// only the input: a sort, set_uniq_in_fsdb's loop, then clusters, records, columns and members as nested loops.  For every tolerance
// in 0, 1, 2, 7 the two must agree; the staged form's results are printed for the test to compare with its own restatement.
//
//   ma_collapse_driver <file>       file: "L n", then n lines "start end rc score mate vote SEQ" (SEQ: the record's columns, "." for none)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_collapse_body.h"

using namespace mia;

struct Input {
  int32_t L = 0;
  int64_t n = 0;
  std::vector<int32_t> start, end, score;
  std::vector<uint8_t> rc, vote;
  std::vector<int64_t> mate, col_off;
  std::string seq;                                           // padded to a multiple of MA_REC_LANE behind col_off[n], as the device's is
};

struct Result {
  std::string seq;
  std::vector<int32_t> members;
  std::vector<int64_t> hist;
  int64_t collapsed = 0, changed = 0;
  bool operator==(const Result& o) const { return seq == o.seq && members == o.members && hist == o.hist && collapsed == o.collapsed && changed == o.changed; }
};

// ---- the duplicate filter's stages (tests/ma_dedup_driver.cpp), as far as the collapse reads their results -----------------------
struct Dedup {
  int64_t M = 0, R = 0, C = 0;
  std::vector<uint32_t> sm, run_id, run_first, cluster_of, anchor;
  std::vector<unsigned long long> best;
};

static Dedup dedup_stages(const Input& in, int32_t t) {
  const int64_t n = in.n;
  const int32_t L = in.L;
  const int W = ma_dedup_width(L);
  Dedup d;
  std::vector<uint64_t> key[2] = {std::vector<uint64_t>((size_t)n), std::vector<uint64_t>((size_t)n)};
  std::vector<uint32_t> val[2] = {std::vector<uint32_t>((size_t)n), std::vector<uint32_t>((size_t)n)};
  for (int64_t r = 0; r < n; r++) {
    key[0][(size_t)r] = ma_dedup_record_key(L, W, in.start.data(), in.end.data(), in.rc.data(), in.mate.data(), r);
    val[0][(size_t)r] = (uint32_t)r;
    if (key[0][(size_t)r] != MA_DEDUP_NO_KEY) d.M++;
  }
  int cur = 0;
  for (int p = 0; p < ma_dedup_passes(L); p++, cur ^= 1) {
    std::vector<int64_t> count(257, 0);
    for (int64_t i = 0; i < n; i++) count[(size_t)((key[cur][(size_t)i] >> (8 * p)) & 255) + 1]++;
    for (int k = 0; k < 256; k++) count[(size_t)k + 1] += count[(size_t)k];
    for (int64_t i = 0; i < n; i++) {
      const int64_t at = count[(size_t)((key[cur][(size_t)i] >> (8 * p)) & 255)]++;
      key[cur ^ 1].at((size_t)at) = key[cur][(size_t)i];
      val[cur ^ 1].at((size_t)at) = val[cur][(size_t)i];
    }
  }
  const std::vector<uint64_t>& sk = key[cur];
  d.sm = val[cur];
  const int64_t M = d.M;
  if (M == 0) return d;
  std::vector<uint64_t> run_key;
  d.run_id.resize((size_t)M);
  for (int64_t i = 0; i < M; i++) {
    if (i == 0 || sk[(size_t)i - 1] != sk[(size_t)i]) { d.run_first.push_back((uint32_t)i); run_key.push_back(sk[(size_t)i]); d.best.push_back(0); }
    d.run_id[(size_t)i] = (uint32_t)(run_key.size() - 1);
    const int64_t f = d.sm[(size_t)i];
    const unsigned long long v = ma_dedup_pack(in.score[(size_t)f], ma_dedup_index(in.mate.data(), f));
    if (v > d.best.back()) d.best.back() = v;
  }
  const int64_t R = d.R = (int64_t)run_key.size();
  d.run_first.push_back((uint32_t)M);
  std::vector<uint32_t> mark((size_t)R, 0);
  for (int64_t k = 0; k < R; k = ma_dedup_next(run_key.data(), R, k, W, t)) mark[(size_t)k] = 1;      // (the orbit of run 0: what the doubling marks)
  d.cluster_of.resize((size_t)R);
  for (int64_t k = 0; k < R; k++) {
    if (mark[(size_t)k]) d.anchor.push_back((uint32_t)k);
    d.cluster_of[(size_t)k] = (uint32_t)(d.anchor.size() - 1);
  }
  d.C = (int64_t)d.anchor.size();
  d.anchor.push_back((uint32_t)R);
  return d;
}

// ---- the collapse in the kernels' stages ----------------------------------------------------------------------------------------------
static Result staged(const Input& in, int32_t t, const std::vector<int32_t>* rec_of) {
  const Dedup dd = dedup_stages(in, t);
  const int64_t n = in.n, T = in.col_off[(size_t)n];
  Result out;
  out.seq.assign(in.seq, 0, (size_t)T);
  out.members.assign((size_t)n, 0);
  out.hist.assign(MA_COL_HIST, 0);
  const int64_t C = dd.C, M = dd.M;
  if (C == 0) return out;
  std::vector<uint8_t> revcom(in.rc);
  const MaRecords v{n, in.L, in.start.data(), revcom.data(), in.col_off.data(), in.seq.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const MaColDedup d{M, C, dd.sm.data(), dd.run_id.data(), dd.run_first.data(), dd.cluster_of.data(), dd.anchor.data(), dd.best.data(), in.mate.data(), in.start.data(),
                     rec_of ? rec_of->data() : nullptr, in.vote.data()};
  // plan
  std::vector<int32_t> rep_f((size_t)C), rep_b((size_t)C);
  std::vector<int64_t> cnt_off((size_t)C + 1);
  int64_t Q = 0;
  for (int64_t c = 0; c < C; c++) {
    int64_t lo, hi;
    int32_t F, B;
    const int64_t size = ma_col_cluster(d, c, &lo, &hi, &F, &B);
    cnt_off[(size_t)c] = Q;
    if (size >= 2) {
      out.members.at((size_t)F) = (int32_t)size;
      if (B >= 0) out.members.at((size_t)B) = (int32_t)size;
      out.hist.at((size_t)ma_col_bin(v.revcom[F] != 0, size, MA_COL_CLUSTERS))++;
      if (ma_col_straddles(lo, hi)) Q += (v.col_off[F + 1] - v.col_off[F]) + (B >= 0 ? v.col_off[B + 1] - v.col_off[B] : 0);
    } else {
      F = B = -1;
    }
    rep_f[(size_t)c] = F;
    rep_b[(size_t)c] = B;
  }
  cnt_off[(size_t)C] = Q;
  std::vector<uint32_t> cnt((size_t)Q * MA_COL_CLASSES, 0);
  auto settle = [&](const MaColDecision& dec, int bin, int64_t at) {
    if (dec.what) out.seq.at((size_t)at) = dec.out;
    out.hist.at((size_t)(bin + MA_COL_COLUMNS)) += dec.voted;
    out.hist.at((size_t)(bin + MA_COL_SPLIT)) += dec.split;
    if (dec.what) out.hist.at((size_t)(bin + dec.what))++;
  };
  // count: a wavefront per chunk, its lanes hold the chunk's entries as voters
  for (int64_t g = 0; g < ma_col_chunks(M); g++) {
    const int64_t g0 = g * MA_COL_K;
    const int held = (int)(M - g0 < MA_COL_K ? M - g0 : MA_COL_K);
    std::vector<MaColVoter> q((size_t)held);
    std::vector<uint32_t> cl((size_t)held);
    for (int l = 0; l < held; l++) { q[(size_t)l] = ma_col_voter(v, d, g0 + l); cl[(size_t)l] = dd.cluster_of.at(dd.run_id.at((size_t)(g0 + l))); }
    for (int j = 0; j < held;) {
      const int64_t c = cl[(size_t)j];
      const int64_t lo = dd.run_first.at(dd.anchor.at((size_t)c)), hi = dd.run_first.at(dd.anchor.at((size_t)c + 1));
      const int jend = (int)((hi < g0 + held ? hi : g0 + held) - g0);
      if (jend <= j) { fprintf(stderr, "staged: entry %lld is not in its cluster\n", (long long)(g0 + j)); exit(2); }
      if (hi - lo >= 2) {
        const bool whole = !ma_col_straddles(lo, hi);
        const int bin = ma_col_bin(v.revcom[rep_f[(size_t)c]] != 0, hi - lo, 0);
        int64_t slot = whole ? 0 : cnt_off[(size_t)c];
        for (int half = 0; half < 2; half++) {
          const int32_t R = half ? rep_b[(size_t)c] : rep_f[(size_t)c];
          if (R < 0) continue;
          const int64_t sR = v.start[R], oR = v.col_off[R], ncol = v.col_off[R + 1] - oR;
          for (int64_t col = 0; col < ncol; col++) {
            uint32_t k5[MA_COL_CLASSES + 1] = {0, 0, 0, 0, 0, 0};
            for (int k = j; k < jend; k++) k5[ma_col_vote(v.seq, q[(size_t)k], sR + col)]++;
            if (whole) settle(ma_col_decide(k5[0], k5[1], k5[2], k5[3], k5[4], v.seq[oR + col], col == 0 || col == ncol - 1), bin, oR + col);
            else for (int k = 0; k < MA_COL_CLASSES; k++) cnt.at((size_t)((slot + col) * MA_COL_CLASSES + k)) += k5[k];
          }
          slot += ncol;
        }
      }
      j = jend;
    }
  }
  // decide
  for (int64_t s = 0; s < Q; s++) {
    int64_t lo = 0, hi = C;
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (cnt_off.at((size_t)mid) <= s) lo = mid; else hi = mid;
    }
    const int64_t c = lo;
    const int32_t F = rep_f.at((size_t)c), B = rep_b.at((size_t)c);
    if (F < 0) { fprintf(stderr, "staged: column %lld of the count array has no cluster\n", (long long)s); exit(2); }
    int64_t col = s - cnt_off[(size_t)c];
    const int64_t nF = v.col_off[F + 1] - v.col_off[F];
    int32_t R = F;
    if (col >= nF) { col -= nF; R = B; }
    if (R < 0) { fprintf(stderr, "staged: column %lld lies behind its cluster's records\n", (long long)s); exit(2); }
    const int64_t oR = v.col_off[R], ncol = v.col_off[R + 1] - oR;
    const uint32_t* w = &cnt.at((size_t)(s * MA_COL_CLASSES));
    const int64_t size = (int64_t)dd.run_first.at(dd.anchor.at((size_t)c + 1)) - (int64_t)dd.run_first.at(dd.anchor.at((size_t)c));
    settle(ma_col_decide(w[0], w[1], w[2], w[3], w[4], v.seq[oR + col], col == 0 || col == ncol - 1), ma_col_bin(v.revcom[F] != 0, size, 0), oR + col);
  }
  for (int b = 0; b < 2 * MA_COL_SIZE_BINS; b++) {
    const int64_t* row = &out.hist[(size_t)b * MA_COL_COUNTS];
    out.collapsed += row[MA_COL_CLUSTERS];
    out.changed += row[MA_COL_TO_BASE] + row[MA_COL_TO_GAP] + row[MA_COL_TO_N];
  }
  return out;
}

// ---- the serial walk ------------------------------------------------------------------------------------------------------------------
struct Mol { int rc; int64_t a, e; int32_t score; int64_t index, front, back; };

static Result serial(const Input& in, int32_t t) {
  const int64_t n = in.n;
  Result out;
  out.seq.assign(in.seq, 0, (size_t)in.col_off[(size_t)n]);
  out.members.assign((size_t)n, 0);
  out.hist.assign(2 * 6 * 6, 0);
  std::vector<Mol> mols;
  for (int64_t r = 0; r < n; r++) {
    const int64_t m = in.mate[(size_t)r];
    if (m == -2) continue;
    if (m < 0) { mols.push_back({in.rc[(size_t)r], in.start[(size_t)r], in.end[(size_t)r], in.score[(size_t)r], r, r, -1}); continue; }
    if (in.start[(size_t)r] > in.start[(size_t)m] || (in.start[(size_t)r] == in.start[(size_t)m] && r < m))
      mols.push_back({in.rc[(size_t)r], in.start[(size_t)r], (int64_t)in.end[(size_t)m] + in.L, in.score[(size_t)r], r < m ? r : m, r, m});
  }
  std::sort(mols.begin(), mols.end(), [](const Mol& x, const Mol& y) {
    if (x.rc != y.rc) return x.rc > y.rc;
    if (x.rc == 0) { if (x.a != y.a) return x.a < y.a; if (x.e != y.e) return x.e > y.e; }
    else { if (x.e != y.e) return x.e > y.e; if (x.a != y.a) return x.a < y.a; }
    if (x.score != y.score) return x.score > y.score;
    return x.index < y.index;
  });
  auto at = [&](int64_t r, int64_t p) -> int {                // the character of record r on reference column p, -1 for none
    if (r < 0 || p < in.start[(size_t)r] || p > in.end[(size_t)r]) return -1;
    return (unsigned char)in.seq[(size_t)(in.col_off[(size_t)r] + p - in.start[(size_t)r])];
  };
  auto close = [&](size_t from, size_t to) {
    const int64_t size = (int64_t)(to - from);
    if (size < 2) return;
    const Mol& rep = mols[from];
    const int sb = size <= 4 ? (int)size - 2 : size <= 8 ? 3 : size <= 16 ? 4 : 5;
    int64_t* row = &out.hist[(size_t)((rep.rc ? 6 : 0) + sb) * 6];
    row[0]++;
    out.collapsed++;
    for (int64_t R : {rep.front, rep.back}) {
      if (R < 0) continue;
      out.members[(size_t)R] = (int32_t)size;
      const int64_t ncol = (int64_t)in.end[(size_t)R] - in.start[(size_t)R] + 1;
      for (int64_t c = 0; c < ncol; c++) {
        const int64_t p = in.start[(size_t)R] + c;
        std::map<char, int64_t> votes;
        for (size_t i = from; i < to; i++) {
          if (!in.vote[(size_t)mols[i].front]) continue;
          int ch = at(mols[i].front, p);
          if (ch < 0) ch = at(mols[i].back, p);
          if (ch < 0) continue;
          const char u = (char)toupper(ch);
          if (!strchr("ACGT-", u) || (u == '-' && (c == 0 || c == ncol - 1))) continue;
          votes[u]++;
        }
        if (votes.empty()) continue;
        int64_t top = 0;
        for (const auto& e : votes) top = std::max(top, e.second);
        std::string ahead;
        for (const auto& e : votes) if (e.second == top) ahead += e.first;
        char& own = out.seq[(size_t)(in.col_off[(size_t)R] + c)];
        row[1]++;
        row[2] += votes.size() > 1;
        const char up = (char)toupper((unsigned char)own);
        if (ahead.size() == 1) {
          if (ahead[0] == up) continue;
          own = ahead[0];
          row[ahead[0] == '-' ? 4 : 3]++;
        } else {
          if (ahead.find(up) != std::string::npos || own == 'N') continue;
          own = 'N';
          row[5]++;
        }
        out.changed++;
      }
    }
  };
  size_t first = 0;
  int64_t ca = 0, ce = 0;
  for (size_t i = 0; i < mols.size(); i++) {
    const Mol& m = mols[i];
    if (i > 0 && m.rc == mols[first].rc && llabs(m.a - ca) <= t && llabs(m.e - ce) <= t) continue;
    close(first, i);
    first = i; ca = m.a; ce = m.e;
  }
  close(first, mols.size());
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "ma_collapse_driver <file>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  Input in;
  long long L = 0, n = 0;
  if (fscanf(f, "%lld %lld", &L, &n) != 2 || L < 1 || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
  in.L = (int32_t)L; in.n = n;
  in.start.resize((size_t)n); in.end.resize((size_t)n); in.score.resize((size_t)n); in.rc.resize((size_t)n); in.vote.resize((size_t)n); in.mate.resize((size_t)n);
  in.col_off.assign(1, 0);
  std::vector<char> word((size_t)L + 16);
  for (long long r = 0; r < n; r++) {
    long long s, e, rc, sc, m, vt;
    if (fscanf(f, "%lld %lld %lld %lld %lld %lld %s", &s, &e, &rc, &sc, &m, &vt, word.data()) != 7) { fprintf(stderr, "bad record %lld\n", r); return 2; }
    in.start[(size_t)r] = (int32_t)s; in.end[(size_t)r] = (int32_t)e; in.rc[(size_t)r] = rc ? 1 : 0; in.score[(size_t)r] = (int32_t)sc; in.mate[(size_t)r] = m;
    in.vote[(size_t)r] = vt ? 1 : 0;
    if ((long long)strlen(word.data()) != (e - s + 1 ? e - s + 1 : 1)) { fprintf(stderr, "record %lld: SEQ is not END - START + 1 long\n", r); return 2; }
    if (e - s + 1 > 0) in.seq.append(word.data(), (size_t)(e - s + 1));
    in.col_off.push_back((int64_t)in.seq.size());
  }
  fclose(f);
  const size_t T = in.seq.size();
  in.seq.resize((T + MA_REC_LANE - 1) / MA_REC_LANE * MA_REC_LANE, '\0');
  in.seq.shrink_to_fit();
  std::vector<int32_t> identity((size_t)n);
  for (long long r = 0; r < n; r++) identity[(size_t)r] = (int32_t)r;
  for (int32_t t : {0, 1, 2, 7}) {
    const Result a = staged(in, t, nullptr), b = serial(in, t), c = staged(in, t, &identity);
    if (!(a == b)) { fprintf(stderr, "tolerance %d: the staged form and the serial walk differ\n", t); return 1; }
    if (!(a == c)) { fprintf(stderr, "tolerance %d: rec_of = identity changes the result\n", t); return 1; }
    printf("%d %lld %lld\n", t, (long long)a.collapsed, (long long)a.changed);
    printf("%s\n", T ? a.seq.c_str() : ".");
    for (int64_t r = 0; r < in.n; r++) printf("%d ", a.members[(size_t)r]);
    printf("\n");
    for (int b2 = 0; b2 < MA_COL_HIST; b2++) printf("%lld ", (long long)a.hist[(size_t)b2]);
    printf("\n");
  }
  return 0;
}
