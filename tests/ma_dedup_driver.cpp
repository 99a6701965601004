// Host caller of the shared code of the duplicate filter (csrc/ma_dedup_body.h: what the kernels of mia_ma_dedup_kernels.h run per
// lane), in the kernels' own stages -- keys, an LSD radix sort over the bits L needs, runs, next, pointer doubling, the scan over the
// marks, histogram and scatter -- in arrays of exactly the device's sizes, so that AddressSanitizer sees every index.  Beside it a
// serial walk (std::sort with fs_comp's order, then set_uniq_in_fsdb's loop) that shares only the input.  For every tolerance in
// 0, 1, 2, 7, 100 the two must agree; the staged form's results are printed for the test to compare with its own restatement.
//
//   ma_dedup_driver <file>          file: "L n", then n lines "start end rc score mate"
//   ma_dedup_driver <file> time     the serial walk alone, five times at tolerance 0: the median in milliseconds
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_dedup_body.h"

using namespace mia;

struct Input {
  int32_t L = 0;
  int64_t n = 0;
  std::vector<int32_t> start, end, score;
  std::vector<uint8_t> rc;
  std::vector<int64_t> mate;
};

struct Result {
  std::vector<uint8_t> keep;
  std::vector<int64_t> rep, hist;
  int64_t molecules = 0, clusters = 0, orphans = 0;
  bool operator==(const Result& o) const {
    return keep == o.keep && rep == o.rep && hist == o.hist && molecules == o.molecules && clusters == o.clusters && orphans == o.orphans;
  }
};

static Result staged(const Input& in, int32_t t) {
  const int64_t n = in.n;
  const int32_t L = in.L;
  const int W = ma_dedup_width(L);
  Result out;
  out.keep.assign((size_t)n, 0); out.rep.assign((size_t)n, -1); out.hist.assign(MA_DEDUP_HIST, 0);
  // keys
  std::vector<uint64_t> key[2] = {std::vector<uint64_t>((size_t)n), std::vector<uint64_t>((size_t)n)};
  std::vector<uint32_t> val[2] = {std::vector<uint32_t>((size_t)n), std::vector<uint32_t>((size_t)n)};
  int64_t M = 0;
  for (int64_t r = 0; r < n; r++) {
    key[0][(size_t)r] = ma_dedup_record_key(L, W, in.start.data(), in.end.data(), in.rc.data(), in.mate.data(), r);
    val[0][(size_t)r] = (uint32_t)r;
    if (in.mate[(size_t)r] == MA_DEDUP_ORPHAN) { out.keep[(size_t)r] = 1; out.rep[(size_t)r] = r; out.orphans++; }
    else if (key[0][(size_t)r] != MA_DEDUP_NO_KEY) M++;
  }
  out.molecules = M;
  // sort
  int cur = 0;
  for (int p = 0; p < ma_dedup_passes(L); p++, cur ^= 1) {
    std::vector<int64_t> count(257, 0);
    for (int64_t i = 0; i < n; i++) count[(size_t)((key[cur][(size_t)i] >> (8 * p)) & 255) + 1]++;
    for (int d = 0; d < 256; d++) count[(size_t)d + 1] += count[(size_t)d];
    for (int64_t i = 0; i < n; i++) {
      const int64_t at = count[(size_t)((key[cur][(size_t)i] >> (8 * p)) & 255)]++;
      key[cur ^ 1].at((size_t)at) = key[cur][(size_t)i];
      val[cur ^ 1].at((size_t)at) = val[cur][(size_t)i];
    }
  }
  const std::vector<uint64_t>& sk = key[cur];
  const std::vector<uint32_t>& sm = val[cur];
  for (int64_t i = 0; i < n; i++) if ((i < M) != (sk[(size_t)i] != MA_DEDUP_NO_KEY)) { fprintf(stderr, "staged: the molecules are not in front\n"); exit(2); }
  if (M == 0) return out;
  // runs
  std::vector<uint32_t> run_id((size_t)M), run_first;
  std::vector<uint64_t> run_key, best;
  for (int64_t i = 0; i < M; i++) {
    if (i == 0 || sk[(size_t)i - 1] != sk[(size_t)i]) { run_first.push_back((uint32_t)i); run_key.push_back(sk[(size_t)i]); best.push_back(0); }
    run_id[(size_t)i] = (uint32_t)(run_key.size() - 1);
    const int64_t f = sm[(size_t)i];
    const uint64_t v = ma_dedup_pack(in.score[(size_t)f], ma_dedup_index(in.mate.data(), f));
    if (v > best.back()) best.back() = v;
  }
  const int64_t R = (int64_t)run_key.size();
  run_first.push_back((uint32_t)M);
  // next, doubling
  std::vector<uint32_t> jump[2] = {std::vector<uint32_t>((size_t)R + 1), std::vector<uint32_t>((size_t)R + 1)}, mark((size_t)R, 0);
  for (int64_t k = 0; k < R; k++) jump[0][(size_t)k] = (uint32_t)ma_dedup_next(run_key.data(), R, k, W, t);
  jump[0][(size_t)R] = (uint32_t)R;
  mark[0] = 1;
  int jc = 0;
  for (int round = 0; round < ma_dedup_rounds(R); round++, jc ^= 1)
    for (int64_t k = R; k >= 0; k--) {                       // (any order: high to low sees no mark of its own round, the device may)
      const uint32_t j = jump[jc].at((size_t)k);
      if (k < R && (int64_t)j < R && mark[(size_t)k]) mark.at(j) = 1;
      jump[jc ^ 1][(size_t)k] = jump[jc].at(j);
    }
  // clusters
  std::vector<uint32_t> cluster_of((size_t)R), anchor;
  for (int64_t k = 0; k < R; k++) {
    if (mark[(size_t)k]) anchor.push_back((uint32_t)k);
    cluster_of[(size_t)k] = (uint32_t)(anchor.size() - 1);
  }
  const int64_t C = (int64_t)anchor.size();
  anchor.push_back((uint32_t)R);
  out.clusters = C;
  for (int64_t c = 0; c < C; c++) {
    const int64_t size = (int64_t)run_first.at(anchor[(size_t)c + 1]) - (int64_t)run_first.at(anchor[(size_t)c]);
    out.hist.at((size_t)ma_dedup_size_bin(ma_dedup_key_forward(run_key.at(anchor[(size_t)c]), W), size))++;
  }
  for (int64_t i = 0; i < M; i++) {
    const int64_t f = sm[(size_t)i];
    const int64_t r = ma_dedup_packed_index(best.at(anchor.at(cluster_of.at(run_id[(size_t)i]))));
    const uint8_t kp = ma_dedup_index(in.mate.data(), f) == r ? 1 : 0;
    out.keep.at((size_t)f) = kp; out.rep.at((size_t)f) = r;
    const int64_t m = in.mate[(size_t)f];
    if (m >= 0) { out.keep.at((size_t)m) = kp; out.rep.at((size_t)m) = r; }
  }
  return out;
}

struct Mol { int rc; int64_t a, e; int32_t score; int64_t index, front, back; };

static Result serial(const Input& in, int32_t t) {
  const int64_t n = in.n;
  Result out;
  out.keep.assign((size_t)n, 0); out.rep.assign((size_t)n, -1); out.hist.assign(MA_DEDUP_HIST, 0);
  std::vector<Mol> mols;
  for (int64_t r = 0; r < n; r++) {
    const int64_t m = in.mate[(size_t)r];
    if (m == MA_DEDUP_ORPHAN) { out.keep[(size_t)r] = 1; out.rep[(size_t)r] = r; out.orphans++; continue; }
    if (m < 0) { mols.push_back({in.rc[(size_t)r], in.start[(size_t)r], in.end[(size_t)r], in.score[(size_t)r], r, r, -1}); continue; }
    if (in.start[(size_t)r] > in.start[(size_t)m] || (in.start[(size_t)r] == in.start[(size_t)m] && r < m))
      mols.push_back({in.rc[(size_t)r], in.start[(size_t)r], (int64_t)in.end[(size_t)m] + in.L, in.score[(size_t)r], r < m ? r : m, r, m});
  }
  out.molecules = (int64_t)mols.size();
  std::sort(mols.begin(), mols.end(), [](const Mol& x, const Mol& y) {
    if (x.rc != y.rc) return x.rc > y.rc;
    if (x.rc == 0) { if (x.a != y.a) return x.a < y.a; if (x.e != y.e) return x.e > y.e; }
    else { if (x.e != y.e) return x.e > y.e; if (x.a != y.a) return x.a < y.a; }
    if (x.score != y.score) return x.score > y.score;
    return x.index < y.index;
  });
  size_t first = 0;                                          // the cluster's first molecule in the sort: its representative
  int64_t ca = 0, ce = 0;
  auto close = [&](size_t from, size_t to) {
    if (to == from) return;
    out.clusters++;
    out.hist[(size_t)ma_dedup_size_bin(mols[from].rc == 0, (int64_t)(to - from))]++;
    for (size_t i = from; i < to; i++)
      for (int64_t r : {mols[i].front, mols[i].back})
        if (r >= 0) { out.keep[(size_t)r] = i == from ? 1 : 0; out.rep[(size_t)r] = mols[from].index; }
  };
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
  if (argc < 2) { fprintf(stderr, "ma_dedup_driver <file> [time]\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  Input in;
  long long L = 0, n = 0;
  if (fscanf(f, "%lld %lld", &L, &n) != 2 || L < 1 || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
  in.L = (int32_t)L; in.n = n;
  in.start.resize((size_t)n); in.end.resize((size_t)n); in.score.resize((size_t)n); in.rc.resize((size_t)n); in.mate.resize((size_t)n);
  for (long long r = 0; r < n; r++) {
    long long s, e, rc, sc, m;
    if (fscanf(f, "%lld %lld %lld %lld %lld", &s, &e, &rc, &sc, &m) != 5) { fprintf(stderr, "bad record %lld\n", r); return 2; }
    in.start[(size_t)r] = (int32_t)s; in.end[(size_t)r] = (int32_t)e; in.rc[(size_t)r] = rc ? 1 : 0; in.score[(size_t)r] = (int32_t)sc; in.mate[(size_t)r] = m;
  }
  fclose(f);
  if (argc > 2 && !strcmp(argv[2], "time")) {
    std::vector<double> ms;
    for (int k = 0; k < 5; k++) {
      const auto t0 = std::chrono::steady_clock::now();
      const Result r = serial(in, 0);
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() + (r.clusters < 0 ? 1 : 0));
    }
    std::sort(ms.begin(), ms.end());
    printf("%.3f\n", ms[2]);
    return 0;
  }
  for (int32_t t : {0, 1, 2, 7, 100}) {
    const Result a = staged(in, t), b = serial(in, t);
    if (!(a == b)) { fprintf(stderr, "tolerance %d: the staged form and the serial walk differ\n", t); return 1; }
    printf("%d %lld %lld %lld\n", t, (long long)a.molecules, (long long)a.clusters, (long long)a.orphans);
    for (int64_t r = 0; r < in.n; r++) printf("%d ", a.keep[(size_t)r]);
    printf("\n");
    for (int64_t r = 0; r < in.n; r++) printf("%lld ", (long long)a.rep[(size_t)r]);
    printf("\n");
    for (int b2 = 0; b2 < MA_DEDUP_HIST; b2++) if (a.hist[(size_t)b2]) printf("%d %lld ", b2, (long long)a.hist[(size_t)b2]);
    printf("\n");
  }
  return 0;
}
