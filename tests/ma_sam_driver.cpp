// Host caller of the SAM export's shared code (csrc/ma_sam_body.h: what k_ma_sam_layout and k_ma_sam_render run on the device):
// reads a .maln as ma_hip does and prints, per record in sorted order, "<NM>\t<body>\n" -- the body being fields 6-10 of its line.
//   ma_sam_driver <file.maln>
// Every body is made twice -- by one caller that takes the walk position by position, and by 64 "lanes" that take it in
// stretches of 64 through the mask functions, as a wavefront does (a first pass for the sizes, a second one that writes at them)
// -- and both must agree.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_sam_body.h"
#include "../mapping-iterative-assembler_amd/host/maln_text.h"

namespace {

using namespace mia;

// position by position
void plain(const MaSamView& v, int64_t r, int64_t walk, std::string* cigar, std::string* seq, int64_t* nm) {
  MaSamRun run{MA_SAM_NONE, 0};
  auto close = [&]() {
    if (run.op == MA_SAM_NONE) return;
    char text[32];
    ma_sam_run_text(run, text);
    cigar->append(text, (size_t)ma_sam_run_bytes(run.len));
  };
  *nm = 0;
  for (int64_t w = 0; w < walk; w++) {
    const MaSamElem e = ma_sam_elem(v, r, w);
    *nm += e.nm ? 1 : 0;
    if (e.op == MA_SAM_NONE) continue;
    if (e.op != MA_SAM_D) *seq += e.ch;
    if (e.op == run.op) run.len++;
    else { close(); run = MaSamRun{e.op, 1}; }
  }
  close();
}

// in stretches of 64, lane by lane; cigar / seq may be null (sizes only)
void lanes(const MaSamView& v, int64_t r, int64_t walk, char* cigar, char* seq, int64_t* cigar_bytes, int64_t* seq_len, int64_t* nm) {
  MaSamRun open{MA_SAM_NONE, 0};
  int64_t c_at = 0, s_at = 0;
  *nm = 0;
  for (int64_t w0 = 0; w0 < walk; w0 += 64) {
    MaSamElem e[64];
    MaSamStretch s{};
    uint64_t heads = 0, counted = 0;
    for (int lane = 0; lane < 64; lane++) {
      e[lane] = w0 + lane < walk ? ma_sam_elem(v, r, w0 + lane) : MaSamElem{MA_SAM_NONE, 0, false};
      if (e[lane].op != MA_SAM_NONE) s.m[e[lane].op] |= 1ull << lane;
      if (e[lane].nm) counted |= 1ull << lane;
    }
    s.act = s.m[MA_SAM_M] | s.m[MA_SAM_I] | s.m[MA_SAM_D] | s.m[MA_SAM_S];
    *nm += ma_sam_count(counted);
    for (int lane = 0; lane < 64; lane++) if (ma_sam_head(s, lane, e[lane].op, open.op)) heads |= 1ull << lane;
    const uint64_t chars = s.m[MA_SAM_M] | s.m[MA_SAM_I] | s.m[MA_SAM_S];
    for (int lane = 0; lane < 64; lane++) {
      if ((heads >> lane) & 1ull) {
        const MaSamRun closed = ma_sam_closed(s, heads, lane, open);
        if (closed.op != MA_SAM_NONE) {
          if (cigar) ma_sam_run_text(closed, cigar + c_at);
          c_at += ma_sam_run_bytes(closed.len);
        }
      }
      if (seq && ((chars >> lane) & 1ull)) seq[s_at + ma_sam_count(chars & ma_sam_below(lane))] = e[lane].ch;
    }
    s_at += ma_sam_count(chars);
    open = ma_sam_carry(s, heads, open);
  }
  if (open.op != MA_SAM_NONE) {
    if (cigar) ma_sam_run_text(open, cigar + c_at);
    c_at += ma_sam_run_bytes(open.len);
  }
  *cigar_bytes = c_at;
  *seq_len = s_at;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: ma_sam_driver <file.maln>\n"); return 2; }
  maln_text::MalnFile m;
  maln_text::read_maln_file(argv[1], &m);
  if (!ma_sam_gaps_ok(m.gaps.data(), m.L)) { fprintf(stderr, "no SAM export\n"); return 1; }
  const int64_t n = (int64_t)m.start.size(), n_ins = (int64_t)m.ins_record.size();
  std::vector<int32_t> rec_ins, ins_list;
  ma_list_pairs(n, n_ins, m.ins_record.data(), m.ins_pos.data(), &rec_ins, &ins_list);
  std::vector<int64_t> cum((size_t)(n_ins + n + 1), -1);
  const MaSamView v{n, m.L, m.start.data(), m.col_off.data(), m.seq.data(), rec_ins.data(), ins_list.data(), m.ins_pos.data(), m.ins_off.data(),
                    m.ins_bases.data(), m.ref_seq.data(), cum.data()};
  // first pass: the index, the sizes and the offsets, as the layout does
  std::vector<int64_t> off((size_t)n + 1, 0), cig((size_t)n + 1, 0), nms((size_t)n + 1, 0);
  for (int64_t r = 0; r < n; r++) {
    const int64_t walk = ma_sam_index(v, r);
    if (walk != ma_sam_walk_len(v, r)) { fprintf(stderr, "record %lld: the index and the walk length disagree\n", (long long)r); return 3; }
    int64_t cb = 0, sl = 0;
    lanes(v, r, walk, nullptr, nullptr, &cb, &sl, &nms[(size_t)r]);
    cig[(size_t)r] = sl > 0 ? cb : 0;
    off[(size_t)r + 1] = off[(size_t)r] + ma_sam_body_bytes(cb, sl);
  }
  // second pass: the bodies at those offsets, as the render does
  std::vector<char> body((size_t)off[(size_t)n] + 1, '?');
  for (int64_t r = 0; r < n; r++) {
    char* out = body.data() + off[(size_t)r];
    const int64_t cb = cig[(size_t)r];
    if (cb == 0) { for (int k = 0; k < MA_SAM_EMPTY_BYTES; k++) out[k] = MA_SAM_EMPTY[k]; continue; }
    for (int k = 0; k < MA_SAM_MID_BYTES; k++) out[cb + k] = MA_SAM_MID[k];
    int64_t got_cb = 0, sl = 0, nm = 0;
    lanes(v, r, ma_sam_walk_len(v, r), out, out + cb + MA_SAM_MID_BYTES, &got_cb, &sl, &nm);
    if (got_cb != cb || out + cb + MA_SAM_MID_BYTES + sl != body.data() + off[(size_t)r + 1] || nm != nms[(size_t)r]) {
      fprintf(stderr, "record %lld: the second pass found other sizes than the first\n", (long long)r);
      return 3;
    }
  }
  if (body[(size_t)off[(size_t)n]] != '?') { fprintf(stderr, "a body was written past its end\n"); return 3; }
  for (int64_t r = 0; r < n; r++) {
    std::string cigar, seq;
    int64_t nm = 0;
    plain(v, r, ma_sam_walk_len(v, r), &cigar, &seq, &nm);
    const std::string want = seq.empty() ? std::string(MA_SAM_EMPTY) : cigar + MA_SAM_MID + seq;
    const std::string got(body.data() + off[(size_t)r], (size_t)(off[(size_t)r + 1] - off[(size_t)r]));
    if (got != want || nm != nms[(size_t)r]) {
      fprintf(stderr, "record %lld: 64 lanes made NM %lld and %s, one caller NM %lld and %s\n", (long long)r, (long long)nms[(size_t)r], got.c_str(), (long long)nm, want.c_str());
      return 3;
    }
    printf("%lld\t", (long long)nm);
    fwrite(got.data(), 1, got.size(), stdout);
    fputc('\n', stdout);
  }
  return 0;
}
