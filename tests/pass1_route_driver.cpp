// Driver of tests/test_pass1_route_cpu.py over csrc/pass1_route.h (plain C++17, no HIP).
//   pass1_route_driver route     stdin: records of N_IN int64 (IN_FIELDS below, in that order; has_cpl / has_plain say whether the alt
//                                switch is set); stdout: for each, N_OUT int64: OUT_FIELDS of the route, the refusal's ABI code and what
//                                pass1_wants_wild() answered
//   pass1_route_driver messages  the three refusals' messages, one per line
//   pass1_route_driver revcom    revcom_char_host of the byte values 0 .. 255, 256 bytes
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/pass1_route.h"

using namespace mia;

#define IN_FIELDS(X) X(n) X(max_len) X(L) X(circular) X(kmer_len) X(max_pos) X(flat) X(bx_ok) X(use_bx) X(use_filter) X(p1_other) X(wild_entries) \
  X(waves_cu) X(cus)
#define OUT_FIELDS(X) X(wl) X(wrap) X(len1) X(cpl) X(plain) X(ch) X(nch) X(mask_words) X(lds) X(rows_p) X(trace_bytes) X(ckpt_words) X(waves_cu) X(grid) \
  X(fast_ok) X(gen_ok) X(filtered) X(want_wild) X(anchored_ok) X(need_todo) X(need_ktab) X(rebuild_ktab_for_anchors) X(ref_mostly_bases) X(wild) \
  X(wild_entries) X(refusal)

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "messages")) {
    for (Pass1Refusal r : {P1_REFUSE_HORIZON, P1_REFUSE_KMER_TABLE, P1_REFUSE_LDS}) printf("%s\n", pass1_refusal_message(r));
    return pass1_refusal_message(P1_REFUSE_NONE)[0] ? 1 : 0;
  }
  if (!strcmp(mode, "revcom")) {
    for (int c = 0; c < 256; c++) putchar((unsigned char)revcom_char_host((char)c));
    return 0;
  }
  if (strcmp(mode, "route")) { fprintf(stderr, "usage: pass1_route_driver route|messages|revcom\n"); return 2; }
  std::vector<long long> rec, out;
  long long v[64];
#define X(f) +1
  const size_t n_in = 0 IN_FIELDS(X) + 4;
#undef X
  while (fread(v, 8, n_in, stdin) == n_in) {
    Pass1RouteIn in;
    size_t k = 0;
#define X(f) in.f = (decltype(in.f))v[k++];
    IN_FIELDS(X)
#undef X
    if (v[k]) in.alt_cpl = (int)v[k + 1];
    if (v[k + 2]) in.alt_plain = (int)v[k + 3];
    const Pass1Route r = pass1_route(in);
#define X(f) out.push_back((long long)r.f);
    OUT_FIELDS(X)
#undef X
    out.push_back(pass1_refusal_code(r.refusal));
    out.push_back(pass1_wants_wild(in));
  }
  fwrite(out.data(), 8, out.size(), stdout);
  return 0;
}
