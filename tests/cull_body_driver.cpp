// Host driver of csrc/cull_body.h for tests/test_cull_body_cpu.py.
// stdin:  L n, then n lines "sk as ae back_slot front_slot0"
// stdout: n lines "records links" (cull_records, cull_links), then one line per block of 256 reads
//         "first total links": the sums of cull_share over the 256 threads of k_cull_records, taken from a partial[] filled
//         the way k_slot_count fills it (blocks, then groups of sixteen, then the groups' links) in cull_partial_words(n) words.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/cull_body.h"

int main() {
  long long L, n;
  if (scanf("%lld %lld", &L, &n) != 2 || n < 1) return 2;
  std::vector<int> rec((size_t)n), lnk((size_t)n);
  for (long long i = 0; i < n; i++) {
    long long sk, as, ae, back, front;
    if (scanf("%lld %lld %lld %lld %lld", &sk, &as, &ae, &back, &front) != 5) return 2;
    rec[(size_t)i] = mia::cull_records(sk != 0, (int)as, (int)ae, (int)L);
    lnk[(size_t)i] = mia::cull_links(sk != 0, sk != 0 && mia::rec_geom((int)as, (int)ae, (int)L).split, back, front);
    printf("%d %d\n", rec[(size_t)i], lnk[(size_t)i]);
  }
  const int nb = (int)((n + 255) / 256), ng = mia::cull_groups(nb);
  const long long words = mia::cull_partial_words(n);
  if (nb + 2 * ng > words) { fprintf(stderr, "partial[] too short: %d + 2 * %d > %lld\n", nb, ng, words); return 3; }
  // exactly `words` entries on the heap: a sanitizer build sees any index past them
  std::vector<int64_t> partial((size_t)words, -1);
  for (int b = 0; b < nb; b++) partial[(size_t)b] = 0;
  for (int g = 0; g < ng; g++) { partial[(size_t)(nb + g)] = 0; partial[(size_t)(nb + ng + g)] = 0; }
  for (long long i = 0; i < n; i++) {
    partial[(size_t)(i / 256)] += rec[(size_t)i];
    partial[(size_t)(nb + i / 4096)] += rec[(size_t)i];
    partial[(size_t)(nb + ng + i / 4096)] += lnk[(size_t)i];
  }
  for (int b = 0; b < nb; b++) {
    mia::CullShare sum = {0, 0, 0};
    for (int t = 0; t < 256; t++) {
      const mia::CullShare s = mia::cull_share(partial.data(), nb, b, t, 256);
      sum.pre += s.pre; sum.tot += s.tot; sum.links += s.links;
    }
    printf("%lld %lld %lld\n", (long long)sum.pre, (long long)sum.tot, (long long)sum.links);
  }
  return 0;
}
