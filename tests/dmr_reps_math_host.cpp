// The f32 arithmetic of replicates (mkp_dmr_reps_math.hpp) alone, for a build under the address and undefined-behaviour sanitizers
// (tests/test_dmr_reps_host.py): reads cases from a file, prints what the Python test compares.
//   b <n_samples> <n_codes> then per sample <has> <total> and n_codes times <n_mod>
//       -> "b <failed> <has> <total>" and the n_codes balanced counts
//   c <n_present> <n> -> "c <pct>"
//   f <hex f32> -> "f <count>": the saturating cast (NaN, infinities and negative values included)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mkp_dmr_reps_math.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'b') {
      uint32_t n = 0, nc = 0;
      if (fscanf(f, "%u %u", &n, &nc) != 2 || !n || n > 64 || nc > MKP_DMR_SITE_MAX_CODES) return 3;
      std::vector<uint64_t> mod((size_t)n * nc), total(n); std::vector<uint32_t> has(n);
      for (uint32_t s = 0; s < n; s++) {
        if (fscanf(f, "%u %" SCNu64, &has[s], &total[s]) != 2) return 3;
        for (uint32_t k = 0; k < nc; k++) if (fscanf(f, "%" SCNu64, &mod[(size_t)s * nc + k]) != 1) return 3;
      }
      uint64_t out_mod[MKP_DMR_SITE_MAX_CODES], out_total = 0; uint32_t out_has = 0;
      const bool ok = mkp::dmr_reps_balance<uint64_t>(mod.data(), has.data(), total.data(), n, nc, out_mod, &out_has, &out_total);
      printf("b %d %u %" PRIu64, ok ? 0 : 1, out_has, out_total);
      for (uint32_t k = 0; k < nc; k++) printf(" %" PRIu64, out_mod[k]);
      printf("\n");
    } else if (kind == 'c') {
      uint32_t p = 0, n = 0;
      if (fscanf(f, "%u %u", &p, &n) != 2) return 3;
      printf("c %u\n", mkp::dmr_reps_pct_samples(p, n));
    } else if (kind == 'f') {
      uint32_t bits = 0; float x;
      if (fscanf(f, "%x", &bits) != 1) return 3;
      memcpy(&x, &bits, 4);
      printf("f %" PRIu64 "\n", mkp::dmr_reps_f32_to_count(x));
    } else return 3;
  }
  fclose(f);
  return 0;
}
