// The single-site arithmetic (mkp_dmr_site_math.hpp) and the batch planner (mkp_dmr_sites.hpp) alone, for a build under the address and
// undefined-behaviour sanitizers (tests/test_dmr_sites_host.py): reads cases from a file, prints what the Python test compares.
//   s <n_codes> <alpha> <beta> <delta> <max a> <max b> <a_has> <a_total> <b_has> <b_total> then n_codes times <a_mod> <b_mod>
//       -> "s <failed> <score> <ln_effect> <ln_null> <p> <effect>" (%a: exact)
//   p <interval> <n_contigs> then per contig <len> and its windows' counts -> "p <n_batches> <n_entries>" and "e <contig> <start> <batch>" lines
//   g -> "g" and the 16 nodes, then the 16 weights
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "mkp_dmr_sites.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 's') {
      uint32_t n = 0, mc[2], a_has, b_has; double alpha, beta, delta; uint64_t a_total, b_total, a_mod[16] = {0}, b_mod[16] = {0};
      if (fscanf(f, "%u %lf %lf %lf %u %u %u %" SCNu64 " %u %" SCNu64, &n, &alpha, &beta, &delta, &mc[0], &mc[1], &a_has, &a_total, &b_has, &b_total) != 10
          || n > 16) return 3;
      for (uint32_t k = 0; k < n; k++) if (fscanf(f, "%" SCNu64 " %" SCNu64, &a_mod[k], &b_mod[k]) != 2) return 3;
      const MkpDmrSiteMath M = mkp::dmr_site_math(alpha, beta, delta, mc);
      double v[5];
      const bool ok = mkp::dmr_site_score(a_mod, a_has, a_total, b_mod, b_has, b_total, n, M, v);
      printf("s %d %a %a %a %a %a\n", ok ? 0 : 1, v[0], v[1], v[2], v[3], v[4]);
    } else if (kind == 'p') {
      uint64_t interval = 0; uint32_t nc = 0;
      if (fscanf(f, "%" SCNu64 " %u", &interval, &nc) != 2 || !interval) return 3;
      std::vector<uint64_t> lens(nc); std::vector<uint32_t> counts;
      for (uint32_t c = 0; c < nc; c++) {
        if (fscanf(f, "%" SCNu64, &lens[c]) != 1) return 3;
        for (uint64_t w = 0; w < mkp::dmr_sites_windows(lens[c], interval); w++) { uint32_t x; if (fscanf(f, "%u", &x) != 1) return 3; counts.push_back(x); }
      }
      std::vector<mkp_dmr_sites_batch> plan;
      const uint64_t nb = mkp::dmr_sites_plan(lens.data(), counts.data(), nc, interval, &plan);
      printf("p %" PRIu64 " %zu\n", nb, plan.size());
      for (const mkp_dmr_sites_batch& e : plan) printf("e %u %" PRIu64 " %" PRIu64 "\n", e.contig, e.start, e.batch);
    } else if (kind == 'g') {
      double x[16], w[16];
      mkp::dmr_gauss_legendre(x, w);
      printf("g");
      for (double v : x) printf(" %a", v);
      for (double v : w) printf(" %a", v);
      printf("\n");
    } else return 3;
  }
  fclose(f);
  return 0;
}
