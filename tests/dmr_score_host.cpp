// The host half of dmr pair (modkit_amd/csrc/mkp_dmr.hpp) alone, as a program: compiled with g++ (no HIP header, no device; with
// -fsanitize=address,undefined where the runtime is installed) and run by tests/test_dmr_pair_host.py on counts it writes into a file.
// in:  n_regions n_codes, the codes; per region: start end rule named a_total b_total a_bad b_bad a_contig b_contig has_ref, then per code
//      a_has a_mod b_has b_mod
// out: per region `S state score(%.17g) score(text)`, then `TABLE` and the table with its header; `F text` for every `f value` line that
//      follows the regions (f64 text of a hex-float value)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "mkp_dmr.hpp"

struct Set { std::vector<mkp_region> regions; std::vector<std::string> chrom, name; };

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  uint32_t n = 0, nc = 0;
  in >> n >> nc;
  std::vector<uint32_t> codes(nc);
  for (auto& c : codes) in >> c;
  Set set;
  std::vector<uint64_t> mod[2], total[2], rows[2]; std::vector<uint8_t> has[2], bad[2], contig[2], ref(n);
  for (int s = 0; s < 2; s++) { mod[s].resize((size_t)n * nc); has[s].resize((size_t)n * nc); total[s].resize(n); rows[s].assign(n, 0); bad[s].resize(n);
    contig[s].resize(n); }
  for (uint32_t r = 0; r < n; r++) {
    mkp_region g{}; unsigned rule = 3, named = 0, v[5];
    in >> g.start >> g.end >> rule >> named >> total[0][r] >> total[1][r];
    for (auto& x : v) in >> x;
    g.strand_rule = (uint8_t)rule; g.tid = 0;
    bad[0][r] = (uint8_t)v[0]; bad[1][r] = (uint8_t)v[1]; contig[0][r] = (uint8_t)v[2]; contig[1][r] = (uint8_t)v[3]; ref[r] = (uint8_t)v[4];
    set.regions.push_back(g); set.chrom.push_back("c0"); set.name.push_back(named ? "r" + std::to_string(r) + " x" : ".");
    for (uint32_t k = 0; k < nc; k++) { unsigned ah, bh; in >> ah >> mod[0][(size_t)r * nc + k] >> bh >> mod[1][(size_t)r * nc + k];
      has[0][(size_t)r * nc + k] = (uint8_t)ah; has[1][(size_t)r * nc + k] = (uint8_t)bh; }
  }
  if (!in) { fprintf(stderr, "short input\n"); return 2; }
  mkp_dmr_out t{};
  t.n_regions = n; t.n_codes = nc; t.code_repr = codes.data();
  for (int s = 0; s < 2; s++) { t.n_mod[s] = mod[s].data(); t.has_code[s] = has[s].data(); t.total[s] = total[s].data(); t.n_rows[s] = rows[s].data();
    t.bad[s] = bad[s].data(); t.contig_has_rows[s] = contig[s].data(); }
  t.has_reference = ref.data();
  std::vector<double> score(n); std::vector<uint8_t> state(n);
  mkp::dmr_judge(t, score.data(), state.data());
  t.score = score.data(); t.state = state.data();
  for (uint32_t r = 0; r < n; r++) printf("S %u %.17g %s\n", (unsigned)state[r], score[r], mkp::f64_display(score[r]).c_str());
  auto f32_text = [](float v) { char buf[128]; auto res = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed); return std::string(buf, res.ptr); };
  printf("TABLE\n%s", mkp::dmr_table_text(set, t, true, f32_text).c_str());
  std::string word, value;
  while (in >> word >> value) if (word == "f") printf("F %s\n", mkp::f64_display(strtod(value.c_str(), nullptr)).c_str());
  return 0;
}
