// The grammar of one bedMethyl line (modkit_amd/csrc/mkp_bedmethyl_line.hpp) on the host: the header the device reader's parse kernel and
// the host reader share, compiled by g++ alone (no HIP header, no device).  tests/test_bedmethyl_line_host.py writes a file of lines,
// this program runs mkp_bedmethyl_parse_line over each — on a heap copy of exactly the line's bytes, so that a read beyond them is
// the sanitizer's — and prints one answer per line:
//   ok <chrom> <pos> <code_repr> <strand> <n_valid> <n_mod> <n_canonical> <n_other> <n_delete> <n_fail> <n_diff> <n_nocall>
//   err <status class> <field>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mkp_bedmethyl_line.hpp"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: bedmethyl_line_host <lines file>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<unsigned char> text; unsigned char buf[65536]; size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.insert(text.end(), buf, buf + got);
  fclose(f);
  for (size_t p = 0; p < text.size();) {
    const void* nl = memchr(text.data() + p, '\n', text.size() - p);
    const size_t e = nl ? (size_t)((const unsigned char*)nl - text.data()) : text.size();
    const uint32_t len = (uint32_t)(e - p);
    uint8_t* line = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(line, text.data() + p, len);
    MkpBedLine L; memset(&L, 0, sizeof(L));
    const uint32_t code = mkp_bedmethyl_parse_line(line, len, &L);
    if (code) printf("err %u %u\n", MKP_BML_CLASS(code), MKP_BML_FIELD(code));
    else printf("ok %s %u %u %c %u %u %u %u %u %u %u %u\n", std::string((const char*)line + L.chrom_off, L.chrom_len).c_str(), L.pos, L.code,
        "+-."[L.strand], L.n_valid, L.n_mod, L.n_canonical, L.n_other, L.n_delete, L.n_fail, L.n_diff, L.n_nocall);
    free(line);
    p = e + 1;
  }
  return 0;
}
