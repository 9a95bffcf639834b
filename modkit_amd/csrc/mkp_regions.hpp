// Host halves of `modkit stats` (EntryStats::run, src/stats/subcommand.rs:65-206): the regions BED and the table text; and of
// `modkit localize` (EntryLocalize, src/localise/subcommand.rs:104-305): its tolerant regions loader, the genome sizes and its table.
// No device here.
#pragma once
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mkp_pack.hpp"

struct mkp_genome_sizes { std::vector<std::string> name; std::vector<uint64_t> length; };
struct mkp_region_set {
  std::vector<mkp_region> regions;          // tid = index into the contig names given to the parser, -1 = not among them
  std::vector<std::string> chrom, name;     // name "." = the line has none
};

namespace mkp {

// One line through GenomeRegion::parse_bed_line (src/util.rs:864-878) and, for the stranded form, the score and strand that follow
// (880-909).  The reference's pieces (src/parsing_utils.rs): a string = one or more characters that are no blank, tab, CR or LF; a number =
// at least one of those four ("multispace") and then decimal digits that fit a u64; the name = any run of the four, then one or more
// characters that are no tab, CR or LF (so a name may hold blanks) — when that fails the line has no name and nothing is consumed.
struct BedLineParser {
  const std::string& l; size_t i = 0;
  explicit BedLineParser(const std::string& line) : l(line) {}
  static bool ms(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
  bool string(std::string* out) { const size_t s = i; while (i < l.size() && !ms(l[i])) i++; out->assign(l, s, i - s); return i > s; }
  bool multispace1() { const size_t s = i; while (i < l.size() && ms(l[i])) i++; return i > s; }
  bool digits(uint64_t* out) {
    if (!multispace1()) return false;
    const size_t s = i; uint64_t v = 0;
    while (i < l.size() && l[i] >= '0' && l[i] <= '9') { const uint64_t d = (uint64_t)(l[i] - '0');
      if (v > (0xffffffffffffffffull - d) / 10) return false;
      v = v * 10 + d; i++; }
    *out = v; return i > s;
  }
  bool name(std::string* out) {
    const size_t keep = i; while (i < l.size() && ms(l[i])) i++;
    const size_t s = i; while (i < l.size() && l[i] != '\t' && l[i] != '\r' && l[i] != '\n') i++;
    if (i == s) { i = keep; return false; }
    out->assign(l, s, i - s); return true;
  }
  // nom's `float` after multispace, or a lone '.': [+-] then digits [. digits] | . digits, an optional exponent; or inf / infinity / nan
  bool score() {
    const size_t keep = i;
    if (!multispace1()) return false;
    const size_t s0 = i; size_t j = i;
    if (j < l.size() && (l[j] == '+' || l[j] == '-')) j++;
    auto word = [&](const char* w) { size_t k = 0; while (w[k] && j + k < l.size() && (l[j + k] | 0x20) == w[k]) k++; return w[k] == 0 ? k : (size_t)0; };
    size_t w;
    if ((w = word("infinity")) || (w = word("inf")) || (w = word("nan"))) { i = j + w; return true; }
    auto dig = [&](size_t k) { return k < l.size() && l[k] >= '0' && l[k] <= '9'; };
    size_t e = j; while (dig(e)) e++;
    bool num = e > j;
    if (num) { if (e < l.size() && l[e] == '.') { e++; while (dig(e)) e++; } }
    else if (e < l.size() && l[e] == '.' && dig(e + 1)) { e++; while (dig(e)) e++; num = true; }
    if (num) {
      if (e < l.size() && (l[e] == 'e' || l[e] == 'E')) { size_t x = e + 1; if (x < l.size() && (l[x] == '+' || l[x] == '-')) x++;
        const size_t d = x; while (dig(x)) x++; if (x > d) e = x; }
      i = e; return true;
    }
    if (s0 < l.size() && l[s0] == '.') { i = s0 + 1; return true; }   // consume_dot
    i = keep; return false;
  }
  bool strand(uint8_t* rule) {
    if (!multispace1() || i >= l.size()) return false;
    const char c = l[i++]; *rule = c == '+' ? 1 : c == '-' ? 2 : c == '.' ? 3 : 0; return *rule != 0;
  }
};

// The regions BED as the reference's three loaders read it: the same line loop under three sets of rules.
//   stats (EntryStats::run): the parser is picked by the TAB-separated fields of the first line that does not start with '#'; a line that
//     fails is fatal; start <= end is checked, and a quote in a name is refused (the table writer does not quote).
//   localize (load_focus_regions up to its contig filters, src/localise/subcommand.rs:105-162): picked by the WHITESPACE-separated fields
//     (split_whitespace: runs of any blank count once, leading ones not at all); a line that fails is counted, not fatal; there is no
//     start <= end check, so start is held to 32 bits as well.
//   dmr (parse_roi_bed, src/dmr/util.rs:389-428): as stats, but the '#' lines in front of the first other line are skipped, not parsed,
//     and a quote in a name is written as it is (the table goes through format!, not the csv writer).
enum class BedRules { stats, localize, dmr };
template <class TidOf> mkp_region_set parse_bed_regions(const std::string& path, TidOf tid_of, BedRules rules, uint32_t* n_skipped) {
  const bool localize = rules == BedRules::localize;
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(MKP_E_IO, "failed to open regions BED " + path);
  std::vector<std::string> lines; std::string line;
  while (std::getline(f, line)) { if (!line.empty() && line.back() == '\r') line.pop_back(); lines.push_back(line); }   // BufRead::lines
  size_t first = 0; while (first < lines.size() && !lines[first].empty() && lines[first][0] == '#') first++;
  if (first >= lines.size()) throw Error(MKP_E_INVALID, "failed to inspect regions BED, no valid lines: " + path);
  size_t fields = 0;
  if (localize) {
    // char::is_whitespace on what a BED line can hold: blank, tab, LF, VT, FF, CR (and the Unicode blanks, which count as field text here)
    auto white = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    bool in = false; for (char c : lines[first]) { const bool wsp = white(c); if (!wsp && !in) fields++; in = !wsp; }
  } else { fields = 1; for (char c : lines[first]) if (c == '\t') fields++; }
  const bool stranded = fields > 4;
  mkp_region_set out; uint32_t skipped = 0;
  for (size_t k = rules == BedRules::dmr ? first : 0; k < lines.size(); k++) {
    BedLineParser p(lines[k]); std::string chrom, name; uint64_t s = 0, e = 0; uint8_t rule = 3;
    bool ok = p.string(&chrom) && p.digits(&s) && p.digits(&e);
    bool has_name = false;
    if (ok) { has_name = p.name(&name); if (stranded) ok = p.score() && p.strand(&rule); }
    auto where = [&]() { return "line " + std::to_string(k + 1) + " of " + path; };
    if (!ok) {
      if (localize) { skipped++; continue; }
      throw Error(MKP_E_INVALID, std::string("failed to parse ") + (stranded ? "stranded (bed4+)" : "un-stranded (bed3/4)") + " " + where() + ": "
          + lines[k]);
    }
    if (!localize && s > e) throw Error(MKP_E_INVALID, where() + ": start > end");
    if (e > 0xffffffffull || (localize && s > 0xffffffffull)) throw Error(MKP_E_UNSUPPORTED, where() + ": coordinate beyond 2^32 - 1");
    if (rules == BedRules::stats) for (const std::string* t : {&chrom, &name}) if (t->find('"') != std::string::npos) throw Error(MKP_E_UNSUPPORTED, where()
        + ": a quote in the contig or region name needs csv quoting, which is not written");
    mkp_region g; memset(&g, 0, sizeof(g)); g.tid = (int32_t)tid_of(chrom); g.start = (uint32_t)s; g.end = (uint32_t)e; g.strand_rule = rule;
    out.regions.push_back(g); out.chrom.push_back(chrom); out.name.push_back(has_name ? name : ".");
  }
  if (out.regions.empty()) throw Error(MKP_E_INVALID, "failed to load any regions from " + path
      + (localize ? ": " + std::to_string(skipped) + " lines failed to parse" : std::string()));
  if (n_skipped) *n_skipped = skipped;
  return out;
}
template <class TidOf> mkp_region_set parse_regions_bed(const std::string& path, TidOf tid_of) {
  return parse_bed_regions(path, tid_of, BedRules::stats, nullptr);
}
template <class TidOf> mkp_region_set parse_localize_regions_bed(const std::string& path, TidOf tid_of, uint32_t* n_skipped) {
  return parse_bed_regions(path, tid_of, BedRules::localize, n_skipped);
}
template <class TidOf> mkp_region_set parse_dmr_regions_bed(const std::string& path, TidOf tid_of) {
  return parse_bed_regions(path, tid_of, BedRules::dmr, nullptr);
}

inline std::string code_text(uint32_t code) { return (code & 0x80000000u) ? std::to_string(code & 0x7fffffffu) : std::string(1, (char)code); }

// MethylationStats::header / into_row (src/stats/mod.rs:24-51) through a tab-delimited csv writer; `f32_text` = f32 Display
template <class F32Text> std::string stats_table_text(const mkp_region_set& set, const mkp_stats_out& t, bool header, F32Text f32_text) {
  if (t.n_regions != set.regions.size()) throw Error(MKP_E_INVALID, "the counts are not those of this region set");
  std::string s;
  if (header) { s = "chrom\tstart\tend\tname\tstrand";
    for (uint32_t k = 0; k < t.n_codes; k++) { const std::string c = code_text(t.code_repr[k]);
      s += "\tcount_" + c + "\tcount_valid_" + c + "\tpercent_" + c; }
    s += '\n'; }
  // (tens of thousands of regions: the shortest-digits search of the f32 text is a microsecond a cell — pieces on the host pool, joined in order)
  const size_t n_pieces = t.n_regions >= 4096 ? 64 : 1;
  std::vector<std::string> piece(n_pieces);
  auto rows_of = [&](size_t pc) {
    std::string& o = piece[pc];
    for (uint32_t r = (uint32_t)((uint64_t)t.n_regions * pc / n_pieces), r1 = (uint32_t)((uint64_t)t.n_regions * (pc + 1) / n_pieces); r < r1; r++) {
      if (!t.contig_has_rows[r]) continue;
      const mkp_region& g = set.regions[r];
      o += set.chrom[r]; o += '\t'; o += std::to_string(g.start); o += '\t'; o += std::to_string(g.end); o += '\t'; o += set.name[r]; o += '\t';
      o += g.strand_rule == 1 ? '+' : g.strand_rule == 2 ? '-' : '.';
      for (uint32_t k = 0; k < t.n_codes; k++) {
        const uint64_t nm = t.n_mod[(size_t)r * t.n_codes + k], nv = t.n_valid[(size_t)r * t.n_codes + k];
        const float pct = nv == 0 ? 0.0f : ((float)nm / (float)nv) * 100.0f;   // ModPositionInfo::percent_modified (src/util.rs:920-936)
        o += '\t'; o += std::to_string(nm); o += '\t'; o += std::to_string(nv); o += '\t'; o += f32_text(pct);
      }
      o += '\n';
    }
  };
  if (n_pieces > 1) HostPool::get().parallel(n_pieces, rows_of); else rows_of(0);
  for (auto& o : piece) s += o;
  return s;
}

// ---- localize
// read_sequence_lengths_file (src/util.rs:969-990): a contig name, blanks, a length; what follows is not looked at; any other line fails;
// collected into an IndexMap: a later line for the same contig replaces the length and keeps the place
inline mkp_genome_sizes parse_genome_sizes(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(MKP_E_IO, "failed to open genome sizes " + path);
  mkp_genome_sizes out; std::string line;
  while (std::getline(f, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    BedLineParser p(line); std::string chrom; uint64_t len = 0;
    if (!(p.string(&chrom) && p.digits(&len))) throw Error(MKP_E_INVALID, "failed to parse sizes " + line);
    size_t k = 0; while (k < out.name.size() && out.name[k] != chrom) k++;
    if (k < out.name.size()) out.length[k] = len; else { out.name.push_back(chrom); out.length.push_back(len); }
  }
  return out;
}

// LocalizedModCounts::get_table (src/localise/util.rs:48-82) through the tab-delimited csv writer; `f32_text` = f32 Display
template <class F32Text> std::string localize_table_text(const mkp_localize_out& t, F32Text f32_text) {
  std::string s = "mod_code\toffset\tn_valid\tn_mod\tpercent_modified\n";
  const int64_t w = (int64_t)t.window; const size_t n_off = 2 * (size_t)t.window + 1;
  for (uint32_t k = 0; k < t.n_codes; k++) {
    const std::string c = code_text(t.code_repr[k]);
    for (size_t o = 0; o < n_off; o++) {
      const size_t i = (size_t)k * n_off + o;
      if (!t.n_rows[i]) continue;
      const uint64_t nm = t.n_mod[i], nv = t.n_valid[i];
      const float pct = nv == 0 ? 0.0f : ((float)nm / (float)nv) * 100.0f;   // ModPositionInfo::percent_modified (src/util.rs:920-936)
      s += c; s += '\t'; s += std::to_string((int64_t)o - w); s += '\t'; s += std::to_string(nv); s += '\t'; s += std::to_string(nm); s += '\t';
      s += f32_text(pct); s += '\n';
    }
  }
  return s;
}

inline void write_text_file(const std::string& path, const std::string& text) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) throw Error(MKP_E_IO, "failed to make output file " + path);
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size(); const bool closed = fclose(f) == 0;
  if (!ok || !closed) throw Error(MKP_E_IO, "short write on " + path);
}

}  // namespace mkp
