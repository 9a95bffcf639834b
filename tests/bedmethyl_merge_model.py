"""An independent model of `modkit bedmethyl merge`, written from the reference (merge_data and EntryMergeBedMethyl::run,
src/bedmethyl_util/subcommands.rs:136-371; BedMethylLine, src/dmr/bedmethyl.rs:40-86; to_line, src/tabix.rs:33-74):

  * every line of every input goes into ONE map keyed (start, mod code, strand) per contig — the code is the name up to its first comma, so
    the two names of a multi-motif run at one position share a key and are summed, also inside one file;
  * summed: valid_coverage (the SCORE, column 5) and the seven counts of columns 12-18; nothing else of a line is kept;
  * order: start, then strand '+' < '-' < '.' (StrandRule, src/util.rs:297-307), then code.  The sort calls `cmp` on the code
    (subcommands.rs:186), that is Ord, which ModCodeRepr DERIVES (src/mod_base_code.rs:105-109): Code(char) before ChEbi(u32), letters by
    code point, numbers by number.  (Its hand-written PartialOrd, 141-150, says the opposite and is not what `cmp` runs.)  A name of one
    character is a letter code even when it is a digit (ModCodeRepr::parse tries char first, 112-122);
  * the line: 18 tab-separated columns, the bare code as the name, score = column 10 = the summed valid_coverage, colour 255,0,0,
    (n_mod as f32 / n_valid as f32) * 100 through {:.2} — `NaN` for 0 / 0, `inf` for n / 0;
  * contigs in the order of the sizes file, those of no input left out; the feeder walks [0, length): a line whose start is not below its
    contig's length, or whose contig the sizes do not list, is dropped (counted here).
Plain dicts and Python integers; the f32 arithmetic through numpy.float32.  '#' lines are skipped, as tabix skips them."""
import numpy as np

STRAND_RANK = {"+": 0, "-": 1, ".": 2}
COUNTS = ("n_valid", "n_mod", "n_canonical", "n_other", "n_delete", "n_fail", "n_diff", "n_nocall")


def parse_line(line):
    """(chrom, start, code text, strand, [valid_coverage, n_mod, n_canonical, n_other, n_delete, n_fail, n_diff, n_nocall])"""
    f = line.split()
    assert len(f) >= 18, line
    return f[0], int(f[1]), f[3].split(",", 1)[0], f[5], [int(f[4])] + [int(x) for x in f[11:18]]


def code_key(code):
    return (0, ord(code)) if len(code) == 1 else (1, int(code))


def sort_key(key):
    start, code, strand = key
    return start, STRAND_RANK[strand], code_key(code)


def percent_text(n_mod, n_valid):
    with np.errstate(divide="ignore", invalid="ignore"):
        pct = np.float32(n_mod) / np.float32(n_valid) * np.float32(100)
    if np.isnan(pct):
        return "NaN"
    if np.isinf(pct):
        return "inf"
    return "%.2f" % float(pct)


def to_line(chrom, start, code, strand, c):
    return "\t".join([chrom, str(start), str(start + 1), code, str(c[0]), strand, str(start), str(start + 1), "255,0,0", str(c[0]),
                      percent_text(c[1], c[0])] + [str(x) for x in c[1:]]) + "\n"


def merge_records(records):
    """records = [(start, code text, strand, [8 counts]), ...] of ONE contig, any order -> the merged ones in output order"""
    table = {}
    for start, code, strand, counts in records:
        key = (start, code, strand)
        if key in table:
            table[key] = [a + b for a, b in zip(table[key], counts)]
        else:
            table[key] = list(counts)
    return [(k[0], k[1], k[2], table[k]) for k in sorted(table, key=sort_key)]


def merge_texts(texts, sizes_text):
    """texts = the inputs' contents; sizes_text = `name<whitespace>length` lines.  Returns (merged text, lines dropped)."""
    sizes = {}
    for l in sizes_text.splitlines():
        name, length = l.split()[:2]
        sizes[name] = int(length)   # (a later line replaces the length and keeps the place: dicts keep insertion order)
    per_contig, dropped = {}, 0
    for text in texts:
        for l in text.splitlines():
            if l.startswith("#"):
                continue
            chrom, start, code, strand, counts = parse_line(l)
            if chrom not in sizes or start >= sizes[chrom]:
                dropped += 1
                continue
            per_contig.setdefault(chrom, []).append((start, code, strand, counts))
    out = []
    for chrom in sizes:
        for start, code, strand, counts in merge_records(per_contig.get(chrom, [])):
            out.append(to_line(chrom, start, code, strand, counts))
    return "".join(out), dropped


def code_text(c):
    c = int(c)
    return str(c & 0x7fffffff) if c & 0x80000000 else chr(c)


def records_of_rows(rows):
    """the records of a dict of row arrays (pos, strand as bytes, code_repr, the eight counts)"""
    cols = [rows[f] for f in COUNTS]
    return [(int(rows["pos"][i]), code_text(rows["code_repr"][i]), chr(rows["strand"][i]), [int(c[i]) for c in cols])
            for i in range(len(rows["pos"]))]
