"""An independent model of `modkit localize <bedMethyl> --regions <bed> --genome-sizes <tsv>` (EntryLocalize, src/localise/subcommand.rs:104-305;
LocalizedModCounts and GenomeRegion::into_localized_mod_counts, src/localise/util.rs:25-82, 189-227; GenomeRegion::midpoint, the BED parsers,
ModPositionInfo and read_sequence_lengths_file, src/util.rs:310-318, 860-936, 969-990; BedMethylLine::overlaps and fetch_region,
src/tabix.rs:24-31, 141-154), written from the reference and not from the library's C++: bedMethyl text, regions text, sizes text and the
options in, the table text out.  The loop is the obvious double one — for each region, for each line.  The reference has no golden for this
command (tests/test_localize.rs only runs --help), so tests/test_localize_host.py pins this model by totals added up by hand.
f32 arithmetic is numpy.float32; Rust's f32 Display is the shortest round-trip digits without an exponent."""
import re

import numpy as np

WS = r"[ \t\r\n]"
_CHROM = re.compile(r"[^ \t\r\n]+")
_NUM = re.compile(WS + r"+([0-9]+)")
_NAME = re.compile(WS + r"*([^\t\r\n]+)")
_FLOAT = re.compile(WS + r"+[+-]?(?:(?:inf(?:inity)?|nan)|(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)", re.IGNORECASE)
_DOT = re.compile(WS + r"+\.")
_STRAND = re.compile(WS + r"+(.)", re.DOTALL)
U64 = 1 << 64


class LocalizeError(ValueError):
    pass


def _lines(text):
    """BufRead::lines: split at LF, a final LF opens no further line, one CR in front of the LF goes."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return [l[:-1] if l.endswith("\r") else l for l in lines]


def _bed_line(line, stranded):
    """(chrom, start, end, strand) through parse_unstranded_bed_line / parse_stranded_bed_line (src/util.rs:864-909), or None."""
    m = _CHROM.match(line)
    if not m:
        return None
    chrom, at = m.group(0), m.end()
    coords = []
    for _ in range(2):
        m = _NUM.match(line, at)
        if not m or int(m.group(1)) >= U64:
            return None
        coords.append(int(m.group(1)))
        at = m.end()
    m = _NAME.match(line, at)   # the optional name: when it does not match, nothing is consumed
    if m:
        at = m.end()
    strand = "."
    if stranded:
        m = _FLOAT.match(line, at) or _DOT.match(line, at)
        if not m:
            return None
        m = _STRAND.match(line, m.end())
        if not m or m.group(1) not in "+-.":
            return None
        strand = m.group(1)
    return chrom, coords[0], coords[1], strand


def parse_regions(text):
    """load_focus_regions up to its contig filters (subcommand.rs:105-162): ([(chrom, start, end, strand), ...] in file order, lines skipped).
    The first line that does not start with '#' picks the parser by its number of whitespace-separated fields; every line of the file then
    goes through it and the ones that fail are counted; only a file without one parsed line fails.  start > end is kept as it is."""
    lines = _lines(text)
    first = next((l for l in lines if not l.startswith("#")), None)
    if first is None:
        raise LocalizeError("failed to inspect regions BED, no valid lines")
    stranded = len(first.split()) > 4
    parsed = [_bed_line(l, stranded) for l in lines]
    regions = [r for r in parsed if r is not None]
    if not regions:
        raise LocalizeError("failed to load any regions")
    return regions, len(parsed) - len(regions)


def parse_sizes(text):
    """read_sequence_lengths_file: {contig: length}; any line that is not `name<blanks>digits...` fails; a later line for a contig holds."""
    sizes = {}
    for line in _lines(text):
        m = _CHROM.match(line)
        n = _NUM.match(line, m.end()) if m else None
        if not n or int(n.group(1)) >= U64:
            raise LocalizeError("failed to parse sizes %r" % line)
        sizes[m.group(0)] = int(n.group(1))
    return sizes


def code_key(code):
    """Order of ModCodeRepr: Code(char) before ChEbi(number)."""
    return (0, code) if len(code) == 1 else (1, int(code))


def parse_code(raw):
    if len(raw) == 1:
        return raw
    if raw.isdigit():
        return str(int(raw))
    raise ValueError("bad mod code %r" % raw)


def bedmethyl_records(bedmethyl_text):
    """(chrom, start, code, strand, n_valid, n_mod) per line; the code is the name column up to the first comma."""
    out = []
    for line in bedmethyl_text.splitlines():
        f = line.split()
        out.append((f[0], int(f[1]), parse_code(f[3].split(",", 1)[0]), f[5], int(f[9]), int(f[11])))
    return out


def overlaps(a, b):
    """StrandRule::overlaps: either side both strands, or the same strand."""
    return a == "." or b == "." or a == b


def window_of(start, end, window, contig_length):
    """(ws, we, anchor) of a region: the window around its midpoint, clipped to the contig, and the midpoint of THAT (subcommand.rs:172-183,
    util.rs:203).  Python integers: nothing wraps."""
    mp = (start + end) // 2
    ws = mp - (window + 1) if mp >= window + 1 else 0          # checked_sub(..).unwrap_or(0)
    we = min(min(mp + window, U64 - 1), contig_length)         # saturating_add, then min with the contig
    return ws, we, (ws + we) // 2


def offset_totals(records, regions, sizes, window=2000, stranded=None, stranded_features=None):
    """{code: {offset: [n_mod, n_valid]}} over all regions (an entry for every cell that had a counted row); LocalizeError when no region is left
    after dropping those whose contig is not in the sizes or has no bedMethyl line (the tabix index does not list it)."""
    assert stranded in (None, "same", "opposite") and stranded_features in (None, "+", "-", ".")
    contigs = {r[0] for r in records}
    kept = [r for r in regions if r[0] in sizes and r[0] in contigs]
    if not kept:
        raise LocalizeError("failed to find any valid regions")
    counts = {}
    for chrom, start, end, strand in kept:
        ws, we, anchor = window_of(start, end, window, sizes[chrom])
        fetch_rule = stranded_features if stranded_features is not None else strand
        for c, pos, code, s, n_valid, n_mod in records:
            if c != chrom or not (ws <= pos < we):   # (we <= ws: nothing is fetched)
                continue
            if not overlaps(s, fetch_rule):
                continue
            if stranded == "same" and not overlaps(strand, s):
                continue
            if stranded == "opposite" and overlaps(strand, s):
                continue
            e = counts.setdefault(code, {}).setdefault(anchor - pos, [0, 0])
            e[0] += n_mod
            e[1] += n_valid
    return counts


def rust_f32(x):
    return np.format_float_positional(np.float32(x), unique=True, trim="-")


def percent(n_mod, n_valid):
    if n_valid == 0:
        return np.float32(0)
    return (np.float32(n_mod) / np.float32(n_valid)) * np.float32(100)


def format_table(counts):
    lines = ["mod_code\toffset\tn_valid\tn_mod\tpercent_modified"]
    for code in sorted(counts, key=code_key):
        for offset in sorted(counts[code]):
            n_mod, n_valid = counts[code][offset]
            lines.append("\t".join([code, str(offset), str(n_valid), str(n_mod), rust_f32(percent(n_mod, n_valid))]))
    return "".join(l + "\n" for l in lines)


def localize_table(bedmethyl_text, regions_text, sizes_text, window=2000, stranded=None, stranded_features=None):
    """The table `modkit localize` writes for these inputs."""
    regions, _skipped = parse_regions(regions_text)
    counts = offset_totals(bedmethyl_records(bedmethyl_text), regions, parse_sizes(sizes_text), window, stranded, stranded_features)
    return format_table(counts)
