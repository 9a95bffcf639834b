"""An independent model of `modkit stats <bedMethyl> --regions <bed>` (EntryStats::run, src/stats/subcommand.rs:65-206; GenomeRegion::into_stats,
src/stats/mod.rs:53-101; the BED parsers of src/util.rs:864-909 over src/parsing_utils.rs), written from the reference's description and not
from the library's C++: bedMethyl lines, a regions BED and the options in, the table text out.  The per-region loop is the obvious one — for
each region, for each line.  f32 arithmetic is numpy.float32 (np.float32(int) rounds as Rust's `as f32` for the totals used here, which stay
below 2^53), and Rust's f32 Display is the shortest round-trip digits without an exponent."""
import re

import numpy as np

WS = r"[ \t\r\n]"
_CHROM = re.compile(r"[^ \t\r\n]+")
_NUM = re.compile(WS + r"+([0-9]+)")
_NAME = re.compile(WS + r"*([^\t\r\n]+)")
_FLOAT = re.compile(WS + r"+[+-]?(?:(?:inf(?:inity)?|nan)|(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)", re.IGNORECASE)
_DOT = re.compile(WS + r"+\.")
_STRAND = re.compile(WS + r"+(.)", re.DOTALL)


class RegionsError(ValueError):
    pass


def _parse_line(line, stranded):
    """(chrom, start, end, name or None, strand) of one BED line, or RegionsError."""
    m = _CHROM.match(line)
    if not m:
        raise RegionsError("no contig: %r" % line)
    chrom, at = m.group(0), m.end()
    coords = []
    for _ in range(2):
        m = _NUM.match(line, at)
        if not m or int(m.group(1)) >= 1 << 64:
            raise RegionsError("no coordinate: %r" % line)
        coords.append(int(m.group(1)))
        at = m.end()
    name = None
    m = _NAME.match(line, at)
    if m:
        name, at = m.group(1), m.end()
    strand = "."
    if stranded:
        m = _FLOAT.match(line, at) or _DOT.match(line, at)
        if not m:
            raise RegionsError("no score: %r" % line)
        m = _STRAND.match(line, m.end())
        if not m or m.group(1) not in "+-.":
            raise RegionsError("no strand: %r" % line)
        strand = m.group(1)
    return chrom, coords[0], coords[1], name, strand


def parse_regions(text):
    """The regions of a BED file's text in file order.  The first line that does not start with '#' decides between the bed3/4 and the
    stranded parser by its number of tab-separated fields; then every line of the file is parsed ('#' lines included: they fail)."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()   # (a final line end closes the last line, it does not open another)
    lines = [l[:-1] if l.endswith("\r") else l for l in lines]
    first = next((l for l in lines if not l.startswith("#")), None)
    if first is None:
        raise RegionsError("no valid lines")
    stranded = len(first.split("\t")) > 4
    out = [_parse_line(l, stranded) for l in lines]
    for r in out:
        if r[1] > r[2]:
            raise RegionsError("start > end")   # (what the tabix iterator does with it is not in the reference tree: refused)
    if not out:
        raise RegionsError("no regions")
    return out


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
    return a == "." or b == "." or a == b


def region_totals(records, regions, codes=None, min_coverage=1):
    """Per region: None when its contig has no bedMethyl line at all (the tabix index does not list it: dropped), else
    {code: [n_mod, n_valid]} with an entry for every code that had a counted row in it."""
    contigs = {r[0] for r in records}
    allowed = None if codes is None else {parse_code(c) for c in codes}
    totals = []
    for chrom, start, end, _name, strand in regions:
        if chrom not in contigs:
            totals.append(None)
            continue
        agg = {}
        for c, pos, code, s, n_valid, n_mod in records:
            if c != chrom or not (start <= pos < end):
                continue
            if n_valid < min_coverage or not overlaps(s, strand) or (allowed is not None and code not in allowed):
                continue
            e = agg.setdefault(code, [0, 0])
            e[0] += n_mod
            e[1] += n_valid
        totals.append(agg)
    return totals


def rust_f32(x):
    return np.format_float_positional(np.float32(x), unique=True, trim="-")


def percent(n_mod, n_valid):
    if n_valid == 0:
        return np.float32(0)
    return (np.float32(n_mod) / np.float32(n_valid)) * np.float32(100)


def columns(totals, codes=None):
    if codes is not None:
        return sorted({parse_code(c) for c in codes}, key=code_key)
    return sorted({c for t in totals if t is not None for c in t}, key=code_key)


def format_table(regions, totals, cols, header=True):
    lines = []
    if header:
        lines.append("\t".join(["chrom", "start", "end", "name", "strand"] + [h % c for c in cols for h in ("count_%s", "count_valid_%s", "percent_%s")]))
    for (chrom, start, end, name, strand), t in zip(regions, totals):
        if t is None:
            continue
        row = [chrom, str(start), str(end), "." if name is None else name, strand]
        for c in cols:
            n_mod, n_valid = t.get(c, (0, 0))
            row += [str(n_mod), str(n_valid), rust_f32(percent(n_mod, n_valid))]
        lines.append("\t".join(row))
    return "".join(l + "\n" for l in lines)


def stats_table(bedmethyl_text, regions_text, codes=None, min_coverage=1, header=True):
    """The table `modkit stats` writes for these inputs."""
    regions = parse_regions(regions_text)
    totals = region_totals(bedmethyl_records(bedmethyl_text), regions, codes, min_coverage)
    return format_table(regions, totals, columns(totals, codes), header)
