"""An independent model of `modkit dmr pair -a A -b B -r regions.bed --ref ref.fa --base C` in its region form (v0.4.4:
src/dmr/subcommands.rs, pairwise.rs, bedmethyl.rs:172-267, llr_model.rs, util.rs:180-428, src/genome_positions.rs:91-127, src/tabix.rs:163-189),
written from those files and not from the library's C++ or its kernel: bedMethyl records of two samples, a regions BED, the reference
sequences and the options in; per region the counts, the score and the table text out.  Everything is the obvious per-region loop over
dicts and sets; the score is math.lgamma in f64; f32 arithmetic is numpy.float32.

The score: `prior.posterior(&data).ln_m(&data)` is the marginal likelihood of the data under the POSTERIOR of a Jeffreys prior, so with k
categories and counts n_i (N their sum)   llk(n) = [sum lnG(1/2 + 2 n_i) - lnG(k/2 + 2N)] - [sum lnG(1/2 + n_i) - lnG(k/2 + N)]   and
score = llk(a) + llk(b) - llk(a + b).  For k > 2 (rv's Dirichlet) this is a reading of rv 0.16 that no reference value pins."""
import math
from decimal import ROUND_HALF_EVEN, Decimal

import numpy as np

from region_stats_model import RegionsError, _parse_line, code_key

# MOD_CODE_TO_DNA_BASE (src/mod_base_code.rs:69-90)
DEFAULT_LOOKUP = {"m": "C", "h": "C", "f": "C", "c": "C", "21839": "C", "C": "C", "a": "A", "A": "A", "17596": "A", "g": "T", "e": "T", "b": "T",
                  "17802": "T", "T": "T", "o": "G", "G": "G", "16450": "T"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
WRITTEN, NO_CONTIG, NO_REFERENCE, BAD, MODEL = 0, 1, 2, 3, 4


def parse_regions(text):
    """parse_roi_bed: the '#' lines in front are skipped, the first other line picks the parser by its tab-separated fields (<= 4: bed3/4),
    every line from there on must parse.  [(chrom, start, end, name, strand)] with the name made up where the line has none."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    lines = [l[:-1] if l.endswith("\r") else l for l in lines]
    while lines and lines[0].startswith("#"):
        lines.pop(0)
    if not lines:
        raise RegionsError("zero non-comment lines in regions")
    stranded = len(lines[0].split("\t")) > 4
    out = []
    for l in lines:
        chrom, start, end, name, strand = _parse_line(l, stranded)
        out.append((chrom, start, end, "%s:%d-%d" % (chrom, start, end) if name is None else name, strand))
    return out


def bedmethyl_records(text):
    """(chrom, pos, code, strand, n_valid, n_mod, n_canonical) of every line of a bedMethyl text"""
    out = []
    for line in text.splitlines():
        f = line.split()
        if not f or f[0].startswith("#"):
            continue
        out.append((f[0], int(f[1]), f[3].split(",")[0], f[5], int(f[9]), int(f[11]), int(f[12])))
    return out


def listed_positions(seq, start, end, strand, bases, mask):
    """get_positions: {position: (strand '+' / '-', reference base)} of [start, end)"""
    pos_set, neg_set = set(bases), {COMPLEMENT[b] for b in bases}
    out = {}
    for p in range(start, end):
        b = seq[p] if mask else seq[p].upper()
        if b in pos_set and strand in "+.":
            out[p] = ("+", b)
        elif b in neg_set and strand in "-.":
            out[p] = ("-", b)
    return out


def aggregate(records, positions, lookup, min_cov):
    """filter_sample_records + aggregate_counts of one sample's records on the region's contig: ({code: n_mod}, total, rows) or None when a
    position is inconsistent"""
    groups = {}
    for _chrom, pos, code, strand, n_valid, n_mod, n_can in records:
        if n_valid < min_cov or code not in lookup:
            continue
        s = "-" if strand == "-" else "+"
        base = COMPLEMENT[lookup[code]] if s == "-" else lookup[code]
        if positions.get(pos) != (s, base):
            continue
        groups.setdefault((pos, s, base), []).append((code, n_valid, n_mod, n_can))
    counts, total, rows = {}, 0, 0
    bad = False
    for g in groups.values():
        rows += len(g)
        if len({x[1] for x in g}) != 1 or len({x[3] for x in g}) != 1:
            bad = True
            continue
        check = g[0][3]
        for code, _v, n_mod, _c in g:
            counts[code] = counts.get(code, 0) + n_mod
            check += n_mod
        if check != g[0][1]:
            bad = True
        total += g[0][1]
    return None if bad else (counts, total, rows)


def llk(n):
    """(value, sum of |lgamma terms|)"""
    k2, N = len(n) / 2.0, float(sum(n))
    twice, once = [math.lgamma(0.5 + 2.0 * x) for x in n], [math.lgamma(0.5 + x) for x in n]
    big2, big1 = math.lgamma(k2 + 2.0 * N), math.lgamma(k2 + N)
    return (sum(twice) - big2) - (sum(once) - big1), sum(abs(t) for t in twice + once + [big2, big1])


def llk_ratio(a_counts, a_total, b_counts, b_total):
    """(score, sum of |lgamma terms|) or None where the reference fails"""
    if sum(a_counts.values()) > a_total or sum(b_counts.values()) > b_total:
        return None
    n_categories = max(len(a_counts), len(b_counts)) + 1
    if n_categories < 2:
        return 0.0, 0.0
    union = sorted(set(a_counts) | set(b_counts), key=code_key)
    if n_categories == 2 and len(union) != 1:
        return None
    a = [a_total - sum(a_counts.values())] + [a_counts.get(c, 0) for c in union]
    b = [b_total - sum(b_counts.values())] + [b_counts.get(c, 0) for c in union]
    (la, ta), (lb, tb), (lab, tab) = llk(a), llk(b), llk([x + y for x, y in zip(a, b)])
    return la + lb - lab, ta + tb + tab


def f64_display(x):
    if x != x:
        return "NaN"
    return np.format_float_positional(np.float64(x), unique=True, trim="-")


def f32_display(x):
    x = np.float32(x)
    if x != x:
        return "NaN"
    return np.format_float_positional(x, unique=True, trim="-")


def pct2(count, total):
    with np.errstate(all="ignore"):
        v = (np.float32(count) / np.float32(total)) * np.float32(100)
    if v != v:
        return "NaN"
    return str(Decimal(float(v)).quantize(Decimal("0.01"), rounding=ROUND_HALF_EVEN))


def counts_text(counts, total=None):
    if not counts:
        return "."
    return ",".join("%s:%s" % (c, counts[c] if total is None else pct2(counts[c], total)) for c in sorted(counts, key=code_key))


def regions_results(records_a, records_b, regions, fasta, bases=("C",), lookup=None, min_cov=0, mask=False):
    """Per region a dict: state, and for a written one: a / b = (counts, total, rows), score, terms (sum of |lgamma terms|)"""
    lookup = DEFAULT_LOOKUP if lookup is None else lookup
    contigs = [{r[0] for r in records_a}, {r[0] for r in records_b}]
    by_chrom = [{}, {}]
    for s, recs in enumerate((records_a, records_b)):
        for r in recs:
            by_chrom[s].setdefault(r[0], []).append(r)
    out = []
    for chrom, start, end, _name, strand in regions:
        if chrom not in contigs[0] or chrom not in contigs[1]:
            out.append({"state": NO_CONTIG})
            continue
        if chrom not in fasta:
            out.append({"state": NO_REFERENCE})
            continue
        positions = listed_positions(fasta[chrom], start, end, strand, bases, mask)
        agg = [aggregate([r for r in by_chrom[s][chrom] if start <= r[1] < end], positions, lookup, min_cov) for s in range(2)]
        if agg[0] is None or agg[1] is None:
            out.append({"state": BAD})
            continue
        ratio = llk_ratio(agg[0][0], agg[0][1], agg[1][0], agg[1][1])
        if ratio is None:
            out.append({"state": MODEL})
            continue
        out.append({"state": WRITTEN, "a": agg[0], "b": agg[1], "score": ratio[0], "terms": ratio[1]})
    return out


HEADER = "\t".join(["chrom", "start", "end", "name", "score", "strand", "a_counts", "a_total", "b_counts", "b_total", "a_mod_percentages",
                    "b_mod_percentages", "a_pct_modified", "b_pct_modified"]) + "\n"


def table_rows(regions, results):
    """The fields of every written region, the score as a float"""
    rows = []
    for (chrom, start, end, name, strand), res in zip(regions, results):
        if res["state"] != WRITTEN:
            continue
        (ac, at, _), (bc, bt, _) = res["a"], res["b"]
        with np.errstate(all="ignore"):
            pa, pb = np.float32(sum(ac.values())) / np.float32(at), np.float32(sum(bc.values())) / np.float32(bt)
        rows.append([chrom, str(start), str(end), name, res["score"], strand, counts_text(ac), str(at), counts_text(bc), str(bt), counts_text(ac, at),
                     counts_text(bc, bt), f32_display(pa), f32_display(pb)])
    return rows


def table_text(regions, results, header=False):
    return (HEADER if header else "") + "".join("\t".join(f64_display(f) if isinstance(f, float) else f for f in row) + "\n"
                                                for row in table_rows(regions, results))


def split_table(text, header=False):
    """(the 13 fields of every row but the score, the scores as text)"""
    lines = text.splitlines()[1 if header else 0:]
    fields = [l.split("\t") for l in lines]
    return [f[:4] + f[5:] for f in fields], [f[4] for f in fields]
