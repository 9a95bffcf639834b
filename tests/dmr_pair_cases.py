"""What the dmr pair tests share: the golden inputs of the reference's dmr regression test, the stand-in reference FASTA, records <-> row
arrays, and the score tolerance."""
import gzip
import os

import numpy as np

import dmr_pair_model as model
from pileup_cases import FIX

TABLE_A = os.path.join(FIX, "lung_00733-m_adjacent-normal_5mc-5hmc_chr20_cpg_pileup.bed.gz")
TABLE_B = os.path.join(FIX, "lung_00733-m_primary-tumour_5mc-5hmc_chr20_cpg_pileup.bed.gz")
REGIONS = os.path.join(FIX, "cpg_chr20_with_orig_names_selection.bed")
GOLDEN = os.path.join(FIX, "test_output_chr20-2.bed")

_cache = {}


def golden_inputs():
    """(records a, records b, regions, fasta dict) of the golden run, read once.  The test's GRCh38_chr20.fa is not among the fixtures: the
    stand-in has C at every '+' row position of either table, G at every '-' row position and N elsewhere, up to the last row — with it every
    row is accepted, as the rows of a CpG pileup are on the real reference."""
    if "golden" not in _cache:
        recs = [model.bedmethyl_records(gzip.open(p, "rt").read()) for p in (TABLE_A, TABLE_B)]
        last = max(r[1] for rs in recs for r in rs)
        seq = bytearray(b"N" * (last + 1))
        for rs in recs:
            for _c, pos, _code, strand, *_ in rs:
                want = ord("G") if strand == "-" else ord("C")
                assert seq[pos] in (ord("N"), want), "a position claimed by both strands"
                seq[pos] = want
        _cache["golden"] = (recs[0], recs[1], model.parse_regions(open(REGIONS).read()), {"chr20": seq.decode()})
    return _cache["golden"]


def write_fasta(path, fasta):
    with open(path, "w") as f:
        for name, seq in fasta.items():
            f.write(">%s\n" % name)
            for i in range(0, len(seq), 60):
                f.write(seq[i:i + 60] + "\n")
    return str(path)


def code_repr(code):
    return ord(code) if len(code) == 1 else (int(code) | (1 << 31))


def rows_of(records):
    """The row arrays Context.dmr_add_rows takes, of records of ONE contig in ascending pos"""
    a = lambda k, dt=np.uint32: np.array([r[k] for r in records], dtype=dt)
    z = np.zeros(len(records), dtype=np.uint32)
    return {"pos": a(1), "strand": np.array([ord(r[3]) for r in records], dtype=np.uint8), "code_repr": np.array([code_repr(r[2]) for r in records], dtype=np.uint32),
            "n_valid": a(4), "n_mod": a(5), "n_canonical": a(6), "n_other": z, "n_delete": z, "n_fail": z, "n_diff": z, "n_nocall": z}


def bedmethyl_text(records):
    """The records as bedMethyl lines (tabs up to column 10, blanks behind, as modkit writes them)"""
    out = []
    for chrom, pos, code, strand, nv, nm, nc in records:
        pct = "%.2f" % (100.0 * nm / nv) if nv else "NaN"
        out.append("%s\t%d\t%d\t%s\t%d\t%s\t%d\t%d\t255,0,0\t%d %s %d %d 0 0 0 0 0\n" % (chrom, pos, pos + 1, code, nv, strand, pos, pos + 1, nv, pct, nm, nc))
    return "".join(out)


def score_tolerance(terms):
    """|score - reference| allowed: 4 * 2^-52 * the sum of the |lgamma terms| of the row — the score is a sum of up to 24 lgamma values of
    size up to ~4e5, each rounded by libm; glibc against the six golden rows stays within 0.41 of that unit, the factor 4 leaves room for
    another libm and another summation order."""
    return 4.0 * 2.0 ** -52 * terms


def check_table(text, regions, results, header=False):
    """`text` against the model: the 13 other columns byte for byte, the printed score within tolerance, without exponent.  Returns the largest
    |difference| / (2^-52 * terms) seen."""
    want_fields, _ = model.split_table(model.table_text(regions, results, header), header)
    got_fields, got_scores = model.split_table(text, header)
    assert got_fields == want_fields
    written = [r for r in results if r["state"] == model.WRITTEN]
    worst = 0.0
    for res, s in zip(written, got_scores):
        assert "e" not in s.lower(), s
        d = abs(float(s) - res["score"])
        assert d <= score_tolerance(res["terms"]), (s, res["score"], d, score_tolerance(res["terms"]))
        if res["terms"]:
            worst = max(worst, d / (2.0 ** -52 * res["terms"]))
    return worst
