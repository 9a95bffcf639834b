"""Pins tests/hemi_model.py on the CPU: against the reference's two pileup-hemi goldens (every row, every count column), and against
the oracle on every directed BAM of tests/hemi_edge_cases.py under every flag set the GPU test (tests/test_gpu_hemi_edges.py) runs.
Then the directed BAMs are checked to hold the shapes they claim (properties of the records, found with the model's own tag parser),
and the model's rows per builder and flag set against the floors of hemi_edge_cases.FLOORS.

The second golden runs with a threshold estimated from a sample (-p), which is outside the model: the model is fed the threshold the
oracle reports for that run.
"""
import bisect
import re
import subprocess

import pytest

import hemi_edge_cases as hc
import hemi_model as hm
from pileup_cases import HEMI_GOLDEN_CASES, fixture, hemi_reference_fasta
from test_column_model import read_bam, read_fasta


def oracle_rows(oracle_bin, bam, out, flags):
    p = subprocess.run([oracle_bin, "pileup-hemi", bam, "-o", out] + flags, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-400:]
    return hm.read_hemi_bed(out), p.stderr


def assert_same(got, want, got_name, records):
    d = hm.first_difference(got, want)
    if d:
        raise AssertionError("%s vs model: first difference at (pos, pattern, base) %r: %s %r, model %r %s; reads over it (index, start, "
                             "flag, op index, op, window): %s" % (got_name, d[0], got_name, d[1], d[2], hm.COUNTS, hm.covering(records, d[0][0])))


@pytest.mark.parametrize("name,flags,bam,golden", HEMI_GOLDEN_CASES, ids=[c[0] for c in HEMI_GOLDEN_CASES])
def test_model_equals_reference_hemi_golden(oracle_bin, tmp_path, name, flags, bam, golden):
    fa = hemi_reference_fasta(tmp_path)
    contigs, recs = read_bam(fixture(bam))
    refs = read_fasta(fa)
    kw, k = dict(threshold=None), 0
    while k < len(flags):
        if flags[k] == "--motif":
            kw["motif"] = (flags[k + 1], int(flags[k + 2])); k += 2
        elif flags[k] == "--cpg":
            kw["motif"] = ("CG", 0)
        elif flags[k] == "--region":
            ctg, _, span = flags[k + 1].partition(":")
            a, b = span.replace(",", "").split("-")
            kw["region"] = (int(a), int(b)); k += 1       # (as the reference parses it: the start as written)
        else:
            assert flags[k] in ("--no-filtering", "--mixed-delim"), flags[k]
        k += 1
    if "--no-filtering" not in flags:
        _, err = oracle_rows(oracle_bin, fixture(bam), str(tmp_path / "o.bed"), flags + ["-r", fa])
        kw["threshold"] = float(re.search(r"threshold C (\S+)", err).group(1))
        assert 0.5 < kw["threshold"] < 1
    want = hm.pileup_hemi(recs[ctg], refs[ctg], **kw)
    got = hm.read_hemi_bed(fixture(golden))
    assert list(got) == [ctg] and len(got[ctg]) > 250
    assert_same(got[ctg], want, "golden", recs[ctg])


# ---------------------------------------------------------------------------------------------------------------------------------
# model vs oracle on the directed BAMs

@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            case = hc.BUILDERS[name](str(tmp_path_factory.mktemp(name) / name))
            case.parsed, case.loaded = hm.parse(case.records), {}
            cache[name] = case
        return cache[name]
    return get


def model_rows(case, flags, **extra):
    kw = hc.model_kwargs(case, flags)
    kw.update(extra)
    thr = kw["threshold"]
    if thr not in case.loaded:        # (the calls do not depend on the focus flags)
        case.loaded[thr] = hm.load(case.records, thr, case.parsed)
    return hm.pileup_hemi(case.records, case.ref, loaded=case.loaded[thr], **kw)


def floors_of(rows):
    """(rows, rows with n_delete > 0, rows with n_nocall > 0, rows whose pattern is not `-,-`, columns with two or more patterns)"""
    cols = {}
    for pos, pattern, base in rows:
        cols.setdefault(pos, set()).add((pattern, base))
    return (len(rows), sum(1 for v in rows.values() if v[5]), sum(1 for v in rows.values() if v[8]),
            sum(1 for k in rows if k[1] != "-,-"), sum(1 for c in cols.values() if len(c) > 1))


@pytest.mark.parametrize("name", sorted(hc.BUILDERS))
def test_model_equals_oracle_on_directed_bams(oracle_bin, built, tmp_path, name):
    case = built(name)
    assert open(case.bam, "rb").read() == open(case.bam_unindexed, "rb").read()     # one oracle run speaks for both files
    sets = hc.flag_sets(case)
    assert len(sets) == len(hc.FLOORS[name])
    for fi, flags in enumerate(sets):
        want = model_rows(case, flags)
        got, _ = oracle_rows(oracle_bin, case.bam, str(tmp_path / ("o%d.bed" % fi)), hc.oracle_flags(flags))
        assert set(got) <= {case.contig}
        try:
            assert_same(got.get(case.contig, {}), want, "oracle", case.records)
        except AssertionError as e:
            raise AssertionError("%s under %s: %s" % (name, " ".join(flags[:-2]), e))
        have, floor = floors_of(want), hc.FLOORS[name][fi]
        assert all(h >= f for h, f in zip(have, floor)), (name, fi, have, floor)
        # the floors in the file are the model's own numbers less a tenth, not something looser
        assert all(f >= int(h * 0.9) - 1 for h, f in zip(have, floor)), (name, fi, have, floor)
        assert have[0] > (hc.FAILED_MIN_ROWS if name == "failed_records" else 100)


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes are what they claim: properties of the records

def _fwd(rec):
    return hc.revcomp(rec[3]) if rec[1] & 16 else rec[3]


def _named(case, prefix):
    return [(i, rec, case.layouts[i]) for i, (rec, nm) in enumerate(zip(case.records, case.read_names)) if nm.startswith(prefix)]


def test_merge_windows_hold_the_listed_group_sizes(built):
    case = built("merge_windows")
    sizes = {}
    for i, rec, layout in _named(case, "mw"):
        assert rec[2] == [(1500, "M")] and hc.LAYOUTS[layout][2] in hc.MERGE_CLASSES
        sizes.setdefault(hm.group_sizes(rec[4], rec[5], _fwd(rec)), set()).add(bool(rec[1] & 16))
    want = set(hc.MERGE_PAIRS) - {(0, 0)}
    assert set(sizes) == want | {None}, sorted(want - set(sizes))      # None: (0, 0), a record that lists nothing fails
    assert all(sizes[p] == {False, True} for p in want), "a size pair on one strand only"
    for side in (0, 1):
        assert {p[side] for p in want} == set(hc.MERGE_SIZES)
    assert {(v, v) for v in hc.MERGE_SIZES if v} <= want and {(1, 193), (193, 1)} <= want
    # a group that lists nothing is written as an empty tag
    assert any(re.search(r"[CG]-[a-z0-9]+\?;", rec[4]) for _, rec, _ in _named(case, "mw")) and any(re.match(r"[CG]\+[a-z0-9]+\?;", rec[4]) for _, rec, _ in _named(case, "mw"))
    # skewed reads: every listed base of one group before (as sequenced) every listed base of the other, in both orders, on both strands
    seen = set()
    for i, rec, layout in _named(case, "sk"):
        g = hm.parse_tags(rec[4], rec[5], _fwd(rec))
        a = [p for (s, _), calls in g.items() if s == "+" for p in calls]
        b = [p for (s, _), calls in g.items() if s == "-" for p in calls]
        assert (len(a), len(b)) in hc.SKEWED and (max(a) < min(b) or max(b) < min(a))
        assert min(len(a), len(b)) > 64                      # the rank of a 64-event batch jumps at least one whole window of the other list
        seen.add((max(a) < min(b), bool(rec[1] & 16), len(a), len(b)))
    assert {(o, s) for o, s, _, _ in seen} == {(True, True), (True, False), (False, True), (False, False)}
    assert {(x, y) for _, _, x, y in seen} == set(hc.SKEWED)
    # reads with one strand called at every pair: every column of theirs is a NoCall
    trace = []
    model_rows(case, hc.flag_sets(case)[0], trace=trace)
    ones = {i for i, _, _ in _named(case, "one")}
    feats = [f for i, pos, f in trace if i in ones]
    assert len(feats) > 50 and all(f[0] == "N" for f in feats)
    nones = _named(case, "none")
    assert len(nones) == len(hc.DIRECTED) and all(hm.parse_tags(rec[4], rec[5], _fwd(rec)) is None for _, rec, _ in nones)


def test_partner_edges_put_plus_halves_on_the_lane_batch_edges(built):
    case = built("partner_edges")
    flags = hc.flag_sets(case)[0]
    loaded = {rd.index: rd for rd in case.loaded.get(None) or hm.load(case.records, None, case.parsed)}
    for motif in hc.MOTIFS:
        trace = []
        model_rows(case, flags, motif=motif, trace=trace)
        tag = "pe_%s%d_" % motif
        mine = {i: hc.LAYOUTS[layout][2] for i, _, layout in _named(case, tag)}
        assert len(mine) == 2 * 3 * len(hc.PARTNER_INDEXES)
        at = {}
        for i, pos, f in trace:
            if i in mine and f[0] in "PF":                   # a '+' half whose partner was found
                rd = loaded[i]
                merged = sorted(set(rd.ref_plus) | set(rd.ref_minus))
                at.setdefault(mine[i] in hc.MERGE_CLASSES, set()).add((merged.index(pos), rd.rev))
        for merge_class in (True, False):
            want = {(k, rev) for k in hc.PARTNER_INDEXES for rev in (False, True)}
            assert want <= at[merge_class], (motif, merge_class, sorted(want - at[merge_class]))
    # the seam motifs are in the reference, their halves either side of the seam
    for text, seams in hc.SEAMS.items():
        for s in seams.values():
            a = s - len(text) // 2
            assert case.ref[a:a + len(text)] == text and a < s < a + len(text)
    assert case.ref[0] == "G" and any(rec[0] == 0 for rec in case.records)
    # every missing-partner shape gives a NoCall (or nothing) at its CpG under --cpg, for the C/G layouts
    trace = []
    model_rows(case, flags, trace=trace)
    for what in ("ends_on_c", "g_clipped", "d_on_g", "n_on_g", "snp_on_g", "n_base_on_g", "snp_on_c", "snp_c_to_g"):
        idx = {i for i, _, layout in _named(case, what + "_") if layout in hc.C_LAYOUTS}
        assert len(idx) == 3
        site = {rec[0] for i, rec, _ in _named(case, what + "_")}
        feats = [(i, pos, f) for i, pos, f in trace if i in idx]
        assert feats and any(f[0] == "N" for _, _, f in feats), what
    for what in ("snp_on_c", "snp_c_to_g"):                  # the NoCall counts on another primary base
        idx = {i for i, _, _ in _named(case, what + "_")}
        assert any(f[0] == "N" and f[1] in "TG" for i, _, f in trace if i in idx), what


def test_cigar_windows_reach_every_decode_class(built):
    case = built("cigar_windows")
    counts, edge_ops = {}, {}
    for i, rec, layout in _named(case, "cw"):
        cls = hc.LAYOUTS[layout][2]
        counts.setdefault(cls, set()).add(len(rec[2]))
        for index in hc.CIGAR_EDGE_INDEXES[0] + hc.CIGAR_EDGE_INDEXES[1]:
            if len(rec[2]) > index + 1:
                edge_ops.setdefault((cls, index), set()).add(rec[2][index][1])
                if rec[2][index][1] in "DINP" and len(rec[2]) >= 515:      # a CpG on the match run on each side of the edge op
                    p = rec[0] + hc.ref_span(rec[2][:index - 1])
                    before = case.ref[p:p + rec[2][index - 1][0]]
                    p = rec[0] + hc.ref_span(rec[2][:index + 1])
                    after = case.ref[p:p + rec[2][index + 1][0]]
                    assert "CG" in before and "CG" in after, (i, index, before, after)
    for cls in (4, 5, 6):
        assert set(hc.CIGAR_OP_COUNTS) <= counts[cls], (cls, sorted(counts[cls]))
        for index in hc.CIGAR_EDGE_INDEXES[0] + hc.CIGAR_EDGE_INDEXES[1]:
            assert set("DINP") <= edge_ops[(cls, index)], (cls, index, edge_ops[(cls, index)])


def test_sparse_steps_hold_a_called_pair_on_the_4096_base_step(built):
    case = built("sparse_steps")
    loaded = {rd.index: rd for rd in case.loaded.get(None) or hm.load(case.records, None, case.parsed)}
    seen = set()
    for i, rec, layout in _named(case, "sp"):
        n = len(rec[3])
        assert rec[2] == [(n, "M")]
        for q in hc.SPARSE_PAIRS:
            if q + 1 < n:
                rd = loaded[i]
                assert rec[3][q:q + 2] == "CG"
                if hc.LAYOUTS[layout][0] == "C":             # both halves called: the C on the '+' strand, the G on the '-' strand
                    assert rec[0] + q in rd.ref_plus and rec[0] + q + 1 in rd.ref_minus
                else:
                    assert rec[0] + q in rd.ref_minus and rec[0] + q + 1 in rd.ref_plus
        seen.add((n, bool(rec[1] & 16), hc.LAYOUTS[layout][2]))
    assert seen == {(n, rev, cls) for n in hc.SPARSE_LENGTHS for rev in (False, True) for cls in (4, 5, 6)}


def test_failed_records_cross_the_listed_intervals(built):
    case = built("failed_records")
    by_index = {rd.index: rd for rd in case.parsed}
    # the work units of --cpg -i 500: a unit that ends inside a CpG is extended over it, so the seams are not all multiples of 500
    starts = [a for a, _, _ in hm.intervals(case.ref, None, hc.FAILED_INTERVAL, ("CG", 0), True)]

    def unit(p):
        return bisect.bisect_right(starts, p) - 1
    crossings = {}
    for i, rec, layout in _named(case, "bad_"):
        assert not by_index[i].ok, case.read_names[i]
        kind = next(k for k in hc.FAILURES if case.read_names[i].startswith(("bad_" + k, "bad_gap_" + k)))
        n = unit(rec[0] + hc.ref_span(rec[2]) - 1) - unit(rec[0]) + 1
        crossings.setdefault(kind, set()).add((n, rec[0] - starts[unit(rec[0])] >= 100))      # (.., starts mid-interval)
    for kind in hc.FAILURES:
        assert {n for n, _ in crossings[kind]} >= set(hc.FAILED_CROSSINGS), (kind, crossings[kind])
        assert {mid for _, mid in crossings[kind]} == {False, True}
    assert all(rd.ok for rd in case.parsed if not case.read_names[rd.index].startswith("bad_"))
    # one NoCall per interval crossed, and under a D / N / `N` base the NoCall moves on: the gapped records still leave five
    flags = [f for f in hc.flag_sets(case) if "-i" in f and "--cpg" in f][0]
    trace = []
    model_rows(case, flags, trace=trace)
    per_read = {}
    for i, pos, f in trace:
        if not by_index[i].ok:
            assert f[0] == "N"
            per_read.setdefault(i, []).append(pos)
    for i, rec, layout in _named(case, "bad_"):
        n = unit(rec[0] + hc.ref_span(rec[2]) - 1) - unit(rec[0]) + 1
        got = per_read.get(i, [])
        assert len({unit(p) for p in got}) == len(got) <= n
        if case.read_names[i].startswith("bad_gap_"):
            assert len(got) == 5
            firsts = [hc.first_hit(case.ref, "CG", (rec[0] // hc.FAILED_INTERVAL + k) * hc.FAILED_INTERVAL) for k in (1, 2, 3)]
            assert not set(firsts) & set(got), "the NoCall sits under a deletion, a ref-skip or an N base"
