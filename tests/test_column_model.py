"""Pins tests/column_model.py on the CPU: against the reference's own golden bedMethyl files (the fixture BAMs read with a minimal BAM
reader, gzip + struct), and against the oracle on every directed BAM of tests/cigar_edge_cases.py, tests/multi_feature_cases.py and
tests/shared_name_cases.py under every flag set the GPU tests (tests/test_gpu_cigar_edges.py, tests/test_gpu_multi_feature.py,
tests/test_gpu_shared_names.py) run.  Every count column and the row set
must be equal; no row is left out.

Goldens outside the model's scope, left out by name:
    test_pileup_with_filt, ..._position_filter, ..._positions_and_traditional   the threshold is estimated from a sample (-p)
    test_pileup_motifs_cg0_cgcg2*       two motifs (rows carry a motif label each)
    test_pileup_with_header             the same rows as test_pileup_no_filt under a header; included (the reader skips the header)
"""
import gzip
import struct
import subprocess

import pytest

import cigar_edge_cases as cases
import column_model as cm
import multi_feature_cases as mf
import shared_name_cases as sn
from pileup_cases import GOLDEN_CASES, REF, fixture

GOLDENS_IN_SCOPE = ["test_pileup_no_filt:23", "test_pileup_with_header:900", "test_pileup_with_region:194", "test_pileup_cpg_motif_filtering:237"] + \
    ["test_pileup_cpg_motif_filtering_strand_combine:257[i=%s]" % i for i in ("10", "88", "89", "90", "91", "92", "93", "94", "10000")] + \
    ["test_pileup_duplex_reads:217", "test_pileup_edge_filter_regression:360", "test_pileup_edge_filter_asymmetric_regression:418", "test_pileup_combine:71"]


def read_bam(path):
    """-> ([(contig, length)], {contig: [(start, flag, cigar, seq, MM, ML)]}) of a BAM file, records in file order."""
    d = gzip.open(path).read()
    assert d[:4] == b"BAM\1"
    o = 8 + struct.unpack_from("<i", d, 4)[0]
    n_ref, = struct.unpack_from("<i", d, o); o += 4
    contigs = []
    for _ in range(n_ref):
        ln, = struct.unpack_from("<i", d, o)
        contigs.append((d[o + 4:o + 4 + ln - 1].decode(), struct.unpack_from("<i", d, o + 4 + ln)[0])); o += 8 + ln
    recs = {name: [] for name, _ in contigs}
    width = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while o < len(d):
        bs, = struct.unpack_from("<i", d, o)
        rec = d[o + 4:o + 4 + bs]; o += 4 + bs
        tid, pos, lrn, _, _, ncig, flag, lseq = struct.unpack_from("<iiBBHHHi", rec, 0)
        a = 32 + lrn
        cigar = [(v >> 4, "MIDNSHP=X"[v & 15]) for v in struct.unpack_from("<%dI" % ncig, rec, a)]; a += 4 * ncig
        seq = "".join("=ACMGRSVTWYHKDBN"[(rec[a + i // 2] >> (0 if i % 2 else 4)) & 15] for i in range(lseq)); a += (lseq + 1) // 2 + lseq
        mm, ml, aux, p = "", b"", rec[a:], 0
        while p < len(aux):
            tag, ty, q = aux[p:p + 2], chr(aux[p + 2]), p + 3
            if ty in width:
                q += width[ty]
            elif ty in "ZH":
                q = aux.index(b"\0", q) + 1
            else:
                assert ty == "B"
                q += 5 + struct.unpack_from("<i", aux, q + 1)[0] * width[chr(aux[q])]
            if tag in (b"MM", b"Mm"):
                mm = aux[p + 3:q - 1].decode()
            elif tag in (b"ML", b"Ml"):
                ml = aux[p + 8:q]
            p = q
        if tid >= 0:
            recs[contigs[tid][0]].append((pos, flag, cigar, seq, mm, list(ml)))
    return contigs, recs


def read_fasta(path):
    out, name = {}, None
    for ln in open(path):
        if ln.startswith(">"):
            name = ln[1:].split()[0]; out[name] = []
        else:
            out[name].append(ln.strip().upper())
    return {k: "".join(v) for k, v in out.items()}


def model_flags(flags, contigs, refs):
    """The reference's command line -> the model's arguments, plus the contigs to run."""
    kw, k, only, edge, inverted = dict(threshold=None, interval=100000), 0, None, None, False
    while k < len(flags):
        f = flags[k]
        if f == "-i":
            kw["interval"] = int(flags[k + 1]); k += 1
        elif f == "--filter-threshold":
            kw["threshold"] = float(flags[k + 1]); k += 1
        elif f == "--cpg":
            kw["motif"] = ("CG", 0)
        elif f == "--motif":
            kw["motif"] = (flags[k + 1], int(flags[k + 2])); k += 2
        elif f == "--combine-strands":
            kw["combine_strands"] = True
        elif f == "--region":
            name, _, span = flags[k + 1].partition(":")
            only = name
            if span:
                a, b = span.replace(",", "").split("-")
                kw["region"] = (int(a), int(b))
            k += 1
        elif f == "--include-bed":
            kw["bed"] = {}
            for ln in open(flags[k + 1]):
                c = ln.split()
                kw["bed"].setdefault(c[0], []).append((int(c[1]), int(c[2]), c[5] if len(c) > 5 else "."))
            k += 1
        elif f == "--edge-filter":            # parse_edge_filter_input (command_utils.rs:243-277): one number trims both ends
            a, _, b = flags[k + 1].partition(",")
            edge = (int(a), int(b) if b else int(a)); k += 1
        elif f == "--invert-edge-filter":
            inverted = True
        elif f == "--combine-mods":
            kw["combine_mods"] = True
        elif f == "--ref":
            k += 1
        else:
            assert f in ("--no-filtering", "--only-tabs", "--mixed-delim", "--with-header"), f
        k += 1
    if edge is not None:
        kw["edge_filter"] = cm.EdgeFilter(edge[0], edge[1], inverted)
    return kw, [c for c in contigs if only in (None, c[0])]


def model_rows(bam_records, contigs, refs, flags):
    """{contig: rows} of the model under the reference's flags"""
    kw, run = model_flags(flags, contigs, refs)
    bed = kw.pop("bed", None)
    out = {}
    for name, ln in run:
        if "motif" in kw and name not in refs:
            continue
        ref = refs.get(name, "N" * ln)
        rows = cm.pileup(bam_records[name], ref, bed=None if bed is None else bed.get(name, []), **kw)
        if rows:
            out[name] = rows
    return out


def assert_same(got, want, got_name, records=None):
    assert sorted(got) == sorted(want), "%s has rows on %s, the model on %s" % (got_name, sorted(got), sorted(want))
    for ctg in want:
        d = cm.first_difference(got[ctg], want[ctg])
        if d:
            where = cm.covering(records[ctg], d[0][0]) if records else ""
            raise AssertionError("%s vs model, %s first difference at (pos, strand, code) %r: %s %r, model %r %s; reads over it "
                                 "(index, start, flag, op index, op, window): %s" % (got_name, ctg, d[0], got_name, d[1], d[2], cm.COUNTS, where))


@pytest.mark.parametrize("name", GOLDENS_IN_SCOPE)
def test_model_equals_reference_golden(name):
    case = [c for c in GOLDEN_CASES if c[0] == name]
    assert len(case) == 1
    _, flags, bam, golden = case[0]
    contigs, recs = read_bam(fixture(bam))
    refs = read_fasta(REF)
    want = model_rows(recs, contigs, refs, flags)
    got = cm.read_bedmethyl(fixture(golden))
    assert sum(len(r) for r in got.values()) >= 6   # (the --region golden holds six rows)
    assert_same(got, want, "golden", recs)


# ---------------------------------------------------------------------------------------------------------------------------------
# model vs oracle on the directed BAMs

def oracle_rows(oracle_bin, bam, out, flags):
    p = subprocess.run([oracle_bin, "pileup", bam, out] + flags, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-400:]
    return cm.read_bedmethyl(out)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = cases.BUILDERS[name](str(tmp_path_factory.mktemp(name) / name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(cases.BUILDERS))
def test_model_equals_oracle_on_directed_bams(oracle_bin, built, tmp_path, name):
    case = built(name)
    n_rows, walked = 0, {}
    for fi, flags in enumerate(cases.flag_sets(case)):
        kw = cases.model_kwargs(case, flags)
        if kw["threshold"] not in walked:      # (the walk does not depend on the focus flags)
            walked[kw["threshold"]] = cm.walk(case.records, kw["threshold"])
        want = cm.pileup(case.records, case.ref, walked=walked[kw["threshold"]], **kw)
        for bam in (case.bam, case.bam_unindexed):
            got = oracle_rows(oracle_bin, bam, str(tmp_path / ("o%d.bed" % fi)), cases.oracle_flags(flags))
            try:
                assert_same(got, {case.contig: want} if want else {}, "oracle", {case.contig: case.records})
            except AssertionError as e:
                raise AssertionError("%s under %s: %s" % (name, " ".join(flags), e))
        n_rows += len(want)
    assert n_rows > 100


def test_directed_cigars_reach_both_decoders(built):
    """The builders' own floor: every op count of the window / chunk / quad list, every edge op on every edge index and every scan-switch
    window exists in a layout the fused slot decoder takes (decode classes 0 / 1) and in one it leaves to the event decoders (2-4)."""
    case = built("window_edges")
    fused, events = cases.op_counts_by_decoder(case)
    assert set(cases.WINDOW_OP_COUNTS) <= fused and set(cases.WINDOW_OP_COUNTS) <= events, (sorted(fused), sorted(events))
    for index in cases.EDGE_INDEXES[0] + cases.EDGE_INDEXES[1]:
        f, e = cases.ops_at_by_decoder(case, index)
        assert set("IDNP") <= f and set("IDNP") <= e, (index, f, e)
    front = [[op for _, op in cigar[:4]] for (_, _, cigar, _, _, _) in case.records]
    assert any(x[:3] == ["S", "I", "M"] or x[:3] == ["S", "I", "="] for x in front) and any(x[:3] == ["H", "S", "I"] for x in front)
    case = built("scan_switch")
    shapes = {}
    for (_, _, cigar, _, _, _), layout in zip(case.records, case.layouts):
        if layout is not None:
            shapes.setdefault(tuple(cigar), set()).add(cases.LAYOUTS[layout][1] in cases.FUSED_CLASSES)
    assert len(shapes) >= 14 and all(v == {True, False} for v in shapes.values())


# ---------------------------------------------------------------------------------------------------------------------------------
# several primary bases, '-' strand tags, `N` tags, the edge filter and --combine-mods: model vs oracle on tests/multi_feature_cases.py

@pytest.fixture(scope="module")
def built_mf(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = mf.BUILDERS[name](str(tmp_path_factory.mktemp(name) / name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(mf.BUILDERS))
def test_model_equals_oracle_on_multi_feature_bams(oracle_bin, built_mf, tmp_path, name):
    """Every flag set of the GPU test, both files; and the floors of multi_feature_cases.FLOORS are the model's own numbers."""
    case = built_mf(name)
    walked, parsed, numbers = {}, {}, []
    for fi, flags in enumerate(mf.flag_sets(case)):
        want, stats = mf.model_rows(cm, case, flags, walked, parsed)
        numbers.append(stats)
        for bam in (case.bam, case.bam_unindexed):
            got = oracle_rows(oracle_bin, bam, str(tmp_path / ("o%d.bed" % fi)), cases.oracle_flags(flags))
            try:
                assert_same(got, {case.contig: want} if want else {}, "oracle", {case.contig: case.records})
            except AssertionError as e:
                raise AssertionError("%s under %s: %s" % (name, " ".join(flags), e))
        assert len(want) > 100
    assert numbers == mf.FLOORS[name], numbers
    if name == "edge_filter":
        assert all(n[3] > 0 for n in numbers)
    assert all(n[1] > 0 for n in numbers) and any(n[2] > 0 for n in numbers)


# ---------------------------------------------------------------------------------------------------------------------------------
# records that share a read name: the model's name-keyed cache vs the oracle's on tests/shared_name_cases.py

@pytest.fixture(scope="module")
def built_sn(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sn.BUILDERS[name](str(tmp_path_factory.mktemp(name) / name))
        return cache[name]
    return get


def check_against_oracle(oracle_bin, case, flags, want, out):
    for bam in (case.bam, case.bam_unindexed):
        got = oracle_rows(oracle_bin, bam, out, cases.oracle_flags(flags))
        try:
            assert_same(got, {case.contig: want} if want else {}, "oracle", {case.contig: case.records})
        except AssertionError as e:
            raise AssertionError("%s under %s: %s" % (case.name, " ".join(flags), e))


@pytest.mark.parametrize("name", sorted(sn.BUILDERS))
def test_model_equals_oracle_on_shared_name_bams(oracle_bin, built_sn, tmp_path, name):
    """Every flag set of the GPU test, both files, every row and count column (`partition` excepted: the oracle has no partition tags);
    the floors of shared_name_cases.FLOORS are the model's own numbers; no record of these BAMs meets owners that disagree."""
    case = built_sn(name)
    walked, numbers = {}, []
    for fi, flags in enumerate(sn.flag_sets(case)):
        want, stats, mixed = sn.model_rows(case, flags, walked)
        assert not mixed, (flags, [case.read_names[i] for i in mixed])
        numbers.append(stats)
        if name != "partition":
            check_against_oracle(oracle_bin, case, flags, want, str(tmp_path / ("o%d.bed" % fi)))
    assert numbers == sn.FLOORS[name], numbers
    assert all(n[0] > 100 and n[1] > 0 for n in numbers)
    assert all(n[2] > 0 for n in numbers) or name == "status"
    if name in ("bases_strands", "ownership"):
        assert all(n[3] > 0 for n in numbers)


@pytest.mark.parametrize("shape", sorted(sn.MIXED_SHAPES))
def test_model_reports_owners_that_disagree(oracle_bin, tmp_path, shape):
    """The model's mixed report on the shapes of shared_name_cases.MIXED_SHAPES; the oracle, which refuses nothing, equals the model on
    all of them."""
    case = sn.mixed(shape, str(tmp_path / shape))
    want, stats, mixed = sn.model_rows(case, case.flags, {})
    assert bool(mixed) == sn.MIXED[shape]
    if mixed:                       # the later record of the name, and only it
        assert [case.read_names[i] for i in mixed] == ["x"] and mixed == [case.index("x", 1)]
    check_against_oracle(oracle_bin, case, case.flags, want, str(tmp_path / "o.bed"))


def test_model_owners_equal_the_planner_table():
    """The owners tests/test_plan_host.py works out by hand for its records A, B, C (window [1000, 4000), intervals of 1000, focus
    positions 1100 1500 | 2500 | 3200 3600, B inside an `N` op over 2500) fall out of the model's loop: A owns the first interval for all
    three, C the other two alone; B is never asked in the second."""
    import test_plan_host as ph
    ref = ["A"] * 5000
    for p in ph.OWN_FOCUS:
        ref[p] = "C"
    ref = "".join(ref)
    members = [ph.A, ph.B, ph.C]
    records = []
    for i in members:
        start, end, _, _, cigar = ph.OWN_READS[i]
        ops = [(n, "MIDN"[op]) for n, op in cigar]
        seq, at = "", start
        for n, op in ops:
            seq += ref[at:at + n] if op == "M" else ""
            at += n
        assert at == end
        records.append((start, 0, ops, seq, "C+m?,0;", [200]))
    report = cm.new_report()
    cm.pileup(records, ref, motif=("C", 0), region=ph.OWN_WIN, interval=1000, names=["n"] * 3, report=report)
    got = {(members[i], (s - ph.OWN_WIN[0]) // 1000): members[o] for i, seen in report["asked"].items() for s, o, _, _ in seen}
    assert got == ph.owners_by_brute_force() == {(ph.A, 0): ph.A, (ph.B, 0): ph.A, (ph.C, 0): ph.A, (ph.C, 1): ph.C, (ph.C, 2): ph.C}
    assert cm.mixed_records(report) == []      # every owner is good and tagged alike
