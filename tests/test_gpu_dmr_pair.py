"""`dmr pair` over regions on the device (mkp_dmr.hip behind mkp_dmr_begin / _set_reference / _add_rows / _add_file / _add_resident / _get and
`mkpileup dmr pair`) against the independent model of tests/dmr_pair_model.py: everything but the score exactly, the score within the
tolerance of dmr_pair_cases.score_tolerance.
1. the reference's golden run, three ways; 2. directed rows on chunk and group edges; 3. each filter alone; 4. each inconsistency alone;
5. a seeded fuzz; 6. seams; 7. resident rows; 8. misuse."""
import gzip
import os
import struct

import numpy as np
import pytest

import dmr_pair_model as model
import modkit_amd
from dmr_pair_cases import (GOLDEN, REGIONS, TABLE_A, TABLE_B, bedmethyl_text, check_table, code_repr, golden_inputs, rows_of, score_tolerance,
                            write_fasta)
from pileup_cases import FIX, REF

pytestmark = pytest.mark.gpu
worst_seen = [0.0]   # the largest |device score - model| in units of 2^-52 * sum|lgamma terms| over the session (printed by the last test)


@pytest.fixture(scope="module")
def ctx():
    c = modkit_amd.Context()
    yield c
    c.close()


def by_chrom(records):
    out = {}
    for r in records:
        out.setdefault(r[0], []).append(r)
    return out


def session(ctx, recs_a, recs_b, regions, fasta, bases=("C",), lookup=None, min_cov=0, mask=False, cut=None):
    """One dmr session through add_rows: regions = [(chrom, start, end, name, strand)]; cut = {(sample, chrom): [row indices]} adds a
    contig in pieces cut there.  Returns dmr_get's dict."""
    chroms = sorted({r[0] for r in regions} | {r[0] for r in recs_a} | {r[0] for r in recs_b})
    lk = None
    if lookup is not None:
        lk = modkit_amd.dmr_default_lookup()
        lk.update({code_repr(c): b for c, b in lookup.items() if c not in model.DEFAULT_LOOKUP})
    ctx.dmr_begin([(chroms.index(c), s, e, st) for c, s, e, _n, st in regions], bases=bases, lookup=lk, min_valid_coverage=min_cov, mask=mask)
    for c, seq in fasta.items():   # as the command does: the span from the lowest region start to the highest region end
        spans = [(s, e) for rc, s, e, _n, _st in regions if rc == c]
        lo, hi = (min(s for s, _ in spans), min(max(e for _, e in spans), len(seq))) if spans else (0, 0)
        ctx.dmr_set_reference(chroms.index(c), seq[lo:max(lo, hi)], offset=lo)
    for sample, recs in enumerate((recs_a, recs_b)):
        for c, rs in by_chrom(recs).items():
            edges = [0] + list((cut or {}).get((sample, c), [])) + [len(rs)]
            for lo, hi in zip(edges, edges[1:]):
                ctx.dmr_add_rows(sample, chroms.index(c), rows_of(rs[lo:hi]))
    return ctx.dmr_get()


def compare(d, results):
    """dmr_get's dict against the model's per-region results"""
    codes = [chr(c) if c < 1 << 31 else str(c & 0x7fffffff) for c in d["codes"].tolist()]
    assert [int(s) for s in d["state"]] == [r["state"] for r in results]
    for r, res in enumerate(results):
        if res["state"] != model.WRITTEN:
            continue
        for s, key in enumerate("ab"):
            counts, total, rows = res[key]
            got = {codes[k]: int(d["n_mod"][s][r, k]) for k in range(len(codes)) if d["has_code"][s][r, k]}
            assert (got, int(d["total"][s][r]), int(d["n_rows"][s][r])) == (counts, total, rows), (r, key)
        diff = abs(float(d["score"][r]) - res["score"])
        assert diff <= score_tolerance(res["terms"]), (r, d["score"][r], res["score"])
        if res["terms"]:
            worst_seen[0] = max(worst_seen[0], diff / (2.0 ** -52 * res["terms"]))


def check(ctx, recs_a, recs_b, regions, fasta, **opts):
    want = model.regions_results(recs_a, recs_b, regions, fasta, bases=opts.get("bases", ("C",)),
                                 lookup=None if opts.get("lookup") is None else {**model.DEFAULT_LOOKUP, **opts["lookup"]},
                                 min_cov=opts.get("min_cov", 0), mask=opts.get("mask", False))
    d = session(ctx, recs_a, recs_b, regions, fasta, **opts)
    compare(d, want)
    return d, want


# ---- 1. the golden run
@pytest.fixture(scope="module")
def golden_fasta(tmp_path_factory):
    return write_fasta(tmp_path_factory.mktemp("dmr_golden") / "chr20_stand_in.fa", golden_inputs()[3])


def test_golden_run_three_ways(ctx, golden_fasta, tmp_path, monkeypatch):
    a, b, regions, fasta = golden_inputs()
    want = model.regions_results(a, b, regions, fasta)
    golden = open(GOLDEN).read()
    argv = ["-a", TABLE_A, "-b", TABLE_B, "-r", REGIONS, "--ref", golden_fasta, "--base", "C"]
    texts = []
    out = tmp_path / "device.bed"
    assert modkit_amd.dmr_pair(argv + ["-o", out]) == 6
    texts.append(out.read_text())
    monkeypatch.setenv("MKP_HOST_BEDMETHYL", "1")
    out = tmp_path / "host.bed"
    assert modkit_amd.dmr_pair(argv + ["-o", out, "--header"]) == 6
    monkeypatch.delenv("MKP_HOST_BEDMETHYL")
    assert out.read_text().startswith(model.HEADER)
    texts.append(out.read_text()[len(model.HEADER):])
    d = session(ctx, a, b, regions, fasta)
    compare(d, want)
    rs = modkit_amd.RegionSet(REGIONS, ["chr20"], dmr=True)
    out = tmp_path / "rows.bed"
    rs.write_dmr_table(d, out)
    texts.append(out.read_text())
    for text in texts:
        check_table(text, regions, want)                         # the model: 13 columns exactly, the score within tolerance
        assert model.split_table(text)[0] == model.split_table(golden)[0]
        for got, ref, res in zip(model.split_table(text)[1], model.split_table(golden)[1], want):
            assert abs(float(got) - float(ref)) <= score_tolerance(res["terms"])
    # the printed score is the f64 dmr_get returned, without exponent
    for got, value in zip(model.split_table(texts[2])[1], d["score"].tolist()):
        assert float(got) == value and "e" not in got.lower()
    assert texts[0] == texts[1] == texts[2]
    with pytest.raises(modkit_amd.MkpError) as e:                # the output exists now
        modkit_amd.dmr_pair(argv + ["-o", tmp_path / "device.bed"])
    assert e.value.status == -2 and "refusing to overwrite" in str(e.value)
    assert modkit_amd.dmr_pair(argv + ["-o", tmp_path / "device.bed", "-f"]) == 6


# ---- 2. chunk and group edges
def ladder(n_pos, chrom="c0", gap=3, first_single=True, sample=0, codes=("h", "m")):
    """Positions 5, 5 + gap, ..: one row per code and position, '+' on a C; with first_single the first position holds one row only, so that
    the two rows of position k are rows 2k - 1 and 2k of the table"""
    recs = []
    for k in range(n_pos):
        pos, nv = 5 + gap * k, 6 + (k + sample) % 5
        use = codes[-1:] if first_single and k == 0 else codes
        mods = [(k * 7 + 3 * j + sample) % 3 for j in range(len(use))]
        for c, nm in zip(use, mods):
            recs.append((chrom, pos, c, "+", nv, nm, nv - sum(mods)))
    return recs


def ladder_fasta(recs, chrom="c0", tail=40):
    seq = bytearray(b"N" * (max(r[1] for r in recs) + tail))
    for r in recs:
        seq[r[1]] = ord("G") if r[3] == "-" else ord("C")
    return {chrom: seq.decode()}


def test_chunk_and_group_edges(ctx):
    a, b = ladder(4101, sample=0), ladder(4101, sample=1)
    assert len(a) == 8201 and a[4095][1] == a[4096][1] != a[4094][1]        # a two-code group on rows 4095 / 4096 of a chunking from row 0
    fasta = ladder_fasta(a)
    fasta["c1"] = "ACGT" * 30
    pos = lambda k: 5 + 3 * k
    end = pos(4100) + 1
    regions = [("c0", 0, end, "all", "."), ("c0", pos(1), end, "from the second position", "."),   # its chunk edge falls between two groups
               ("c0", pos(0), pos(2048) + 1, "ends with the edge group", "."), ("c0", pos(2048), end, "starts with it", "."),
               ("c0", pos(2048) + 1, end, "starts behind it", "."), ("c0", 0, end, "all", "."), ("c0", 0, end, "plus only", "+"),
               ("c0", 0, end, "minus only", "-"), ("c0", pos(10), pos(10), "empty", "."), ("c0", pos(10) + 1, pos(11), "no row", "."),
               ("c0", end + 5, end + 30, "behind the rows", "."), ("c1", 0, 100, "only a has c1", "."), ("c2", 0, 100, "nobody has c2", ".")]
    regions += [("c0", pos(k), pos(k + span), "nest %d %d" % (k, span), ".") for k in (100, 2000, 2040) for span in (1, 3, 70, 1500, 2050)]
    regions += [("c0", pos(30 * k), pos(30 * k + 45), "overlap %d" % k, "+.-"[k % 3]) for k in range(40)]
    assert len(regions) < 100
    d, want = check(ctx, a + [("c1", 3, "m", "+", 4, 1, 3)], b, regions, fasta)
    states = [r["state"] for r in want]
    assert states[11] == states[12] == model.NO_CONTIG and states[7] == states[8] == states[9] == states[10] == model.WRITTEN
    assert want[0]["a"][2] == 8201 and want[7]["a"][2] == 0 and want[0]["a"] == want[5]["a"] == want[6]["a"]
    assert model.BAD not in states


# ---- 3. each filter alone
def small_case():
    """Twelve positions three apart from 10 on; a and b alike but for the counts.  ref: C at '+' / '.' positions, G at '-' positions."""
    def table(shift):
        recs = []
        for k in range(12):
            strand = "+-."[k % 3] if k < 9 else "+"
            nv = 10 + k + shift
            recs += [("c0", 10 + 3 * k, "h", strand, nv, 1 + shift, nv - 4 - 2 * shift), ("c0", 10 + 3 * k, "m", strand, nv, 3 + shift, nv - 4 - 2 * shift)]
        return recs
    a, b = table(0), table(1)
    return a, b, ladder_fasta(a), [("c0", 0, 28, "left", "."), ("c0", 28, 40, "middle", "."), ("c0", 40, 60, "right", "."), ("c0", 0, 60, "all", ".")]


def totals(d, want):
    return [(r["a"][1], r["a"][2]) if r["state"] == model.WRITTEN else None for r in want]


def test_filters_one_at_a_time(ctx):
    a, b, fasta, regions = small_case()
    d0, base = check(ctx, a, b, regions, fasta)
    assert [r["state"] for r in base] == [0, 0, 0, 0] and base[3]["a"][2] == 24
    def variant(a2=None, fasta2=None, regions2=None, **opts):
        _, w = check(ctx, a if a2 is None else a2, b, regions if regions2 is None else regions2, fasta if fasta2 is None else fasta2, **opts)
        return w
    seq = fasta["c0"]
    put = lambda p, ch: {"c0": seq[:p] + ch + seq[p + 1:]}
    # wrong reference base under a '+' position: its two rows leave
    w = variant(fasta2=put(10, "T"))
    assert w[3]["a"][2] == 22 and w[0]["a"][1] == base[0]["a"][1] - 10
    # a '-' row needs the complement: C under position 13 ('-') removes it, G keeps it
    assert variant(fasta2=put(13, "C"))[3]["a"][2] == 22
    # a '.' row counts as '+': position 16 ('.') on C is in, on G out
    assert a[4][3] == "." and variant(fasta2=put(16, "G"))[3]["a"][2] == 22
    # the strand rule of a region: '+' keeps the C positions ('+' and '.' rows), '-' the G positions
    w = variant(regions2=[("c0", 0, 60, "plus", "+"), ("c0", 0, 60, "minus", "-")])
    assert (w[0]["a"][2], w[1]["a"][2]) == (18, 6)
    # an unknown code is no row at all; assigned to C it takes part (and its position must then add up)
    extra = a + [("c0", 50, "x", "+", 9, 2, 7)]
    fx = {"c0": seq[:50] + "C" + seq[51:]}
    assert variant(a2=extra, fasta2=fx)[3]["a"] == base[3]["a"]
    w = variant(a2=extra, fasta2=fx, lookup={"x": "C"})
    assert w[3]["a"][2] == 25 and w[3]["a"][0]["x"] == 2
    w = variant(a2=extra, fasta2=fx, lookup={"x": "A"})                      # assigned to another base than the reference shows: out
    assert w[3]["a"] == base[3]["a"]
    # --mask: a lower-case reference base is no base
    low = put(10, "c")
    assert variant(fasta2=low)[3]["a"] == base[3]["a"] and variant(fasta2=low, mask=True)[3]["a"][2] == 22
    # --min-valid-coverage: whole positions leave; one row of a group leaving (unequal coverage) leaves a group that does not add up
    w = variant(min_cov=15)
    assert w[3]["a"][2] == 2 * sum(1 for k in range(12) if 10 + k >= 15)
    uneven = list(a)
    uneven[2] = ("c0", 13, "h", "-", 5, 0, a[3][6])
    assert variant(a2=uneven, min_cov=8)[0]["state"] == model.BAD
    healed = list(a)
    healed[2], healed[3] = ("c0", 13, "h", "-", 5, 0, 6), ("c0", 13, "m", "-", 10, 4, 6)
    w = variant(a2=healed, min_cov=8)
    assert w[0]["state"] == model.WRITTEN and variant(a2=healed)[0]["state"] == model.BAD
    # two --base: A rows on A ('+') and T ('-'); with C and G both given, a C is listed '+' and a G-code row on '-' there stays out
    two = a + [("c0", 70, "a", "+", 8, 3, 5), ("c0", 73, "a", "-", 9, 4, 5), ("c0", 76, "a", "+", 7, 1, 6)]
    f2 = {"c0": seq + "N" * 40}
    f2 = {"c0": f2["c0"][:70] + "A" + f2["c0"][71:73] + "T" + f2["c0"][74:76] + "C" + f2["c0"][77:]}
    r2 = regions + [("c0", 60, 90, "adenines", ".")]
    w = variant(a2=two, fasta2=f2, regions2=r2, bases=("C", "A"))
    assert w[4]["a"] == ({"a": 7}, 17, 2)
    assert variant(a2=two, fasta2=f2, regions2=r2)[4]["a"] == ({}, 0, 0)
    # C and G both given: every C and G is listed '+' (the positive set is asked first), so the '-' rows leave, an 8-oxo-G row on '-' over a C too
    cg = a[:2] + [("c0", 10, "o", "-", 10, 2, 8)] + a[2:]
    w = variant(a2=cg, bases=("C", "G"))
    assert w[3]["a"][2] == 18 and "o" not in w[3]["a"][0]
    w = variant(a2=cg, bases=("G",))                                         # G alone: a C is listed '-': only the 8-oxo-G row on '-' pairs with it
    assert w[3]["a"] == ({"o": 2}, 10, 1)


# ---- 4. each inconsistency alone
@pytest.mark.parametrize("kind", ["n_valid", "n_canonical", "sum"])
def test_one_inconsistent_position_drops_its_region_only(ctx, kind):
    a, b, fasta, regions = small_case()
    _, base = check(ctx, a, b, regions, fasta)
    chrom, pos, code, strand, nv, nm, nc = a[7]                             # position 19, in "left"
    a2 = list(a)
    a2[7] = {"n_valid": (chrom, pos, code, strand, nv + 1, nm, nc), "n_canonical": (chrom, pos, code, strand, nv, nm, nc + 1),
             "sum": (chrom, pos, code, strand, nv, nm + 1, nc)}[kind]
    d, w = check(ctx, a2, b, regions, fasta)
    assert [r["state"] for r in w] == [model.BAD, 0, 0, model.BAD]
    assert w[1] == base[1] and w[2] == base[2]
    assert d["bad"][0].tolist() == [1, 0, 0, 1] and d["bad"][1].tolist() == [0, 0, 0, 0]
    d, w = check(ctx, b, a2, regions, fasta)                                # the other sample
    assert [r["state"] for r in w] == [model.BAD, 0, 0, model.BAD] and d["bad"][1].tolist() == [1, 0, 0, 1]


# ---- 5. seeded fuzz
def fuzz_case(seed):
    """Two tables of about 1000 rows each over one contig of 6 kb and 40 regions: up to three codes, every strand letter, rows on wrong bases,
    low coverage, and one or two inconsistent positions"""
    rng = np.random.default_rng(9000 + seed)
    codes = [["m"], ["h", "m"], ["h", "m", "21839"]][seed % 3]
    n_pos = 340 + int(rng.integers(0, 60))
    positions = np.sort(rng.choice(np.arange(5, 6000), size=n_pos, replace=False))
    strands = rng.choice(list("+-."), size=n_pos, p=[0.45, 0.45, 0.1])
    seq = bytearray(b"N" * 6050)
    for p, s in zip(positions, strands):
        seq[p] = ord(rng.choice(list("CGcgT"), p=[0.02, 0.9, 0.04, 0.02, 0.02]) if s == "-" else rng.choice(list("CGcgT"), p=[0.9, 0.02, 0.02, 0.04, 0.02]))
    tables = []
    for sample in range(2):
        recs = []
        broken = set(rng.choice(n_pos, size=int(rng.integers(0, 3)), replace=False).tolist())
        for k, (p, s) in enumerate(zip(positions.tolist(), strands.tolist())):
            if rng.random() < 0.1:
                continue                                                     # the sample has no row here
            use = [c for c in codes if rng.random() < 0.9] or codes[:1]
            nv = int(rng.integers(0, 40))
            mods = [int(x) for x in rng.multinomial(nv, [0.15] * len(use) + [1 - 0.15 * len(use)])[:len(use)]]
            for j, c in enumerate(use):
                wrong = k in broken and j == 0
                recs.append(("c0", p, c, s, nv + (1 if wrong and seed % 2 else 0), mods[j] + (1 if wrong and not seed % 2 else 0), nv - sum(mods)))
        tables.append(recs)
    regions = []
    for k in range(40):
        start = int(rng.integers(0, 5600))
        regions.append(("c0", start, start + int(rng.integers(0, 400)), "r%d" % k, "+-."[int(rng.integers(0, 3))] if k % 4 else "."))
    return tables[0], tables[1], regions, {"c0": seq.decode()}


def test_seeded_fuzz(ctx):
    n_bad = n_written = 0
    for seed in range(50):
        a, b, regions, fasta = fuzz_case(seed)
        opts = {"min_cov": [0, 0, 5][seed % 3], "mask": seed % 5 == 0}
        _, want = check(ctx, a, b, regions, fasta, **opts)
        bad = sum(1 for r in want if r["state"] == model.BAD)
        assert bad <= len(regions) // 4, (seed, bad)                        # the generator's promise, held on the model alone
        n_bad += bad
        n_written += sum(1 for r in want if r["state"] == model.WRITTEN)
    assert n_bad > 20 and n_written > 1500


# ---- 6. seams
def test_a_table_in_pieces_with_a_region_over_the_seam(ctx, tmp_path, monkeypatch):
    a, b = ladder(700, sample=0, first_single=False), ladder(700, sample=1, first_single=False)
    fasta = ladder_fasta(a)
    regions = [("c0", 0, 5 + 3 * 700, "all", "."), ("c0", 5 + 3 * 340, 5 + 3 * 360, "over the seam", "."), ("c0", 5 + 3 * 350, 5 + 3 * 350 + 1, "the seam's position", ".")]
    whole, want = check(ctx, a, b, regions, fasta)
    for cut in ([700], [701], [700, 701, 702], [1, 1399]):                   # between two positions; inside one; one-row pieces; at the ends
        d = session(ctx, a, b, regions, fasta, cut={(0, "c0"): cut, (1, "c0"): cut[:1]})
        compare(d, want)
        assert d["n_rows"][0].tolist() == whole["n_rows"][0].tolist()
    # the device reader with pieces of 64 KiB of text: seams wherever they fall
    files = []
    for name, recs in (("a.bed", a), ("b.bed", b)):
        (tmp_path / name).write_text(bedmethyl_text(recs))
        assert (tmp_path / name).stat().st_size > 70_000
        files.append(str(tmp_path / name))
    (tmp_path / "r.bed").write_text("".join("%s\t%d\t%d\t%s\n" % r[:4] for r in regions))
    fa = write_fasta(tmp_path / "ref.fa", fasta)
    monkeypatch.setenv("MKP_BEDMETHYL_PIECE_KB", "64")
    assert modkit_amd.dmr_pair(["-a", files[0], "-b", files[1], "-r", tmp_path / "r.bed", "--ref", fa, "--base", "C", "-o", tmp_path / "out.bed"]) == 3
    check_table((tmp_path / "out.bed").read_text(), regions, want)


# ---- 7. resident rows
def bam_contigs(path):
    raw = gzip.open(path, "rb").read(1 << 20)
    l_text = struct.unpack_from("<i", raw, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    out = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, at)[0]
        out.append((raw[at + 4:at + 4 + l_name - 1].decode(), struct.unpack_from("<i", raw, at + 4 + l_name)[0]))
        at += 8 + l_name
    return out


def test_resident_rows_equal_added_rows(ctx):
    bam = os.path.join(FIX, "bc_anchored_10_reads.sorted.bam")
    name, length = bam_contigs(bam)[0]
    seq = "".join(l.strip() for l in open(REF).read().split(">" + name + "\n")[1].split(">")[0].splitlines())
    assert len(seq) == length
    regions = [(0, 0, length, "."), (0, 10, 60, "+"), (0, 40, 120, "-"), (0, 70, 71, ".")]
    c = modkit_amd.Context()
    try:
        c.set_caller(default_threshold=0.0)
        rows = modkit_amd.rows_to_numpy(c.process_region(bam, 0, 0, length))
        assert len(rows["pos"]) > 50
        c.dmr_begin(regions)
        c.dmr_set_reference(0, seq)
        c.dmr_add_resident(0)
        c.dmr_add_resident(1)
        resident = c.dmr_get()
    finally:
        c.close()
    ctx.dmr_begin(regions)
    ctx.dmr_set_reference(0, seq)
    ctx.dmr_add_rows(0, 0, rows)
    ctx.dmr_add_rows(1, 0, rows)
    added = ctx.dmr_get()
    assert int(added["n_rows"][0][0]) > 10 and added["state"].tolist() == [0, 0, 0, 0]
    for f in ("codes", "has_reference", "score", "state"):
        assert resident[f].tolist() == added[f].tolist()
    for f in ("n_mod", "has_code", "total", "n_rows", "bad", "contig_has_rows"):
        assert [x.tolist() for x in resident[f]] == [x.tolist() for x in added[f]]
    recs = [(name, int(p), chr(cd) if cd < 1 << 31 else str(cd & 0x7fffffff), chr(s), int(v), int(m), int(k)) for p, cd, s, v, m, k in
            zip(rows["pos"], rows["code_repr"], rows["strand"], rows["n_valid"], rows["n_mod"], rows["n_canonical"])]
    compare(added, model.regions_results(recs, recs, [(name, s, e, "r", st) for _t, s, e, st in regions], {name: seq}))


# ---- 8. misuse
def test_misuse_and_the_largest_score_error(ctx):
    a, b, fasta, regions = small_case()
    c = modkit_amd.Context()
    try:
        for call in (lambda: c.dmr_add_rows(0, 0, rows_of(a)), lambda: c.dmr_add_resident(0), c.dmr_get, lambda: c.dmr_set_reference(0, "ACGT")):
            with pytest.raises(modkit_amd.MkpError) as e:
                call()
            assert e.value.status == -1 and "mkp_dmr_begin" in str(e.value)
        c.dmr_begin([(0, 0, 60, ".")])
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_add_rows(2, 0, rows_of(a))
        assert e.value.status == -1 and "sample" in str(e.value)
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_add_resident(0)                                            # nothing is resident
        assert e.value.status == -1
        c.dmr_add_rows(0, 0, rows_of(a))
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_set_reference(0, fasta["c0"])                              # after the contig's rows
        assert e.value.status == -1
        with pytest.raises(modkit_amd.MkpError) as e:
            c.dmr_add_rows(0, 0, rows_of(a[:4]))                             # a piece in front of the one before
        assert e.value.status == -1 and "ascending" in str(e.value)
        for bases in ((), ("N",)):
            with pytest.raises(modkit_amd.MkpError) as e:
                c.dmr_begin([(0, 0, 60, ".")], bases=bases)
            assert e.value.status == -1
        c.dmr_begin([(0, 0, 60, ".")])                                      # no reference for the contig: not written
        c.dmr_add_rows(0, 0, rows_of(a))
        c.dmr_add_rows(1, 0, rows_of(b))
        assert c.dmr_get()["state"].tolist() == [modkit_amd.DMR_NO_REFERENCE]
    finally:
        c.close()
    print("largest |device score - model| in units of 2^-52 * sum|lgamma terms|: %.3f" % worst_seen[0])
    assert worst_seen[0] <= 4.0
