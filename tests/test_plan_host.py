"""The shard planner's stages (modkit_amd/csrc/mkp_plan.hpp) on the host: tests/plan_host.cpp is compiled with g++ (no HIP header, no
device; with -fsanitize=address,undefined when g++'s sanitizer runtime is installed) and run on read headers written by hand.  What it
prints is checked against expectations worked out here from the definitions, by brute force over positions.

Candidate reads.  A tile [r0, r1) keeps tallies for its halo range [r0 - 16, r1 + 16); a read is a candidate when its span [ref_start,
ref_end) holds a position of that range (slot tiles: a focus position of it).  A tile is kept iff it has a candidate; [first, last) of a
kept tile holds every candidate; `first` is the least read index whose end lies beyond the range's start (reads are sorted by start, so no
earlier read can reach the range: the prefix-max bound), `last` the first read that starts at or beyond the range's end.

Name owners, worked by hand (the rule quoted in plan_name_owners: in every interval the record asked about first owns the name — its first
column that is a focus position and not inside one of its ref-skips, file order breaking ties).  Window [1000, 4000), intervals
[1000, 2000) [2000, 3000) [3000, 4000), focus positions 1100 1500 | 2500 | 3200 3600.  Records of one name, in file order:
  A  [1050, 1400)  350M               interval 0: first column 1100.                            Ends before intervals 1 and 2.
  B  [1200, 3100)  1200M 200N 500M    interval 0: 1500.  Interval 1: its only focus position 2500 lies in the N [2400, 2600): B is
                                      never asked there.  Interval 2: no focus position in [3000, 3100).
  C  [1300, 3700)  2400M              interval 0: 1500.  Interval 1: 2500.  Interval 2: 3200.
  D  [4100, 4300)                     wholly outside the window: in no interval.
Owners: interval 0: A (1100 is the least column) for A, B and C; interval 1: C, alone — B, earlier in the file, would own it but for its
N; interval 2: C, alone.  So A is an ordinary record, B is answered from A in [1000, 2000) (one segment), C from A in [1000, 2000) and
from itself in [2000, 3000) and [3000, 4000), merged into one segment [2000, 4000).  B and C, and only they, get an MkpDupCons."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = 16
M, N = 0, 3   # CIGAR ops


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_host")
    base = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "modkit_amd", "csrc"),
            "-I", os.path.join(ROOT, "include")]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        san = []   # no sanitizer runtime on this machine: the same checks without it
    exe = d / "plan_host"
    subprocess.check_call(base + san + ["-o", str(exe), os.path.join(ROOT, "tests", "plan_host.cpp"), "-lz", "-lpthread"])
    count = [0]

    def run(win, reads, focus=(), intervals=(), tile=0):
        count[0] += 1
        scn = d / ("scenario%d.txt" % count[0])
        words = [win[0], win[1], tile, len(focus)] + list(focus) + [len(intervals)] + list(intervals) + [len(reads)]
        for start, end, cap, name, cigar in reads:
            words += [start, end, cap, "%x" % name, len(cigar)] + [x for op in cigar for x in op]
        scn.write_text(" ".join(str(w) for w in words) + "\n")
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("MKP_")}
        p = subprocess.run([str(exe), str(scn)], capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        out = {"read": [], "tile": [], "stile": [], "cons": [], "seg": [], "error": None, "plan": None}
        for ln in p.stdout.splitlines():
            w = ln.split()
            if w[0] == "error":
                out["error"] = (int(w[1]), " ".join(w[2:]))
            elif w[0] == "plan":
                out["plan"] = dict(zip(w[1::2], (int(x) for x in w[2::2])))
            else:
                out[w[0]].append(tuple(int(x) for x in w[1:]))
        return out
    return run


WIN = (10000, 14096)
READS = [   # (ref_start, ref_end): sorted by start
    (9000, 9900),      # ends before the window (and its halo)
    (10000, 10100),
    (10100, 10250),    # spans three 64-position tiles
    (10300, 11500),    # a long read ...
    (10400, 10500),    # ... with two reads nested in it: behind them the prefix-max of the ends is still the long read's
    (10600, 10650),
    (12000, 12300),    # [11500, 12000): no read
    (12000, 12010),
    (12290, 12900),
    (13000, 13001),    # one position, not a focus position
    (13500, 14146),    # runs past the window's end
    (14090, 14200),
]


def read_rows(spans):
    return [(s, e, 4, 0x1000000000000000 + 16 * i, [(e - s, M)]) for i, (s, e) in enumerate(spans)]


def check_candidates(tiles, ranges, spans, hits):
    """tiles: what the planner kept, as (key, first, last); ranges: every tile the plan considers, key -> (lo, hi) of its halo range in the
    coordinate of `spans`; hits(i, key): read i holds a position of the tile's range (brute force)"""
    kept = {k: (f, l) for k, f, l in tiles}
    assert len(kept) == len(tiles)
    n_kept = 0
    for key, (lo, hi) in ranges.items():
        cand = [i for i in range(len(spans)) if hits(i, key)]
        assert (key in kept) == bool(cand), (key, cand)
        if not cand:
            continue
        n_kept += 1
        first, last = kept[key]
        assert first <= min(cand) and max(cand) < last, (key, cand, first, last)
        assert first == min(i for i, (s, e) in enumerate(spans) if e > lo), key
        assert last == sum(1 for s, e in spans if s < hi), key
    assert n_kept == len(tiles) and 0 < n_kept < len(ranges)   # some tiles are dropped: the gap without reads
    return n_kept


def test_candidate_reads_dense(planner):
    out = planner(WIN, read_rows(READS), tile=64)
    assert out["error"] is None and out["plan"]["stream"] == 0 and not out["stile"]
    ranges = {(r0, min(r0 + 64, WIN[1])): (r0 - HALO, min(r0 + 64, WIN[1]) + HALO) for r0 in range(WIN[0], WIN[1], 64)}
    hits = lambda i, key: any(READS[i][0] <= p < READS[i][1] for p in range(*ranges[key]))
    n = check_candidates([((r0, r1), f, l) for r0, r1, f, l in out["tile"]], ranges, READS, hits)
    assert out["plan"]["n_tiles"] == n
    assert [t[:2] for t in out["tile"]] == sorted(t[:2] for t in out["tile"])
    # the read that spans three tiles is a candidate of each of them; the nested reads' tiles still start at the long read
    by_r0 = {t[0]: t for t in out["tile"]}
    assert all(by_r0[r0][2] <= 2 < by_r0[r0][3] for r0 in (10064, 10128, 10192))
    assert by_r0[10640][2] == 3 and by_r0[11024][2:] == (3, 6)


FOCUS = sorted(set(p for p in range(*WIN) if p % 7 == 3 and not 11000 <= p < 11200 and not 13100 <= p < 13400) | set(range(12000, 12040)))


def test_slot_ranges_and_candidate_reads_on_slot_tiles(planner):
    """a focus set placed by hand: every seventh position, 200 positions without one ([11000, 11200), under the long read), a second hole
    and a run of 40 adjacent ones; with tile_positions = 64 a slot tile holds 32 slots (a quarter of it, at least 32)"""
    out = planner(WIN, read_rows(READS), focus=FOCUS, tile=64)
    assert out["error"] is None and out["plan"]["stream"] == 1 and not out["tile"]   # (the cov_off guard does not fire at these sizes)
    below = lambda p: sum(1 for f in FOCUS if f < p)
    off = 0
    for i, (s, e) in enumerate(READS):
        gs0, n_sl, cov_off = out["read"][i][1:4]
        assert gs0 == below(s) and n_sl == sum(1 for f in FOCUS if s <= f < e), i
        assert cov_off == off, i
        off += (n_sl + 3) // 4 * 4
    assert out["plan"]["cov_bytes"] == off
    assert out["read"][0][2] == 0 and out["read"][9][2] == 0 and out["read"][3][2] > 100   # reads without a focus position, and the long one
    slot_spans = [(out["read"][i][1], out["read"][i][1] + out["read"][i][2]) for i in range(len(READS))]
    ranges, geometry = {}, {}
    for g0 in range(0, len(FOCUS), 32):
        g1 = min(len(FOCUS), g0 + 32)
        r0, r1 = FOCUS[g0], FOCUS[g1 - 1] + 1
        geometry[(g0, g1)] = (below(r0 - HALO), below(r1 + HALO), r0, r1)
        ranges[(g0, g1)] = (r0 - HALO, r1 + HALO)
    for t in out["stile"]:
        assert geometry[t[:2]] == t[2:6], t
    # candidates by reference position: a read holding a FOCUS position of the tile's halo range; the bounds are checked in slots
    hits = lambda i, key: any(READS[i][0] <= f < READS[i][1] for f in FOCUS if ranges[key][0] <= f < ranges[key][1])
    n = check_candidates([(t[:2], t[6], t[7]) for t in out["stile"]], {k: geometry[k][:2] for k in ranges}, slot_spans, hits)
    assert out["plan"]["n_tiles"] == n


NAME, OTHER = 0x1234567890abcdef, 0x1fedcba987654321
OWN_WIN, OWN_IV, OWN_FOCUS = (1000, 4000), [1000, 2000, 3000], [1100, 1500, 2500, 3200, 3600]
OWN_READS = [   # (ref_start, ref_end, event_cap, name hash, CIGAR)
    (1050, 1400, 4, NAME, [(350, M)]),                              # A
    (1200, 3100, 8, NAME, [(1200, M), (200, N), (500, M)]),         # B
    (1300, 3700, 16, NAME, [(2400, M)]),                            # C
    (1350, 1500, 2, OTHER, [(150, M)]),                             # another name
    (4100, 4300, 32, NAME, [(200, M)]),                             # D
]
A, B, C, D = 0, 1, 2, 4


def owners_by_brute_force():
    """{(record, interval): owner} from the rule, position by position"""
    members = [i for i, r in enumerate(OWN_READS) if r[3] == NAME and r[1] > OWN_WIN[0] and r[0] < OWN_WIN[1]]
    asked = {}
    for i in members:
        s, e, _, _, cigar = OWN_READS[i]
        p, skipped = s, set()
        for ln, op in cigar:
            if op == N:
                skipped |= set(range(p, p + ln))
            p += ln
        assert p == e
        asked[i] = [q for q in range(s, e) if q in OWN_FOCUS and q not in skipped]
    own = {}
    for k, a in enumerate(OWN_IV):
        b = OWN_IV[k + 1] if k + 1 < len(OWN_IV) else OWN_WIN[1]
        first = {i: min(q for q in asked[i] if a <= q < b) for i in members if any(a <= q < b for q in asked[i])}
        if first:
            owner = min(first, key=lambda i: (first[i], i))
            for i in first:
                own[(i, k)] = owner
    return own


def test_name_owners_per_interval(planner):
    out = planner(OWN_WIN, OWN_READS, focus=OWN_FOCUS, intervals=OWN_IV)
    assert out["error"] is None and out["plan"]["groups"] == 1
    own = owners_by_brute_force()
    assert own == {(A, 0): A, (B, 0): A, (C, 0): A, (C, 1): C, (C, 2): C}   # the docstring's table: B owns nothing, least of all interval 1
    assert [r[5] for r in out["read"]] == [1, 1, 1, 0, 0]                       # D lies outside the window: no member
    event_off = [r[4] for r in out["read"]]
    assert event_off == [0, 4, 12, 28, 30]
    # per record its segments: one per interval, adjacent intervals of one owner merged
    want_cons, want_segs, eff = [], [], sum(r[2] for r in OWN_READS)
    for i in (A, B, C):
        segs = []
        for k, a in enumerate(OWN_IV):
            if (i, k) not in own:
                continue
            b = OWN_IV[k + 1] if k + 1 < len(OWN_IV) else OWN_WIN[1]
            if segs and segs[-1][3] == own[(i, k)] and segs[-1][1] == a:
                segs[-1] = (segs[-1][0], b) + segs[-1][2:]
            else:
                segs.append((a, b, event_off[own[(i, k)]], own[(i, k)]))
        if all(s[3] == i for s in segs):
            continue   # answered by itself everywhere: no MkpDupCons
        cap = sum(OWN_READS[s[3]][2] for s in segs)
        want_cons.append((i, len(want_segs), len(segs), event_off[i], eff, cap))
        want_segs += segs
        eff += cap
    assert [c[0] for c in want_cons] == [B, C]
    assert want_segs == [(1000, 2000, 0, A), (1000, 2000, 0, A), (2000, 4000, 12, C)]   # C's two own intervals are one segment
    assert out["cons"] == want_cons and out["seg"] == want_segs
    assert out["plan"]["events_cap"] == eff


def test_unsorted_records_are_refused(planner):
    reads = read_rows(READS)
    reads[4], reads[5] = reads[5], reads[4]
    out = planner(WIN, reads, tile=64)
    assert out["error"] is not None and out["error"][0] < 0 and out["error"][1] == "records must be coordinate sorted"
    assert not out["tile"] and not out["read"]
