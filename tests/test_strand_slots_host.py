"""The planner's slot-entry lists and the fused reads' runs in them (modkit_amd/csrc/mkp_plan.hpp: window_slots, plan_read_entries,
build_work_records) on the host: tests/strand_slots_host.cpp is compiled with g++ (no HIP header, no device; with
-fsanitize=address,undefined when g++'s sanitizer runtime is installed) and run on focus bytes and read headers written by hand.

Expected, by brute force over the focus bytes.  The slots are the positions with a rule, numbered in genome order (the global index);
`all` lists every slot, `plus` those whose rule has bit 0, `minus` those whose rule has bit 1, each as (position, global index), and the
three are concatenated in that order.  A fused read spans the slots inside [ref_start, ref_end).  It needs tally strand aln (1 for a
reverse read) and, since every fused read here has a tag, also aln ^ sg0.  With one needed strand s whose list is strictly shorter than
`all` it decodes the slots of its span whose rule has bit s — a contiguous run of list s; otherwise, and always under
MKP_STRAND_SLOTS=0, every slot of its span — a run of `all`.  gs0, n_sl and cov_off are what they are without the lists, and the work
records come in descending order of the entry count."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUS, MINUS, BOTH = 1, 2, 3
FWD, REV = 0, 1
T_POS, T_NEG, T_NONE = 0, 1, 2      # `C+m?`, `C-m?` (sg0 = 1), no MM tag (not a fused read)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("strand_slots_host")
    base = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "modkit_amd", "csrc"),
            "-I", os.path.join(ROOT, "include")]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        san = []   # no sanitizer runtime on this machine: the same checks without it
    exe = d / "strand_slots_host"
    subprocess.check_call(base + san + ["-o", str(exe), os.path.join(ROOT, "tests", "strand_slots_host.cpp"), "-lz", "-lpthread"])
    count = [0]

    def run(win, focus, reads, knob=None):
        count[0] += 1
        scn = d / ("scenario%d.txt" % count[0])
        words = [win[0], win[1], len(focus)] + [x for pr in focus for x in pr] + [len(reads)] + [x for rd in reads for x in rd]
        scn.write_text(" ".join(str(w) for w in words) + "\n")
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("MKP_")}
        if knob is not None:
            env["MKP_STRAND_SLOTS"] = knob
        p = subprocess.run([str(exe), str(scn)], capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        out = {"ent": [], "rank": [], "work": [], "cover": [], "error": None, "lists": None}
        for ln in p.stdout.splitlines():
            w = ln.split()
            if w[0] == "error":
                out["error"] = " ".join(w[1:])
            elif w[0] == "lists":
                out["lists"] = tuple(int(x) for x in w[1:])
            else:
                out[w[0]].append(tuple(int(x) for x in w[1:]))
        return out
    return run


def check(out, win, focus, reads, knob_off=False):
    """everything the program printed against brute force; returns {read id: (list name, entries)}"""
    assert out["error"] is None, out["error"]
    assert all(win[0] <= p < win[1] for p, _ in focus) and [p for p, _ in focus] == sorted(set(p for p, _ in focus))
    slots = [(p, g, rule) for g, (p, rule) in enumerate(focus)]
    lists = {"all": [(p, g) for p, g, _ in slots], "plus": [(p, g) for p, g, r in slots if r & PLUS],
             "minus": [(p, g) for p, g, r in slots if r & MINUS]}
    n_all, n_plus, n_minus = len(lists["all"]), len(lists["plus"]), len(lists["minus"])
    assert out["lists"][:4] == (n_all, n_plus, n_minus, n_all + n_plus + n_minus)
    assert out["ent"] == lists["all"] + lists["plus"] + lists["minus"]
    # the rank arrays: entries of the strand list in front of global slot g, for g = 0 .. n_all
    assert out["rank"] == [(sum(1 for _, h, r in slots if h < g and r & PLUS), sum(1 for _, h, r in slots if h < g and r & MINUS))
                           for g in range(n_all + 1)]
    offset = {"all": 0, "plus": n_all, "minus": n_all + n_plus}
    fused = [i for i, rd in enumerate(reads) if rd[3] != T_NONE]
    assert sorted(w[0] for w in out["work"]) == fused and sorted(c[0] for c in out["cover"]) == [i for i in range(len(reads)) if i not in fused]
    cov_off, want_cov = 0, {}
    for i, (s, e, rev, tags) in enumerate(reads):
        n_sl = sum(1 for p, _, _ in slots if s <= p < e)
        want_cov[i] = cov_off
        cov_off += (n_sl + 3) // 4 * 4
    chosen, total_ent, total_sl = {}, 0, 0
    for rid, gs0, n_sl, cov, ent_off, n_ent in out["work"]:
        s, e, rev, tags = reads[rid]
        span = [(p, g, r) for p, g, r in slots if s <= p < e]
        assert gs0 == sum(1 for p, _, _ in slots if p < s) and n_sl == len(span) and cov == want_cov[rid], rid
        own = "minus" if rev else "plus"
        one_strand = tags == T_POS                       # sg0 = 0: calls and coverage on the alignment strand
        if not knob_off and one_strand and len(lists[own]) < n_all:
            name, want = own, [(p, g) for p, g, r in span if r & (MINUS if rev else PLUS)]
        else:
            name, want = "all", [(p, g) for p, g, _ in span]
        assert n_ent == len(want), (rid, name, n_ent, want)
        if want:   # (the offset of an empty run is not looked at)
            assert ent_off >= offset[name] and out["ent"][ent_off:ent_off + n_ent] == want, (rid, name, ent_off)
            assert ent_off + n_ent <= offset[name] + len(lists[name]), rid
        # every byte the read writes lies inside its own run of the stream
        assert all(0 <= g - gs0 < n_sl for _, g in want), rid
        chosen[rid] = (name, want)
        total_ent += n_ent
        total_sl += n_sl
    assert out["lists"][4:] == (total_ent, total_sl)
    counts = [w[5] for w in out["work"]]
    assert counts == sorted(counts, reverse=True), "launch order: by entry count, longest first"
    return chosen


WIN = (1000, 3000)


def alternating(lo, hi, step=10):
    """'+' at p, '-' at p + 1: the C and the G of a CpG"""
    return [x for p in range(lo, hi, step) for x in ((p, PLUS), (p + 1, MINUS))]


def test_alternating_rules(planner):
    focus = alternating(1100, 2900)
    reads = [
        (1050, 1500, FWD, T_POS), (1050, 1500, REV, T_POS),      # in front of the first slot to between two CpGs
        (1100, 1101, FWD, T_POS), (1100, 1101, REV, T_POS),      # one position: a '+' slot — a reverse read with a global slot and none of its own
        (1101, 1102, FWD, T_POS), (1101, 1102, REV, T_POS),      # one position: a '-' slot
        (1101, 1700, FWD, T_POS),                                # first global slot '-' (the other strand's), last '-'
        (1101, 1701, FWD, T_POS),                                # first '-', last '+'
        (1200, 1801, REV, T_POS),                                # first global slot '+' (the other strand's), last '+'
        (1200, 1802, REV, T_POS),                                # first '+', last '-'
        (1202, 1210, FWD, T_POS), (1202, 1210, REV, T_NEG),      # between two CpGs: no slot at all
        (1300, 2950, FWD, T_NEG), (1300, 2950, REV, T_NEG),      # sg0 = 1: both tally strands, the run of `all`
        (1400, 2000, FWD, T_NONE),                               # no tag: not a fused read
        (2891, 3100, FWD, T_POS), (2891, 3100, REV, T_POS),      # runs past the window: the last '-' slot only
    ]
    out = planner(WIN, focus, reads)
    chosen = check(out, WIN, focus, reads)
    assert chosen[3] == ("minus", []) and chosen[4] == ("plus", [])
    assert chosen[2][1] == [(1100, 0)] and chosen[5][1] == [(1101, 1)]
    assert chosen[6][0] == "plus" and len(chosen[6][1]) == 59 and chosen[7][1][-1][0] == 1700
    assert chosen[8][0] == "minus" and chosen[8][1][0][0] == 1201 and chosen[8][1][-1][0] == 1791 and chosen[9][1][-1][0] == 1801
    assert chosen[12][0] == chosen[13][0] == "all" and len(chosen[12][1]) == 2 * 160
    assert chosen[15] == ("plus", []) and chosen[16][1] == [(2891, 359)]
    # about half of the slots the one-strand reads span
    one = [i for i in chosen if reads[i][3] == T_POS]
    assert sum(len(chosen[i][1]) for i in one) * 2 <= sum(w[2] for w in out["work"] if w[0] in one) + len(one)


def test_every_position_with_both_rules(planner):
    """--include-bed without a strand: no list is shorter than `all`, every read stays on it"""
    focus = [(p, BOTH) for p in range(1100, 1400)]
    reads = [(1050, 1200, FWD, T_POS), (1100, 1400, REV, T_POS), (1150, 1151, FWD, T_POS), (1399, 1500, REV, T_NEG)]
    chosen = check(planner(WIN, focus, reads), WIN, focus, reads)
    assert all(name == "all" for name, _ in chosen.values())
    assert [len(chosen[i][1]) for i in range(4)] == [100, 300, 1, 1]


def test_window_without_a_minus_rule(planner):
    """only '+' rules: `plus` is as long as `all` (forward reads stay on `all`), `minus` is empty (reverse reads decode nothing)"""
    focus = [(p, PLUS) for p in range(1100, 1900, 7)]
    reads = [(1050, 1500, FWD, T_POS), (1050, 1500, REV, T_POS), (1100, 1900, REV, T_NEG), (1600, 2500, REV, T_POS)]
    out = planner(WIN, focus, reads)
    chosen = check(out, WIN, focus, reads)
    assert chosen[0][0] == "all" and len(chosen[0][1]) == len([p for p, _ in focus if p < 1500])
    assert chosen[1] == ("minus", []) and chosen[3] == ("minus", [])
    assert chosen[2][0] == "all" and len(chosen[2][1]) == len(focus)


def test_mixed_rules_and_a_mostly_plus_window(planner):
    """rules 1, 2 and 3 mixed: a slot with both rules is in both strand lists"""
    focus = [(p, (PLUS, MINUS, BOTH, PLUS, PLUS)[(p // 3) % 5]) for p in range(1002, 2998, 3)]
    reads = [(1000 + 37 * k, 1000 + 37 * k + 90 + 11 * (k % 7), k % 2, (T_POS, T_POS, T_NEG)[k % 3]) for k in range(50)]
    chosen = check(planner(WIN, focus, reads), WIN, focus, reads)
    assert {name for name, _ in chosen.values()} == {"all", "plus", "minus"}


def test_knob_sends_every_read_to_all(planner):
    focus = alternating(1100, 2900)
    reads = [(1050, 1500, FWD, T_POS), (1050, 1500, REV, T_POS), (1100, 1101, REV, T_POS), (1101, 1700, FWD, T_POS),
             (1300, 2950, REV, T_NEG)]
    chosen = check(planner(WIN, focus, reads, knob="0"), WIN, focus, reads, knob_off=True)
    assert all(name == "all" for name, _ in chosen.values())
    assert len(chosen[0][1]) == 80 and chosen[2][1] == [(1100, 0)]
    # any other value leaves the strand lists on
    chosen = check(planner(WIN, focus, reads, knob="1"), WIN, focus, reads)
    assert chosen[0][0] == "plus" and chosen[1][0] == "minus"
