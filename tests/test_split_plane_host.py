"""The planner's stage that lays the fused reads into the slot decoder's two planes and counts what a pass reads of them
(build_work_records and plane_lookup_bytes, modkit_amd/csrc/mkp_plan.hpp), on the host: tests/split_plane_host.cpp is compiled with g++
(no HIP header, no device; with -fsanitize=address,undefined when g++'s sanitizer runtime is installed) and run on read headers written by
hand.  The expectations are worked out here from the definitions.

The planes.  Per fused read and 32 stored bases one 8-byte entry in the call plane and one in the base plane behind it; a read's entries
start at the same index (MkpWork.pad) of either, reads in launch order: pad = the words of the reads before it, plane_bytes = 16 per word.

The algorithmic bytes of one pass.  A read decodes n_ent slots.  It gathers one 8-byte entry per slot from ONE plane (the call plane when
it has calls, the base plane otherwise): no more entries than it has, so 8 * min(words, n_ent).  A read with calls also asks the base
plane for 4 bytes under every match slot without a listed call.  At most n_calls slots carry a listed call, so a read whose slots are all
matches makes at least n_ent - n_calls requests (none when it has more calls than slots): the host's bound.  A read without calls — no
tags, a tag without calls, a tag error, a probability-sum error — reads no base dword beyond its gather."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_REVERSE, RF_BAD, RF_SUMERR, RF_CIGW = 1, 2, 4, 32


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("split_plane_host")
    base = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "modkit_amd", "csrc"),
            "-I", os.path.join(ROOT, "include")]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        san = []   # no sanitizer runtime on this machine: the same checks without it
    exe = d / "split_plane_host"
    subprocess.check_call(base + san + ["-o", str(exe), os.path.join(ROOT, "tests", "split_plane_host.cpp"), "-lz", "-lpthread"])
    count = [0]

    def run(reads, queries=()):
        count[0] += 1
        scn = d / ("scenario%d.txt" % count[0])
        words = [len(reads)] + [x for r in reads for x in r] + [len(queries)] + [x for q in queries for x in q]
        scn.write_text(" ".join(str(int(w)) for w in words) + "\n")
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("MKP_")}
        p = subprocess.run([str(exe), str(scn)], capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        out = {"work": [], "bound": [], "plan": None, "error": None}
        for ln in p.stdout.splitlines():
            w = ln.split()
            if w[0] == "plan":
                out["plan"] = dict(zip(w[1::2], (int(x) for x in w[2::2])))
            elif w[0] == "error":
                out["error"] = " ".join(w[1:])
            else:
                out[w[0]].append(tuple(int(x) for x in w[1:]))
        return out
    return run


def words(l_seq):
    return (l_seq + 31) // 32


def with_calls(flags, n_tags, calls0):
    return not (flags & RF_BAD) and n_tags != 0 and calls0 != 0 and not (flags & RF_SUMERR)


def lookup_bytes(l_seq, n_ent, calls, n_calls):
    return 8 * min(words(l_seq), n_ent) + (4 * max(n_ent - n_calls, 0) if calls else 0)


# (l_seq, n_ent, flags, n_tags, calls of tag 0, calls of tag 1, n_cigar)
READS = [
    (10000, 104, 0, 1, 110, 0, 600),            # more calls than slots: no base request counted
    (10000, 104, RF_REVERSE, 1, 96, 0, 600),    # 8 slots cannot be listed
    (9000, 90, 0, 2, 40, 40, 500),              # two tags share the delta list: the read's calls are tag 0's
    (5000, 50, 0, 0, 0, 0, 300),                # no tags: the base plane only
    (5000, 50, 0, 1, 0, 0, 300),                # a tag without calls
    (5000, 50, RF_BAD, 1, 30, 0, 300),          # a tag error
    (5000, 50, RF_SUMERR, 2, 30, 30, 300),      # a probability-sum error
    (33, 2, RF_CIGW, 1, 1, 0, 3),               # two words, two slots
    (32, 5, 0, 1, 2, 0, 1),                     # one word under five slots: one entry to gather
    (1, 1, 0, 1, 1, 0, 1),
    (0, 0, 0, 0, 0, 0, 0),                      # no SEQ, no slot: no word, nothing read
    (65, 1, RF_REVERSE, 0, 0, 0, 1),
]


def test_plane_layout_and_bytes_bound(planner):
    out = planner(READS)
    assert out["error"] is None
    pad, looked = 0, 0
    for k, (l_seq, n_ent, flags, n_tags, c0, c1, n_cigar) in enumerate(READS):
        n_calls = c0 if n_tags and not (flags & RF_BAD) else 0
        assert out["work"][k] == (k, pad, n_calls), k
        pad += words(l_seq)
        looked += lookup_bytes(l_seq, n_ent, with_calls(flags, n_tags, c0), c0)
    assert pad == sum(words(r[0]) for r in READS) and pad > 1000
    assert out["plan"]["plane_bytes"] == 16 * pad      # two planes of 8-byte entries, one behind the other
    assert out["plan"]["looked_up"] == looked
    assert out["plan"]["entries"] == sum(r[1] for r in READS)
    # by hand, the reads in turn: gather + base requests
    by_hand = [8 * 104 + 0, 8 * 104 + 4 * 8, 8 * 90 + 4 * 50, 8 * 50, 8 * 50, 8 * 50, 8 * 50, 8 * 2 + 4 * 1, 8 * 1 + 4 * 3, 8 * 1, 0, 8 * 1]
    assert looked == sum(by_hand)
    # never more per read than the one 16-byte entry per slot of the single plane, and half of it for a read without calls
    for (l_seq, n_ent, flags, n_tags, c0, c1, n_cigar), b in zip(READS, by_hand):
        assert b <= 16 * n_ent
        if not with_calls(flags, n_tags, c0):
            assert b == 8 * min(words(l_seq), n_ent)


def test_bound_is_below_what_any_placement_of_the_calls_requests(planner):
    """brute force: place a read's calls on stored bases at random (focus slots and other bases alike), count the match slots without a
    listed call — each is one 4-byte request — and compare with the host's count, which must never exceed it for a read of matches"""
    r = random.Random(77)
    queries, requests = [], []
    for _ in range(300):
        l_seq = r.choice([1, 31, 32, 33, 64, 65, 200, 3000])
        slots = sorted(r.sample(range(l_seq), r.randrange(0, min(l_seq, 120) + 1)))
        n_calls = r.randrange(0, l_seq + 1)
        calls = r.random() < 0.8 and n_calls > 0
        on_slots = r.random() < 0.5   # calls placed on the slots first (every call a focus position) or anywhere
        order = list(dict.fromkeys(slots + r.sample(range(l_seq), l_seq))) if on_slots else r.sample(range(l_seq), l_seq)
        listed = set(order[:n_calls])
        queries.append((l_seq, len(slots), int(calls), n_calls))
        requests.append(sum(1 for q in slots if q not in listed) if calls else 0)
    out = planner([], queries)
    assert len(out["bound"]) == len(queries)
    tight = 0
    for (l_seq, n_ent, calls, n_calls), req, (got,) in zip(queries, requests, out["bound"]):
        assert got == lookup_bytes(l_seq, n_ent, calls, n_calls)
        base = got - 8 * min(words(l_seq), n_ent)
        assert base <= 4 * req, (l_seq, n_ent, calls, n_calls, req)
        tight += calls and n_ent > 0 and base == 4 * req
    assert tight > 20   # the bound is met where every call sits on a slot
