"""The reads sampler's schedule (modkit_amd/csrc/mkp_sample_schedule.hpp) on the host: tests/sample_schedule_host.cpp is compiled with g++
(nothing but that header; with -fsanitize=address,undefined when g++'s sanitizer runtime is installed) and run on scenarios written by hand.
The expectations are worked out here from the definitions the header's comments quote (sampling_schedule.rs:171-273, 440-615,
interval_chunks.rs:563-643).

Quotas (from_num_reads).  A contig with c of the T counted reads gets min(ceil(N * c / T), c); T counts the unmapped reads only when they are
sampled, and then their share ceil(N * U / T) counts in the sum.  While sum / N > 1.5, contigs whose quota is at or under a floor (1, 2, ..)
are dropped in ascending tid until the sum is N or less.
  {0: 30}, N = 10                      ceil(10 * 30 / 30) = 10
  {0: 30}, N = 500                     ceil(500) = 500, capped by the count: 30
  {0: 1000, 1: 1, 2: 1, 3: 1}, N = 2   ceil(2 * 1000 / 1003) = 2 and three times ceil(2 / 1003) = 1: sum 5 > 1.5 * 2.  Floor 1: contig 0 (2)
                                       stays, contigs 1, 2, 3 go one by one, the sum 4, 3, 2 — reached N.  {0: 2}
  {0: 60, 1: 20}, U = 20, N = 10       with the unmapped reads T = 100: ceil(6.0) = 6, ceil(2.0) = 2 (and 2 for the unmapped: sum 10)
                                       without them T = 80: ceil(7.5) = 8, ceil(2.5) = 3; the sum 11 stays, 11 / 10 <= 1.5
  no reads                             refused: "zero reads found in bam index"
from_sample_frac: ceil(count * f) per contig, `all` at f = 1.

Super batches.  The targets are cut into intervals of the interval size; a feeder group collects intervals, across contigs, until it holds
an interval's worth of bases; a super batch is `batch size` groups (0 behaves as 1), its intervals by contig and start.
  [0, 2000), 500, batch 1              four groups of one interval: four batches
  [0, 2000), 500, batch 6              one batch of the four
  [0, 700) on 0, [0, 300) on 1, 500    (0, 0, 500) fills a group; (0, 500, 700) holds 200 bases, (1, 0, 300) brings them to 500
  a region [250, 1350), 500, batch 2   (250, 750) (750, 1250) | (1250, 1350)

Grouping (accumulate_sample_counts).  Per contig: left = ceil((batch length / contig size) * (quota - sampled so far)), nothing when the
quota is used up; per interval ceil(left * interval length / batch length of the contig); an interval under 50 reads is held back and
merged with the next one of its contig until the sum reaches 50, and flushed as it is when the contig changes or the batch ends.  Four
intervals of 500 on a contig of 2000:
  quota 400                            left 400, 100 each
  quota 100                            25 each: 25 + 25 = 50 -> [0, 1000) 50, [1000, 2000) 50
  quota 100, 60 sampled                left 40, 10 each: 10, 20, 30, 40 never reach 50 -> [0, 2000) 40 at the end of the batch
  quota 100, 100 sampled               nothing
  quota 300, 20 sampled                left 280, 70 each
  quota all                            the four intervals, each `all`
  quota 400, first two intervals only  left ceil(0.5 * 400) = 200, 100 each
  (0, 0, 100) quota 10 and (1, 0, 1000) quota 200, contig sizes 100 and 1000: 10 is held back, the contig changes -> (0, 0, 100) 10 then
  (1, 0, 1000) 200; a third contig without a quota is dropped

`extract calls --num-reads`: per interval ceil(contig quota * interval length / length of the whole super batch).  One contig [0, 2000),
quota 10, intervals of 500: one group per super batch -> ceil(10 * 500 / 500) = 10 each; all four in one -> ceil(10 * 500 / 2000) = 3 each;
a contig without a quota is marked -2 (never fetched).

Owner rank: the scheduled contigs laid end to end, an interval belongs to rank min(W - 1, midpoint * W / grid length)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def schedule(tmp_path_factory):
    d = tmp_path_factory.mktemp("sample_schedule_host")
    base = ["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "modkit_amd", "csrc")]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + ["-o", str(d / "probe"), str(probe)], capture_output=True).returncode != 0:
        san = []   # no sanitizer runtime on this machine: the same checks without it
    exe = d / "sample_schedule_host"
    subprocess.check_call(base + san + ["-o", str(exe), os.path.join(ROOT, "tests", "sample_schedule_host.cpp")])
    count = [0]

    def run(*words):
        count[0] += 1
        scn = d / ("scenario%d.txt" % count[0])
        scn.write_text(" ".join(str(w) for w in words) + "\n")
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith("MKP_")}
        p = subprocess.run([str(exe), str(scn)], capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        return [ln.split() for ln in p.stdout.splitlines()]
    return run


def flat(rows):
    return [len(rows)] + [x for r in rows for x in r]


def quotas(schedule, counts, n, unmapped=0, include_unmapped=False):
    out = schedule("quota", n, int(include_unmapped), unmapped, *flat(sorted(counts.items())))
    if out and out[0][0] == "error":
        return " ".join(out[0][1:])
    return {int(w[1]): (w[2] if w[2] == "all" else int(w[2])) for w in out}


def test_quotas_from_num_reads(schedule):
    assert quotas(schedule, {0: 30}, 10) == {0: 10}
    assert quotas(schedule, {0: 30}, 500) == {0: 30}
    assert quotas(schedule, {0: 1000, 1: 1, 2: 1, 3: 1}, 2) == {0: 2}
    assert quotas(schedule, {0: 60, 1: 20}, 10, unmapped=20, include_unmapped=True) == {0: 6, 1: 2}
    assert quotas(schedule, {0: 60, 1: 20}, 10, unmapped=20) == {0: 8, 1: 3}
    assert quotas(schedule, {}, 10) == "zero reads found in bam index"
    assert quotas(schedule, {0: 0}, 10, unmapped=5) == "zero reads found in bam index"   # unmapped reads that are not sampled do not count


def test_quotas_from_sample_frac(schedule):
    out = lambda f, counts: {int(w[1]): (w[2] if w[2] == "all" else int(w[2])) for w in schedule("frac", f, *flat(sorted(counts.items())))}
    assert out("1.0", {0: 30, 1: 0, 2: 7}) == {0: "all", 2: "all"}
    assert out("0.5", {0: 30, 2: 7}) == {0: 15, 2: 4}
    assert out("0.1", {0: 31}) == {0: 4}


def batches(schedule, contigs, interval, batch):
    out = {}
    for w in schedule("batches", interval, batch, *flat(contigs)):
        out.setdefault(int(w[1]), []).append(tuple(int(x) for x in w[2:]))
    assert sorted(out) == list(range(len(out)))
    return [out[k] for k in sorted(out)]


def test_super_batches(schedule):
    four = [(0, 0, 500), (0, 500, 1000), (0, 1000, 1500), (0, 1500, 2000)]
    assert batches(schedule, [(0, 0, 2000)], 500, 1) == [[iv] for iv in four]
    assert batches(schedule, [(0, 0, 2000)], 500, 6) == [four]
    across = [[(0, 0, 500)], [(0, 500, 700), (1, 0, 300)]]
    assert batches(schedule, [(0, 0, 700), (1, 0, 300)], 500, 1) == across
    assert batches(schedule, [(0, 0, 700), (1, 0, 300)], 500, 0) == across
    assert batches(schedule, [(0, 250, 1100)], 500, 2) == [[(0, 250, 750), (0, 750, 1250)], [(0, 1250, 1350)]]


FOUR = [(0, 0, 500), (0, 500, 1000), (0, 1000, 1500), (0, 1500, 2000)]


def grouped(schedule, ivs, sizes, quota, so_far=()):
    q = [(t, 1, 0) if n == "all" else (t, 0, n) for t, n in quota]
    out = schedule("group", *(flat(ivs) + flat(sizes) + flat(q) + flat(so_far)))
    return [(int(w[1]), int(w[2]), int(w[3]), w[4] if w[4] == "all" else int(w[4])) for w in out]


def test_grouping_of_a_super_batch(schedule):
    size = [(0, 2000)]
    assert grouped(schedule, FOUR, size, [(0, 400)]) == [iv + (100,) for iv in FOUR]
    assert grouped(schedule, FOUR, size, [(0, 100)]) == [(0, 0, 1000, 50), (0, 1000, 2000, 50)]
    assert grouped(schedule, FOUR, size, [(0, 100)], [(0, 60)]) == [(0, 0, 2000, 40)]
    assert grouped(schedule, FOUR, size, [(0, 100)], [(0, 100)]) == []
    assert grouped(schedule, FOUR, size, [(0, 300)], [(0, 20)]) == [iv + (70,) for iv in FOUR]
    assert grouped(schedule, FOUR, size, [(0, "all")]) == [iv + ("all",) for iv in FOUR]
    assert grouped(schedule, FOUR[:2], size, [(0, 400)]) == [iv + (100,) for iv in FOUR[:2]]


def test_slack_is_flushed_when_the_contig_changes(schedule):
    ivs = [(0, 0, 100), (1, 0, 1000), (2, 0, 700)]
    got = grouped(schedule, ivs, [(0, 100), (1, 1000), (2, 700)], [(0, 10), (1, 200)])
    assert got == [(0, 0, 100, 10), (1, 0, 1000, 200)]


def test_extract_interval_quotas(schedule):
    ivq = lambda batch, contigs, quota: [tuple(int(x) for x in w[1:]) for w in schedule("extract", 500, batch, *(flat(contigs) + flat(quota)))]
    assert ivq(1, [(0, 0, 2000)], [(0, 10)]) == [iv + (10,) for iv in FOUR]
    assert ivq(4, [(0, 0, 2000)], [(0, 10)]) == [iv + (3,) for iv in FOUR]
    got = ivq(1, [(0, 0, 1000), (1, 0, 500)], [(0, 10)])
    assert got == [(0, 0, 500, 10), (0, 500, 1000, 10), (1, 0, 500, -2)]


@pytest.mark.parametrize("world", [2, 3])
def test_owner_rank_of_a_sampling_interval(schedule, world):
    contigs = [(0, 0, 12000), (3, 100, 2900)]
    rows = [tuple(int(x) for x in w[1:]) for w in schedule("owner", world, 1000, *flat(contigs))]
    assert [r[:3] for r in rows] == [(0, s, s + 1000) for s in range(0, 12000, 1000)] + [(3, s, min(s + 1000, 3000)) for s in range(100, 3000, 1000)]
    owners = [r[3] for r in rows]
    assert all(0 <= o < world for o in owners)                 # exactly one owner each (the function names one rank) ...
    assert owners == sorted(owners)                            # ... in contiguous runs along the grid
    assert owners[0] == 0 and owners[-1] == world - 1 and set(owners) == set(range(world))
    # by the definition: the midpoint's place in the grid of 14900 bases
    grid, off = 14900, {0: 0, 3: 12000 - 100}
    assert owners == [min(world - 1, (off[t] + s + (e - s) // 2) * world // grid) for t, s, e in (r[:3] for r in rows)]
