"""The piece seams of the device bedMethyl reader, run as a program of its own by tests/test_gpu_bedmethyl_in.py with
MKP_BEDMETHYL_PIECE_KB=64 in a fresh process (a piece then holds 64 KiB of text, so a file of a few hundred KB has several seams):
lines that straddle the seams, a contig run that goes on over a seam and one that comes back in a later piece, the order check across a
seam, the longest line a piece holds and the first that it does not, BGZF pieces with empty blocks, and a bad line in a later piece named
as the host reader names it.  Prints `ok <checks>`; an assertion that fails ends it with a traceback."""
import os
import random
import sys
import tempfile

import modkit_amd
from bedmethyl_in_cases import BAD, INVALID, UNSUPPORTED, bgzf_bytes, line, model_runs, random_cuts, random_file, runs_as_records

P = 65536
assert os.environ.get("MKP_BEDMETHYL_PIECE_KB") == "64"
checks = 0


def write(d, name, data):
    path = os.path.join(d, name)
    with open(path, "wb") as f:
        f.write(data.encode() if isinstance(data, str) else data)
    return path


def same_as_host_and_model(ctx, path, text):
    global checks
    dev, host = ctx.read_bedmethyl_runs(path), modkit_amd.read_bedmethyl_runs(path)
    assert runs_as_records(dev) == runs_as_records(host) == model_runs(text), path
    checks += 1
    return dev


def refused(ctx, path, status, word=None, same_message_as_host=False):
    global checks
    try:
        ctx.read_bedmethyl_runs(path)
    except modkit_amd.MkpError as e:
        assert e.status == status and (word is None or word in str(e)), (path, str(e))
        if same_message_as_host:
            try:
                modkit_amd.read_bedmethyl_runs(path)
            except modkit_amd.MkpError as h:
                assert (h.status, str(h)) == (e.status, str(e)), (str(h), str(e))
            else:
                raise AssertionError("the host reader takes " + path)
        checks += 1
        return str(e)
    raise AssertionError("the device reader takes " + path)


def sized_line(n_bytes, start, chrom="c", **kw):
    """a data line of exactly n_bytes ('\\n' included), sized by its chrom name"""
    base = line(chrom, start, "m", "+", [3, 1, 1, 1, 0, 0, 0, 0], **kw)
    out = line(chrom + "x" * (n_bytes - len(base)), start, "m", "+", [3, 1, 1, 1, 0, 0, 0, 0], **kw)
    assert len(out) == n_bytes
    return out


def main():
    global checks
    r = random.Random(99)
    ctx = modkit_amd.Context()
    with tempfile.TemporaryDirectory() as d:
        # 1. four pieces, lines of varying length: both inner seams fall inside a line; chrA goes on over the first seam, chrB over the second,
        #    chrA comes back behind it
        lines, n = [], 0
        for chrom, until in (("chrA", P + P // 2), ("chrB", 2 * P + P // 3), ("chrA", 3 * P + 999)):
            pos = 10
            while n < until:
                pos += r.randrange(0, 40)
                l = line(chrom, pos, r.choice(["m", "h", "21839", "m,CG,0"]), r.choice("+-."), [r.randrange(2**24) for _ in range(8)],   # (rows that share a key are summed below)
                         sep=r.choice(["\t", " ", "\t "]))
                lines.append(l); n += len(l)
        text = "".join(lines)
        for seam in (P, 2 * P, 3 * P):
            assert text[seam - 1] != "\n" and text[seam] != "\n"
        dev = same_as_host_and_model(ctx, write(d, "four_pieces.bed", text), text)
        assert [c for c, _ in dev] == ["chrA", "chrB", "chrA"]          # a run cut by a seam comes back as ONE run
        same_as_host_and_model(ctx, write(d, "four_pieces.bed.gz", bgzf_bytes(text, random_cuts(r, len(text)))), text)
        # BGZF whose blocks end exactly on a piece's end, with empty blocks between the pieces, and without the EOF block
        same_as_host_and_model(ctx, write(d, "cuts_on_pieces.bed.gz", bgzf_bytes(text, (P, P, 2 * P, 2 * P + 1, 3 * P, 3 * P), eof=False)), text)
        # the join takes the runs of every piece
        ctx.merge_begin([2**31, 2**31])
        assert ctx.merge_add_file(write(d, "again.bed", text), ["chrA", "chrB"]) == len(lines)
        merged = {tid: ctx.merge_get(tid)[0] for tid in (0, 1)}
        assert sum(len(m["pos"]) for m in merged.values()) == len({(l.split()[0], l.split()[1], l.split()[3].split(",")[0], l.split()[5]) for l in lines})
        checks += 1

        # 2. lines of 64 bytes: every seam falls between two lines, nothing is carried; the order check still sees the row in front
        rows = [sized_line(64, 5 * k) for k in range(3 * P // 64 + 10)]
        text = "".join(rows)
        n_runs = len(same_as_host_and_model(ctx, write(d, "aligned.bed", text), text))   # (the chrom sizes the line: a run per digit count)
        k = P // 64                                                         # the first line of the second piece
        rows[k] = sized_line(64, 5 * k - 6)
        msg = refused(ctx, write(d, "descends_at_seam.bed", "".join(rows)), INVALID, "ascending")
        assert "line %d of " % (k + 1) in msg
        rows[k] = sized_line(64, 5 * k)
        rows[k + 7] = sized_line(64, 5 * k - 100)                           # (as many digits: the chrom, which sizes the line, stays the same)
        msg = refused(ctx, write(d, "descends_inside.bed", "".join(rows)), INVALID, "ascending")
        assert "line %d of " % (k + 8) in msg
        rows[k + 7] = sized_line(64, 3, chrom="d")                          # another contig between: two new runs, nothing descends
        text = "".join(rows)
        dev = same_as_host_and_model(ctx, write(d, "other_contig.bed", text), text)
        assert len(dev) == n_runs + 2

        # 3. the longest line a piece holds has P - 1 bytes in front of its '\n'
        head, tail = sized_line(100, 1), sized_line(100, 9)
        for name, n_bytes, ok in (("fits", P, True), ("too_long", P + 1, False), ("line_of_70000", 70001, False)):
            text = head + sized_line(n_bytes, 5) + tail
            for path in (write(d, name + ".bed", text), write(d, name + ".bed.gz", bgzf_bytes(text, random_cuts(r, len(text))))):
                if ok:
                    same_as_host_and_model(ctx, path, text)
                else:
                    assert "line 2 of " in refused(ctx, path, UNSUPPORTED, "MKP_BEDMETHYL_PIECE_KB")
        text = sized_line(P + 1, 5)[:-1]                                    # ... also when it is the last line and has no '\n'
        refused(ctx, write(d, "last_line_too_long.bed", text), UNSUPPORTED, "MKP_BEDMETHYL_PIECE_KB")
        text = sized_line(P, 5)[:-1]
        same_as_host_and_model(ctx, write(d, "last_line_fits.bed", text), text)

        # 4. a bad line in the third piece is named as the host reader names it
        good = "".join(sized_line(61 + k % 7, 3 * k) for k in range(2 * P // 60 + 50))
        for k, case in enumerate(sorted(BAD)):
            bad_text, status, _ = BAD[case]
            text = good + bad_text + sized_line(100, 10**9)
            path = write(d, case + ".bed", text) if k % 2 else write(d, case + ".bed.gz", bgzf_bytes(text, random_cuts(r, len(text))))
            msg = refused(ctx, path, status, same_message_as_host=True)
            assert "line %d of %s" % (good.count("\n") + 1, path) in msg, msg

        # 5. seeded files of a few pieces, plain and BGZF
        for k in range(4):
            text = random_file(r, n_lines=r.randrange(1500, 2500))
            data = text if k % 2 else bgzf_bytes(text, random_cuts(r, len(text)), eof=bool(k & 2))
            same_as_host_and_model(ctx, write(d, "seeded%d.bed" % k, data), text)
    ctx.close()
    print("ok %d" % checks)


if __name__ == "__main__":
    sys.exit(main())
