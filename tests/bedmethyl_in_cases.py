"""What the tests of the bedMethyl readers share (tests/test_bedmethyl_line_host.py on the CPU, tests/test_gpu_bedmethyl_in.py on the
device): the READER and BAD texts of tests/test_bedmethyl_merge_host.py (copied: that file stays as it is), a BGZF writer whose block
cuts the caller chooses, the model's view of a text, and seeded generators of lines and files.  Nothing here imports the library."""
import os
import random
import struct
import zlib

import bedmethyl_merge_model as model

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modkit_fixtures")
LUNG = [os.path.join(FIX, "lung_00733-m_%s_5mc-5hmc_chr20_cpg_pileup.bed.gz" % t) for t in ("adjacent-normal", "primary-tumour")]
CHR20_LENGTH = 64444167   # GRCh38_chr20.fa.fai
IO, UNSUPPORTED, INVALID, DEVICE = -2, -3, -1, -4
# the status classes of mkp_bedmethyl_parse_line (modkit_amd/csrc/mkp_bedmethyl_line.hpp)
FEW_FIELDS, NOT_NUMBER, BEYOND_32, BAD_CODE, BAD_STRAND = 1, 2, 3, 4, 5
NUMERIC_FIELDS = [2, 3, 5, 7, 8, 10, 12, 13, 14, 15, 16, 17, 18]


def line(chrom, start, name, strand, counts, sep="\t", tail_sep=None):
    """one bedMethyl line; counts = [valid, mod, canonical, other, delete, fail, diff, nocall]"""
    tail_sep = sep if tail_sep is None else tail_sep
    head = sep.join([chrom, str(start), str(start + 1), name, str(counts[0]), strand, str(start), str(start + 1), "255,0,0"])
    return head + sep + tail_sep.join([str(counts[0]), "12.50"] + [str(c) for c in counts[1:]]) + "\n"


READER = {
    "tabs": line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7]) + line("c1", 5, "h", "-", [8, 7, 6, 5, 4, 3, 2, 1]),
    "mixed_delim": line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7], tail_sep=" ") + line("c1", 6, "a", ".", [1, 1, 0, 0, 0, 0, 0, 0], sep=" "),
    "chebi_and_motif_names": line("c1", 5, "21839", "+", [9, 1, 2, 3, 4, 5, 6, 7]) + line("c1", 5, "m,CG,0", "+", [3, 1, 1, 1, 0, 0, 0, 0])
                             + line("c1", 5, "m,CGCG,2", "+", [3, 1, 1, 1, 0, 0, 0, 0]) + line("c1", 9, "76792,A,0", "-", [2, 2, 0, 0, 0, 0, 0, 0]),
    "comment_lines": "#chrom\tstart\n" + line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7]) + "# a note\n" + line("c2", 1, "m", "-", [1, 0, 1, 0, 0, 0, 0, 0]),
    "contig_runs": line("c1", 5, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0]) + line("c2", 1, "m", "+", [2, 1, 0, 0, 0, 0, 0, 0])
                   + line("c2", 4, "m", "+", [3, 1, 0, 0, 0, 0, 0, 0]) + line("c1", 2, "m", "+", [4, 1, 0, 0, 0, 0, 0, 0]),
    "no_final_newline_crlf": line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7]).replace("\n", "\r\n") + line("c1", 6, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0])[:-1],
    "large_counts": line("c1", 4000000000, "m", "+", [4294967295, 4294967295, 0, 0, 0, 0, 0, 4294967295]),
    "the_score_is_the_coverage": "c1\t5\t6\tm\t9\t+\t5\t6\t255,0,0\t77\t1.00\t1\t2\t3\t4\t5\t6\t7\n",
    "empty": "",
}

# text, status, (status class, field) of the line function
BAD = {
    "too_few_fields": ("c1\t5\t6\tm\t9\t+\t5\t6\t255,0,0\t9\t1.00\t1\t2\t3\t4\t5\t6\n", IO, (FEW_FIELDS, 17)),
    "count_not_a_number": (line("c1", 5, "m", "+", [9, 1, 2, 3, 4, 5, 6, 7]).replace("\t7\n", "\tx\n"), IO, (NOT_NUMBER, 18)),
    "bad_strand": (line("c1", 5, "m", "*", [9, 1, 2, 3, 4, 5, 6, 7]), IO, (BAD_STRAND, 6)),
    "bad_code": (line("c1", 5, "mh", "+", [9, 1, 2, 3, 4, 5, 6, 7]), IO, (BAD_CODE, 4)),
    "blank_line_between": ("\n" + line("c1", 6, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0]), IO, (FEW_FIELDS, 0)),
    "count_beyond_32_bits": (line("c1", 5, "m", "+", [4294967296, 1, 0, 0, 0, 0, 0, 0]), UNSUPPORTED, (BEYOND_32, 5)),
}
BAD_PREFIX = line("c1", 1, "m", "+", [1, 1, 0, 0, 0, 0, 0, 0]) + "# skipped, still counted as a line\n"   # the bad line is line 3


def model_runs(text):
    """[(chrom, [(start, code text, strand, [8 counts]), ...]), ...]: the runs of lines on one contig, by the model's parse_line"""
    out = []
    lines = text.split("\n")
    if lines[-1] == "":
        lines.pop()   # (behind the last '\n' there is no line)
    for l in lines:
        if l.startswith("#"):
            continue
        chrom, start, code, strand, counts = model.parse_line(l)
        if not out or out[-1][0] != chrom:
            out.append((chrom, []))
        out[-1][1].append((start, code, strand, counts))
    return out


def runs_as_records(runs):
    return [(chrom, model.records_of_rows(rows)) for chrom, rows in runs]


def bgzf_block(data, level=6):
    """one BGZF block (SAM spec 4.1) holding `data` (at most 64 KiB; may be empty)"""
    assert len(data) <= 65536
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = co.compress(data) + co.flush()
    bsize = len(payload) + 25   # 18 bytes of header + payload + CRC32 + ISIZE, minus 1
    assert bsize < 65536
    head = b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize)
    return head + payload + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def bgzf_bytes(data, cuts=(), eof=True):
    """`data` as BGZF: a block boundary at every offset of `cuts` (an offset given twice, or one at either end, makes an empty block
    there); eof: the empty EOF block at the end"""
    if isinstance(data, str):
        data = data.encode()
    edges = [0] + sorted(min(max(int(c), 0), len(data)) for c in cuts) + [len(data)]
    blocks = [bgzf_block(data[a:b]) for a, b in zip(edges, edges[1:])] if data or cuts else []
    return b"".join(blocks) + (bgzf_block(b"") if eof else b"")


def random_cuts(r, n, most=6):
    """block cuts of n bytes of text: a few random offsets, no block beyond 60 000 bytes"""
    cuts = set(r.randrange(0, n + 1) for _ in range(r.randrange(0, most + 1))) if n else set()
    edges = sorted(cuts | {0, n})
    for a, b in zip(edges, edges[1:]):
        cuts.update(range(a + 60000, b, 60000))
    return sorted(cuts)


# ---- seeded lines: valid, or with exactly one defect
def _sep(r):
    return "".join(r.choice("\t ") for _ in range(r.choice([1, 1, 1, 2, 3])))


def _code(r):
    k = r.randrange(4)
    if k == 0:
        return r.choice("mhacfgeboZ1907")                  # one character, a digit included
    if k == 1:
        return str(r.choice([10, 21839, 76792, 2**31 - 1, r.randrange(10, 2**31)]))   # a ChEBI number (two or more digits)
    if k == 2:
        return r.choice("mha") + "," + r.choice(["CG", "CGCG", "A"]) + "," + str(r.randrange(3))
    return str(r.randrange(10, 99999)) + ",A,0"


def _count(r):
    return r.choice([0, 1, 9, 10, 255, 65535, 65536, 2**31, 2**32 - 1, r.randrange(2**32), r.randrange(1000)])


def random_fields(r, chrom=None, start=None):
    """the 18 (or more) fields of a valid line, as strings"""
    start = _count(r) if start is None else start
    f = [chrom or r.choice(["chr1", "c", "chr20_random", "7", "scaffold.1|x"]), str(start), str(_count(r)), _code(r), str(_count(r)), r.choice("+-."),
         str(_count(r)), str(_count(r)), r.choice(["255,0,0", "0", "x"]), str(_count(r)), r.choice(["12.50", "NaN", "inf", "0.00"])]
    f += [str(_count(r)) for _ in range(7)]
    f += ["extra%d" % k for k in range(r.choice([0, 0, 0, 1, 3]))]
    return f


def join_fields(r, f):
    text = _sep(r) if r.random() < 0.1 else ""          # separators in front of the chrom are skipped
    for k, x in enumerate(f):
        text += (_sep(r) if k else "") + x
    if r.random() < 0.1:
        text += _sep(r)
    return text + ("\r" if r.random() < 0.2 else "")


def random_line(r):
    """(the line without '\\n', None) for a valid line, or (the line, (status class, field)) with exactly one defect"""
    f = random_fields(r)
    if r.random() < 0.5:
        return join_fields(r, f), None
    kind = r.randrange(5)
    if kind == 0:
        k = r.randrange(0, 18)
        return join_fields(r, f[:k]), (FEW_FIELDS, k)
    if kind == 1:
        k = r.choice(NUMERIC_FIELDS)
        v = f[k - 1]
        f[k - 1] = r.choice([v + "x", "x" + v, "-" + v, "+" + v, v[:1] + "." + v[1:], "1e3", "0x10"])
        return join_fields(r, f), (NOT_NUMBER, k)
    if kind == 2:
        k = r.choice(NUMERIC_FIELDS)
        f[k - 1] = str(r.choice([2**32, 2**32 + 1, 10**10, 2**64 - 1, 2**64, 10**30]))
        return join_fields(r, f), (BEYOND_32, k)
    if kind == 3:
        f[3] = r.choice(["mh", "mh,CG,0", ",CG,0", str(2**31), "99999999999", "1x", "x1", "-5", str(2**31) + ",A,0"])
        return join_fields(r, f), (BAD_CODE, 4)
    f[5] = r.choice(["*", "++", "+-", "plus", "0", "+."])
    return join_fields(r, f), (BAD_STRAND, 6)


def random_file(r, n_lines=None):
    """a valid bedMethyl text: 1-4 contigs in runs (a contig may come back), positions ascending inside a run, 1-3 codes, the three
    strands, counts up to 2^32 - 1, random delimiters, '#' lines here and there, the final newline sometimes missing"""
    contigs = ["chr%d" % k for k in range(1, r.randrange(1, 5) + 1)]
    codes = r.sample(["m", "h", "a", "21839", "m,CG,0", "76792,A,0"], r.randrange(1, 4))
    n_lines = r.randrange(1, 400) if n_lines is None else n_lines
    out, chrom, pos = [], r.choice(contigs), r.randrange(1000)
    for _ in range(n_lines):
        if r.random() < 0.03:
            other = r.choice(contigs)
            if other != chrom:
                chrom, pos = other, r.randrange(1000)
        if r.random() < 0.02:
            out.append("#" + "x" * r.randrange(0, 40))
        pos += r.choice([0, 0, 1, 1, 2, 50, r.randrange(10**6)])
        pos = min(pos, 2**32 - 1)
        f = random_fields(r, chrom, pos)
        f[3], f[5] = r.choice(codes), r.choice("+-.")
        out.append(join_fields(r, f))
    return "\n".join(out) + ("\n" if r.random() < 0.8 else "")
