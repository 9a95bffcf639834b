#!/usr/bin/env python3
"""A seeded bedMethyl table of a chosen size, for measuring the readers of `bedmethyl merge` (profiles/bedmethyl_in.txt).

    gen_bedmethyl.py --mb 210 --seed 7 out.bed            # plain text, tab separated, as `mkpileup pileup` writes it
    gen_bedmethyl.py --mb 210 --seed 7 --bgzf out.bed.gz  # the same text in BGZF blocks of 65 280 bytes, with the EOF block (no index)

One contig (`--chrom`, default chr20), ascending positions a few bases apart, an `h` and an `m` line per position on one strand, counts
of a ~30x run.  The same seed and size give the same bytes in both forms."""
import argparse
import random
import struct
import zlib


def lines(seed, n_bytes, chrom):
    r = random.Random(seed)
    pos, made = 60000, 0
    while made < n_bytes:
        pos += r.randrange(1, 80)
        strand = "+-"[r.randrange(2)]
        cov = r.randrange(18, 42)
        h = r.randrange(0, 4)
        m = r.randrange(0, cov - h + 1)
        rest = "\t%d\t%d\t%d\t%d" % (r.randrange(3), r.randrange(4), r.randrange(2), r.randrange(3))
        head = "%s\t%d\t%d\t" % (chrom, pos, pos + 1)
        mid = "\t%d\t%s\t%d\t%d\t255,0,0\t%d\t" % (cov, strand, pos, pos + 1, cov)
        out = (head + "h" + mid + "%.2f\t%d\t%d\t%d" % (100.0 * h / cov, h, cov - h - m, m) + rest + "\n"
               + head + "m" + mid + "%.2f\t%d\t%d\t%d" % (100.0 * m / cov, m, cov - h - m, h) + rest + "\n")
        made += len(out)
        yield out


def bgzf_block(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = co.compress(data) + co.flush()
    head = b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(payload) + 25)
    return head + payload + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out")
    ap.add_argument("--mb", type=float, default=210.0, help="least size of the text in MB (10^6 bytes)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--chrom", default="chr20")
    ap.add_argument("--bgzf", action="store_true")
    ap.add_argument("--level", type=int, default=4, help="deflate level of --bgzf")
    a = ap.parse_args()
    n_lines = n_text = 0
    with open(a.out, "wb") as f:
        pending = []
        size = 0
        for l in lines(a.seed, int(a.mb * 1e6), a.chrom):
            pending.append(l); size += len(l); n_lines += 2
            if size >= 1 << 22:
                data = "".join(pending).encode(); pending, size = [], 0
                n_text += len(data)
                if a.bgzf:
                    # (blocks are cut where the bytes fall, also inside a line, as bgzip cuts them)
                    keep = len(data) % 65280
                    for o in range(0, len(data) - keep, 65280):
                        f.write(bgzf_block(data[o:o + 65280], a.level))
                    pending, size = [data[len(data) - keep:].decode()], keep
                    n_text -= keep
                else:
                    f.write(data)
        data = "".join(pending).encode()
        n_text += len(data)
        if a.bgzf:
            for o in range(0, len(data), 65280):
                f.write(bgzf_block(data[o:o + 65280], a.level))
            f.write(bgzf_block(b"", a.level))
        else:
            f.write(data)
    print("%s: %d lines, %d bytes of text" % (a.out, n_lines, n_text))


if __name__ == "__main__":
    main()
