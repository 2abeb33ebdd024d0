"""BGZF output (ntc_bgzf_compress, `decode --bgzf`): a model of the member plan in Python integers,
a parser of BGZF members, and the texts the tests share.  Nothing here calls the library's plan:
the model restates the rule of DESIGN.md section 28 from its wording."""
import bisect
import functools
import gzip
import struct
import zlib

import numpy as np

M = 65280  # text bytes per member at most
G = 61440  # grid step of the record-aligned cuts
HALF = 32768  # a member's first chunk
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_MEMBER = M + 36


def plan(n, off=None):
    """[(text offset, text bytes)] of the members of an n-byte text; off: the record offsets"""
    if off is None:
        cuts = [min(j * M, n) for j in range(-(-n // M) + 1)]
    else:
        off = [int(o) for o in off]
        assert off[0] == 0 and off[-1] == n and all(a <= b for a, b in zip(off, off[1:]))
        cuts = [off[bisect.bisect_right(off, j * G) - 1] for j in range(-(-n // G) + 1)]
        assert cuts[0] == 0 and cuts[-1] == n
    members = []
    for a, b in zip(cuts, cuts[1:]):
        while a < b:
            members.append((a, min(M, b - a)))
            a += members[-1][1]
    return members


def chunks(length):
    """the chunks of a member of `length` bytes: (offset in the member, bytes, last)"""
    out = [(0, min(length, HALF), length <= HALF)]
    if length > HALF:
        out.append((HALF, length - HALF, True))
    return out


def bound(n):
    return n + 36 * (-(-n // G) + n // M)


def parse(blob):
    """the BGZF members blob consists of -> [(place, bytes, crc, isize)]; every header byte and
    BSIZE are checked, and nothing may be left over"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 16] == HEADER, at
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        assert 26 <= size <= MAX_MEMBER and at + size <= len(blob), (at, size)
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        out.append((at, size, crc, isize))
        at += size
    return out


def check(blob, table, text, off=None):
    """blob and the library's member table against the model, the parser, zlib and gzip"""
    want = plan(len(text), off)
    assert [(int(t["text_off"]), int(t["text_bytes"])) for t in table] == want
    members = parse(blob)
    assert [(p, b) for p, b, _, _ in members] == [(int(t["place"]), int(t["bytes"])) for t in table]
    for (p, b, crc, isize), (a, length) in zip(members, want):
        piece = text[a:a + length]
        assert isize == length and crc == zlib.crc32(piece)
        assert b <= length + 36
        assert zlib.decompress(blob[p + 18:p + b - 8], -15) == piece
    assert len(blob) <= bound(len(text))
    if blob:
        assert gzip.decompress(blob) == text
    assert gzip.decompress(blob + EOF) == text
    return members


# ---- texts ------------------------------------------------------------------------------------------
def fasta_records(n, seed, lo=40, hi=120, first=1):
    rng = np.random.default_rng(seed)
    return [b">seq.%d\n" % (first + i) + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(ln))) + b"\n"
            for i, ln in enumerate(rng.integers(lo, hi + 1, n))]


def fastq_records(n, seed, lo=40, hi=120):
    rng = np.random.default_rng(seed)
    out = []
    for i, ln in enumerate(rng.integers(lo, hi + 1, n)):
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(ln)))
        qual = bytes(rng.choice(np.frombuffer(b"FFFFF:,#", np.uint8), int(ln)))
        out.append(b"@read%d/1\n" % i + seq + b"\n+\n" + qual + b"\n")
    return out


def offsets(records):
    return np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)


def filler(n, seed=5):
    """n bytes of FASTA-like text"""
    t = b"".join(fasta_records(n // 60 + 2, seed))
    return t[:n]


def fixed(total, size=60):
    """records of `size` bytes (the last shorter) that fill exactly `total` bytes"""
    return [b"%-*d\n" % (min(size, total - a) - 1, a) if min(size, total - a) > 1 else b"\n" * min(size, total - a)
            for a in range(0, total, size)]


def over_grid_point(reclen):
    """short records up to G - reclen + 1, one record of reclen bytes over the grid point G (it
    ends at G + 1), short records up to exactly 2 G, and a tail: cell 1 is G + reclen - 1 bytes"""
    recs = fixed(G - reclen + 1) + [b"L" * (reclen - 1) + b"\n"] + fixed(G - 1) + fixed(1000)
    assert sum(len(r) for r in recs) == 2 * G + 1000
    return recs


@functools.lru_cache(maxsize=None)
def shapes():
    """{name: (text, offsets or None)}: the edge shapes of the plan and the contents of the coder"""
    rng = np.random.default_rng(28)
    s = {}
    for n in (0, 1, 32768, 32769, 65280, 65281, 130560):
        s["plain%d" % n] = (filler(n), None)
    s["R0"] = (b"", np.zeros(1, np.uint64))
    s["R1"] = (filler(100), np.array([0, 100], np.uint64))

    def with_records(name, recs):
        s[name] = (b"".join(recs), offsets(recs))

    with_records("ends_on_grid", fixed(G))  # the last record ends exactly on the grid point, none starts there
    with_records("starts_on_grid", fixed(2 * G) + fixed(500))  # boundaries exactly on G and 2 G, records start there
    with_records("over3841", over_grid_point(3841))
    with_records("over3842", over_grid_point(3842))
    with_records("one140000", [filler(140000, 6)])
    with_records("long_between", fasta_records(300, 7) + [filler(140000, 8)] + fasta_records(300, 9))
    zl = fixed(G - 30) + [b""] * 5 + fixed(60) + [b""] * 3 + fixed(3000)
    assert sum(len(r) for r in zl[:len(fixed(G - 30)) + 5]) < G < sum(len(r) for r in zl)
    with_records("zero_runs", [b""] * 4 + zl + [b""] * 6)
    with_records("zero_on_grid", fixed(G) + [b""] * 3 + fixed(G // 2))  # a run of empty records exactly on the grid point
    with_records("fasta", fasta_records(3000, 10))
    with_records("fastq", fastq_records(1500, 11))
    s["one_byte"] = (b"A" * 100000, None)
    s["random"] = (bytes(rng.integers(0, 256, 150000, dtype=np.uint8)), None)
    s["largest"] = (bytes(rng.integers(0, 256, 0xFF00, dtype=np.uint8)), None)
    return s


def many_members(n_members, with_offsets=True):
    """a periodic text (cheap for the one-lane host coder) of n_members members"""
    if with_offsets:
        recs = fixed(n_members * G - 100, 64)
        return b"".join(recs), offsets(recs)
    return (b"ACGTTGCAAGGCTTAC" * (n_members * M // 16 + 1))[:n_members * M - 7], None
