"""The checker for quality smoothing inside long reference matches, in numpy and independent of
the C++ (qsmooth_core.h, quality.hip): the rule by its definition.

A read of n bases has its records in archive order, rightmost first, with lengths L_0 .. L_{m-1}
summing to n.  Record j covers positions [e_j - L_j, e_j), e_0 = n, e_{j+1} = e_j - L_j.  A record
is long when flag bit 1 of its byte 7 is clear.  Position i is trusted iff it lies in a long
record with L_j >= M.  With tab the mode's table, q the byte after the table, floor = tab['#']
and target = tab[T]: a trusted q > floor becomes target, every other byte stays.

The records come from the CPU oracle (OracleIndex.encode), never from the code under test; the
expected sections are qual_lib's / qrans_lib's over the smoothed text."""
import numpy as np

import qual_lib as ql


def rec_lengths(recs):
    recs = np.asarray(recs, dtype=np.uint64)
    flags = (recs >> np.uint64(56)).astype(np.int64)
    long_len = ((recs >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.int64)
    short = (flags & 2) != 0
    return np.where(short, flags >> 2, long_len), ~short


def trusted_of_read(n, recs, M):
    """-> bool[n]: the trusted positions of one read from its records (archive order)."""
    lens, is_long = rec_lengths(recs)
    assert int(lens.sum()) == n, (int(lens.sum()), n)
    t = np.zeros(n, dtype=bool)
    e = n
    for L, lg in zip(lens.tolist(), is_long.tolist()):
        if lg and L >= M:
            t[e - L:e] = True
        e -= L
    return t


def trusted(offs, recs, roff, M):
    """-> bool[total]: the trusted positions of a batch (offs: base offsets, roff: record offsets)."""
    offs = np.asarray(offs, dtype=np.int64)
    roff = np.asarray(roff, dtype=np.int64)
    out = np.zeros(int(offs[-1] - offs[0]), dtype=bool)
    for r in range(len(offs) - 1):
        a, b = int(offs[r] - offs[0]), int(offs[r + 1] - offs[0])
        out[a:b] = trusted_of_read(b - a, recs[roff[r]:roff[r + 1]], M)
    return out


def floor_target(mode, to=b"I"):
    tab = ql.mode_table(mode)
    return int(tab[ord("#")]), int(tab[to[0] if isinstance(to, (bytes, bytearray)) else int(to)])


def smooth(q, mask, mode, to=b"I"):
    """q: the bytes after the mode's table; mask: the trusted positions -> (q', bytes replaced)."""
    floor, target = floor_target(mode, to)
    assert target > floor
    hit = np.asarray(mask, dtype=bool) & (np.asarray(q) > floor)
    out = np.array(q, dtype=np.uint8, copy=True)
    out[hit] = target
    return out, int(hit.sum())


def oracle_records(oracle, reads):
    """reads: list of bytes over ACGT -> (recs, roff, offs) from the CPU oracle."""
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    bases = np.frombuffer(b"".join(reads) or b"\0", dtype=np.uint8)[:int(offs[-1])]
    recs, roff = oracle.encode(bases, offs)
    return recs, roff, offs


def smoothed(oracle, reads, quals, M, mode="keep", to=b"I"):
    """reads (as the encoder sees them: masked where they held other symbols), quals: lists of
    bytes -> (the smoothed quality lines, bytes replaced, the trusted mask of the batch).  The
    lines are the mode's images, on which the table is the identity."""
    recs, roff, offs = oracle_records(oracle, reads)
    mask = trusted(offs, recs, roff, M)
    q = ql.mode_table(mode)[np.frombuffer(b"".join(quals), dtype=np.uint8)]
    assert q.all()
    out, count = smooth(q, mask, mode, to)
    o = offs.astype(np.int64)
    return [out[o[r]:o[r + 1]].tobytes() for r in range(len(reads))], count, mask


def fastq_text(reads, lines, first_id=1):
    """The text a decode with the smoothed sections prints (lines: smoothed())."""
    return ql.fastq_text(list(zip(reads, lines)), first_id, "keep")
