"""The checker of the non-ACGT tests (test_nonacgt.py, test_gpu_nonacgt.py): numpy only,
independent of the code under test.  mask() replaces every byte that is not A/C/G/T by the
substitute base; runs_of() lists the canonical exception runs -- maximal stretches of one
identical non-ACGT symbol inside one read, in (read, pos) order.  Plus the batches both test
files share."""
import numpy as np

SYMS = list(b"N-BDHVRYSWKM")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NX_RUN = np.dtype([("read", "<u8"), ("pos", "<u4"), ("len", "<u4"), ("sym", "<u4"), ("reserved", "<u4")])


def nonacgt(bases):
    return ~np.isin(bases, ACGT)


def mask(bases, sub):
    out = np.array(bases, dtype=np.uint8, copy=True)
    out[nonacgt(out)] = ord(sub) if isinstance(sub, str) else int(sub)
    return out


def runs_of(bases, offs):
    offs = np.asarray(offs, dtype=np.int64)
    B = np.asarray(bases, dtype=np.uint8)[offs[0]:offs[-1]]
    rel = offs - offs[0]
    n = len(B)
    m = nonacgt(B)
    read = np.searchsorted(rel, np.arange(n), side="right") - 1  # the read each position lies in
    first = np.ones(n, dtype=bool)  # differs from the position before, or starts a read
    first[1:] = (B[1:] != B[:-1]) | (read[1:] != read[:-1])
    last = np.ones(n, dtype=bool)
    last[:-1] = first[1:]
    s, e = np.flatnonzero(m & first), np.flatnonzero(m & last)
    assert len(s) == len(e)
    runs = np.zeros(len(s), dtype=NX_RUN)
    runs["read"] = read[s]
    runs["pos"] = s - rel[read[s]]
    runs["len"] = e - s + 1
    runs["sym"] = B[s]
    return runs


def _acgt(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def hand_batch(lead=0, tail=0, shift=0, seed=11):
    """The smallest shapes that can go wrong, in one batch.  lead: bytes in front of the first
    read (read_offsets[0]); shift (0..2) moves the first read's runs, which start and end at
    batch positions 13..20 and 61..70, by that much, so that over the three shifts runs start
    and end at each of 15, 16, 17, 63, 64, 65; without tail the batch is a multiple of 64
    long, tail adds that many bases."""
    rng = np.random.default_rng(seed)
    reads = []
    r0 = _acgt(rng, 128 + shift)
    for a, b, s in ((13, 15, "N"), (16, 16, "R"), (17, 20, "N"), (30, 31, "Y"), (61, 63, "K"), (64, 64, "N"),
                    (65, 70, "S"), (100, 127, "N")):
        r0[shift + a:shift + b + 1] = ord(s)
    reads.append(r0)
    reads.append(np.frombuffer(b"N", dtype=np.uint8))                      # a read of one N
    for n in (1, 150, 5000):                                               # all-N reads
        reads.append(np.full(n, ord("N"), dtype=np.uint8))
    a, b = _acgt(rng, 40), _acgt(rng, 33)                                  # ...NN | NN...: two runs
    a[-2:] = ord("N")
    b[:2] = ord("N")
    reads += [a, b]
    c = _acgt(rng, 21)
    c[8:13] = np.frombuffer(b"NNRRN", dtype=np.uint8)                      # three runs
    reads.append(c)
    d = _acgt(rng, 90)                                                     # all twelve symbols,
    d[3:15] = SYMS                                                         # adjacent (twelve runs)
    for i, s in enumerate(SYMS):                                           # and apart
        d[20 + 5 * i:22 + 5 * i] = s
    reads.append(d)
    reads.append(np.frombuffer(b"NNRRN", dtype=np.uint8))                  # a whole read of runs
    total = sum(len(r) for r in reads)
    reads.append(_acgt(rng, (-total) % 64 or 64))                          # to a multiple of 64
    if tail:
        t = _acgt(rng, tail)
        t[-1] = ord("W")                                                   # the batch ends in a run
        reads.append(t)
    bases = np.concatenate([_acgt(rng, lead)] + reads + [_acgt(rng, 3)])   # bytes past the batch too
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[0] = lead
    offs[1:] = lead + np.cumsum([len(r) for r in reads])
    return bases, offs


def ragged_batch(rng, n_reads, max_len=400, frac=0.3):
    """n_reads reads of 1..max_len bases, runs of random length and symbol in frac of them."""
    lens = rng.integers(1, max_len + 1, n_reads)
    offs = np.zeros(n_reads + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    bases = _acgt(rng, int(offs[-1]))
    for r in np.flatnonzero(rng.random(n_reads) < frac):
        a, L = int(offs[r]), int(lens[r])
        for _ in range(int(rng.integers(1, 4))):
            p = int(rng.integers(0, L))
            n = int(min(L - p, rng.integers(1, 40)))
            bases[a + p:a + p + n] = SYMS[int(rng.integers(0, 12))]
    return bases, offs
