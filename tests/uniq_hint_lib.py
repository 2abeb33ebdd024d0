"""Shared by tests/test_uniq_hint.py (CPU, emulator) and tests/test_gpu_uniq_hint.py: the
indexes and read sets the run-length code of colex_at (encode_core.h uniq_code, ctx option
"uniq_hint") is tested on.  Each case returns (sequences, index, reads as a list of str)."""
import functools

import numpy as np

import ntcomp_amd as nt
from oracle_lib import OracleIndex, pack_reads

COMP = str.maketrans("ACGT", "TGCA")
# distances below a record end at which the first non-singleton position must fall: around
# the three thresholds of the code (r >= 32, 64, 128 means the first clear bit is 33, 65, 129 below)
EDGES = (31, 32, 33, 63, 64, 65, 127, 128, 129)


def revcomp(s):
    return s.translate(COMP)[::-1]


def chop(bases, L):
    s = bases.tobytes().decode()
    return [s[i:i + L] for i in range(0, len(s), L)]


def singleton_bits(ix, k):
    """bit per node: alone in its (k-1)-suffix group (derived.cpp: head and alone)"""
    lcs = np.asarray(ix.lcs, dtype=np.int64)
    nxt = np.append(lcs[1:], 0)
    return (lcs < k - 1) & (nxt < k - 1)


@functools.lru_cache(maxsize=None)
def repeat_index(k):
    g = nt.synth_genome(44, 60_000).tobytes()
    seqs = [g[:500] * 30, g[:7000]]
    return seqs, nt.Index.build(seqs, k)


@functools.lru_cache(maxsize=None)
def repeat_case(k):
    """The repeat genome g[:500] * 30 + g[:7000].  For every t of EDGES, probe reads that end
    (the first record's end, d = k) exactly t positions above a non-singleton position q with
    d = k, every position between being a singleton with d = k; then the same end with the
    test's cap (read length - k - 1) at t - 2 ... t + 1, where the code alone decides, and
    with a substitution k - 1, k or k + 1 below q, so that the run entry's d = k stretch ends
    at q or next to it; plus reads with errors.
    Returns (seqs, ix, reads, probes = [(index into reads, t)])."""
    seqs, ix = repeat_index(k)
    orc = OracleIndex(ix.n, k, ix.rows, ix.C, ix.lcs)
    uniq = singleton_bits(ix, k)
    reads, probes = [], []

    def sub(r, p):
        return r[:p] + "ACGT"[("ACGT".index(r[p]) + 1) % 4] + r[p + 1:]

    g2 = seqs[1].decode()
    for text in (g2, revcomp(g2)):
        d, s = orc.ms(text.encode())
        d = np.asarray(d, dtype=np.int64)
        ok = (d == k) & uniq[np.asarray(s, dtype=np.int64)]   # a step of the left-extension test
        bad = (d == k) & ~ok
        run = np.zeros(len(text) + 1, dtype=np.int64)         # run[q] = ok positions straight above q
        for q in range(len(text) - 1, -1, -1):
            run[q] = run[q + 1] + 1 if q + 1 < len(text) and ok[q + 1] else 0
        for q in np.flatnonzero(bad):
            if run[q] < max(EDGES) + 1:
                continue
            for t in EDGES:
                x = int(q) + t                       # the read's last position
                L = k + 1 + t + 20                   # cap = L - k - 1 > t: the test reaches q
                if x + 1 - L < 0:
                    continue
                r = text[x + 1 - L:x + 1]
                probes.append((len(reads), t))
                reads.append(r)
                for cap in (t - 2, t - 1, t, t + 1):
                    reads.append(r[-(k + 1 + cap):])
                for p in (19, 20, 21):               # q is read position 20: a substitution k below it
                    e = L - 1 - t - k + (p - 20)       # and next to that (e < 0 for k > 21: left out)
                    if e >= 0:
                        reads.append(sub(r, e))
                # (behind a substitution: the record end is no longer the read's end)
                tail = text[x + 1:x + 40]
                if len(tail) == 39:
                    reads.append(r + sub(tail, 5))
    joined = np.frombuffer((seqs[0] + seqs[1]), dtype=np.uint8)
    reads += chop(nt.synth_reads(joined, 7, 0, 300, 300, 10_000), 300)
    return seqs, ix, reads, probes


@functools.lru_cache(maxsize=None)
def random_case(k):
    """C91 / C31 shapes: a 60 kb random genome, 2,000 reads of 150 bp with 1 % errors"""
    g = nt.synth_genome(100 + k, 60_000)
    seqs = [g.tobytes()]
    return seqs, nt.Index.build(seqs, k), chop(nt.synth_reads(g, 5, 0, 2000, 150, 10_000), 150)


@functools.lru_cache(maxsize=None)
def long_case():
    """400 and 1,000 bp reads at k = 31: the cap exceeds 128, the hint and the fallback mix"""
    seqs, ix, _ = random_case(31)
    g = np.frombuffer(seqs[0], dtype=np.uint8)
    reads = chop(nt.synth_reads(g, 6, 0, 150, 400, 5_000), 400) + chop(nt.synth_reads(g, 7, 0, 60, 1000, 5_000), 1000)
    return seqs, ix, reads


@functools.lru_cache(maxsize=None)
def ragged_case(k):
    """read lengths k + 2 ... k + 140, three reads of each (two with an error)"""
    seqs, ix, _ = random_case(k)
    g = seqs[0].decode()
    rng = np.random.default_rng(k)
    reads = []
    for L in range(k + 2, k + 141):
        for j in range(3):
            a = int(rng.integers(0, len(g) - L))
            r = g[a:a + L]
            if j:
                p = int(rng.integers(0, L))
                r = r[:p] + "ACGT"[("ACGT".index(r[p]) + j) % 4] + r[p + 1:]
            reads.append(revcomp(r) if (L + j) % 2 else r)
    return seqs, ix, reads


@functools.lru_cache(maxsize=None)
def read_start_case(k):
    """Reads ending at every position around the repeat genome's junctions (the end of the
    repeated unit inside g[:7000], both strands), where the path cover breaks and a run goes on
    in a new entry: among them the reads whose d = k record ends on the first position of a
    run entry, where the code must not be used."""
    seqs, ix = repeat_index(k)
    g2 = seqs[1].decode()
    reads = []
    for text in (g2, revcomp(g2)):
        j = 500 if text is g2 else len(g2) - 500
        for x in range(j - 8, j + k + 24):
            for L in (k + 3, k + 40, 150):
                if x + 1 - L >= 0 and x + 1 <= len(text):
                    reads.append(text[x + 1 - L:x + 1])
    return seqs, ix, reads


@functools.lru_cache(maxsize=None)
def strain_case():
    """a genome and five strains at k = 23: short unitigs, entries are joint runs"""
    gg = nt.synth_genome(45, 40_000)
    st = nt.synth_strains(gg, 5, 40, 2000)
    seqs = [gg.tobytes()] + [st[i].tobytes() for i in range(5)]
    texts = np.concatenate([np.frombuffer(s, dtype=np.uint8) for s in seqs])
    return seqs, nt.Index.build(seqs, 23), chop(nt.synth_reads(texts, 2, 0, 1500, 150, 10_000), 150)


def oracle_records(ix, k, reads):
    bases, offs = pack_reads(reads)
    exp, eoff = OracleIndex(ix.n, k, ix.rows, ix.C, ix.lcs).encode(bases, offs)
    return bases, offs, exp, eoff
