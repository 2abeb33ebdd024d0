"""Shared by tests/test_parse_stage.py (CPU, the stand-alone sanitizer program) and
tests/test_gpu_parse_stage.py: the batches k_parse4's query stage (kernels.hip, NTC_PARSE_QLDS)
is tested on.  A block of 256 reads stages the words of the 2-bit query stream its reads cover
when they fit 1536 words (49,088 bases at the least), so the shapes put blocks on both sides of
that size and the block's first and last word in every alignment.  A case is (reads as a list
of str, lead): lead bytes lie in front of the batch, offs[0] = lead."""
import functools

import numpy as np

import ntcomp_amd as nt

COMP = str.maketrans("ACGT", "TGCA")
GENOME_BP = 50_000
STAGE_WORDS = 1536   # kernels.hip kParseStageWords
BLOCK = 256          # reads per block of k_parse4


def revcomp(s):
    return s.translate(COMP)[::-1]


@functools.lru_cache(maxsize=None)
def genome():
    return nt.synth_genome(2024, GENOME_BP)


@functools.lru_cache(maxsize=None)
def index(k):
    return nt.Index.build([genome().tobytes()], k)


def draw(rng, L):
    """a read of L bases: a genome piece, 1 % substitutions, every second one reverse-complemented"""
    g = genome().tobytes().decode()
    a = int(rng.integers(0, len(g) - L))
    r = list(g[a:a + L])
    for p in np.flatnonzero(rng.random(L) < 0.01):
        r[p] = "ACGT"[("ACGT".index(r[p]) + 1 + int(rng.integers(0, 3))) % 4]
    r = "".join(r)
    return revcomp(r) if rng.integers(0, 2) else r


def reads_of(lengths, seed):
    rng = np.random.default_rng(seed)
    return [draw(rng, int(L)) for L in lengths]


def stage_words(b, e):
    """encode_core.h stage_word_count: words a block whose reads cover stream positions [b, e) reads"""
    return ((e - 1) >> 5) + 2 - (b >> 5)


def blocks_staged(reads):
    """per block of 256 reads: does it fit the stage (the kernel's rule, with its even first word)"""
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    out = []
    for r0 in range(0, len(reads), BLOCK):
        b, e = int(offs[r0]), int(offs[min(r0 + BLOCK, len(reads))])
        out.append(((b >> 5) & 1) + stage_words(b, e) <= STAGE_WORDS)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (reads, lead)"""
    c = {}
    # four blocks, the last one partial, all staged
    c["bench_1000x150"] = (reads_of([150] * 1000, 1), 0)
    # lengths 1 ... 400 twice, ascending: blocks of 16,512 (staged), 49,280 (1,541 words: just
    # past the stage), 82,048 (not staged) and 12,560 bases (staged)
    c["ragged_1_400"] = (reads_of(np.repeat(np.arange(1, 401), 2), 2), 0)
    # 64,000 bases per full block: they parse from global memory, the last 88 reads stage
    c["long_600x250"] = (reads_of([250] * 600, 3), 0)
    # one long read in the middle block: with 5,000 bases the block is 43,250 bases and still
    # stages (1,352 words), with 12,000 it parses from global memory between two staged blocks
    c["one_5000_read"] = (reads_of([150] * 300 + [5000] + [150] * 299, 4), 0)
    c["one_12000_read"] = (reads_of([150] * 300 + [12000] + [150] * 299, 14), 0)
    # offs[0] = 37: the batch's bases are not 16-byte aligned and not a multiple of 32 in
    # front; 523 reads of 149 bases put the blocks' first words at odd and even indexes
    c["lead_37"] = (reads_of([149] * 523, 5), 37)
    # the batch's last read ends exactly on a word boundary / one base past it
    for name, rem in (("ends_on_word", 0), ("ends_one_past_word", 1)):
        lens = [150] * 300
        lens.append(33 + (rem - (sum(lens) + 33)) % 32)
        assert sum(lens) % 32 == rem
        c[name] = (reads_of(lens, 6 + rem), 0)
    for n in (1, 255, 256, 257):
        c[f"n_reads_{n}"] = (reads_of([150] * n, 10 + n), 0)
    return c


def check_shapes():
    """the cases hold what their comments say"""
    c = cases()
    assert blocks_staged(c["bench_1000x150"][0]) == [True] * 4
    assert blocks_staged(c["ragged_1_400"][0]) == [True, False, False, True]
    assert blocks_staged(c["long_600x250"][0]) == [False, False, True]
    assert blocks_staged(c["one_5000_read"][0]) == [True, True, True]
    assert blocks_staged(c["one_12000_read"][0]) == [True, False, True]
    assert blocks_staged(c["lead_37"][0]) == [True] * 3


def batch(reads, lead):
    """-> (bases with lead filler bytes in front, offsets with offs[0] = lead)"""
    body = "".join(reads).encode()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    offs += np.uint64(lead)
    return np.frombuffer(b"T" * lead + body, dtype=np.uint8).copy(), offs
