"""Fixtures and models for two size thresholds no other test crosses, in plain Python / numpy
(the genome comes from the package's host generator; nothing here touches a GPU).

Part A: one device call over 2^32 + 2 B bases.  The CPU oracle cannot check 4.3 G bases, but a
read's records do not depend on where the read lies in its batch: the batch is one *period* of P
reads and B bases, repeated R = ceil((2^32 + 2 B) / B) times, and every expected value is the
oracle's on one period, tiled.  B is odd, so no power of two is a multiple of it: a position
truncated to any number of bits lands in other content, and the repetitions start at every
alignment modulo 16 and 32.  test_big_batch.py asserts the fixture's conditions on the host.

Part B: scan_excl_t (kernels.hip) works on tiles of SCAN_TILE = 256 x 16 items and recurses on the
tile sums: one level up to SCAN_TILE items, two up to SCAN_TILE^2, three past that.  tiny_fastq
makes FASTQ text of that many records for the parser, whose kept counts go through the scan; the
expected bases and offsets are the generator's own arrays."""
import functools
from typing import NamedTuple

import numpy as np

import ntcomp_amd as nt

K = 31
TWO32 = 1 << 32
BLOCK = 65536      # reads per digest block (the calls' default)
REC_SLOT = 8       # kRecSlot (encode_core.h): records of a read in its dense slot; more spill
GENOME_SEED, GENOME_LEN = 41, 300_000
N_READS = 267      # odd, 3 x 89: no multiple of BLOCK below 89 blocks is a multiple of it
SHORT = (1, 7, 30)  # a read of one base and two more below k

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_POW10 = np.array([10 ** d for d in range(1, 20)], dtype=np.uint64)


def revcomp(s):
    return s.translate(_COMP)[::-1]


class Period(NamedTuple):
    genome: bytes
    reads: list        # P reads (bytes)
    origin: list       # per read: (start in the genome, reverse strand, substituted positions)
    bases: np.ndarray  # uint8[B], the reads back to back
    offs: np.ndarray   # uint64[P + 1]
    P: int
    B: int
    R: int             # repetitions: the batch holds R P reads and R B >= 2^32 + 2 B bases
    trim: int          # bases the tuning took off the longest read


def digits(ids):
    """decimal digits of each id (uint64 array)"""
    return 1 + np.searchsorted(_POW10, np.asarray(ids, dtype=np.uint64), side="right").astype(np.int64)


def text_layout(lens, first_id=1):
    """FASTA text ">seq.%d\\n%s\\n" of reads of these lengths -> (header bytes of each read, newline
    included; text offsets [n + 1]).  The last offset is the text's size: 7 bytes and the id's digits
    per read, plus the bases."""
    lens = np.asarray(lens, dtype=np.int64)
    head = 5 + digits(np.uint64(first_id) + np.arange(len(lens), dtype=np.uint64)) + 1
    toffs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(head + lens + 1, out=toffs[1:])
    return head, toffs


def repetitions(B):
    return -(-(TWO32 + 2 * B) // B)


def conditions(reads, first_id=1):
    """what test_big_batch.py asserts of the fixture, as a dict of booleans (and the figures behind
    them under '_')"""
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    P, B = len(reads), int(lens.sum())
    R = repetitions(B)
    offs = np.concatenate([[0], np.cumsum(lens)])
    at = TWO32 % B                                       # base 2^32 within its period
    r = int(np.searchsorted(offs, at, side="right")) - 1
    head, toffs = text_layout(np.tile(lens, R), first_id)
    t = int(np.searchsorted(toffs, TWO32, side="right")) - 1  # the read whose text holds byte 2^32
    in_line = int(toffs[t]) + int(head[t]) <= TWO32 < int(toffs[t]) + int(head[t]) + int(lens[t % P])
    n_blocks = -(-R * P // BLOCK)
    return {
        "B_odd": B % 2 == 1,
        "covers": (R - 1) * B < TWO32 + 2 * B <= R * B,
        "base_2_32_inside_a_long_read": int(offs[r]) < at < int(offs[r + 1]) and int(lens[r]) >= 2 * K,
        "text_byte_2_32_in_a_sequence_line": in_line,
        "reads_no_multiple_of_64": (R * P) % 64 != 0 and (R * P) % 256 != 0,
        "digest_blocks_off_the_periods": all((b * BLOCK) % P for b in range(1, n_blocks)) and n_blocks >= 3,
        "_": dict(P=P, B=B, R=R, read_at_2_32=r, text_read_at_2_32=t, n_blocks=n_blocks),
    }


@functools.lru_cache(maxsize=None)
def period(seed=1):
    """The period: N_READS reads of the genome, some from the reverse strand, ragged lengths from 1 to
    40,000 with a mean near 15,000, 0 to 4 substitutions each.  The longest read then loses bases
    from its end, as few as make every condition of conditions() hold."""
    rng = np.random.default_rng(seed)
    genome = nt.synth_genome(GENOME_SEED, GENOME_LEN).tobytes()
    n_drawn = N_READS - len(SHORT)
    lens = np.concatenate([rng.integers(1000, 40_001, n_drawn // 2), rng.integers(2, 20_001, n_drawn - n_drawn // 2),
                           np.array(SHORT)])
    lens = lens[rng.permutation(len(lens))]
    reads, origin = [], []
    for L in lens.tolist():
        start = int(rng.integers(0, len(genome) - L + 1))
        rev = bool(rng.random() < 0.4)
        s = bytearray(revcomp(genome[start:start + L]) if rev else genome[start:start + L])
        subs = sorted(set(rng.integers(0, L, int(rng.integers(0, 5))).tolist()))
        for p in subs:
            s[p] = b"ACGT"[(b"ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
        reads.append(bytes(s))
        origin.append((start, rev, tuple(subs)))
    longest = int(np.argmax(lens))
    whole = reads[longest]
    for trim in range(2000):
        reads[longest] = whole[:len(whole) - trim]
        c = conditions(reads)
        if all(v for k, v in c.items() if k != "_"):
            break
    else:
        raise AssertionError("no trim of the longest read meets the conditions")
    start, rev, subs = origin[longest]  # (the start of a reverse read's strand is its end in the genome)
    origin[longest] = (start + trim if rev else start, rev, tuple(p for p in subs if p < len(reads[longest])))
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return Period(genome, reads, origin, bases, offs, len(reads), len(bases), repetitions(len(bases)), trim)


# ---- the batch, from one period ------------------------------------------------------------------
def tiled_offsets(offs, step, R):
    """offsets [P + 1] of one period -> offsets [R P + 1] of R periods, `step` apart (numpy arithmetic)"""
    offs = np.asarray(offs, dtype=np.uint64)
    out = np.empty(R * (len(offs) - 1) + 1, dtype=np.uint64)
    out[:-1] = (np.arange(R, dtype=np.uint64)[:, None] * np.uint64(step) + offs[None, :-1]).ravel()
    out[-1] = np.uint64(R) * np.uint64(step)
    return out


def tiled_records(recs, roffs, R):
    """the oracle's records and record offsets of one period -> those of R periods"""
    return np.tile(recs, R), tiled_offsets(roffs, int(roffs[-1]), R)


def record_lengths(recs):
    """bases each record stands for, and which are short records (oracle_lib.OracleIndex.decode's rule)"""
    flags = (recs >> np.uint64(56)).astype(np.uint8)
    short = (flags & 2) != 0
    return np.where(short, flags >> 2, (recs >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.int64), short


def check_regions(B, R):
    """The byte ranges of the R B decoded bases that the GPU tests copy back and compare: the first
    three periods (where a write truncated to 32 bits from the region past 2^32 would land), every
    16th period after them, and everything from 2^32 - B to the end.  -> sorted, disjoint [lo, hi)"""
    tail = TWO32 - B
    out = [(0, 3 * B)]
    out += [(j * B, (j + 1) * B) for j in range(16, R, 16) if (j + 1) * B <= tail]
    out.append((tail, R * B))
    assert all(a[1] <= b[0] for a, b in zip(out, out[1:]))
    return out


def expected_bases(bases, lo, hi):
    """bytes [lo, hi) of the period's bases repeated for ever"""
    B = len(bases)
    return np.resize(np.roll(bases, -(lo % B)), hi - lo)


def check_periods(P, R, toffs, B):
    """The reads whose text the whole-text test compares, as [first, last) ranges of reads: the first
    three periods, every 16th period, and every read whose text starts at or after byte 2^32 - B."""
    first_tail = int(np.searchsorted(toffs, TWO32 - B, side="left"))
    out = [(0, 3 * P)]
    out += [(j * P, (j + 1) * P) for j in range(16, R, 16) if (j + 1) * P <= first_tail]
    out.append((first_tail, R * P))
    return out


def fasta_text(reads, first, last, first_id=1):
    """the model ">seq.%d\\n%s\\n" of reads [first, last) of the period repeated for ever"""
    P = len(reads)
    return b"".join(b">seq.%d\n%s\n" % (first_id + i, reads[i % P]) for i in range(first, last))


# ---- Part B: the scan's levels ---------------------------------------------------------------------
SCAN_TILE = 256 * 16  # kScanThreads x kScanItems (kernels.hip)
N_TWO_LEVELS = SCAN_TILE ** 2              # the largest two-level scan: level 2 is one full tile
N_THREE_LEVELS = SCAN_TILE ** 2 + 1        # the smallest three-level scan: 4,097 tile sums, two tiles
N_LEVEL2_TAIL = SCAN_TILE ** 2 + SCAN_TILE + 1  # 4,098 tile sums: a level-2 tail of two items
SCAN_CASES = (N_TWO_LEVELS, N_THREE_LEVELS, N_LEVEL2_TAIL)


def scan_levels(n):
    """how often scan_excl_t calls itself for n items, the first call included, and the items of each level"""
    items = [n]
    while -(-items[-1] // SCAN_TILE) > 1:
        items.append(-(-items[-1] // SCAN_TILE))
    return len(items), items


class TinyFastq(NamedTuple):
    text: np.ndarray    # uint8: n records "@\n<1-3 bases>\n+\n<qualities>\n"
    bases: np.ndarray   # uint8: what a parser must find
    offs: np.ndarray    # uint64[n + 1]
    starts: np.ndarray  # int64[n + 1]: where each record starts in text


def tiny_fastq(n, seed):
    """n records of 1 to 3 bases of ACGT with qualities of '!'..'~' and an empty name, vectorised.
    Lengths, bases and qualities are drawn per record, so the kept counts vary and the offsets are no
    arithmetic sequence."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, n, dtype=np.int64)
    o = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=o[1:])
    total = int(o[-1])
    bases = _ACGT[rng.integers(0, 4, total, dtype=np.uint8)]
    quals = rng.integers(33, 127, total, dtype=np.uint8)
    starts = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(6 + 2 * lens, out=starts[1:])
    text = np.empty(int(starts[-1]), dtype=np.uint8)
    s, o0 = starts[:-1], o[:-1]
    text[s] = ord("@")
    text[s + 1] = text[s + 2 + lens] = text[s + 4 + lens] = text[s + 5 + 2 * lens] = ord("\n")
    text[s + 3 + lens] = ord("+")
    for j in range(3):
        m = np.flatnonzero(lens > j)
        text[s[m] + 2 + j] = bases[o0[m] + j]
        text[s[m] + 5 + lens[m] + j] = quals[o0[m] + j]
    return TinyFastq(text, bases, o.astype(np.uint64), starts)


def tiny_cut(t, n):
    """the first n records of t (the text cut at a record boundary)"""
    return TinyFastq(t.text[:int(t.starts[n])], t.bases[:int(t.offs[n])], t.offs[:n + 1], t.starts[:n + 1])


def tiny_damage(t, r):
    """t's text with the last quality byte of record r taken out: its sequence line is then longer
    than its quality line, and every line count stays"""
    at = int(t.starts[r + 1]) - 2
    assert t.text[at + 1] == 10 and t.text[at] != 10
    return np.concatenate([t.text[:at], t.text[at + 1:]])


# the makers test themselves on import, at sizes that cost nothing
assert tiny_fastq(3, 1).text.tobytes().count(b"\n") == 12 and tiny_fastq(3, 1).text.tobytes()[:2] == b"@\n"
assert digits([1, 9, 10, 99, 100, 10 ** 19]).tolist() == [1, 1, 2, 2, 3, 20]
assert int(text_layout([3, 1], 9)[1][-1]) == len(b">seq.9\nACG\n>seq.10\nA\n")
assert scan_levels(SCAN_TILE)[0] == 1 and scan_levels(SCAN_TILE + 1)[0] == 2
assert expected_bases(np.arange(5, dtype=np.uint8), 7, 13).tolist() == [2, 3, 4, 0, 1, 2]
