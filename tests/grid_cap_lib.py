"""Batches that take the per-read text kernels past their grid cap, in plain Python / numpy and
independent of the library.

Eight launches of the FASTQ / FASTA text path run "one wave per record, grid-stride" on a grid
capped at 65,536 workgroups of four waves: launch_fastq_parse (k_fq_recs, k_fq_norm),
launch_names_pack (k_n_measure), launch_named_text (k_named), launch_fastq_text (k_fastq),
launch_fasta (k_fasta), and in pairs.hip launch_pair_weave (k_pw_copy), launch_pair_check
(k_pm_check) and launch_pair_split (k_ps_copy).  Past CAP records a wave takes a second trip
round its loop; the batches here have CAP + 5 records so that it does.

Every record depends on its index, and no record at index r >= CAP equals record r - CAP in name,
bases or qualities: a wave that repeated its first trip, or wrote the first trip's bytes in the
second trip's place, changes the output.

The reads have 1 to 3 bases, which keeps CAP + 5 records near 5 MB of text, but for one read in
every block of the archive: a block whose reads are all shorter than k holds no long record, and
the format drops such a block (status NTC_ERR_EMPTY_READ, include/ntcomp_codec.h), so a decode
would have nothing to format.  Read 1 of every BLOCK reads is therefore LONG bases of a text the
caller draws from its indexed genome (long_read)."""
import numpy as np

import names_lib as nl

# std::min((n + 3) / 4, 65536) workgroups of 256 threads = 4 waves, in every launcher named above
CAP = 4 * 65536
N = CAP + 5        # no multiple of 4, 64 or 256: the last workgroup's second trip is partly empty
N_PAIRS = CAP + 5  # k_pw_copy and k_pm_check loop over pairs, k_ps_copy over 2 * N_PAIRS reads
BLOCK = 65536      # reads per block of the archive (the calls' default)
LONG = 40          # bases of a block's one long read

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
# sequence lines for the parser alone: IUPAC symbols, lower case, blanks, u / . / ~ and junk
_MESSY = [b"aC gT", b"n\tRy", b"SwKm ", b" bdhv", b"uU.~x", b"B D\tH", b"*0-Nn"]


def _cut(flat, lens):
    ends = np.cumsum(lens).tolist()
    return [flat[a:b] for a, b in zip([0] + ends[:-1], ends)]


def _reads_quals(rng, n):
    """n reads of 1 to 3 bases of ACGT and their qualities of '!'..'~'; records r >= CAP are drawn
    again until they differ from record r - CAP in bases and in qualities"""
    lens = rng.integers(1, 4, n)
    total = int(lens.sum())
    reads = _cut(_ACGT[rng.integers(0, 4, total)].tobytes(), lens)
    quals = _cut(rng.integers(33, 127, total, dtype=np.uint8).tobytes(), lens)
    for r in range(CAP, n):
        while reads[r] == reads[r - CAP] or quals[r] == quals[r - CAP]:
            reads[r] = _ACGT[rng.integers(0, 4, int(rng.integers(1, 4)))].tobytes()
            quals[r] = rng.integers(33, 127, len(reads[r]), dtype=np.uint8).tobytes()
    return reads, quals


def _anchor(rng, reads, quals, long_read, every):
    """read 1 of every `every` reads: LONG bases of long_read, from an offset the block gives"""
    if long_read is None:
        return
    for b, i in enumerate(range(1, len(reads), every)):
        assert len(long_read) >= b + LONG
        reads[i] = long_read[b:b + LONG]
        quals[i] = rng.integers(33, 127, LONG, dtype=np.uint8).tobytes()


def assert_trips_differ(names, reads, quals, step=CAP):
    """the condition of the module's docstring"""
    assert len(names) == len(reads) == len(quals)
    for r in range(step, len(names)):
        assert names[r] != names[r - step] and reads[r] != reads[r - step] and quals[r] != quals[r - step], r


def batch(seed=1, n=N, blanks=False, long_read=None):
    """-> (names, reads, quals), n of each: names r<i> (blanks: records beyond CAP carry a comment
    after a space or a tab, two in three of them), 1 to 3 bases of ACGT, qualities of '!'..'~';
    long_read: see the module's docstring"""
    rng = np.random.default_rng(seed)
    reads, quals = _reads_quals(rng, n)
    _anchor(rng, reads, quals, long_read, BLOCK)
    names = [b"r%d" % i for i in range(n)]
    if blanks:
        for i in range(CAP, n):
            names[i] += (b" c%d x" % i, b"\tt%d" % i, b"")[i % 3]
    assert_trips_differ(names, reads, quals)
    return names, reads, quals


def records(names, reads, quals, eol=b"\n"):
    """the FASTQ records one by one (their join is names_lib.make_fastq's text)"""
    return [b"@" + n + eol + r + eol + b"+" + eol + q + eol for n, r, q in zip(names, reads, quals)]


def messy(reads, quals):
    """-> (sequence lines, quality lines) for the parser: records beyond CAP get a sequence line
    of _MESSY and one more letter, and a quality line as long as that line is raw; the others stay"""
    lines, qs = list(reads), list(quals)
    for i in range(CAP, len(reads)):
        lines[i] = _MESSY[i % len(_MESSY)] + b"acgtnACGTN"[i % 10:i % 10 + 1]
        qs[i] = b"I" * len(lines[i])
    return lines, qs


def pairs(seed=2, n_pairs=N_PAIRS, long_read=None):
    """-> (names1, reads1, quals1), (names2, reads2, quals2): mates named x<i>/1 and x<i>/2, or
    x<i> 1:N and x<i>\\t2:N (both strip rules on both sides of CAP), reads and qualities as batch();
    long_read goes into mate 1 of pair 1 of every BLOCK / 2 pairs: a block of the woven archive"""
    rng = np.random.default_rng(seed)
    sides = []
    for m in (1, 2):
        reads, quals = _reads_quals(rng, n_pairs)
        if m == 1:
            _anchor(rng, reads, quals, long_read, BLOCK // 2)
        names = [b"x%d/%d" % (i, m) if i % 2 == 0 else b"x%d" % i + (b" 1:N", b"\t2:N")[m - 1] for i in range(n_pairs)]
        assert_trips_differ(names, reads, quals)
        sides.append((names, reads, quals))
    return sides


def swap(recs, changes):
    """the text of recs with the records of changes ({index: bytes}) in place of theirs"""
    out = list(recs)
    for i, r in changes.items():
        out[i] = r
    return b"".join(out)


# the maker tests itself on import, at a size that costs nothing
assert [len(x) for x in batch(3, 7)] == [7, 7, 7] and batch(3, 7) == batch(3, 7)
assert all(1 <= len(r) == len(q) <= 3 for _, rs, qs in [batch(4, 50)] for r, q in zip(rs, qs))
assert b"".join(records(*batch(3, 7))) == nl.make_fastq(*batch(3, 7))
assert swap([b"a", b"b", b"c"], {1: b"X"}) == b"aXc"
assert [len(r) for r in batch(3, 7, long_read=b"ACGT" * 11)[1]][:3] == [len(batch(3, 7)[1][0]), LONG, len(batch(3, 7)[1][2])]
