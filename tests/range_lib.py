"""A range of reads: the checker of the tests, plain Python and independent of the code under
test (DESIGN.md "Decoding a range").

The reference of every range test is the full decode: a range's text must be the cut of it.
  records(text)               the records of a FASTA (">": 2 lines) or FASTQ ("@": 4 lines) text
  cut(text, a, b)             records [a, b) of it, from 0, byte for byte
  window_sizes(sizes, f, c)   the per-read sizes a window [f, f + c) leaves: 0 outside it
  window_ok(f, c, n, paired)  the window's rule: not empty, inside the batch, whole pairs
  block_range(reads, f, c)    blocks [b0, b1] that hold reads [f, f + c), with the reads before
                              b0, the reads of b0 left out and the reads of b1 left out
  shard(i, n, nb)             blocks [lo, hi) of the i-th (from 1) of n slices of nb blocks
  parse_reads(spec)           "A-B", "A", "A-", "-B" (1-based, inclusive) -> (a, b or None), or None
  parse_shard(spec)           "I/N" -> (i, n), or None"""


def lines_per_record(text):
    if not text:
        return 2
    assert text[:1] in (b">", b"@"), "neither FASTA nor FASTQ"
    return 2 if text[:1] == b">" else 4


def records(text):
    """every record with its line ends as they are (the decoder writes LF and a last newline)"""
    if not text:
        return []
    k = lines_per_record(text)
    lines = text.split(b"\n")
    assert lines[-1] == b"", "the text does not end in a newline"
    lines = [ln + b"\n" for ln in lines[:-1]]
    assert len(lines) % k == 0, "the text does not hold whole records"
    recs = [b"".join(lines[i:i + k]) for i in range(0, len(lines), k)]
    assert all(r[:1] == text[:1] for r in recs), "a record starts with another character"
    return recs


def cut(text, a, b):
    recs = records(text)
    assert 0 <= a <= b <= len(recs), "the cut reaches past the text"
    return b"".join(recs[a:b])


def window_ok(first, count, n_reads, paired=False):
    if count <= 0 or first < 0 or first + count > n_reads:
        return False
    return not paired or (first % 2 == 0 and count % 2 == 0)


def window_sizes(sizes, first, count):
    return [s if first <= r < first + count else 0 for r, s in enumerate(sizes)]


def block_range(block_reads, first, count):
    """(b0, b1, before, head_skipped, tail_skipped) for reads [first, first + count) of an
    archive whose blocks hold block_reads reads each"""
    assert count > 0 and first + count <= sum(block_reads)
    ends, tot = [], 0
    for n in block_reads:
        tot += n
        ends.append(tot)
    b0 = next(i for i, e in enumerate(ends) if e > first)
    b1 = next(i for i, e in enumerate(ends) if e >= first + count)
    before = ends[b0] - block_reads[b0]
    return b0, b1, before, first - before, ends[b1] - (first + count)


def shard(i, n, n_blocks):
    assert 1 <= i <= n
    return (i - 1) * n_blocks // n, i * n_blocks // n


def parse_reads(spec):
    digits = "0123456789"
    if spec.count("-") > 1 or not spec or any(c not in digits + "-" for c in spec):
        return None
    lo, dash, hi = spec.partition("-")
    if not dash:
        hi = lo
    if not lo and not hi:
        return None
    a, b = int(lo) if lo else 1, int(hi) if hi else None
    if a < 1 or (b is not None and b < a):
        return None
    return a, b


def parse_shard(spec):
    i, slash, n = spec.partition("/")
    if not slash or not i.isdigit() or not n.isdigit() or not i.isascii() or not n.isascii():
        return None
    return (int(i), int(n)) if 1 <= int(i) <= int(n) else None


# the checker tests itself on import
_FA = b">seq.1\nAC\n>seq.2\n\n>seq.3\nGGT\n"
_FQ = b"@a\nAC\n+\nII\n@b x\nG\n+\nJ\n"
assert records(_FA) == [b">seq.1\nAC\n", b">seq.2\n\n", b">seq.3\nGGT\n"] and records(b"") == []
assert records(_FQ) == [b"@a\nAC\n+\nII\n", b"@b x\nG\n+\nJ\n"]
assert cut(_FA, 0, 3) == _FA and cut(_FA, 1, 2) == b">seq.2\n\n" and cut(_FA, 2, 2) == b"" and cut(_FQ, 1, 2) == b"@b x\nG\n+\nJ\n"
assert b"".join(cut(_FA, a, b) for a, b in ((0, 1), (1, 3))) == _FA
assert window_ok(0, 3, 3) and window_ok(2, 1, 3) and not window_ok(2, 2, 3) and not window_ok(1, 0, 3) and not window_ok(3, 1, 3)
assert window_ok(2, 2, 4, True) and not window_ok(1, 2, 4, True) and not window_ok(0, 3, 4, True)
assert window_sizes([5, 6, 7, 8], 1, 2) == [0, 6, 7, 0] and window_sizes([5, 6], 0, 2) == [5, 6]
assert block_range([4, 4, 2], 0, 10) == (0, 2, 0, 0, 0) and block_range([4, 4, 2], 4, 4) == (1, 1, 4, 0, 0)
assert block_range([4, 4, 2], 3, 2) == (0, 1, 0, 3, 3) and block_range([4, 4, 2], 9, 1) == (2, 2, 8, 1, 0)
assert [shard(i, 3, 7) for i in (1, 2, 3)] == [(0, 2), (2, 4), (4, 7)] and shard(1, 2, 0) == (0, 0)
assert parse_reads("3-9") == (3, 9) and parse_reads("7") == (7, 7) and parse_reads("7-") == (7, None) and parse_reads("-4") == (1, 4)
assert all(parse_reads(s) is None for s in ("", "-", "0", "0-3", "5-4", "1-2-3", "a-b", "1,2", " 3", "--4"))
assert parse_shard("2/4") == (2, 4) and all(parse_shard(s) is None for s in ("0/4", "5/4", "2", "/4", "2/", "a/b", "1/0"))
