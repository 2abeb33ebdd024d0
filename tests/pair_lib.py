"""Paired-end reads: the checker of the tests, plain Python and independent of the code under
test (DESIGN.md "Paired-end reads").

A paired archive alternates: read 2p is mate 1 of pair p, read 2p + 1 its mate 2.
  weave(t1, t2)               the record-wise interleaving of two FASTQ texts
  split(text, lines)          the two parts of a decoded text: even records, odd records
  mates_agree(n1, n2)         the mate rule on two names
  first_bad_pair(n1s, n2s)    the lowest pair whose mates disagree, or None"""


def _records(text, lines_per_record):
    """the records of a text, each with its line ends as they are; a last line without its
    newline gets one"""
    if not text:
        return []
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    lines = [ln + b"\n" for ln in lines]
    assert len(lines) % lines_per_record == 0, "the text does not hold whole records"
    return [b"".join(lines[i:i + lines_per_record]) for i in range(0, len(lines), lines_per_record)]


def weave(t1, t2):
    r1, r2 = _records(t1, 4), _records(t2, 4)
    assert len(r1) == len(r2), "mate texts hold different record counts"
    return b"".join(a + b for a, b in zip(r1, r2))


def split(text, lines_per_record):
    recs = _records(text, lines_per_record)
    assert len(recs) % 2 == 0, "an odd number of records"
    return b"".join(recs[0::2]), b"".join(recs[1::2])


def _id(name):
    for i, c in enumerate(name):
        if c in b" \t":
            return name[:i]
    return name


def mates_agree(n1, n2):
    a, b = _id(n1), _id(n2)
    if a.endswith(b"/1") and b.endswith(b"/2"):
        a, b = a[:-2], b[:-2]
    return a == b


def first_bad_pair(names1, names2):
    for p, (a, b) in enumerate(zip(names1, names2)):
        if not mates_agree(a, b):
            return p
    return None


# the checker tests itself on import
assert weave(b"@a\nA\n+\nI\n@b\nC\n+\nI", b"@c\r\nG\r\n+\r\nI\r\n@d\nT\n+\nI\n") == \
    b"@a\nA\n+\nI\n@c\r\nG\r\n+\r\nI\r\n@b\nC\n+\nI\n@d\nT\n+\nI\n"
assert weave(b"", b"") == b""
assert split(b">a\nA\n>b\nC\n>c\nG\n>d\nT\n", 2) == (b">a\nA\n>c\nG\n", b">b\nC\n>d\nT\n")
assert mates_agree(b"x/1", b"x/2") and mates_agree(b"", b"") and mates_agree(b"x 1:N", b"x\t2:N")
assert not mates_agree(b"x/1", b"x") and not mates_agree(b"x/2", b"x/1") and mates_agree(b"/1", b"/2")
assert first_bad_pair([b"a", b"b/1"], [b"a", b"c/2"]) == 1 and first_bad_pair([b"a"], [b"a x"]) is None
