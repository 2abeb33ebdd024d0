"""The checker for FASTQ quality scores, in numpy and independent of the C++ (quality_core.h,
quality.hip): the mode tables, the per-block alphabet, the width rule and the bit packing of
the canonical packed form (include/ntcomp_codec.h), the sections expected for a FASTQ text,
and the FASTQ text expected from a decode."""
import numpy as np

LO, HI = 33, 126  # '!' .. '~'
MODES = {"drop": 0, "keep": 1, "bin8": 2}
BIN8 = [(2, None), (10, 6), (20, 15), (25, 22), (30, 27), (35, 33), (40, 37)]  # (q below, level)


def bin8(q):
    """Phred q -> its level on the 8-level scale (q < 2 stays)."""
    for below, level in BIN8:
        if q < below:
            return q if level is None else level
    return 40


def mode_table(mode):
    """256 entries: the byte kept for each input byte, 0 = not a quality byte."""
    t = np.zeros(256, dtype=np.uint8)
    for c in range(LO, HI + 1):
        t[c] = LO + bin8(c - LO) if MODES.get(mode, mode) == 2 else c
    return t


def width(n_syms):
    for w, most in ((0, 1), (1, 2), (2, 4), (4, 16)):
        if n_syms <= most:
            return w
    return 8


def n_words(n_quals, w):
    return (n_quals * w + 63) // 64


def pack(codes, w):
    """codes (ints < 2^w) -> little-endian bit stream as uint64 words, unused high bits zero."""
    if w == 0:
        return np.zeros(0, dtype=np.uint64)
    per = 64 // w
    c = np.zeros(n_words(len(codes), w) * per, dtype=np.uint64)
    c[:len(codes)] = codes
    shifts = (np.arange(per, dtype=np.uint64) * np.uint64(w))
    return np.bitwise_or.reduce(c.reshape(-1, per) << shifts, axis=1)


def unpack(words, n, w):
    if w == 0:
        return np.zeros(n, dtype=np.uint64)
    per = 64 // w
    shifts = (np.arange(per, dtype=np.uint64) * np.uint64(w))
    c = (np.asarray(words, dtype=np.uint64)[:, None] >> shifts) & np.uint64((1 << w) - 1)
    return c.reshape(-1)[:n]


_KEEP = b"ACGTN-BDHVRYSWKM"


def normalise(seq):
    """The sequence line as the parser keeps it (fastq.hip norm_of): whitespace dropped."""
    out = bytearray()
    for c in seq:
        ch = bytes([c])
        if ch in b" \t\r\n":
            continue
        if ch.upper() in _KEEP:  # (a one-byte substring test: one of the sixteen)
            out += ch.upper()
        elif ch in b"uU":
            out += b"T"
        elif ch in b".~":
            out += b"-"
        else:
            out += b"N"
    return bytes(out)


def records(text):
    """FASTQ text of whole 4-line records -> [(normalised bases, quality bytes)]; one trailing
    '\\r' is stripped from each line, the last line may lack its newline."""
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    strip = lambda l: l[:-1] if l.endswith(b"\r") else l
    return [(normalise(strip(lines[i + 1])), strip(lines[i + 3])) for i in range(0, len(lines), 4)]


def sections(text, block_reads, mode="keep"):
    """-> (list of dicts n_reads, n_quals, width, n_syms, alphabet, payload_off, payload_bytes;
    the payload as uint64 words): every block starts on a word boundary."""
    tab = mode_table(mode)
    recs = records(text)
    metas, words = [], []
    off = 0
    for b in range(0, len(recs), block_reads):
        blk = recs[b:b + block_reads]
        q = tab[np.frombuffer(b"".join(r[1] for r in blk), dtype=np.uint8)]
        assert q.all(), "a quality byte outside '!'..'~'"
        alphabet = np.unique(q)
        w = width(len(alphabet))
        p = pack(np.searchsorted(alphabet, q), w)
        metas.append(dict(n_reads=len(blk), n_quals=len(q), width=w, n_syms=len(alphabet),
                          alphabet=alphabet.tobytes(), payload_off=8 * off, payload_bytes=8 * len(p)))
        words.append(p)
        off += len(p)
    return metas, (np.concatenate(words) if words else np.zeros(0, dtype=np.uint64))


def fastq_text(recs, first_id=1, mode="keep"):
    """[(bases, qualities)] -> the text a decode with the sections prints."""
    tab = mode_table(mode)
    out = bytearray()
    for i, (s, q) in enumerate(recs):
        out += b"@seq.%d\n" % (first_id + i) + s + b"\n+\n" + tab[np.frombuffer(q, dtype=np.uint8)].tobytes() + b"\n"
    return bytes(out)


def meta_dict(m):
    """A ctypes QualMeta (ntcomp_amd) as the dict sections() gives."""
    return dict(n_reads=int(m.n_reads), n_quals=int(m.n_quals), width=int(m.width), n_syms=int(m.n_syms),
                alphabet=bytes(m.alphabet)[:m.n_syms], payload_off=int(m.payload_off),
                payload_bytes=int(m.payload_bytes))


def make_fastq(reads, quals, eol=b"\n", last_newline=True):
    """reads, quals: lists of bytes -> FASTQ text with names r0, r1, ..."""
    t = b"".join(b"@r%d" % i + eol + s + eol + b"+" + eol + q + eol for i, (s, q) in enumerate(zip(reads, quals)))
    return t if last_newline else t[:-len(eol)]


_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def random_alphabet(rng, n):
    return np.sort(rng.choice(np.arange(LO, HI + 1, dtype=np.uint8), n, replace=False))


def ragged_batch(rng, n_syms_per_block, block_reads, n_reads, ends=(63, 1, 0)):
    """Ragged reads of 1..300 bases in blocks of block_reads.  Block b draws its qualities from an
    alphabet of n_syms_per_block[b] symbols, each of which occurs; block b < len(ends) holds
    ends[b] qualities modulo 64, so with (63, 1, 0) blocks end one quality before a word
    boundary, one after, and on it, whatever the width.  -> (reads, quals) as lists of bytes."""
    lens = rng.integers(1, 301, n_reads)
    lens[5] = 1
    reads, quals = [], []
    for b, r0 in enumerate(range(0, n_reads, block_reads)):
        r1 = min(r0 + block_reads, n_reads)
        if b < len(ends):
            before = int(lens[r0:r1 - 1].sum())
            lens[r1 - 1] = (ends[b] - before) % 64 or 64
        total = int(lens[r0:r1].sum())
        alpha = random_alphabet(rng, n_syms_per_block[b])
        q = alpha[rng.integers(0, len(alpha), total)]
        q[rng.permutation(total)[:len(alpha)]] = alpha  # every symbol occurs
        s = _ACGT[rng.integers(0, 4, total)]
        at = 0
        for L in lens[r0:r1]:
            reads.append(s[at:at + L].tobytes())
            quals.append(q[at:at + L].tobytes())
            at += int(L)
    return reads, quals
