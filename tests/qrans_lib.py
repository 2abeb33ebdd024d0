"""The checker for the order-1 rANS coder of the quality sections, in numpy and plain Python
and independent of the C++ (qrans_core.h, qrans.hip): the (context, symbol) counts, the
normalisation to 4096, the byte-wise span coder and decoder, the section body of a block, the
sections expected for a FASTQ text, the version-2 "NTCQ" file, and a seeded order-1 Markov
quality source.  The format is in include/ntcomp_codec.h and DESIGN.md section 18."""
import struct

import numpy as np

import qual_lib as ql

SPAN = 2048
BITS = 12
TOTAL = 1 << BITS
L = 1 << 23


def n_spans(n_quals):
    return (n_quals + SPAN - 1) // SPAN


def span_bound(n):
    """the most bytes a span of n symbols can take (the derivation is in qrans_core.h)"""
    return n + n // 2 + 4


def counts(syms, n_syms):
    """(n_syms + 1, n_syms) counts over the whole block: row = the symbol before it in the span,
    n_syms at a span's start."""
    syms = np.asarray(syms, dtype=np.int64)
    ctx = np.empty_like(syms)
    ctx[1:] = syms[:-1]
    ctx[::SPAN] = n_syms
    c = np.zeros((n_syms + 1, n_syms), dtype=np.int64)
    np.add.at(c, (ctx, syms), 1)
    return c


def normalise(row):
    """one row of counts -> frequencies that sum to 4096 (all zero for an empty row)"""
    row = [int(v) for v in row]
    total = sum(row)
    if total == 0:
        return [0] * len(row)
    f = [0 if c == 0 else max(1, c * TOTAL // total) for c in row]
    best = row.index(max(row))  # the lowest index on ties
    f[best] += TOTAL - sum(f)
    assert f[best] >= 1 and sum(f) == TOTAL
    return f


def table(c):
    return [normalise(r) for r in c]


def encode_span(syms, tab, n_syms):
    """the span's stream: the final state as u32 LE, then the bytes in reverse order of emission"""
    cum = [np.concatenate(([0], np.cumsum(r))).tolist() for r in tab]
    syms = [int(s) for s in syms]
    x, out = L, bytearray()
    for i in range(len(syms) - 1, -1, -1):
        s = syms[i]
        ctx = syms[i - 1] if i else n_syms
        f, c = tab[ctx][s], cum[ctx][s]
        assert f > 0
        while x >= (f << 19):
            out.append(x & 0xFF)
            x >>= 8
        x = ((x // f) << BITS) + (x % f) + c
    assert L <= x < (1 << 31)
    return struct.pack("<I", x) + bytes(reversed(out))


def decode_span(stream, n, tab, n_syms):
    """-> (symbols, ok): ok is False for a slot in no symbol, a byte needed past the end, a final
    state other than L, or bytes left over.  Never raises on a damaged stream."""
    cum = [np.concatenate(([0], np.cumsum(r))).tolist() for r in tab]
    ok = len(stream) >= 4
    data = bytes(stream) + bytes(4)
    x, = struct.unpack_from("<I", data, 0)
    pos, ctx, out = 4, n_syms, []
    ok = ok and L <= x < (1 << 31)
    for _ in range(n):
        slot = x & (TOTAL - 1)
        row = cum[ctx]
        if slot >= row[-1]:
            ok = False
            s = 0
        else:
            s = max(k for k in range(n_syms) if row[k] <= slot)
        f, c = tab[ctx][s], row[s]
        x = (f * (x >> BITS) + slot - c) & 0xFFFFFFFF
        for _ in range(2):
            if x < L:
                if pos < len(stream):
                    x = (x << 8 | data[pos]) & 0xFFFFFFFF
                    pos += 1
                else:
                    ok = False
                    x = (x << 8) & 0xFFFFFFFF
        if x < L:
            ok = False
        out.append(s)
        ctx = s
    return out, ok and x == L and pos == len(stream)


def body(syms, n_syms):
    """the section body of a block whose qualities have these symbols (ranks in its alphabet)"""
    if n_syms <= 1:
        return b""
    tab = table(counts(syms, n_syms))
    spans = [encode_span(syms[i:i + SPAN], tab, n_syms) for i in range(0, len(syms), SPAN)]
    return np.asarray(tab, dtype="<u2").tobytes() + b"".join(struct.pack("<I", len(s)) for s in spans) + b"".join(spans)


def split_body(b, n_quals, n_syms):
    """-> (table as rows, span sizes, span streams)"""
    if n_syms <= 1:
        return [], [], []
    tb = 2 * (n_syms + 1) * n_syms
    tab = np.frombuffer(b, dtype="<u2", count=(n_syms + 1) * n_syms).reshape(n_syms + 1, n_syms).tolist()
    ns = n_spans(n_quals)
    sizes = list(struct.unpack_from("<%dI" % ns, b, tb))
    at, streams = tb + 4 * ns, []
    for s in sizes:
        streams.append(b[at:at + s])
        at += s
    return tab, sizes, streams


def decode_body(b, n_quals, n_syms, alphabet):
    """-> (quality bytes, ok)"""
    if n_syms <= 1:
        return bytes(alphabet[:1]) * n_quals, len(b) == 0
    tab, sizes, streams = split_body(b, n_quals, n_syms)
    out, ok = bytearray(), sum(sizes) + 2 * (n_syms + 1) * n_syms + 4 * len(sizes) == len(b)
    for j, st in enumerate(streams):
        syms, good = decode_span(st, min(SPAN, n_quals - j * SPAN), tab, n_syms)
        ok = ok and good
        out += bytes(alphabet[s] for s in syms)
    return bytes(out), ok


def sections(text, block_reads, mode="keep"):
    """-> (list of dicts as qual_lib.sections gives, plus coder = 1; the payload as bytes): every
    body starts 8-aligned, payload_bytes is exact, the bytes between bodies are zero."""
    tab = ql.mode_table(mode)
    recs = ql.records(text)
    metas, pay = [], bytearray()
    for b in range(0, len(recs), block_reads):
        blk = recs[b:b + block_reads]
        q = tab[np.frombuffer(b"".join(r[1] for r in blk), dtype=np.uint8)]
        assert q.all(), "a quality byte outside '!'..'~'"
        alphabet = np.unique(q)
        bd = body(np.searchsorted(alphabet, q), len(alphabet))
        metas.append(dict(n_reads=len(blk), n_quals=len(q), width=ql.width(len(alphabet)), n_syms=len(alphabet),
                          alphabet=alphabet.tobytes(), payload_off=len(pay), payload_bytes=len(bd), coder=1))
        pay += bd + bytes(-len(bd) % 8)
    return metas, bytes(pay)


def meta_dict(m):
    """A ctypes QualMeta (ntcomp_amd) as the dict sections() gives."""
    return dict(ql.meta_dict(m), coder=int(m.reserved[0]))


def header(mode):
    return b"NTCQ" + struct.pack("<IBB", 2, ql.MODES.get(mode, mode), 1) + bytes(22)


def section_bytes(m, bd):
    return struct.pack("<QQBBHI", m["n_reads"], m["n_quals"], m["width"], m["n_syms"], 0, len(bd)) + m["alphabet"] + bd


def file_bytes(text, block_reads, mode="keep"):
    """the version-2 side file of a text"""
    metas, pay = sections(text, block_reads, mode)
    return header(mode) + b"".join(section_bytes(m, pay[m["payload_off"]:m["payload_off"] + m["payload_bytes"]])
                                   for m in metas)


def markov_quals(rng, alphabet, n, p):
    """n quality bytes of an order-1 Markov source: the symbol stays with probability p, otherwise
    another one is drawn uniformly."""
    k = len(alphabet)
    stay = rng.random(n) < p
    jump = rng.integers(1, max(k, 2), n)
    s = np.empty(n, dtype=np.int64)
    cur = int(rng.integers(0, k))
    for i in range(n):
        if not stay[i] and k > 1:
            cur = (cur + int(jump[i])) % k
        s[i] = cur
    return np.frombuffer(bytes(alphabet), dtype=np.uint8)[s]


def markov_fastq(seed, n_reads, read_len, n_syms=4, p=0.9):
    """-> FASTQ text of n_reads reads of read_len bases with Markov qualities over n_syms symbols"""
    rng = np.random.default_rng(seed)
    alphabet = ql.random_alphabet(rng, n_syms)
    q = markov_quals(rng, alphabet, n_reads * read_len, p)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n_reads * read_len)]
    reads = [s[i * read_len:(i + 1) * read_len].tobytes() for i in range(n_reads)]
    quals = [q[i * read_len:(i + 1) * read_len].tobytes() for i in range(n_reads)]
    return ql.make_fastq(reads, quals)
