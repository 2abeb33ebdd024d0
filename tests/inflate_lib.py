"""What the tests of `--inflate gpu` share: the corpus of sound gzip members (made with Python's
zlib and wrapped here), the damaged ones with the status each must get, the seeded mutants, and
the checker (Python's zlib, which verifies the header, CRC-32 and ISIZE).

The statuses and the size limit are restated here from ntcomp_amd/csrc/inflate_core.h and
include/ntcomp_codec.h; the tests fail if they drift apart."""
import functools
import struct
import zlib

import numpy as np

import ntcomp_amd as nt

MAX_OUT = 65536  # kInfMaxOut, NTC_INFLATE_MAX_OUT
OK, BAD_HEADER, BAD_BLOCK, BAD_CODE, BAD_DISTANCE, OUTPUT, INPUT, CRC, ISIZE, TOO_LARGE = range(10)
STATUS_NAMES = ["kInfOk", "kInfBadHeader", "kInfBadBlock", "kInfBadCode", "kInfBadDistance", "kInfOutput", "kInfInput",
                "kInfCrc", "kInfIsize", "kInfTooLarge"]
# bgzip's end-of-file marker: a BGZF member of no bytes
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

SIZES = [1, 2, 3, 257, 258, 259, 65279, 65280, 65535, 65536]
LEVELS = [0, 1, 6, 9]
STRATEGIES = {"fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE, "filtered": zlib.Z_FILTERED}


# ---- wrapping ---------------------------------------------------------------------------------
def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH):
    """a raw deflate stream of data; flush_at: offsets at which the coder is flushed"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out, at = b"", 0
    for f in list(flush_at) + [len(data)]:
        out += c.compress(data[at:f])
        if f < len(data):
            out += c.flush(flush)
        at = f
    return out + c.flush()


def trailer(data):
    return struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def bgzf(raw, data):
    """raw wrapped as a BGZF member of data (its size must fit BSIZE)"""
    size = 18 + len(raw) + 8
    assert size <= 65536
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + raw + trailer(data)


def gzip_member(raw, data, fname=None, fcomment=None, fhcrc=False, extra=None, ftext=False):
    """raw wrapped as a plain gzip member with the optional header fields"""
    flg = (1 if ftext else 0) | (2 if fhcrc else 0) | (4 if extra is not None else 0) | (8 if fname is not None else 0) \
        | (16 if fcomment is not None else 0)
    h = bytes([0x1f, 0x8b, 8, flg, 1, 2, 3, 4, 2, 3])
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + raw + trailer(data)


def wrap(raw, data):
    """BGZF where the member fits one, else a plain gzip member (random bytes of 65,280 and more)"""
    return bgzf(raw, data) if 18 + len(raw) + 8 <= 65536 else gzip_member(raw, data)


# ---- contents ---------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def fastq_text(n, seed=3):
    r = _rng(seed)
    out = []
    size = 0
    i = 0
    while size < n:
        L = int(r.integers(50, 151))
        seq = bytes(r.choice(np.frombuffer(b"ACGT", np.uint8), L))
        q = bytes(r.choice(np.frombuffer(b"FFFFFF:,#", np.uint8), L))
        rec = b"@read.%d/1 lane=%d\n%s\n+\n%s\n" % (i, seed, seq, q)
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n]


def fib_bytes(n, seed=5):
    """exact Fibonacci counts over 22 symbols (46,367 bytes; with the end-of-block symbol the
    unlimited Huffman code is over 15 bits deep), shuffled and cut to n"""
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    a = np.frombuffer(b"".join(bytes([40 + i]) * c for i, c in enumerate(f)), np.uint8).copy()
    _rng(seed).shuffle(a)
    return a.tobytes()[:n]


def content(kind, n, seed=7):
    r = _rng(seed)
    if kind == "fastq":
        return fastq_text(n, seed)
    if kind == "random":
        return r.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "all256":
        a = np.resize(np.arange(256, dtype=np.uint8), n)
        r.shuffle(a)
        return a.tobytes()
    if kind == "zero":  # distance 1, length 258: overlapping copies; one distinct byte and one distinct distance
        return bytes(n)
    if kind.startswith("period"):
        return np.resize(r.integers(0, 256, int(kind[6:]), dtype=np.uint8), n).tobytes()
    if kind == "fib":
        return fib_bytes(n, seed)
    if kind == "onedist":  # random bytes whose second half repeats the first: every match has one distance
        half = r.integers(0, 256, n // 2, dtype=np.uint8).tobytes()
        return (half + half)[:n]
    raise ValueError(kind)


KINDS = ["fastq", "random", "all256", "zero", "period3", "period32768", "fib", "onedist"]


def own_member(data):
    """the member this project's own coder makes of data (ntc_deflate_stream, engine 3)"""
    import deflate_lib as dl
    return dl.member_of(data)


@functools.lru_cache(maxsize=None)
def sound():
    """(name, member, data) of every sound member"""
    out = [("eof", EOF_MEMBER, b"")]

    def add(name, data, raw=None, member=None):
        out.append((name, member if member is not None else wrap(raw, data), data))

    for n in SIZES:  # the sizes, as text (dynamic blocks) and as random bytes (stored blocks)
        add("size%d-fastq" % n, fastq_text(n, n), raw_deflate(fastq_text(n, n)))
        add("size%d-random-l1" % n, content("random", n, n), raw_deflate(content("random", n, n), 1))
    for k in KINDS:  # the contents under every level and strategy
        data = content(k, 40000 if k != "period32768" else 65536)
        for lv in LEVELS:
            add("%s-l%d" % (k, lv), data, raw_deflate(data, lv))
        for sn, st in STRATEGIES.items():
            add("%s-%s" % (k, sn), data, raw_deflate(data, 6, st))
    add("empty-plain", b"", raw_deflate(b""))
    add("one-byte-huffman", b"A", raw_deflate(b"A", 6, zlib.Z_HUFFMAN_ONLY))
    add("one-distinct-byte", b"A" * 1000, raw_deflate(b"A" * 1000, 9))
    # several blocks in a member
    text = fastq_text(30000, 11)
    add("sync-flush", text, raw_deflate(text, 6, flush_at=(1, 9999, 20000)))
    add("full-flush", text, raw_deflate(text, 6, flush_at=(10000, 10001, 29999), flush=zlib.Z_FULL_FLUSH))
    parts = [(content("random", 5000, 1), 0, zlib.Z_DEFAULT_STRATEGY), (text[:7000], 6, zlib.Z_FIXED),
             (text[7000:19000], 9, zlib.Z_DEFAULT_STRATEGY), (b"", 0, zlib.Z_DEFAULT_STRATEGY),
             (content("zero", 3000), 6, zlib.Z_FIXED), (content("fib", 9000), 6, zlib.Z_HUFFMAN_ONLY),
             (content("random", 70, 2), 0, zlib.Z_DEFAULT_STRATEGY)]
    raw = b""
    for i, (d, lv, st) in enumerate(parts):  # each piece a stream of its own, all but the last ended by a full flush
        c = zlib.compressobj(lv, zlib.DEFLATED, -15, 8, st)
        raw += c.compress(d) + (c.flush() if i + 1 == len(parts) else c.flush(zlib.Z_FULL_FLUSH))
    add("mixed-blocks", b"".join(p[0] for p in parts), raw)
    # headers
    raw = raw_deflate(text)
    add("fname", text, member=gzip_member(raw, text, fname=b"reads.fastq"))
    add("fcomment", text, member=gzip_member(raw, text, fcomment=b"a comment"))
    add("fhcrc", text, member=gzip_member(raw, text, fhcrc=True))
    add("all-fields", text, member=gzip_member(raw, text, fname=b"n", fcomment=b"", fhcrc=True, extra=b"XY\x03\0abc", ftext=True))
    add("plain", text, member=gzip_member(raw, text))
    add("extra-not-bc", text, member=gzip_member(raw, text, extra=b"AB\x01\0z"))
    add("extra-empty", text, member=gzip_member(raw, text, extra=b""))
    # this project's own coder: one chunk, two chunks, every encoding
    for name, data in (("own-text", fastq_text(40000, 13)), ("own-random", content("random", 32768 + 808, 3)),
                       ("own-zero", bytes(65536)), ("own-fib", fib_bytes(40000)), ("own-empty", b""), ("own-8", b"ACGTACGT")):
        add(name, data, member=own_member(data))
    assert len({n for n, _, _ in out}) == len(out)
    return out


# ---- hand-built streams --------------------------------------------------------------------------
class Bits:
    """a deflate bit stream written bit by bit"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, k):  # k bits of v, low bit first (header fields, extra bits)
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        return self

    def code(self, c, k):  # a Huffman code of k bits, high bit first
        for i in range(k - 1, -1, -1):
            self.put((c >> i) & 1, 1)
        return self

    def align(self):
        self.n = -(-self.n // 8) * 8
        return self

    def bytes(self):
        return self.acc.to_bytes(-(-self.n // 8), "little")


def canon(lens):
    """canonical codes of lens (symbol -> (code, length)), as RFC 1951 assigns them"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# a complete code-length code over all 19 symbols: 13 codes of 4 bits, 6 of 5
CL_FULL = [4] * 13 + [5] * 6


def dyn_header(b, lit_lens, dist_lens, final=1, cl_lens=None, cl_syms=None, hlit=None, hdist=None):
    """the header of a dynamic block: the lengths sent one by one (no repeats) unless cl_syms gives
    the sequence of (symbol, extra value) outright"""
    cl_lens = CL_FULL if cl_lens is None else cl_lens
    b.put(final, 1).put(2, 2)
    b.put((len(lit_lens) if hlit is None else hlit) - 257, 5).put((len(dist_lens) if hdist is None else hdist) - 1, 5)
    b.put(19 - 4, 4)
    for s in CL_ORDER:
        b.put(cl_lens[s], 3)
    codes = canon(cl_lens)
    seq = [(l, 0) for l in list(lit_lens) + list(dist_lens)] if cl_syms is None else cl_syms
    for s, x in seq:
        if s in codes:
            b.code(*codes[s])
        b.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
    return b


def lit_lens_of(used, length_of=None):
    """literal/length code lengths over 257 + symbols: `used` maps symbol -> length"""
    n = max(257, max(used) + 1)
    return [used.get(s, 0) for s in range(n)]


def finish(b, data, pad=24):
    """the stream as a plain gzip member of data, zero bytes behind the blocks so that a decoder that
    goes on reading stays inside the member, then the trailer"""
    return gzip_member(b.align().bytes() + bytes(pad), data)


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


@functools.lru_cache(maxsize=None)
def damaged():
    """(name, member, claimed_out, status) of every damaged member"""
    out = []
    text = fastq_text(5000, 17)
    good = bgzf(raw_deflate(text), text)
    n = len(text)

    def add(name, member, status, claimed=None):
        out.append((name, bytes(member), n if claimed is None else claimed, status))

    # truncation: inside the header, inside a block, inside the trailer
    add("cut-header-5", good[:5], INPUT)
    add("cut-header-17", good[:17], INPUT)
    add("cut-extra", good[:11] + b"\xff" + good[12:40], INPUT)  # XLEN runs past the member
    add("cut-block", good[:len(good) // 2], INPUT)
    add("cut-block-1", good[:19], INPUT)
    add("cut-trailer-7", good[:-1], INPUT)
    add("cut-trailer-0", good[:-8], INPUT)
    add("bytes-behind", good + b"\0", INPUT)
    stored = bgzf(raw_deflate(text, 0), text)
    add("cut-stored", stored[:1000], INPUT)
    # the trailer
    add("crc-flipped", good[:-8] + bytes([good[-8] ^ 1]) + good[-7:], CRC)
    add("isize-plus", good[:-4] + struct.pack("<I", n + 1), ISIZE, n + 1)
    add("isize-minus", good[:-4] + struct.pack("<I", n - 1), ISIZE, n)
    add("isize-minus-claimed", good[:-4] + struct.pack("<I", n - 1), OUTPUT, n - 1)
    add("claimed-small", good, OUTPUT, n - 1)
    add("claimed-zero", good, OUTPUT, 0)
    add("claimed-large", good, ISIZE, n + 1)
    add("claimed-small-stored", stored, OUTPUT, n - 1)
    zeros = bgzf(raw_deflate(bytes(5000)), bytes(5000))
    add("claimed-small-match", zeros, OUTPUT, 4999)
    # the header
    add("magic", b"\x1f\x8c" + good[2:], BAD_HEADER)
    add("method", good[:2] + b"\x07" + good[3:], BAD_HEADER)
    add("reserved-flag", good[:3] + b"\x24" + good[4:], BAD_HEADER)
    h = gzip_member(raw_deflate(text), text, fhcrc=True)
    add("header-crc", h[:10] + bytes([h[10] ^ 0x40]) + h[11:], BAD_HEADER)
    add("fname-open", bytes([0x1f, 0x8b, 8, 8]) + b"\1" * 40, INPUT)
    # blocks
    add("type3", finish(Bits().put(1, 1).put(3, 2), b""), BAD_BLOCK, 0)
    add("stored-nlen", finish(Bits().put(1, 1).put(0, 2).align().put(5, 16).put(0xFFFA ^ 1, 16).put(0, 40), b""), BAD_BLOCK, 0)
    lit2 = lit_lens_of({65: 1, 256: 1})  # 'A' and end of block, a bit each
    add("hlit-287", finish(dyn_header(Bits(), lit2, [1, 1], hlit=287), b""), BAD_BLOCK, 0)
    add("hdist-31", finish(dyn_header(Bits(), lit2, [1, 1], hdist=31), b""), BAD_BLOCK, 0)
    add("hdist-32", finish(dyn_header(Bits(), lit2, [1, 1], hdist=32), b""), BAD_BLOCK, 0)
    # the code-length code
    add("cl-over", finish(dyn_header(Bits(), lit2, [1, 1], cl_lens=[1, 1, 1] + [0] * 16, cl_syms=[]), b""), BAD_CODE, 0)
    add("cl-incomplete", finish(dyn_header(Bits(), lit2, [1, 1], cl_lens=[1] + [0] * 18, cl_syms=[]), b""), BAD_CODE, 0)
    add("cl-incomplete-2", finish(dyn_header(Bits(), lit2, [1, 1], cl_lens=[2, 2, 2] + [0] * 16, cl_syms=[]), b""), BAD_CODE, 0)
    add("cl-none", finish(dyn_header(Bits(), lit2, [1, 1], cl_lens=[0] * 19, cl_syms=[]), b""), BAD_CODE, 0)
    # the code lengths
    add("repeat-first", finish(dyn_header(Bits(), lit2, [1, 1], cl_syms=[(16, 0)] + [(0, 0)] * 300), b""), BAD_CODE, 0)
    seq = [(0, 0)] * 65 + [(1, 0)] + [(18, 127)] + [(18, 41)] + [(1, 0)] + [(1, 0), (17, 0)]  # 257 + 2 lengths, the last run is 3
    add("repeat-past-end", finish(dyn_header(Bits(), lit2, [1, 1], cl_syms=seq), b""), BAD_CODE, 0)
    add("no-end-of-block", finish(dyn_header(Bits(), lit_lens_of({65: 1, 66: 1}) , [1, 1]), b""), BAD_CODE, 0)
    add("lit-over", finish(dyn_header(Bits(), lit_lens_of({65: 1, 66: 1, 256: 1}), [1, 1]), b""), BAD_CODE, 0)
    add("lit-incomplete", finish(dyn_header(Bits(), lit_lens_of({65: 2, 66: 2, 256: 2}), [1, 1]), b""), BAD_CODE, 0)
    add("lit-one-code-of-2", finish(dyn_header(Bits(), lit_lens_of({256: 2}), [1, 1]), b""), BAD_CODE, 0)
    add("dist-over", finish(dyn_header(Bits(), lit2, [1, 1, 1]), b""), BAD_CODE, 0)
    add("dist-incomplete", finish(dyn_header(Bits(), lit2, [2, 2, 2]), b""), BAD_CODE, 0)
    add("dist-one-code-of-2", finish(dyn_header(Bits(), lit2, [2]), b""), BAD_CODE, 0)
    # tokens.  lit3: 'A' 1 bit, end of block 2 bits, length symbol 257 (3 bytes) 2 bits
    lit3 = lit_lens_of({65: 1, 256: 2, 257: 2})
    c3 = canon(lit3)
    b = dyn_header(Bits(), lit3, [1])  # one distance code, of one bit: sound (see sound_handbuilt), its other bit is no code
    b.code(*c3[65]).code(*c3[257]).put(1, 1)
    add("dist-unused-code", finish(b, b""), BAD_CODE, 4)
    b = dyn_header(Bits(), lit_lens_of({256: 1}), [0])  # one literal/length code of one bit: its other bit is no code
    b.put(1, 1)
    add("lit-unused-code", finish(b, b""), BAD_CODE, 0)
    b = dyn_header(Bits(), lit3, [0])  # no distance code at all, and a match
    b.code(*c3[65]).code(*c3[257]).put(0, 1)
    add("dist-no-code", finish(b, b""), BAD_CODE, 4)
    b = dyn_header(Bits(), lit3, [1, 1])  # distance 2 after one byte
    b.code(*c3[65]).code(*c3[257]).code(1, 1)
    add("distance-too-far", finish(b, b""), BAD_DISTANCE, 4)
    b = Bits().put(1, 1).put(1, 2).code(0b0000001, 7).code(0, 5)  # a fixed block that starts with a match
    add("distance-at-start", finish(b, b""), BAD_DISTANCE, 3)
    fx = canon(FIXED_LIT)
    for s in (286, 287):
        b = Bits().put(1, 1).put(1, 2).code(*fx[65]).code(*fx[s])
        add("fixed-length-%d" % s, finish(b, b""), BAD_CODE, 4)
    for s in (30, 31):
        b = Bits().put(1, 1).put(1, 2).code(*fx[65]).code(*fx[257]).code(s, 5)
        add("fixed-distance-%d" % s, finish(b, b""), BAD_CODE, 4)
    # 65,537 bytes
    big = content("fastq", MAX_OUT + 1)
    add("too-large", gzip_member(raw_deflate(big), big), TOO_LARGE, MAX_OUT + 1)
    add("too-large-claimed-64k", gzip_member(raw_deflate(big), big), OUTPUT, MAX_OUT)
    assert len({x[0] for x in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def sound_handbuilt():
    """(name, member, data): the forms zlib accepts that its own deflate never writes"""
    out = []
    lit3 = lit_lens_of({65: 1, 256: 2, 257: 2})
    c3 = canon(lit3)
    b = dyn_header(Bits(), lit3, [1])  # one distance code of one bit (incomplete, allowed): A, then 3 bytes from 1 back
    b.code(*c3[65]).code(*c3[257]).put(0, 1).code(*c3[256])
    out.append(("single-distance-code", gzip_member(b.align().bytes(), b"AAAA"), b"AAAA"))
    b = dyn_header(Bits(), lit_lens_of({256: 1}), [0])  # one literal/length code of one bit: end of block alone
    b.put(0, 1)
    out.append(("single-literal-code", gzip_member(b.align().bytes(), b""), b""))
    b = dyn_header(Bits(), lit_lens_of({65: 1, 256: 1}), [0], final=0)  # no distance code; then an empty stored, an empty fixed block
    c = canon(lit_lens_of({65: 1, 256: 1}))
    b.code(*c[65]).code(*c[65]).code(*c[256])
    b.put(0, 1).put(0, 2).align().put(0, 16).put(0xFFFF, 16)
    b.put(0, 1).put(1, 2).code(0, 7)
    b.put(1, 1).put(1, 2).code(*canon(FIXED_LIT)[66]).code(0, 7)
    out.append(("no-distance-code", gzip_member(b.align().bytes(), b"AAB"), b"AAB"))
    # repeats: 65 zeros, 'A' = 1, 138 + 52 zeros by symbol 18, end of block = 1, then two distance lengths
    seq = [(0, 0)] * 65 + [(1, 0)] + [(18, 127)] + [(18, 41)] + [(1, 0)] + [(1, 0), (1, 0)]
    b = dyn_header(Bits(), lit_lens_of({65: 1, 256: 1}), [1, 1], cl_syms=seq)
    b.code(*c[65]).code(*c[256])
    out.append(("repeats", gzip_member(b.align().bytes(), b"A"), b"A"))
    return out


def all_sound():
    return list(sound()) + list(sound_handbuilt())


# ---- the checker ---------------------------------------------------------------------------------
def zlib_accepts(member):
    """(True, data) when zlib takes member as exactly one whole gzip member, else (False, None)"""
    d = zlib.decompressobj(31)
    try:
        data = d.decompress(member)
    except zlib.error:
        return False, None
    if not d.eof or d.unused_data:
        return False, None
    return True, data


def claimed_of(member):
    """what a BGZF reader takes a member's output size to be: its ISIZE field.  Every size past the
    limit is handed over as MAX_OUT + 1, which is as much too large and needs no room of gigabytes"""
    return min(struct.unpack("<I", member[-4:])[0], MAX_OUT + 1) if len(member) >= 4 else 0


@functools.lru_cache(maxsize=None)
def mutants(seed=20240, per_member=56):
    """seeded single-bit and single-byte changes of three dozen sound members of modest size:
    list of (name, member)"""
    r = _rng(seed)
    small = {n: m for n, m, d in all_sound()}
    extra = [("mut-text-%d-%s" % (i, k), wrap(raw_deflate(fastq_text(1500 + 97 * i, 100 + i), lv, st), fastq_text(1500 + 97 * i, 100 + i)))
             for i, (k, lv, st) in enumerate([("l1", 1, 0), ("l6", 6, 0), ("l9", 9, 0), ("fixed", 6, zlib.Z_FIXED),
                                              ("huff", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE), ("l0", 0, 0)] * 4)]
    text = fastq_text(900, 99)
    base = extra + [(n, m) for n, m, d in sound_handbuilt()] + [(n, small[n]) for n in ("eof", "size257-fastq", "one-distinct-byte")]
    base.append(("mut-all-fields", gzip_member(raw_deflate(text), text, fname=b"n", fcomment=b"c", fhcrc=True, extra=b"XY\x01\0a")))
    assert len(base) == 36
    out = []
    for name, m in base:
        for j in range(per_member):
            a = bytearray(m)
            # half of the changes fall in the first 64 bytes, where the headers and the code descriptions are
            pos = int(r.integers(0, min(len(a), 64))) if j % 2 else int(r.integers(0, len(a)))
            if j % 4 < 2:
                a[pos] ^= 1 << int(r.integers(0, 8))
                kind = "bit"
            else:
                a[pos] = (a[pos] + int(r.integers(1, 256))) & 0xFF
                kind = "byte"
            out.append(("%s/%s%d@%d" % (name, kind, j, pos), bytes(a)))
    return out


def layout(members, claimed, gap=32):
    """members laid into one blob with `gap` bytes between them and their outputs likewise ->
    (blob, INFLATE_MEMBER array, output capacity)"""
    m = np.zeros(len(members), dtype=nt.INFLATE_MEMBER)
    parts, size, at = [], 0, gap
    for i, (mem, c) in enumerate(zip(members, claimed)):
        parts += [b"\xEE" * gap, mem]
        m[i] = (size + gap, len(mem), c, at)
        size += gap + len(mem)
        at += c + gap
    return b"".join(parts) + b"\xEE" * gap, m, at


def run_all(ctx, members, claimed, fill=0xC3):
    """every member in one call, outputs and inputs 32 bytes apart -> (per-member output bytes or
    None, results); the bytes between and around the outputs must stay as they were"""
    blob, m, cap = layout(members, claimed)
    out = np.full(cap, fill, dtype=np.uint8)
    got, res = nt.inflate_members(ctx, blob, m, out=out)
    assert got is out
    mask = np.ones(cap, dtype=bool)
    outs = []
    for d, r in zip(m, res):
        a, b = int(d["dst_off"]), int(d["dst_off"]) + int(d["out_bytes"])
        if r["status"] == 0:
            mask[a:b] = False
            outs.append(out[a:b].tobytes())
        else:
            outs.append(None)
    assert (out[mask] == fill).all(), "a byte outside the sound members' outputs was written"
    return outs, res
