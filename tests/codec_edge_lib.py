"""Edge cases of the block codec's decoders: a plain reference and a case table.

Test infrastructure only; it shares no code with ntcomp_amd/csrc.  Three parts:

  * stream builders on the BitString writer of tests/golden/make_codec_golden.py (imported,
    not copied): a Rice stream from (values, p) with p chosen freely, a minimal-binary
    stream from (values, max), optional codes past num_u64 and trailing words;
  * a decoder in Python integers restating src/decode.rs:51-149 (read_rice,
    read_minimal_binary's v - 1, num_u64 / encoded_size, zip_block_contents and its errors);
  * a model of unpack.hip's Rice segment rules (512-bit segments, every segment decoded
    from its first bit, the 8-segment limit, dead chains), which says for a stream whether
    the device flags it not-simple or serial and how many segments its true chain runs
    through -- what ntc_ctx_get_option reports as unpack_rice_*.

CASES is the table: name -> Case (four streams, the expected records or None = rejected).
tests/test_unpack_edges.py runs it through the host decoder, tests/test_gpu_unpack_edges.py
through the GPU unpacker.
"""
import importlib.util
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_codec_golden", os.path.join(HERE, "golden", "make_codec_golden.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)
BitString = mk.BitString

M64 = (1 << 64) - 1
SEG = 512          # unpack.hip kRiceSegBits, restated
SEG_LIMIT = 8      # segments a continuation may cross before the stream is flagged serial
NOT_SIMPLE, SERIAL = 1, 2


class Rejected(Exception):
    """the reference's decoder returns Err (or panics) on this block"""


# ---- streams ------------------------------------------------------------------------------
class Stream:
    def __init__(self, words, num_u64, param, encoded_size=None):
        self.payload = b"".join(w.to_bytes(8, "big") for w in words)
        self.num_u64 = num_u64
        self.param = param
        self.encoded_size = len(words) if encoded_size is None else encoded_size


def rice(values, p, num_u64=None, extra=(), trailing=()):
    """values (then extra codes past num_u64) as Rice codes of parameter p, then trailing words"""
    w = BitString()
    for v in list(values) + list(extra):
        w.rice(v, p)
    return Stream(w.words() + list(trailing), len(values) if num_u64 is None else num_u64, p)


def minimal_binary(values, mx, num_u64=None, extra=(), trailing=(), raw=False):
    """values as minimal-binary codes of v + 1 below mx (raw: the written numbers themselves)"""
    w = BitString()
    for v in list(values) + list(extra):
        w.minimal_binary(v if raw else v + 1, mx)
    return Stream(w.words() + list(trailing), len(values) if num_u64 is None else num_u64, mx)


def split4(recs):
    """split_encoded_dictionary (make_codec_golden.split), with a short record's bases taken
    from bits 0-55 alone (encode.rs:216-221 reads bytes 0..7: bases 28.. are A)"""
    s1, s2, s3, _, _ = mk.split([r for r in recs if not (r >> 57) & 1]) if any(not (r >> 57) & 1 for r in recs) \
        else ([], [], [], [], 0)
    s3 = [r >> 56 for r in recs]
    bases = []
    for r in recs:
        if (r >> 57) & 1:
            bases += [((r & ((1 << 56) - 1)) >> (2 * i)) & 3 for i in range(r >> 58)]
    return s1, s2, s3, [mk.as_2bit(bases[i:i + 31]) for i in range(0, len(bases), 31)]


def packer_streams(recs):
    """the four streams the reference's packer writes for these records (make_codec_golden)"""
    s1, s2, s3, s4 = split4(recs)
    out = []
    for vals, is_rice in ((s1, False), (s2, True), (s3, True), (s4, False)):
        words, param = mk.rice_stream(vals) if is_rice else mk.minimal_binary_stream(vals)
        out.append(Stream(words, len(vals), param))
    return out


# ---- the decoder, in Python integers (decode.rs:51-149) -----------------------------------
def bit_string(payload):
    return bin(int.from_bytes(payload, "big"))[2:].zfill(8 * len(payload)) if payload else ""


def read_rice(s, n, p):
    if p > 63:
        raise Rejected("rice parameter")
    out, pos = [], 0
    for _ in range(n):
        i = s.find("1", pos)
        if i < 0 or i + 1 + p > len(s):
            raise Rejected("rice code past the stream")
        r = int(s[i + 1:i + 1 + p], 2) if p else 0
        out.append((((i - pos) << p) | r) & M64)
        pos = i + 1 + p
    return out


def read_minimal_binary(s, n, mx):
    if n == 0:
        return []
    if mx < 1:
        raise Rejected("minimal binary max 0")
    l = mx.bit_length() - 1
    limit = (1 << (l + 1)) - mx
    out, pos = [], 0
    for _ in range(n):
        if pos + l > len(s):
            raise Rejected("minimal binary code past the stream")
        v = int(s[pos:pos + l], 2) if l else 0
        pos += l
        if v >= limit:
            if pos + 1 > len(s):
                raise Rejected("minimal binary code past the stream")
            v = ((v << 1) | int(s[pos])) - limit
            pos += 1
        if v == 0:
            raise Rejected("minimal binary v == 0")
        out.append(v - 1)
    return out


def zip_block(c1, c2, fl, bn):
    """-> (records, rows whose value only the host decoder defines)"""
    if len(c1) != len(c2):
        raise Rejected("c1.len != c2.len")
    T = sum(((f & 0xFC) >> 2) for f in fl)
    if T and len(bn) != (T + 30) // 31:
        raise Rejected("s4.n != ceil(T / 31)")
    out, host_rows, i, j = [], [], 0, 0
    for r, f in enumerate(fl):
        flag = f & 0xFF
        if flag & 2 == 0:
            if i >= len(c1):
                raise Rejected("long record past s1")
            w = (c1[i] & 0xFFFFFFFF) | ((c2[i] & 0xFFFFFF) << 32)
            i += 1
        else:
            L = flag >> 2
            if j + L > T:
                raise Rejected("bases past T")
            w = 0
            for u in range(L):  # past 32 bases as_2bit panics: the host decoder's wrapping shifts
                q = j + u
                w |= ((bn[q // 31] >> (2 * (q % 31))) & 3) << ((2 * u) & 63)
            if L > 32:
                host_rows.append(r)
            w &= (1 << 56) - 1
            j += L
        out.append(w | (flag << 56))
    return out, host_rows


def decode_streams(streams):
    """the four streams -> (records, host-defined rows), or raises Rejected"""
    vals = []
    for k, st in enumerate(streams):
        if len(st.payload) != 8 * st.encoded_size:
            raise Rejected("encoded.len() != header.encoded_size")
        s = bit_string(st.payload)
        vals.append(read_rice(s, st.num_u64, st.param) if k in (1, 2) else read_minimal_binary(s, st.num_u64, st.param))
    return zip_block(*vals)


# ---- the Rice segment model (unpack.hip's k_rice_a / k_rice_b / k_rice_walk / k_rice_count) --
def _rice_len(s, pos, p):
    i = s.find("1", pos)
    return 0 if i < 0 or i + 1 + p > len(s) else i + 1 + p - pos


def rice_segment_model(payload, p):
    """-> (flags, through): NOT_SIMPLE | SERIAL as the device sets them for this stream, and the
    active segments its true chain runs through (0 for a simple or a serial stream)"""
    s = bit_string(payload)
    nbits = len(s)
    nseg = (nbits + SEG - 1) // SEG
    marks, end = set(), []
    for g in range(nseg):  # every segment decoded from its first bit
        pos, b = g * SEG, min((g + 1) * SEG, nbits)
        while pos < b:
            n = _rice_len(s, pos, p)
            if not n:
                pos = None  # dead: it ran past the stream's end
                break
            marks.add(pos)
            pos += n
        end.append(pos)
    flags, nxt = 0, []
    for g in range(nseg):  # on from its end until a start a later segment marked
        b, nx = min((g + 1) * SEG, nbits), None
        if end[g] is None:
            q = nbits
            if b < nbits:
                flags |= NOT_SIMPLE
        else:
            q = end[g]
            while q < nbits:
                if q in marks:
                    nx = q // SEG
                    break
                if q >= b + SEG_LIMIT * SEG:
                    flags |= SERIAL
                    break
                n = _rice_len(s, q, p)
                if not n:
                    break
                q += n
            if b < nbits and nx != g + 1:
                flags |= NOT_SIMPLE
        nxt.append(nx)
    if flags & SERIAL or not flags & NOT_SIMPLE:
        return flags, 0
    on, v = set(), 0
    while v is not None:  # the true chain's segments
        on.add(v)
        v = nxt[v]
    return flags, nseg - len(on)


def model_counters(streams):
    """(not_simple, serial, through) summed over a block's Rice streams that run on the device"""
    tot = [0, 0, 0]
    for st in streams[1:3]:
        if st.num_u64 == 0 or st.param > 63 or st.encoded_size == 0:
            continue
        fl, thr = rice_segment_model(st.payload, st.param)
        tot[0] += bool(fl & NOT_SIMPLE)
        tot[1] += bool(fl & SERIAL)
        tot[2] += thr
    return tuple(tot)


def rice_class(st):
    fl, _ = rice_segment_model(st.payload, st.param)
    return "serial" if fl & SERIAL else "not-simple" if fl & NOT_SIMPLE else "simple"


# ---- cases --------------------------------------------------------------------------------
class Case:
    def __init__(self, name, streams, intended=None, packable=False, s2_class=None, note=""):
        self.name, self.streams, self.note = name, streams, note
        self.intended = intended    # the records the builder meant (None: the decoder alone says)
        self.packable = packable    # the host packer writes exactly these streams for `intended`
        self.s2_class = s2_class    # the class the segment model must give s2 (None: unstated)
        try:
            recs, self.host_rows = decode_streams(streams)
            self.expected = np.array(recs, dtype=np.uint64)
        except Rejected as e:
            self.expected, self.host_rows, self.why = None, [], str(e)
        self.counters = model_counters(streams)

    @property
    def rejected(self):
        return self.expected is None

    def reads_bases(self):
        fl = self.expected >> np.uint64(56)
        short = (fl & np.uint64(2)) != 0
        ln = np.where(short, fl >> np.uint64(2), (self.expected >> np.uint64(32)) & np.uint64(0xFFFFFF))
        return int((fl & np.uint64(1)).sum()), int(ln.sum())


def lrec(colex, length, flag):
    return (colex & 0xFFFFFFFF) | ((length & 0xFFFFFF) << 32) | (flag << 56)


def srec(codes, first):
    return sum(c << (2 * i) for i, c in enumerate(codes[:28])) | (((int(first) + 2) | (len(codes) << 2)) << 56)


def block_of(lengths, seed, colex=None, short_every=9, colex_bits=20):
    """one long record per length (raw values: the record keeps their low 24 bits), a short
    record of 1..11 bases after every short_every of them and one at the end"""
    rng = random.Random(seed)
    recs = []
    for i, ln in enumerate(lengths):
        recs.append(lrec(rng.getrandbits(colex_bits) if colex is None else colex[i], ln, int(rng.random() < 0.3)))
        if i % short_every == short_every - 1 or i == len(lengths) - 1:
            recs.append(srec([rng.randrange(4) for _ in range(rng.randint(1, 11))], rng.random() < 0.3))
    return recs


def _build():
    cases = []

    def add(name, streams, **kw):
        cases.append(Case(name, streams, **kw))

    def with_s2(name, lengths, p, s2_class=None, seed=1, **kw):
        recs = block_of(lengths, seed)
        st = packer_streams(recs)
        st[1] = rice(lengths, p, **kw)
        add(name, st, intended=recs, s2_class=s2_class)
        return st

    def with_s1(name, colex, mx, seed=2, **kw):
        recs = block_of([12 + i % 5 for i in range(len(colex))], seed, colex=colex)
        st = packer_streams(recs)
        st[0] = minimal_binary(colex, mx, **kw)
        add(name, st, intended=recs)
        return st

    rng = random.Random(20261020)
    small = [rng.randint(12, 16) for _ in range(6000)]
    tiny = lambda n: [rng.randrange(8) for _ in range(n)]  # 4-bit codes at p = 3
    LONG = 2_400_000  # p = 3: a 300,004-bit code, past a 262,144-bit walk chunk

    # Rice, valid streams -- simple
    with_s2("rice_p3_small", [rng.randint(12, 40) for _ in range(3000)], 3, "simple")
    with_s2("rice_p0_zeros", [0] * 3000, 0, "simple")
    with_s2("rice_p63_wide", [rng.getrandbits(63) for _ in range(2000)], 63, "simple")
    # not-simple
    v = list(small)
    v[3000] = (1 << 24) - 1
    with_s2("rice_through_16_segments", v, 11, "not-simple")
    long_mid = None
    for where, at, cls in (("first", 0, "not-simple"), ("middle", 1500, "not-simple"), ("last", 2999, "serial")):
        v = [rng.randint(12, 40) for _ in range(3000)]
        v[at] = LONG
        st = with_s2("rice_walk_chunk_" + where, v, 3, cls)
        if where == "middle":
            long_mid = st
    v = [rng.randint(12, 40) for _ in range(3000)]
    v[1200], v[1201] = (600 - 4) << 3 | 5, (5000 - 4) << 3 | 2
    with_s2("rice_two_long_codes", v, 3, "not-simple")
    v = tiny(256) + [((3 * SEG - 4) << 3) | 6] + tiny(1000)  # bits 1024 .. 2559: segments 2, 3, 4 exactly
    with_s2("rice_long_code_fills_segments", v, 3, "not-simple")
    v = tiny(8190) + [((2000 - 4) << 3) | 1] + tiny(1000)  # bits 32,760 .. 34,759 over the 32,768-bit tile edge
    with_s2("rice_long_code_over_tile_edge", v, 3, "not-simple")
    # never synchronising
    serial_p20 = with_s2("rice_all_ones_p20", [(1 << 20) - 1] * 3000, 20, "serial")
    with_s2("rice_p62_random", [rng.getrandbits(63) for _ in range(2000)], 62, "serial")
    # stream ends
    with_s2("rice_ends_on_last_bit", tiny(3200), 3)
    with_s2("rice_63_padding_bits", tiny(1599) + [9], 3)  # 4 * 1599 + 5 = 6401 = 100 * 64 + 1 bits
    with_s2("rice_40_trailing_zero_words", [rng.randint(12, 40) for _ in range(3000)], 3, "not-simple",
            trailing=[0] * 40)
    with_s2("rice_garbage_past_num_u64", [rng.randint(12, 40) for _ in range(3000)], 3,
            extra=[rng.randrange(500) for _ in range(300)], trailing=[rng.getrandbits(64) for _ in range(3)])

    # minimal binary
    with_s1("mb_max2", [0] * 3000, 2)
    with_s1("mb_max3", [rng.randrange(2) for _ in range(3000)], 3)
    for l in (1, 20, 32, 62, 63):
        with_s1("mb_fixed_width_%d" % l, [rng.randrange((1 << l) - 1) for _ in range(3000)], 1 << l)
    for l1 in (33, 63, 64):
        with_s1("mb_all_long_%d" % l1, [rng.randrange((1 << l1) - 2) for _ in range(3000)], (1 << l1) - 1)
    col = [rng.randrange(1000) for _ in range(3000)]
    with_s1("mb_zero_code_inside", [c + 1 for c in col[:2000]] + [0] + [c + 1 for c in col[2001:]], 1 << 10, raw=True)
    with_s1("mb_zero_code_after", col, 1 << 10, extra=[-1, 5, -1])  # (v + 1 = 0 is written past num_u64)
    for mx in (0, 1):
        st = packer_streams(block_of(small[:500], 3))
        st[0].param = mx
        add("mb_max%d" % mx, st)
    shorts = [srec([rng.randrange(4) for _ in range(rng.randint(1, 11))], i % 3 == 0) for i in range(500)]
    _, _, s3v, s4v = split4(shorts)
    for name, s1 in (("mb_num_u64_zero", Stream([rng.getrandbits(64)], 0, 5)), ("mb_num_u64_zero_max0", Stream([], 0, 0))):
        add(name, [s1, Stream([], 0, 3), rice(s3v, 4), minimal_binary(s4v, max(s4v) + 2)], intended=shorts)

    # zip
    recs = block_of(small[:3000], 5)
    st = packer_streams(recs)
    st[2] = rice([(r >> 56) + 256 * rng.randrange(4) for r in recs], 5)
    add("zip_flags_past_255", st, intended=recs)
    wide1 = [rng.getrandbits(40) for _ in range(3000)]
    wide2 = [rng.getrandbits(30) for _ in range(3000)]
    recs = block_of(wide2, 6, colex=wide1)
    st = packer_streams(recs)
    st[0], st[1] = minimal_binary(wide1, 1 << 41), rice(wide2, 26)
    add("zip_values_wider_than_fields", st, intended=recs)
    recs = block_of(small, 7)  # (past one 4,096-record zip segment: the base cursor crosses it)
    recs = [r | (rng.choice([0, 4, 0x54, 0xFC]) << 56) if not (r >> 57) & 1 else r for r in recs]
    st = packer_streams(recs)
    T = sum((r >> 58) for r in recs)  # every flag's bits 2..7: the long records' too
    assert T > 31 * st[3].num_u64
    # the short records take the first bases (only they move the base cursor); the chunks the
    # long records' length bits ask for hold anything
    bn = split4(recs)[3]
    bn += [rng.getrandbits(62) for _ in range((T + 30) // 31 - len(bn))]
    st[3] = minimal_binary(bn, 1 << 63)
    add("zip_long_flags_with_length_bits", st, intended=recs)
    for L in (12, 31, 32, 33, 63):
        recs = block_of(small[:300], 8 + L)
        recs = [srec([rng.randrange(4) for _ in range(L)], r >> 56 & 1) if (r >> 57) & 1 else r for r in recs]
        if L <= 32:
            add("zip_short_%d_bases" % L, packer_streams(recs), intended=recs, packable=True)
        else:  # as_2bit takes no more than 32: chunks by hand, and only the host decoder defines the value
            bases = [rng.randrange(4) for _ in range(L * sum((r >> 57) & 1 for r in recs))]
            st = packer_streams([r for r in recs if not (r >> 57) & 1] + [srec([0], False)])
            st[2] = rice([r >> 56 for r in recs], 4)
            st[3] = minimal_binary([mk.as_2bit(bases[i:i + 31]) for i in range(0, len(bases), 31)], 1 << 63)
            add("zip_short_%d_bases" % L, st)
    recs = [lrec(5, 40, 1)] + [srec([rng.randrange(4) for _ in range(31)], i % 2) for i in range(40)]
    add("zip_T_multiple_of_31", packer_streams(recs), intended=recs, packable=True)
    recs = [lrec(rng.getrandbits(20), rng.randint(12, 16), int(i % 5 == 0)) for i in range(5000)]
    for i in range(4093, 4100):  # 20 bases each: record 4095 holds bases 40 .. 59, 4096 holds 60 .. 79 (chunk edge 62)
        recs[i] = srec([rng.randrange(4) for _ in range(20)], i % 2)
    add("zip_shorts_over_segment_edge", packer_streams(recs), intended=recs, packable=True)
    recs = [lrec(i, 12 + i % 7, i % 2) for i in range(700)]
    st = packer_streams(recs + [srec([1], False)])
    st[2] = rice([r >> 56 for r in recs], 0)
    add("zip_no_short_bases_s4_unused", st, intended=recs)

    # damage
    st = list(long_mid)
    cut = long_mid[1]
    st[1] = Stream([int.from_bytes(cut.payload[8 * i:8 * i + 8], "big") for i in range(cut.encoded_size // 2)],
                   cut.num_u64, cut.param)
    add("damaged_cut_inside_long_code", st)
    n = serial_p20[1].num_u64
    recs = block_of([(1 << 20) - 1] * (n + 1), 1)
    st = packer_streams(recs)
    st[1] = Stream([int.from_bytes(serial_p20[1].payload[8 * i:8 * i + 8], "big")
                    for i in range(serial_p20[1].encoded_size)], n + 1, 20)
    add("damaged_serial_one_value_more", st)
    st = packer_streams(block_of(small[:500], 9))
    st[1].param = 64
    add("damaged_rice_param_64", st)
    st = packer_streams(block_of(small[:500], 10))
    st[1] = rice(small[:499], 3)
    add("damaged_s1_s2_sizes_differ", st)
    st = packer_streams(block_of(small[:500], 11))
    st[3] = minimal_binary(split4(block_of(small[:500], 11))[3] + [0], st[3].param)
    add("damaged_one_chunk_too_many", st)
    recs = block_of(small[:500], 12)
    st = packer_streams(recs)
    st[0], st[1] = minimal_binary([r & 0xFFFFFFFF for r in recs if not (r >> 57) & 1][:-1], st[0].param), \
        rice(small[:499], st[1].param)
    add("damaged_long_record_past_s1", st)
    return {c.name: c for c in cases}


CASES = _build()
VALID = [n for n in CASES if not CASES[n].rejected]
REJECTED = [n for n in CASES if CASES[n].rejected]


# ---- the large block ----------------------------------------------------------------------
RICE_TILE_BITS = 64 * 512      # unpack.hip: 64 segments of 512 bits per Rice tile, restated
MB_TILE_BITS = 256 * 256       # 256 segments of 256 bits per minimal-binary tile


def large_block_records(n=600_000):
    """long records with 32-bit colex values and lengths up to 2^24 - 1, a short record every
    1000.  The lengths are exponential (mean 2^20): their Rice quotients vary, so the chains
    meet and s2 is not serial -- with uniform lengths its codes are nearly all 24 or 25 bits,
    the model says serial, and one lane would decode 600,000 codes past k_rice_scan."""
    rng = np.random.default_rng(600)
    ln = np.minimum(12 + rng.exponential(1 << 20, n).astype(np.uint64), (1 << 24) - 1).astype(np.uint64)
    ln[5] = (1 << 24) - 1
    recs = rng.integers(0, 1 << 32, n, dtype=np.uint64) | (ln << np.uint64(32)) \
        | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(56))
    L = rng.integers(1, 12, n, dtype=np.uint64)
    short = (rng.integers(0, 1 << 22, n, dtype=np.uint64) & ((np.uint64(1) << (np.uint64(2) * L)) - np.uint64(1))) \
        | ((np.uint64(2) | (L << np.uint64(2)) | rng.integers(0, 2, n, dtype=np.uint64)) << np.uint64(56))
    at = np.arange(999, n, 1000)
    recs[at] = short[at]
    return recs
