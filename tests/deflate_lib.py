"""What the tests of `--deflate gpu` share: the size and content list, the checkers (Python's
zlib), the stream wrapper around ntc_deflate_stream, and the small C91-shaped block.

C, B and the member's shape are restated here from ntcomp_amd/csrc/deflate_core.h and DESIGN.md
§26; the tests fail if the two drift apart."""
import ctypes
import struct
import zlib

import numpy as np

import ntcomp_amd as nt

C = 32768          # kDfChunk
B = 5              # kDfB
GZ_HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])
ENGINE_GPU = 3     # NTC_DEFLATE_GPU

# the sizes of the issue, in bytes; the last three are the stored-block limit
SIZES = [0, 1, 2, 3, 4, C - 1, C, C + 1, 2 * C, 2 * C + 1, 65535, 65536, 65537]
# A stream of the container is whole 64-bit words, so the C ABI (and the device call, which
# takes block metas) can carry multiples of 8 only.  Through them every size above goes that is
# one, and for each other one the multiples of 8 next to it on both sides; the byte-exact list
# runs through the stand-alone program, which takes any size.
WORD_SIZES = sorted({s for x in SIZES for s in ((x // 8) * 8, -(-x // 8) * 8)})

SUB, MULTI = 4096 + 8, 2 * C + 4096 + 8  # one size inside a chunk, one over several


def bound(n):
    return 18 + n + B * -(-n // C) + 5


def _rng(seed):
    return np.random.default_rng(seed)


def content(kind, n, seed=7):
    """n bytes of the named kind"""
    r = _rng(seed)
    if kind == "zero":
        a = np.zeros(n, np.uint8)
    elif kind == "two":
        a = r.integers(0, 2, n, dtype=np.uint8) * 0xA5
    elif kind == "all256":
        a = np.resize(np.arange(256, dtype=np.uint8), n)
        r.shuffle(a)
    elif kind == "random":
        a = r.integers(0, 256, n, dtype=np.uint8)
    elif kind == "fib":  # frequencies follow the Fibonacci numbers over 28 symbols
        f = [1, 1]
        while len(f) < 28:
            f.append(f[-1] + f[-2])
        p = np.array(f, np.float64)
        reps = np.maximum(1, np.floor(p / p.sum() * n)).astype(np.int64)
        a = np.repeat(np.arange(28, dtype=np.uint8) + 40, reps)
        a = np.resize(a, n)
        r.shuffle(a)
    elif kind.startswith("period"):
        p = int(kind[6:])
        a = np.resize(r.integers(0, 256, p, dtype=np.uint8), n)
    elif kind.startswith("repeat"):  # a random block, random filler, the block again `dist` later
        dist = int(kind[6:])
        a = r.integers(0, 256, n, dtype=np.uint8)
        if n > dist:
            k = min(300, n - dist)
            a[dist:dist + k] = a[:k]
    elif kind == "straddle":  # a repeat whose copy runs over the chunk boundary
        a = r.integers(0, 256, n, dtype=np.uint8)
        if n > C + 100:
            a[C - 100:C + 100] = a[C - 400:C - 200]
    elif kind == "far":  # a random block, zeros, the block again C - 300 later: nothing takes its buckets,
        a = np.zeros(n, np.uint8)  # so the copy is found, at a distance of the last distance code
        a[:300] = r.integers(1, 256, 300, dtype=np.uint8)
        if n >= C:
            a[C - 300:C] = a[:300]
    elif kind == "one3":  # random bytes, one 3-byte string twice
        a = r.integers(0, 256, n, dtype=np.uint8)
        if n > 1000:
            a[900:903] = a[100:103]
    else:
        raise ValueError(kind)
    return a.tobytes()


KINDS = (["zero", "two", "all256", "random", "fib", "one3"] + ["period%d" % p for p in (1, 2, 3, 4, 257, 258, 259)]
         + ["repeat32768", "repeat%d" % (C - 1), "far", "straddle"])


def cases():
    """(name, bytes) for the whole size x content list, sizes in bytes"""
    out = [("size%d" % n, content("random" if n % 2 else "fib", n, seed=n)) for n in SIZES]
    for k in KINDS:
        for n in (SUB, MULTI):
            if (k.startswith("repeat") or k == "far") and n == SUB:
                n = C  # the far distances need a whole chunk
            out.append(("%s-%d" % (k, n), content(k, n)))
    return out


def word_cases():
    """the same for the interfaces that carry whole words"""
    out = [("size%d" % n, content("random" if (n // 8) % 2 else "fib", n, seed=n)) for n in WORD_SIZES]
    return out + [c for c in cases() if not c[0].startswith("size")]


def check_member(member, data):
    """one gzip member, consumed whole, that inflates to data: header, CRC-32 and ISIZE (zlib
    checks both), exactly one member, and the size bound"""
    assert member[:10] == GZ_HEADER
    assert zlib.decompress(member, 31) == data
    d = zlib.decompressobj(-15)
    got = d.decompress(member[10:])
    assert got == data and d.eof and len(d.unused_data) == 8
    assert struct.unpack("<II", d.unused_data) == (zlib.crc32(data), len(data) & 0xFFFFFFFF)
    assert len(member) <= bound(len(data))


def all_stored(member, n):
    """the member of n bytes whose every chunk is stored: its exact size"""
    return len(member) == 18 + n + 5 * max(1, -(-n // C))


def meta_for(sizes_words):
    """a block meta over four streams of the given word counts laid back to back"""
    m = nt.BlockMeta()
    off = 0
    for s, w in enumerate(sizes_words):
        m.stream[s].num_u64 = w
        m.stream[s].encoded_size = w
        m.stream[s].param = 3
        m.stream[s].offset = off
        off += 8 * w
    m.num_records = 1
    m.n_recs = 1
    m.status = 0
    return m, off


def deflate_stream_rc(meta, stream, payload, engine):
    """ntc_deflate_stream -> (rc, bytes)"""
    buf = np.frombuffer(payload, dtype=np.uint8) if len(payload) else np.zeros(8, np.uint8)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    rc = nt.lib().ntc_deflate_stream(ctypes.byref(meta), stream, buf.ctypes.data_as(ctypes.c_void_p), engine,
                                     ctypes.byref(out), ctypes.byref(n))
    data = ctypes.string_at(out, n.value) if rc == 0 else b""
    if out:
        nt.lib().ntc_buffer_free(out)
    return rc, data


def member_of(data, engine=ENGINE_GPU):
    """the gzip member ntc_deflate_stream makes of data (a multiple of 8 bytes) as stream 0"""
    assert len(data) % 8 == 0
    meta, _ = meta_for([len(data) // 8, 0, 0, 0])
    rc, part = deflate_stream_rc(meta, 0, data, engine)
    assert rc == 0, "ntc_deflate_stream: %d" % rc
    assert struct.unpack("<I", part[:4])[0] == len(part) - 32  # BlockHeader.block_size
    return part[32:]


def c91_block(n_reads=8192, genome=200_000):
    """the small C91-shaped block: meta and payload of the host packer over the oracle's records"""
    from oracle_lib import OracleIndex
    g = nt.synth_genome(1, genome)
    ix = nt.Index.build([g.tobytes()], 91)
    reads = nt.synth_reads(g, 2, 0, n_reads, 150, 10_000)
    offs = np.arange(0, n_reads * 150 + 1, 150, dtype=np.uint64)
    recs, _ = OracleIndex(ix.n, 91, ix.rows, ix.C, ix.lcs).encode(reads, offs)
    return nt.pack_block(recs, n_reads)
