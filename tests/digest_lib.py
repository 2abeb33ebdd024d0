"""Per-block content digests and the "NTCD" side file, restated in plain Python from their
definition (include/ntcomp_codec.h, DESIGN.md "Content digests") and not from the C++: the
checker of tests/test_digest.py and tests/test_gpu_digest.py.

All arithmetic is modulo 2^64:
    mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
    h(s)  =  mix((n + 1) K0 + sum_j mix(w_j + (j + 1) K1)),  w_j = little-endian u64 of s[8j : 8j + 8], zero-padded
    D(s_0 .. s_{m-1}) = sum_i mix(h(s_i) + (i + 1) K1)
"""
import functools
import struct

import numpy as np

M = (1 << 64) - 1
K0, K1 = 0xD6E8FEB86659FD93, 0x9E3779B97F4A7C15
SEQ, SYM, QUAL, NAME = 1, 2, 4, 8
COMPONENTS = ("seq", "sym", "qual", "name")
FIELDS = ("n_reads", "n_bases", "d_seq", "d_sym", "d_qual", "d_name", "components")


def mix(x):
    x &= M
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M
    x ^= x >> 31
    return x


def _mix_np(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


@functools.lru_cache(maxsize=None)
def h(s):
    s = bytes(s)
    n = len(s)
    if n > 4096:  # the same sum, vectorised for the long reads of the GPU tests
        w = np.frombuffer(s + b"\0" * (-n % 8), dtype="<u8").astype(np.uint64)
        with np.errstate(over="ignore"):
            j = np.arange(1, len(w) + 1, dtype=np.uint64)
            inner = int(_mix_np(w + j * np.uint64(K1)).sum(dtype=np.uint64))
        return mix((n + 1) * K0 + inner)
    inner = 0
    for j in range((n + 7) // 8):
        w = int.from_bytes(s[8 * j:8 * j + 8], "little")
        inner += mix(w + (j + 1) * K1)
    return mix((n + 1) * K0 + inner)


def D(strings):
    return sum(mix(h(s) + (i + 1) * K1) for i, s in enumerate(strings)) & M


def metas(block_reads, seq, sym=None, qual=None, name=None):
    """The metas (dicts) of reads cut into blocks of block_reads: seq is the list of base
    strings as encoded; sym, qual, name the other components' strings, or None where absent."""
    comps = [seq, sym, qual, name]
    out = []
    for r0 in range(0, len(seq), block_reads):
        m = {"n_reads": len(seq[r0:r0 + block_reads]), "n_bases": sum(len(s) for s in seq[r0:r0 + block_reads]),
             "components": 0}
        for c, (key, col) in enumerate(zip(COMPONENTS, comps)):
            m["d_" + key] = D(col[r0:r0 + block_reads]) if col is not None else 0
            m["components"] |= (1 << c) if col is not None else 0
        out.append(m)
    return out


def pack_meta(m):
    return struct.pack("<6QII", m["n_reads"], m["n_bases"], m["d_seq"], m["d_sym"], m["d_qual"], m["d_name"],
                       m["components"], 0)


def file_bytes(components, k, n_nodes, ms):
    """An "NTCD" file: header of 32 bytes, one 56-byte section per block."""
    return b"NTCD" + struct.pack("<IB3xIQ8x", 1, components, k, n_nodes) + b"".join(pack_meta(m) for m in ms)


def parse_file(data):
    """-> (components, k, n_nodes, metas) of a well-formed file."""
    assert data[:4] == b"NTCD" and len(data) >= 32 and (len(data) - 32) % 56 == 0
    version, components, k, n_nodes = struct.unpack("<IB3xIQ8x", data[4:32])
    assert version == 1
    ms = []
    for at in range(32, len(data), 56):
        v = struct.unpack("<6QII", data[at:at + 56])
        assert v[7] == 0
        ms.append(dict(zip(FIELDS, v[:7])))
    return components, k, n_nodes, ms
