"""Shared by tests/test_subst.py (CPU) and tests/test_gpu_subst.py: the loader of the
TEST-ONLY shim tests/subst_cpu (the host emulation tests/emu/emu.cpp compiled with the
NTC_STAT counters on, plus the host-built path stream), a direct evaluation of the
substitution word's definition (encode_core.h subst_clean) from the set of k-mers, and the
read shapes the substitution shortcut is tested on."""
import ctypes
import math
import os
import subprocess

import numpy as np

import ntcomp_amd as nt
from emu_lib import _p, make_view
from oracle_lib import REPO, pack_reads

COMP = str.maketrans("ACGT", "TGCA")
SHIM_SO = os.path.join(REPO, "tests", "subst_cpu", "libntc_subst_cpu.so")
_shim = None


def revcomp(s):
    return s.translate(COMP)[::-1]


def shim():
    global _shim
    if _shim is None:
        csrc = os.path.join(REPO, "ntcomp_amd", "csrc")
        src = [os.path.join(REPO, "tests", "subst_cpu", "subst_cpu.cpp"), os.path.join(csrc, "derived.cpp")]
        deps = src + [os.path.join(REPO, "tests", "emu", "emu.cpp"), os.path.join(csrc, "derived.h"),
                      os.path.join(csrc, "encode_core.h")]
        stale = lambda: (not os.path.exists(SHIM_SO)) or any(os.path.getmtime(SHIM_SO) < os.path.getmtime(d)
                                                              for d in deps)
        if stale():
            import fcntl  # one build at a time across pytest-xdist workers (re-checked under the lock)
            with open(os.path.join(REPO, "tests", "subst_cpu", ".build.lock"), "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if stale():
                    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared",
                                    "--offload-arch=gfx950", "-DNTC_STATS", "-o", SHIM_SO] + src, check=True,
                                   capture_output=True, text=True)
                fcntl.flock(lock, fcntl.LOCK_UN)
        L = ctypes.CDLL(SHIM_SO)
        P, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.emu_encode.restype = ctypes.c_int
        L.emu_encode.argtypes = [P, P, P, u64, P, u64, P, P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.subst_host_words.restype = ctypes.c_int
        L.subst_host_words.argtypes = [P, ctypes.c_uint32, P, u64, P]
        L.subst_stats.argtypes = [P]
        _shim = L
    return _shim


class Env:
    """environment of one emulator call (the emulator reads it at every call)"""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def host_words(ix, k, tab_u=0, subst=1):
    """-> dict(text, end, word (one 0/1 per text position), U, tab_pos, t_jump, hash)"""
    v, keep = make_view(ix.n, k, ix.rows, ix.C, ix.lcs)
    cap = 4 * ((ix.n * (k + 1) + k) // 32 + 16)  # a path per node at the most
    out = np.zeros(cap, dtype=np.uint32)
    info = np.zeros(6, dtype=np.uint64)
    with Env(NTC_EMU_JOINT=0, NTC_SUBST=subst):
        rc = shim().subst_host_words(ctypes.byref(v), tab_u, _p(out), cap, _p(info))
    assert rc == 0, rc
    groups, tlen = int(info[0]), int(info[1])
    g = out[: 4 * groups].reshape(groups, 4)
    chars = g[:, 0].astype(np.uint64) | (g[:, 1].astype(np.uint64) << np.uint64(32))
    sh = np.arange(32, dtype=np.uint64) * np.uint64(2)
    codes = ((chars[:, None] >> sh[None, :]) & np.uint64(3)).astype(np.uint8).reshape(-1)
    bit = np.arange(32, dtype=np.uint32)
    end = ((g[:, 2][:, None] >> bit[None, :]) & 1).astype(np.uint8).reshape(-1)
    word = ((g[:, 3][:, None] >> bit[None, :]) & 1).astype(np.uint8).reshape(-1)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes().decode()
    return dict(text=text, end=end, word=word, tlen=tlen, U=int(info[2]), tab_pos=int(info[3]),
                t_jump=int(info[4]), hash=int(info[5]))


def brute_words(genome, k, hw):
    """clean(t) for every text position, from the definition and the set of k-mers"""
    U, text, end, tlen = hw["U"], hw["text"], hw["end"], hw["tlen"]
    out = np.zeros(len(hw["word"]), dtype=np.uint8)
    seqs = [genome, revcomp(genome)]
    kmers = {s[i:i + k] for s in seqs for i in range(len(s) - k + 1)}
    n_nodes = None
    # the index's nodes: the k-mers, and for a k-mer no other k-mer leads to, its proper prefixes
    suf = {x[1:] for x in kmers}
    dummies = {x[:i] for x in kmers if x[:-1] not in suf for i in range(1, k)}
    n_nodes = 1 + len(kmers) + len(dummies)
    assert hw["t_jump"] == max(1, math.ceil(math.log(n_nodes) / math.log(4.0)) + 2)
    if not (U >= 4 and U >= hw["t_jump"]):  # tab_pos: the table carries no path positions
        assert hw["tab_pos"] == 0
        return out
    assert hw["tab_pos"] == 1
    present = {x[i:i + U] for x in kmers for i in range(k - U + 1)}
    ends_with = {}  # nodes by their U-suffix
    for x in list(kmers) + [y for y in dummies if len(y) >= U]:
        ends_with[x[-U:]] = ends_with.get(x[-U:], 0) + 1
    run = np.zeros(len(end) + 1, dtype=np.int64)  # run[t] = consecutive set end bits ending at t - 1
    for t in range(len(end)):
        run[t + 1] = run[t] + 1 if end[t] else 0
    for t in range(1, tlen - U - 1):
        if run[t + U + 2] < U + 3:  # end bits at t - 1 .. t + U + 1
            continue
        if ends_with.get(text[t + 1:t + U + 1], 0) != 1:
            continue
        ok = True
        for a in "ACGT":
            if a == text[t]:
                continue
            s = text[t - U + 1:t] + a + text[t + 1:t + U + 1]
            P = [s[i:i + U] in present for i in range(U)]
            if P[0] or P[U - 1] or any(P[i] and P[i + 1] for i in range(U - 1)):
                ok = False
                break
        out[t] = ok
    return out


def emu_run(ix, k, reads, subst):
    bases, offs = pack_reads(reads)
    v, keep = make_view(ix.n, k, ix.rows, ix.C, ix.lcs)
    total = int(offs[-1])
    recs = np.zeros(total + 1, dtype=np.uint64)
    roff = np.zeros(len(offs), dtype=np.uint64)
    d = np.zeros(total + 1, dtype=np.uint32)
    s = np.zeros(total + 1, dtype=np.uint32)
    bad = ctypes.c_int64(-1)
    st = np.zeros(16, dtype=np.uint64)
    with Env(NTC_EMU_JOINT=0, NTC_SUBST=subst):
        shim().subst_stats(_p(st))
        rc = shim().emu_encode(ctypes.byref(v), _p(bases), _p(offs), len(offs) - 1, _p(recs), len(recs), _p(roff),
                             ctypes.byref(bad), _p(d), _p(s), 4, 1, 0)
        shim().subst_stats(_p(st))
    assert rc == 0, (rc, bad.value)
    return recs[: int(roff[-1])], roff, d[:total], s[:total], int(st[13]), int(st[14])


def sub(read, i, rng=None):
    """read with another base at i"""
    c = "ACGT"[("ACGT".index(read[i]) + (1 if rng is None else int(rng.integers(1, 4)))) % 4]
    return read[:i] + c + read[i + 1:]


def repeat_genome(seed, k):
    """random sequence with a repeated block longer than k: the path cover breaks around it"""
    parts = [nt.synth_genome(seed + i, n).tobytes().decode() for i, n in enumerate((6000, 7000, 7000))]
    rep = nt.synth_genome(seed + 9, k + 40).tobytes().decode()
    return parts[0] + rep + parts[1] + rep + parts[2]


def text_reads(hw, k, L, want):
    """(read, text position of its first character) for windows of one path's text with the
    text position `want(t)` picks inside"""
    end, text = hw["end"], hw["text"]
    run = np.zeros(len(end) + 1, dtype=np.int64)
    for t in range(len(end)):
        run[t + 1] = run[t] + 1 if end[t] else 0
    out = []
    for a in range(0, hw["tlen"] - L, 7):
        if run[a + L] >= L:  # a k-mer ends at every position of the window: inside one path
            t = want(a)
            if t is not None:
                out.append((text[a:a + L], a, t))
    return out


def shape_reads(genome, k, U, L, n, seed, rep0=6000):
    """n reads of the shapes the shortcut must survive, every other one reverse-complemented,
    and reads over the edges of repeat_genome's repeated block at rep0 (a path end)"""
    rng = np.random.default_rng(seed)
    reads = []
    G = len(genome)
    for i in range(n):
        a = int(rng.integers(0, G - L))
        r = genome[a:a + L]
        p = int(rng.integers(k + 5, L - 2 * U - 8)) if L - 2 * U - 8 > k + 5 else L // 2
        kind = i % 13
        if kind < 4:  # two substitutions U - 1, U, U + 1, U + 2 apart
            r = sub(sub(r, p, rng), p + U - 1 + kind, rng)
        elif kind == 4:  # within U + 1 of the read's end
            r = sub(r, L - 1 - int(rng.integers(0, U + 2)), rng)
        elif kind == 5:  # within U of its start
            r = sub(r, int(rng.integers(0, U + 1)), rng)
        elif kind == 6:  # insertion
            r = (r[:p] + "ACGT"[int(rng.integers(0, 4))] + r[p:])[:L]
        elif kind == 7:  # deletion
            r = r[:p] + r[p + 1:]
        elif kind == 8:  # three substitutions in a row of windows
            r = sub(sub(sub(r, p, rng), p + U + 1, rng), p + 2 * U + 2, rng)
        elif kind == 9:  # substitution then deletion
            r = sub(r, p, rng)
            r = r[:p + U + 3] + r[p + U + 4:]
        elif kind == 10:  # lone, late in a long run
            r = sub(r, L - U - 4, rng)
        elif kind == 11:  # error free
            pass
        else:  # many
            for _ in range(6):
                r = sub(r, int(rng.integers(0, len(r))), rng)
        reads.append(revcomp(r) if i % 2 else r)
    # reads crossing a path end: windows over the edges of the repeated block
    for off in range(-L + 5, k + 40, 9):
        a = rep0 + off
        r = genome[a:a + L]
        reads.append(sub(r, L // 2) if off % 2 else r)
        reads.append(revcomp(sub(r, L // 3)))
    return reads


def lone_reads(hw, k, L):
    """reads of one path's text with one substitution each, at text positions = 0, 31, 1
    (mod 32: the bit at a group-word edge; 32 is 0 of the next group), 5 and 17, after a run
    of more than 64 characters; and how many of those positions are clean"""
    U = hw["U"]
    reads, clean = [], 0
    for res in (0, 31, 1, 5, 17):  # (32 = 0 of the next group: residues 31 and 0 are both edges)
        def want(a, res=res):
            t = a + k + 70 + (res - (a + k + 70)) % 32
            return t if t + U + 2 < a + L else None
        picks = text_reads(hw, k, L, want)
        picks = picks[:: max(1, len(picks) // 60)][:60]
        for read, a, t in picks:
            reads.append(sub(read, t - a))
            clean += int(hw["word"][t])
    return reads, clean
