"""Shared by tests/test_derived.py (CPU) and tests/test_gpu_derived.py: every index table the
upload derives on the device -- walk table, two-character rank chunks, suffix table levels
1..U, presence bitmaps, pair words, window words -- stated BY DEFINITION from the node set
(built as tests/golden/make_golden.py builds it: k-mers of the sequences and of their reverse
complements, dummies, root, colex order) and from the index's rows and C, in numpy, without
any of the per-entry functions the kernels and the emulator share (encode_core.h tab_make,
pair_word, win_word, rank2_make, walk_compose).  Also the loader of the TEST-ONLY shim
tests/derived_cpu, which exports what the emulator's host build derives for the same index,
the cases both tests run on, and the mismatch reports."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

import ntcomp_amd as nt
from emu_lib import _p, make_view
from oracle_lib import REPO
from subst_lib import Env, revcomp

K_TAB_SHORT = 0xFFFFFF00  # y >= K_TAB_SHORT: absent, m = y & 0xFF
K_TAB_POS = 0x80000000    # top level with path positions: y = K_TAB_POS | position
NO_NODE = 0xFFFFFFFF
WALK_SPAN = 112
FULL_MAX_U = 10           # the whole table by definition up to here; present keys alone deeper
U32, U64 = np.uint32, np.uint64


# ---- sizes (encode_core.h, restated) ---------------------------------------------------
def tab_base(u):
    return (4 ** u - 4) // 3


def tab_bits_words(U):
    return 4 ** U // 32 if U >= 3 else 1


def pair_words_count(U):
    return 4 ** (U - 1)


def win_words_count(U):
    return 4 ** (U - 3)


def rank2_blocks(n):
    return n // 32 + 2


def filter_level(U):
    return U - 2 if U >= 12 else 0


# ---- the shim ----------------------------------------------------------------------------
SHIM_SO = os.path.join(REPO, "tests", "derived_cpu", "libntc_derived_cpu.so")
ARRAYS = ("walk", "rank2", "tab", "bits", "fbits", "pair", "win", "pos", "pstream")
_shim = None


def shim():
    global _shim
    if _shim is None:
        csrc = os.path.join(REPO, "ntcomp_amd", "csrc")
        src = [os.path.join(REPO, "tests", "derived_cpu", "derived_cpu.cpp"), os.path.join(csrc, "derived.cpp")]
        deps = src + [os.path.join(REPO, "tests", "emu", "emu.cpp"), os.path.join(csrc, "derived.h"),
                      os.path.join(csrc, "encode_core.h")]
        stale = lambda: (not os.path.exists(SHIM_SO)) or any(os.path.getmtime(SHIM_SO) < os.path.getmtime(d)
                                                              for d in deps)
        if stale():
            import fcntl  # one build at a time across pytest-xdist workers (re-checked under the lock)
            with open(os.path.join(REPO, "tests", "derived_cpu", ".build.lock"), "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if stale():
                    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared",
                                    "--offload-arch=gfx950", "-o", SHIM_SO] + src, check=True,
                                   capture_output=True, text=True)
                fcntl.flock(lock, fcntl.LOCK_UN)
        L = ctypes.CDLL(SHIM_SO)
        P = ctypes.c_void_p
        L.derived_host_build.restype = ctypes.c_int
        L.derived_host_build.argtypes = [P, ctypes.c_uint32, P]
        L.derived_host_get.restype = ctypes.c_int
        L.derived_host_get.argtypes = [ctypes.c_int, P, ctypes.c_uint64]
        _shim = L
    return _shim


def host_build(ix, tab_u):
    """what the emulator's load() derives on the host for ix at depth tab_u (0: default), with
    rank chunks, pair words and window words on: dict of the arrays (uint32 words, the walk and
    rank tables by entry) and U, tab_pos, t_jump, has_paths, tlen, absent"""
    v, keep = make_view(ix.n, ix.k, ix.rows, ix.C, ix.lcs)
    info = np.zeros(8 + len(ARRAYS), dtype=U64)
    with Env(NTC_EMU_EXT2=1, NTC_EMU_WIN=1, NTC_EMU_PAIR_BYTES=1, NTC_EMU_JOINT=0):
        rc = shim().derived_host_build(ctypes.byref(v), tab_u, _p(info))
        assert rc == 0, rc
        out = dict(U=int(info[0]), tab_pos=int(info[1]), t_jump=int(info[2]), has_paths=int(info[3]),
                   tlen=int(info[4]), filt=int(info[5]), absent=int(info[6]), n=int(info[7]))
        for i, name in enumerate(ARRAYS):
            nbytes = int(info[8 + i])
            a = np.zeros(nbytes // 2 if name == "pair" else nbytes // 4, dtype=np.uint16 if name == "pair" else U32)
            if nbytes:
                rc = shim().derived_host_get(i, _p(a), nbytes)
                assert rc == 0, (name, rc)
            out[name] = a
    out["walk"] = out["walk"].view(U64).reshape(-1, 4)
    out["rank2"] = out["rank2"].reshape(-1, 16)
    out["tab"] = out["tab"].reshape(-1, 2)
    out["win"] = out["win"].reshape(-1, 8)
    return out


# ---- the node set ------------------------------------------------------------------------
class Nodes:
    """the index's nodes in colex order, from the sequences alone"""

    def __init__(self, seqs, k):
        self.k = k
        kmers = {t[i:i + k] for s in seqs for t in (s, revcomp(s)) for i in range(len(t) - k + 1)}
        suf = {x[1:] for x in kmers}
        nodes = set(kmers)
        for x in kmers:  # a k-mer no other k-mer leads to: its proper prefixes, '$'-padded
            if x[:-1] not in suf:
                for i in range(k):
                    nodes.add("$" * (k - i) + x[:i])
        nodes.add("$" * k)
        order = sorted(nodes, key=lambda s: s[::-1])  # '$' < A < C < G < T in ASCII
        self.n = n = len(order)
        lut = np.full(256, -1, dtype=np.int8)
        for i, ch in enumerate(b"ACGT"):
            lut[ch] = i
        self.cd = lut[np.frombuffer("".join(order).encode(), dtype=np.uint8).reshape(n, k)]  # -1: '$'
        self.ln = (self.cd >= 0).sum(axis=1)  # characters of the label
        assert np.all((self.cd >= 0) == (np.arange(k)[None, :] >= (k - self.ln)[:, None]))  # '$' only in front
        last = self.cd[:, k - 1]
        self.C = [1 + int((last[1:] < c).sum()) for c in range(4)] + [n]  # nodes ending with c: [C[c], C[c+1])
        self.t_jump = max(1, math.ceil(math.log(n) / math.log(4.0)) + 2)
        self._keys = {0: np.zeros(n, dtype=np.int64)}

    def keys(self, u):
        """per node, the key of its last u characters (first character in the low bits)"""
        if u not in self._keys:
            self._keys[u] = np.where(self.ln >= u, self.cd[:, self.k - u].astype(np.int64) | (self.keys(u - 1) << 2), -1)
        return self._keys[u]

    def level(self, u):
        """(keys, x, y) of the u-mers that end a label of at least u characters, by key"""
        ku = self.keys(u)
        idx = np.flatnonzero(self.ln >= u)
        kk = ku[idx]
        assert np.all(kk[1:] >= kk[:-1])  # colex order = key order among the labels long enough
        keys, first, cnt = np.unique(kk, return_index=True, return_counts=True)
        x = idx[first]
        y = x + cnt
        assert np.array_equal(idx[first + cnt - 1], y - 1)  # the nodes of a u-mer are consecutive
        return keys, x, y


@functools.lru_cache(maxsize=4)
def nodes_of(seqs, k):
    return Nodes(seqs, k)


def path_text(hb):
    """2-bit codes of the host cover's path text"""
    g = hb["pstream"].reshape(-1, 4)
    chars = g[:, 0].astype(U64) | (g[:, 1].astype(U64) << U64(32))
    sh = np.arange(32, dtype=U64) * U64(2)
    return ((chars[:, None] >> sh[None, :]) & U64(3)).astype(np.int8).reshape(-1)


# ---- the definitions ---------------------------------------------------------------------
def pack_bits(flags):
    """bit i of word i / 32"""
    if len(flags) < 32:
        return np.array([int(sum(int(b) << i for i, b in enumerate(flags)))], dtype=U32)
    return np.packbits(flags.astype(np.uint8), bitorder="little").view(U32)


class Reference:
    """the derived tables of one index at depth U, by definition"""

    def __init__(self, nd, ix, U, pos, text):
        self.nd, self.U, self.n, self.k = nd, U, nd.n, nd.k
        n, k = nd.n, nd.k
        assert n == ix.n and nd.C[:4] == ix.C[:4], (n, ix.n, nd.C, ix.C)
        self.rowbits = [np.unpackbits(r.view(np.uint8), bitorder="little")[:n] for r in ix.rows]
        # pos_of_node is the host cover's (path_hash pins it against the device): every k-mer node
        # has a position, no dummy has, and the path text there spells the node's label
        assert len(pos) == n
        real = nd.ln == k
        assert np.array_equal(pos != NO_NODE, real)
        at = pos[real].astype(np.int64)[:, None] + np.arange(k)[None, :]
        assert np.array_equal(text[at], nd.cd[real])
        self.pos = pos
        self.tab_pos = int(U >= nd.t_jump and n < 2 ** 31)  # every index here has a path cover
        self.levels = {u: nd.level(u) for u in range(1, U + 1)}
        self.full = U <= FULL_MAX_U
        self.present = {}
        for u in sorted({U, filter_level(U)} - {0}):
            f = np.zeros(4 ** u, dtype=bool)
            f[self.levels[u][0]] = True
            self.present[u] = f

    # -- suffix table ---------------------------------------------------------------
    def top_y(self, x, y):
        """second word of the top-level entries of the intervals [x, y)"""
        y = y.astype(np.int64).copy()
        if self.tab_pos:
            p = self.pos[x].astype(np.int64)
            withpos = (y == x + 1) & (p != NO_NODE)
            y[withpos] = K_TAB_POS | p[withpos]
        return y

    def level_entries(self, u):
        """level u whole: (4^u, 2) uint32"""
        keys, x, y = self.levels[u]
        ex = np.zeros(4 ** u, dtype=np.int64)
        ey = np.full(4 ** u, -1, dtype=np.int64)
        ex[keys] = x
        ey[keys] = self.top_y(x, y) if u == self.U else y
        todo = ey < 0
        allk = np.arange(4 ** u, dtype=np.int64)
        for m in range(u - 1, 0, -1):  # the longest proper suffix that is present
            mk, mx, _ = self.levels[m]
            sx = np.full(4 ** m, -1, dtype=np.int64)
            sx[mk] = mx
            s = sx[allk[todo] >> (2 * (u - m))]
            hit = np.flatnonzero(todo)[s >= 0]
            ex[hit] = s[s >= 0]
            ey[hit] = K_TAB_SHORT | m
            todo[hit] = False
        ex[todo] = 0
        ey[todo] = K_TAB_SHORT
        return np.stack([ex, ey], axis=1).astype(U32)

    def table(self):
        assert self.full
        return np.concatenate([self.level_entries(u) for u in range(1, self.U + 1)])

    def bitmap(self, u):
        return pack_bits(self.present[u])

    # -- pair words -----------------------------------------------------------------
    def pair_words(self):
        U = self.U
        keys, x, y = self.levels[U]
        single = np.zeros(4 ** U, dtype=bool)
        single[keys[y - x == 1]] = True
        pres = self.present[U]
        M = np.arange(pair_words_count(U), dtype=np.int64)
        w = np.zeros(len(M), dtype=np.int64)
        for a in range(4):  # the U-mer a.M
            key = a | (M << 2)
            w |= (pres[key].astype(np.int64) << a) | (single[key].astype(np.int64) << (8 + a))
        for c in range(4):  # the U-mer M.c
            key = M | (c << (2 * (U - 1)))
            w |= (pres[key].astype(np.int64) << (4 + c)) | (single[key].astype(np.int64) << (12 + c))
        return w.astype(np.uint16)

    # -- window words: scattered from the present U-mers --------------------------------
    def win_words(self):
        U = self.U
        assert U >= 4
        keys = self.levels[U][0]
        flags = np.zeros(win_words_count(U) * 256, dtype=bool)
        for j in range(4):  # the U-mer = (3 - j characters) . K . (j characters)
            lo = 2 * (3 - j)
            pre = keys & ((1 << lo) - 1)
            K = (keys >> lo) & (4 ** (U - 3) - 1)
            post = keys >> (2 * (U - j))
            flags[K * 256 + 64 * j + (pre | (post << lo))] = True
        return pack_bits(flags).reshape(-1, 8)

    # -- rank chunks ------------------------------------------------------------------
    def rank2(self):
        n, C = self.n, self.nd.C
        blocks = rank2_blocks(n)
        pad = [np.concatenate([r, np.zeros(96, dtype=np.uint8)]) for r in self.rowbits]
        before = [np.concatenate([[0], np.cumsum(r, dtype=np.int64)]) for r in self.rowbits]  # rank_c(i), i <= n
        sh = np.arange(32, dtype=np.int64)

        def bits32(c, p):  # row c at p .. p + 31, zero past n
            return (pad[c][p[:, None] + sh[None, :]].astype(np.int64) << sh[None, :]).sum(axis=1)

        out = np.zeros((4, blocks, 16), dtype=np.int64)
        x0 = 32 * np.arange(blocks, dtype=np.int64)
        inside = x0 <= n
        for c1 in range(4):
            base = C[c1] + before[c1][np.minimum(x0, n)]
            out[c1, :, 0] = base
            out[c1, :, 1] = np.where(inside, bits32(c1, np.minimum(x0, n)), 0)
            assert np.all(base <= n)
            for c2 in range(4):
                out[c1, :, 2 + c2] = C[c2] + before[c2][base]
                out[c1, :, 6 + c2] = bits32(c2, base)
        return out.reshape(4 * blocks, 16).astype(U32)

    # -- walk table -------------------------------------------------------------------
    def walk(self):
        n, k, C = self.n, self.k, self.nd.C
        pred = np.zeros(n, dtype=np.int64)
        code = np.zeros(n, dtype=np.int64)
        for c in range(4):  # node C[c] + r is reached from the r-th set position of row c
            at = np.flatnonzero(self.rowbits[c])
            assert len(at) == C[c + 1] - C[c]
            pred[C[c]:C[c + 1]] = at
            code[C[c]:C[c + 1]] = c
        assert pred[0] == 0 and code[0] == 0
        T = np.zeros((n, WALK_SPAN), dtype=np.int64)  # t0 .. t111, t111 = the node's last character
        cur = np.arange(n)
        for s in range(WALK_SPAN):
            T[:, WALK_SPAN - 1 - s] = code[cur]
            cur = pred[cur]
        # independently: the characters walked spell the node's own label ('$' reads as 0: the
        # walk of a dummy reaches the root and stays there)
        m = min(k, WALK_SPAN)
        assert np.array_equal(T[:, WALK_SPAN - m:], np.maximum(self.nd.cd[:, k - m:], 0))
        pack = lambda a: (a.astype(U64) << (np.arange(a.shape[1], dtype=U64) * U64(2))[None, :]).sum(axis=1, dtype=U64)
        out = np.zeros((n, 4), dtype=U64)
        out[:, 0] = pack(T[:, 80:112])
        out[:, 1] = pack(T[:, 48:80])
        out[:, 2] = pack(T[:, 16:48])
        out[:, 3] = pack(T[:, 0:16]) | (cur.astype(U64) << U64(32))
        return out

    # -- how many entries of each kind the case holds -------------------------------------
    def kinds(self):
        U = self.U
        keys, x, y = self.levels[U]
        single = y - x == 1
        haspos = self.pos[x] != NO_NODE
        out = dict(multi=int((~single).sum()), single_pos=int((single & haspos).sum()),
                   single_nopos=int((single & ~haspos).sum()), bits_set=len(keys), bits_clear=4 ** U - len(keys))
        F = filter_level(U)
        if F:
            out["fbits_set"] = len(self.levels[F][0])
            out["fbits_clear"] = 4 ** F - out["fbits_set"]
        if self.full:
            ey = self.level_entries(U)[:, 1]
            short = ey[ey >= K_TAB_SHORT] & 0xFF
            for m in range(U):
                out[f"short_m{m}"] = int((short == m).sum())
        out["pair_hi"] = int(((self.pair_words() & 0xFF00) != 0).sum())
        if U >= 4:
            w = self.win_words()
            for j in range(4):
                out[f"win_j{j}"] = int(np.unpackbits(w[:, 2 * j:2 * j + 2].copy().view(np.uint8)).sum())
        return out


# ---- mismatch reports ----------------------------------------------------------------------
def first_diff(got, exp):
    """None, or the first index (along axis 0) where two arrays of one shape differ"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    ne = got != exp
    if ne.size == 0:
        return None
    if ne.ndim > 1:
        ne = ne.reshape(len(ne), -1).any(axis=1)
    i = int(np.argmax(ne)) if len(ne) else 0
    return i if len(ne) and ne[i] else None


def tab_where(i):
    """(level, key) of entry i of the suffix table"""
    u = 1
    while tab_base(u + 1) <= i:
        u += 1
    return u, i - tab_base(u)


def check_equal(what, got, exp, where=lambda i: i):
    i = first_diff(got, exp)
    assert i is None, f"{what}: first difference at {where(i)} (index {i}): got {got[i]!r}, expected {exp[i]!r}"


def check_tables(what, got, exp, n, U):
    """every derived array of `got` against `exp` (dicts as host_build gives them), whole"""
    blocks = rank2_blocks(n)
    check_equal(f"{what}: walk entry of node", got["walk"], exp["walk"])
    check_equal(f"{what}: rank chunk (block, c1)", got["rank2"], exp["rank2"], lambda i: (i % blocks, i // blocks))
    check_equal(f"{what}: suffix table (level, key)", got["tab"], exp["tab"], tab_where)
    check_equal(f"{what}: level-{U} bitmap word (keys from)", got["bits"], exp["bits"], lambda i: 32 * i)
    check_equal(f"{what}: filter bitmap word (keys from)", got["fbits"], exp["fbits"], lambda i: 32 * i)
    check_equal(f"{what}: pair word of the {U - 1}-mer", got["pair"], exp["pair"])
    check_equal(f"{what}: window words of the {U - 3}-mer", got["win"], exp["win"])


def reference_tables(ref):
    """the Reference's arrays in host_build's layout (a full-depth case)"""
    U = ref.U
    F = filter_level(U)
    return dict(walk=ref.walk(), rank2=ref.rank2(), tab=ref.table(), bits=ref.bitmap(U),
                fbits=ref.bitmap(F) if F else np.zeros(0, dtype=U32), pair=ref.pair_words(),
                win=ref.win_words() if U >= 4 else np.zeros((0, 8), dtype=U32))


# ---- the cases -------------------------------------------------------------------------------
def contigs(seed, count, length):
    return tuple(nt.synth_genome(seed + i, length).tobytes().decode() for i in range(count))


def cg_genome(seed, length):
    """a genome over C and G only"""
    g = nt.synth_genome(seed, length)
    return (np.frombuffer(b"CG", dtype=np.uint8)[(g >> 1) & 1].tobytes().decode(),)


def strain_collection(seed, length, strains):
    g = nt.synth_genome(seed, length)
    st = nt.synth_strains(g, seed + 1, strains, 10_000)
    return tuple(t.tobytes().decode() for t in [g] + [st[i] for i in range(strains)])


@functools.lru_cache(maxsize=None)
def mod32_genomes(k=15):
    """{n % 32: genome} for residues 0, 1 and 31: a 400 bp genome shortened one base at a time
    (n is odd unless the two strands' first k-mers share a prefix, hence the search)"""
    g = nt.synth_genome(77, 400).tobytes().decode()
    found = {}
    while len(g) > 2 * k and len(found) < 3:
        r = nt.Index.build([g.encode()], k).n % 32
        if r in (0, 1, 31) and r not in found:
            found[r] = g
        g = g[1:]
    assert len(found) == 3, sorted(found)
    return found


A_SEQS = lambda: contigs(100, 6, 300)
C_SEQS = lambda: contigs(290, 24, 700)  # (a seed with 50 multi-node 12-mers)
# name -> (sequences, k, tab_u (0: the default depth), the depth expected)
CASES = {}
for u in (1, 2, 3, 4, 5, 8):
    CASES[f"A-u{u}"] = (A_SEQS, 31, u, u)
CASES["B-k8"] = (A_SEQS, 8, 8, 8)
CASES["B-k9"] = (A_SEQS, 9, 8, 8)
CASES["C-default"] = (C_SEQS, 31, 0, 10)
CASES["C-u12"] = (C_SEQS, 31, 12, 12)
CASES["D-cg"] = (lambda: cg_genome(300, 3000), 15, 0, None)
CASES["E-strains"] = (lambda: strain_collection(400, 5000, 4), 31, 0, None)
for r in (0, 1, 31):
    CASES[f"F-n%32={r}"] = (lambda r=r: (mod32_genomes()[r],), 15, 0, None)
CASES["F-n<112"] = (lambda: contigs(500, 1, 30), 11, 0, None)  # no repeated 10-mer: no cycle
CASES["F-k255"] = (lambda: contigs(600, 1, 400), 255, 0, None)

FIFTY = ("multi", "single_pos", "single_nopos", "bits_set", "bits_clear", "pair_hi", "win_j0", "win_j1", "win_j2",
         "win_j3")
# what each case is there for: kind -> the least count the reference must show
FLOORS = {
    "A-u1": dict(multi=4, bits_set=4),
    "A-u2": dict(multi=16, bits_set=16),
    "A-u3": dict(multi=50, bits_set=50),
    "A-u4": dict(multi=50, win_j0=50, win_j1=50, win_j2=50, win_j3=50),
    "A-u5": dict(multi=50, win_j0=50, win_j1=50, win_j2=50, win_j3=50),
    "A-u8": dict({k: 50 for k in FIFTY}, short_m4=50, short_m5=50, short_m6=50, short_m7=50),
    "B-k8": dict(single_pos=50, bits_clear=50, pair_hi=50),
    "B-k9": dict(single_pos=50, multi=1, pair_hi=50),
    "C-default": dict({k: 50 for k in FIFTY}, short_m7=50, short_m8=50, short_m9=50),
    "C-u12": dict({k: 50 for k in FIFTY}, fbits_set=50, fbits_clear=50),
    "D-cg": dict(short_m0=50, multi=50, bits_clear=50),
    # dummies at the top level: the strains start and end as the genome does, so there are two
    # source k-mers, each with k - U = 21 dummy labels of at least U characters, each alone
    # unless its U-mer occurs again (rare at 4^10): 42 less a few
    "E-strains": dict(multi=50, single_nopos=30, single_pos=50),
}


@functools.lru_cache(maxsize=2)
def load_case(name):
    """-> (index, Reference, host build) of a case; the floors of its kinds asserted and printed"""
    seqs_of, k, tab_u, want_u = CASES[name]
    seqs = seqs_of()
    ix = nt.Index.build([s.encode() for s in seqs], k)
    hb = host_build(ix, tab_u)
    U = hb["U"]
    assert want_u is None or U == want_u, (U, want_u)
    nd = nodes_of(seqs, k)
    ref = Reference(nd, ix, U, hb["pos"], path_text(hb))
    assert hb["has_paths"] == 1 and hb["t_jump"] == nd.t_jump and hb["tab_pos"] == ref.tab_pos
    assert hb["filt"] == filter_level(U) and hb["n"] == nd.n
    assert hb["absent"] == sum(1 << c for c in range(4) if nd.C[c + 1] == nd.C[c])
    kinds = ref.kinds()
    sizes = {a: int(hb[a].size * hb[a].itemsize) for a in ARRAYS[:7]}
    print(f"{name}: n={nd.n} k={k} U={U} t_jump={nd.t_jump} tab_pos={ref.tab_pos} kinds={kinds} bytes={sizes}")
    for kind, floor in FLOORS.get(name, {}).items():
        assert kinds[kind] >= floor, (name, kind, kinds[kind], floor)
    return ix, ref, hb
