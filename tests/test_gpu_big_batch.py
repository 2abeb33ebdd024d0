"""One device call past 2^32 bases, and the third level of the scan.

Part A.  Host-buffer calls cut themselves into passes of 2^30 bases, so only the device entry
points and the text decode of a whole batch (how the file pipeline decodes long reads) reach the
64-bit positions the kernels carry.  The batch is big_batch_lib.py's period repeated R times in
HBM, 2^32 + 2 B bases and more; every expected value is the CPU oracle's on one period, tiled
(test_big_batch.py pins the period, its conditions and the tiling on the host).  The tests run in
file order, smallest device footprint first, each freeing what no later one needs; the peak is
about 20 GB of HBM.  No FASTQ form of the windowed text is tested: qualities for 4.3 G bases
would have to be made and packed first, which costs more than the rest of this file.

Part B.  ntc_fastq_parse scans its kept counts with scan_excl_t: 4,096^2 records are its largest
two-level scan, one more its smallest three-level one.  The expected offsets and bases are the
generator's own arrays.

The context is this module's own and is closed at the end, so the grown workspaces do not stay
with the session."""
import ctypes

import numpy as np
import pytest

import big_batch_lib as bb
import digest_lib as dl
import ntcomp_amd as nt
from big_batch_lib import BLOCK, K, TWO32
from oracle_lib import OracleIndex

pytestmark = pytest.mark.gpu
CAPACITY, FORMAT, DIGEST = 5, 8, 12
SENTINEL = 0x5A  # 'Z': no base, no newline, no digit
PAD = 64


@pytest.fixture(scope="module")
def per():
    return bb.period()


@pytest.fixture(scope="module")
def index(per):
    return nt.Index.build([per.genome], K)


@pytest.fixture(scope="module")
def ctx(index):
    c = nt.GpuContext(0)
    c.upload(index)
    yield c
    c.close()


class Dev:
    """the test's own device buffers by name: freed once, by the test that last needs them or at the end"""

    def __init__(self, ctx):
        self.ctx, self.p = ctx, {}

    def alloc(self, name, nbytes):
        self.free(name)
        self.p[name] = self.ctx.alloc(nbytes)
        return self.p[name]

    def free(self, *names):
        for n in names:
            if n in self.p:
                self.ctx.free(self.p.pop(n))

    def fill(self, name, nbytes, chunk):
        """nbytes at the buffer's start from repeated copies of chunk, at increasing addresses"""
        for at in range(0, nbytes, len(chunk)):
            self.ctx.h2d(self.p[name] + at, chunk[:min(len(chunk), nbytes - at)])


@pytest.fixture(scope="module")
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.free(*list(d.p))


@pytest.fixture(scope="module")
def want(per, index):
    """the oracle on one period, tiled: records, record offsets, read offsets of the whole batch"""
    recs, roffs = OracleIndex(index.n, K, index.rows, index.C, index.lcs).encode(per.bases, per.offs)
    all_recs, all_roffs = bb.tiled_records(recs, roffs, per.R)
    return dict(recs=recs, roffs=roffs, all_recs=all_recs, all_roffs=all_roffs,
                offs=bb.tiled_offsets(per.offs, per.B, per.R), n=per.R * per.P, total=per.R * per.B)


def _first_difference(got, exp, offs=None):
    k = min(len(got), len(exp))
    d = np.flatnonzero(got[:k] != exp[:k])
    at = int(d[0]) if len(d) else k
    where = "" if offs is None else f", read {int(np.searchsorted(offs, at, side='right')) - 1}"
    return f"{len(got)} for {len(exp)}; first difference at {at}{where}: {got[at:at + 4]} for {exp[at:at + 4]}"


def _same(got, exp, offs=None):
    assert np.array_equal(got, exp), _first_difference(got, exp, offs)


# ---- refusals at the stated limits, without the bytes ---------------------------------------------
def test_the_limits_refuse_before_anything_runs(ctx, dev):
    d = dev.alloc("tiny", 64)
    before = ctx.get_option("workspace_bytes")
    buf, offs = np.zeros(16, np.uint8), np.zeros(2, np.uint64)
    nb, bad, used, nm = ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_uint64()
    # the FASTQ parse: 4 GiB of text
    rc = ctx.L.ntc_fastq_parse(ctx.h, buf.ctypes.data, TWO32, 1, buf.ctypes.data, 16, offs.ctypes.data, ctypes.byref(nb), ctypes.byref(bad))
    assert rc == CAPACITY and "split the batch" in ctx.L.ntc_last_error(ctx.h).decode()
    rc = ctx.L.ntc_fastq_parse(ctx.h, buf.ctypes.data, TWO32 + 7, 1, buf.ctypes.data, 16, offs.ctypes.data, ctypes.byref(nb), ctypes.byref(bad))
    assert rc == CAPACITY
    # BGZF: 4 GiB of text (the capacity offered is the bound, so the size alone is refused)
    rc = ctx.L.ntc_bgzf_compress_device(ctx.h, d, TWO32, None, 0, d, nt.bgzf_bound(TWO32), None, 0, ctypes.byref(nm), ctypes.byref(used))
    msg = ctx.L.ntc_last_error(ctx.h).decode()
    assert rc == CAPACITY and "4 GiB" in msg and "split the batch" in msg
    # encode: n_reads x max_read_len = 2^38 and more
    for n_reads, max_len in [(1 << 30, 256), (1 << 31, 150), ((1 << 38) // 151 + 1, 151)]:
        assert n_reads * max_len >= 1 << 38
        rc = ctx.L.ntc_encode_batch_device(ctx.h, d, d, n_reads, max_len, d, 0, d)
        msg = ctx.L.ntc_last_error(ctx.h).decode()
        assert rc == CAPACITY and "2^38" in msg and "split the batch" in msg
    assert ctx.get_option("workspace_bytes") == before  # no workspace was sized for any of them
    dev.free("tiny")


# ---- Part B: the scan at 4,096^2 items and just past it --------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """one record more than the largest case: the scrub parses the records from the second on"""
    return bb.tiny_fastq(bb.N_LEVEL2_TAIL + 1, 11)


def _parse(ctx, text, n):
    bases = np.zeros(len(text) // 2 + 1, dtype=np.uint8)
    offs = np.zeros(n + 1, dtype=np.uint64)
    nb, bad = ctypes.c_uint64(), ctypes.c_int64(-1)
    rc = ctx.L.ntc_fastq_parse(ctx.h, text.ctypes.data, len(text), n, bases.ctypes.data, len(bases), offs.ctypes.data,
                               ctypes.byref(nb), ctypes.byref(bad))
    return rc, bases[:nb.value], offs, int(nb.value), int(bad.value)


def _scrub(ctx, tiny, n):
    """The cases are prefixes of one text, and a context keeps its workspaces: a scan that skipped a
    store would find the right word there from the case before.  So before each, the n records
    from the second on go through the same workspaces; nearly every offset of theirs differs."""
    text = tiny.text[int(tiny.starts[1]):int(tiny.starts[n + 1])]
    assert _parse(ctx, text, n)[0] == 0


@pytest.mark.parametrize("n", bb.SCAN_CASES)
def test_parse_offsets_at_the_scan_level_edges(ctx, tiny, n):
    """scan_excl_u32(kept, n) inside ntc_fastq_parse: two levels with a full second tile, three
    levels with 4,097 and with 4,098 tile sums; all n + 1 offsets and every base"""
    assert bb.scan_levels(n)[0] == (2 if n == bb.N_TWO_LEVELS else 3)
    _scrub(ctx, tiny, n)
    t = bb.tiny_cut(tiny, n)
    rc, bases, offs, nb, bad = _parse(ctx, t.text, n)
    assert (rc, bad) == (0, -1) and nb == int(t.offs[-1]) == len(t.bases)
    _same(offs, t.offs)
    _same(bases, t.bases, t.offs)


def test_a_bad_record_behind_three_scan_levels_is_named(ctx, tiny):
    n = bb.N_LEVEL2_TAIL
    t = bb.tiny_cut(tiny, n)
    r = n - 2000  # among the last 4,097 records
    rc, _, _, _, bad = _parse(ctx, bb.tiny_damage(t, r), n)
    assert rc == FORMAT and bad == r
    rc, bases, offs, _, bad = _parse(ctx, t.text, n)  # no status word is carried over
    assert (rc, bad) == (0, -1)
    _same(offs, t.offs)
    _same(bases, t.bases, t.offs)


# ---- Part A ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(ctx, dev, per, want):
    """the batch in HBM: R copies of the period at increasing addresses, and its read offsets"""
    dev.alloc("bases", want["total"] + PAD)
    dev.fill("bases", want["total"], np.tile(per.bases, 8))
    dev.alloc("offs", want["offs"].nbytes)
    ctx.h2d(dev.p["offs"], want["offs"])
    return dev


@pytest.fixture(scope="module")
def encoded(ctx, batch, want):
    """test 1's call: ntc_encode_batch_device over all R P reads, max_read_len 0 -> records in HBM"""
    n, n_recs = want["n"], len(want["all_recs"])
    batch.alloc("recs", (n_recs + PAD) * 8)
    batch.alloc("roffs", (n + 1) * 8)
    ctx.encode_device(batch.p["bases"], batch.p["offs"], n, 0, batch.p["recs"], n_recs + PAD, batch.p["roffs"])
    return ctx.encode_status()


def test_1_encode_of_the_whole_batch(ctx, encoded, batch, want):
    """one ntc_encode_batch_device call over 2^32 + 2 B bases: every record and record offset"""
    assert encoded == len(want["all_recs"])
    roffs = ctx.d2h(np.zeros(want["n"] + 1, dtype=np.uint64), batch.p["roffs"])
    _same(roffs, want["all_roffs"])
    recs = ctx.d2h(np.zeros(encoded, dtype=np.uint64), batch.p["recs"])
    _same(recs, want["all_recs"], want["all_roffs"])


def test_2_encode_with_far_offsets(ctx, batch, per, want):
    """the last two periods alone, d_offs advanced to their reads: offs[0] > 2^32, positions from 0"""
    first = want["n"] - 2 * per.P
    assert int(want["offs"][first]) > TWO32
    exp, eoffs = bb.tiled_records(want["recs"], want["roffs"], 2)
    batch.alloc("recs2", (len(exp) + 2 * PAD) * 8)
    batch.alloc("roffs2", (2 * per.P + 1) * 8)
    # Periods are alike, so test 1 left in the workspaces (packed bases, entries, record slots) just
    # what this call must make for its first 2 P reads: the 2 P reads from the second on go through
    # first, whose every slot differs (and whose records are the oracle's too)
    lo, hi = int(want["all_roffs"][1]), int(want["all_roffs"][2 * per.P + 1])
    ctx.encode_device(batch.p["bases"], batch.p["offs"] + 8 * (first - per.P + 1), 2 * per.P, 0, batch.p["recs2"],
                      len(exp) + 2 * PAD, batch.p["roffs2"])
    assert ctx.encode_status() == hi - lo
    _same(ctx.d2h(np.zeros(hi - lo, dtype=np.uint64), batch.p["recs2"]), want["all_recs"][lo:hi])
    ctx.encode_device(batch.p["bases"], batch.p["offs"] + 8 * first, 2 * per.P, 0, batch.p["recs2"], len(exp) + PAD,
                      batch.p["roffs2"])
    assert ctx.encode_status() == len(exp)
    _same(ctx.d2h(np.zeros(2 * per.P + 1, dtype=np.uint64), batch.p["roffs2"]), eoffs)
    _same(ctx.d2h(np.zeros(len(exp), dtype=np.uint64), batch.p["recs2"]), exp, eoffs)
    batch.free("recs2", "roffs2")


def test_3_decode_of_the_whole_batch(ctx, encoded, batch, per, want):
    """One ntc_decode_batch_device call on test 1's records into a buffer prefilled with 'Z'.  All
    R P + 1 read offsets are compared.  Of the 4.3 GB of bases, these regions are copied back and
    compared (big_batch_lib.check_regions): everything from offset 2^32 - B to the end; the first
    three periods, where a write truncated to 32 bits from the region past 2^32 would land; and
    every 16th period in between.  The 64 bytes behind the last base stay 'Z'."""
    batch.free("bases", "offs", "roffs")
    n, total = want["n"], want["total"]
    batch.alloc("out", total + PAD)
    batch.fill("out", total + PAD, np.full(1 << 25, SENTINEL, dtype=np.uint8))
    batch.alloc("doffs", (n + 1) * 8)
    ctx.decode_device(batch.p["recs"], encoded, batch.p["out"], total + PAD, batch.p["doffs"], n + 1)
    assert ctx.decode_status() == (n, total)
    _same(ctx.d2h(np.zeros(n + 1, dtype=np.uint64), batch.p["doffs"]), want["offs"])
    for lo, hi in bb.check_regions(per.B, per.R):
        got = ctx.d2h(np.zeros(hi - lo, dtype=np.uint8), batch.p["out"] + lo)
        assert np.array_equal(got, bb.expected_bases(per.bases, lo, hi)), (lo, hi, _first_difference(got, bb.expected_bases(per.bases, lo, hi)))
    assert (ctx.d2h(np.zeros(PAD, dtype=np.uint8), batch.p["out"] + total) == SENTINEL).all()
    batch.free("out", "doffs", "recs")


def _decode_fasta(ctx, want, out, cap):
    """ntc_decode_fasta over the whole batch's records (host buffer), first_id 1 -> (rc, *out_len)"""
    recs, got = want["all_recs"], ctypes.c_uint64()
    rc = ctx.L.ntc_decode_fasta(ctx.h, recs.ctypes.data, len(recs), want["n"], want["total"], 1,
                                out.ctypes.data if out is not None else None, cap, ctypes.byref(got))
    return rc, int(got.value)


def test_4_digests_over_decoded_bases_past_2_32(ctx, per, want):
    """what verify does: expected digests set, ntc_decode_fasta under discard_text; the last of the
    65,536-read blocks holds base 2^32 and every read past it"""
    metas = dl.metas(BLOCK, per.reads * per.R)
    assert len(metas) == -(-want["n"] // BLOCK) and int(want["offs"][(len(metas) - 1) * BLOCK]) < TWO32 < want["total"]
    exp = [nt.DigestMeta(m["n_reads"], m["n_bases"], m["d_seq"], 0, 0, 0, dl.SEQ, 0) for m in metas]
    ctx.set_option("discard_text", 1)
    try:
        ctx.decode_set_digests(exp)
        assert _decode_fasta(ctx, want, None, 0)[0] == 0
        assert [m.as_dict() for m in ctx.decode_digests()] == [m.as_dict() for m in exp]
        last = len(exp) - 1
        bad = list(exp[:last]) + [nt.DigestMeta(exp[last].n_reads, exp[last].n_bases, exp[last].d_seq ^ 1, 0, 0, 0, dl.SEQ, 0)]
        ctx.decode_set_digests(bad)
        assert _decode_fasta(ctx, want, None, 0)[0] == DIGEST
        msg = ctx.L.ntc_last_error(ctx.h).decode()
        assert f"block {last}," in msg and "component seq" in msg  # (block b's first read is read 65,536 b)
        assert [m.as_dict() for m in ctx.decode_digests()] == [m.as_dict() for m in exp]  # what was computed stands
    finally:
        ctx.set_option("discard_text", 0)


@pytest.fixture(scope="module")
def layout(per, want):
    """the text model of the whole batch under first_id 1: header bytes and text offsets of every read"""
    return bb.text_layout(np.diff(want["offs"].astype(np.int64)), 1)


def test_5_windowed_text(ctx, per, want, layout):
    """three windows of a few reads through ntc_decode_fasta: one holding the read with base 2^32,
    one wholly past it, the batch's last reads; each is the model's bytes, and the caller's buffer
    of the full size stays zero everywhere else (checked next to each window as it comes, and over
    the whole buffer once at the end)"""
    _, toffs = layout
    n, need = want["n"], int(toffs[-1])
    r232 = int(np.searchsorted(want["offs"], TWO32, side="right")) - 1
    out = np.zeros(need, dtype=np.uint8)
    for first, count in [(r232 - 1, 4), (r232 + 300, 5), (n - 3, 3)]:
        assert first + count <= n and (first > r232) == (int(want["offs"][first]) > TWO32)
        ctx.set_window(first, count)
        rc, got = _decode_fasta(ctx, want, out, need)
        assert rc == 0 and got == int(toffs[first + count] - toffs[first])
        assert out[:got].tobytes() == bb.fasta_text(per.reads, first, first + count), (first, count)
        assert not out[got:got + (1 << 20)].any()
        out[:got] = 0
    assert not out.any()


def test_6_whole_text(ctx, per, want, layout):
    """One un-windowed ntc_decode_fasta into need > 2^32 bytes.  *out_len is the model's size; header
    and sequence line are compared for every read whose text starts at or after byte 2^32 - B, for
    the reads of the first three periods, and for those of every 16th period in between
    (big_batch_lib.check_periods)."""
    _, toffs = layout
    need = int(toffs[-1])
    assert need > TWO32 + want["n"]
    out = np.empty(need, dtype=np.uint8)
    rc, got = _decode_fasta(ctx, want, out, need)
    assert rc == 0 and got == need
    for first, last in bb.check_periods(per.P, per.R, toffs, per.B):
        lo, hi = int(toffs[first]), int(toffs[last])
        assert out[lo:hi].tobytes() == bb.fasta_text(per.reads, first, last), (first, last)
