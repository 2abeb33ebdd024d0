"""BGZF members made on the GPU (bgzf.hip): ntc_bgzf_compress with a context and
ntc_bgzf_compress_device give the bytes and the member table of the host restatement (itself held
to the plan model, zlib and gzip in test_bgzf.py), and a text decode under the context option
"bgzf_text" gives members that inflate to the plain call's text and end on record boundaries."""
import ctypes
import gzip

import numpy as np
import pytest

import bgzf_lib as bl
import names_lib as nl
import ntcomp_amd as nt

pytestmark = pytest.mark.gpu
SHAPES = bl.shapes()


@pytest.fixture(scope="module")
def ctx():
    c = nt.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    """the host restatement's answer on every shape, computed once"""
    return {name: nt.bgzf_compress(text, off) for name, (text, off) in SHAPES.items()}


def same_table(a, b):
    return len(a) == len(b) and all((a[f] == b[f]).all() for f in ("text_off", "text_bytes", "place", "bytes"))


def device_to_device(ctx, text, off):
    n = len(text)
    cap = nt.bgzf_bound(n)
    d_text, d_out = ctx.alloc(max(64, n)), ctx.alloc(max(64, cap))
    d_off = ctx.alloc(8 * len(off)) if off is not None else 0
    try:
        if n:
            ctx.h2d(d_text, np.frombuffer(text, dtype=np.uint8))
        if off is not None:
            ctx.h2d(d_off, np.ascontiguousarray(off, dtype=np.uint64).view(np.uint8))
        ctx.h2d(d_out, np.full(max(64, cap), 0x5A, dtype=np.uint8))
        table, used = ctx.bgzf_compress_device(d_text, n, d_out, cap, d_off, 0 if off is None else len(off) - 1)
        out = ctx.d2h(np.zeros(max(64, cap), dtype=np.uint8), d_out)
    finally:
        for p in (d_text, d_out, d_off):
            if p:
                ctx.free(p)
    assert (out[used:] == 0x5A).all()  # nothing is written past the members
    return out[:used].tobytes(), table


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_host_to_host(ctx, host, name):
    text, off = SHAPES[name]
    blob, table = nt.bgzf_compress(text, off, ctx=ctx)
    assert blob == host[name][0] and same_table(table, host[name][1])
    counts, last = ctx.bgzf_last()
    assert same_table(last, table)
    assert (counts["members"], counts["text_bytes"], counts["bytes"]) == (len(table), len(text), len(blob))
    n_chunks = sum(len(bl.chunks(int(t["text_bytes"]))) for t in table)
    assert counts["chunks_stored"] + counts["chunks_huffman"] + counts["chunks_matches"] == n_chunks
    if name in ("random", "largest"):
        assert counts["chunks_stored"] == n_chunks


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_device_to_device(ctx, host, name):
    text, off = SHAPES[name]
    blob, table = device_to_device(ctx, text, off)
    assert blob == host[name][0] and same_table(table, host[name][1])


def test_a_call_after_a_larger_one(ctx, host):
    """the workspaces are grown, never shrunk: a small call after a large one, and each twice"""
    for name in ("fasta", "long_between", "fasta", "R1", "plain65281", "R1", "plain0", "long_between"):
        text, off = SHAPES[name]
        blob, table = nt.bgzf_compress(text, off, ctx=ctx)
        assert blob == host[name][0] and same_table(table, host[name][1]), name


def test_refusals_launch_nothing(ctx, host):
    text, off = SHAPES["fasta"]
    with pytest.raises(nt.NtcError) as e:
        nt.bgzf_compress(text, off, ctx=ctx, cap=bl.bound(len(text)) - 1)
    assert e.value.code == 5 and e.value.needed == bl.bound(len(text))
    bad = off.copy()
    bad[3], bad[4] = bad[4], bad[3]
    with pytest.raises(nt.NtcError) as e:
        nt.bgzf_compress(text, bad, ctx=ctx)
    assert e.value.code == 1
    d_text, d_off, d_out = ctx.alloc(len(text)), ctx.alloc(8 * len(off)), ctx.alloc(bl.bound(len(text)))
    try:
        ctx.h2d(d_text, np.frombuffer(text, dtype=np.uint8))
        ctx.h2d(d_off, bad.view(np.uint8))
        ctx.h2d(d_out, np.full(bl.bound(len(text)), 0x5A, dtype=np.uint8))
        with pytest.raises(nt.NtcError) as e:
            ctx.bgzf_compress_device(d_text, len(text), d_out, bl.bound(len(text)), d_off, len(off) - 1)
        assert e.value.code == 1
        with pytest.raises(nt.NtcError) as e:
            ctx.bgzf_compress_device(d_text, len(text), d_out, bl.bound(len(text)) - 1)
        assert e.value.code == 5
        assert (ctx.d2h(np.zeros(bl.bound(len(text)), dtype=np.uint8), d_out) == 0x5A).all()
    finally:
        for p in (d_text, d_off, d_out):
            ctx.free(p)
    assert nt.bgzf_compress(text, off, ctx=ctx)[0] == host["fasta"][0]


def test_three_workgroups_take_many_rounds(ctx):
    """20 members are 40 chunks: with 3 workgroups the grid-stride loop runs 14 rounds, each
    workgroup's DfWork and token space used again and again"""
    text, off = bl.many_members(20)
    want, table = nt.bgzf_compress(text, off, ctx=ctx)
    assert len(table) == 20 and len(bl.parse(want)) == 20 and gzip.decompress(want) == text
    assert ctx.get_option("bgzf_workgroups") == 0
    ctx.set_option("bgzf_workgroups", 3)
    try:
        got, t3 = nt.bgzf_compress(text, off, ctx=ctx)
        # a mix of contents, so that stored and Huffman chunks follow one another in one workgroup
        mixed = SHAPES["random"][0][:70000] + SHAPES["fasta"][0][:90000] + SHAPES["one_byte"][0][:50000] + SHAPES["random"][0][:40000]
        m3 = nt.bgzf_compress(mixed, None, ctx=ctx)[0]
    finally:
        ctx.set_option("bgzf_workgroups", 0)
    assert got == want and same_table(t3, table)
    assert m3 == nt.bgzf_compress(mixed, None, ctx=ctx)[0] == nt.bgzf_compress(mixed)[0]


@pytest.mark.parametrize("with_offsets", [True, False])
def test_600_members_cross_the_scan_tiles(ctx, with_offsets):
    """the plan's and the layout's scans work in tiles of 256 cells / members: 600 cross two edges"""
    text, off = bl.many_members(600, with_offsets)
    blob, table = nt.bgzf_compress(text, off, ctx=ctx)
    assert len(table) == 600
    assert [(int(t["text_off"]), int(t["text_bytes"])) for t in table] == bl.plan(len(text), off)
    members = bl.parse(blob)
    assert [(p, b) for p, b, _, _ in members] == [(int(t["place"]), int(t["bytes"])) for t in table]
    assert gzip.decompress(blob) == text
    # the host restatement on the members around the tile edges (the whole text would take it seconds)
    for m in (0, 255, 256, 257, 511, 512, 599):
        a, n = int(table[m]["text_off"]), int(table[m]["text_bytes"])
        one, _ = nt.bgzf_compress(text[a:a + n])
        assert one == blob[int(table[m]["place"]):int(table[m]["place"]) + int(table[m]["bytes"])], m


# ---- text decode under "bgzf_text" ---------------------------------------------------------------
N_READS = 2000


@pytest.fixture(scope="module")
def decoder():
    genome = nt.synth_genome(28, 300_000)
    ix = nt.Index.build([genome.tobytes()], 31)
    c = nt.GpuContext(0)
    c.upload(ix)
    rng = np.random.default_rng(281)
    g = genome.tobytes()
    reads = [g[s:s + ln] for s, ln in zip(rng.integers(0, len(g) - 60, N_READS).tolist(), rng.integers(40, 61, N_READS).tolist())]
    names = [b"pair%d/%d" % (i // 2, i % 2 + 1) for i in range(N_READS)]
    quals = [bytes(rng.integers(35, 74, len(r), dtype=np.uint8)) for r in reads]
    enc = c.encode_pack_fastq(nl.make_fastq(names, reads, quals), N_READS, block_reads=512, qualities="keep", names="keep")
    yield c, enc
    c.close()


def decode(ctx, enc, kind, bgzf, window=None):
    """one batch through ntc_decode_fasta (records from the host), sized by a query first"""
    metas, payload, _, (qm, qp), (nm, npay) = enc
    arr = (nt.BlockMeta * len(metas))(*metas)
    ok, n_reads, n_bases = ctx.unpack(arr, payload, len(metas))
    assert (ok, n_reads) == (len(metas), N_READS)
    recs = ctx.unpacked_records()
    ctx.bgzf_text = bgzf
    try:
        n = ctypes.c_uint64()
        out = np.zeros(1, dtype=np.uint8)
        for attempt in range(2):
            if "named" in kind:
                ctx.set_names(nm, npay)
            if "fastq" in kind:
                ctx.set_qualities(qm, qp)
            if window is not None:
                ctx.set_window(*window)
            rc = ctx.L.ntc_decode_fasta(ctx.h, recs.ctypes.data, len(recs), n_reads, n_bases, 1, out.ctypes.data,
                                        len(out) if attempt else 0, ctypes.byref(n))
            if attempt == 0:
                assert rc == 5
                out = np.full(n.value + 32, 0x5A, dtype=np.uint8)
        assert rc == 0, ctx.L.ntc_last_error(ctx.h)
        assert (out[n.value:] == 0x5A).all()
        return out[:n.value].tobytes()
    finally:
        ctx.bgzf_text = False


def check_decode(ctx, plain, blob, place=0):
    """blob: members that inflate to plain and are cut at its record boundaries; the context's
    table from `place` on describes them"""
    counts, table = ctx.bgzf_last()
    mine = [t for t in table if place <= int(t["place"]) < place + len(blob)]
    members = bl.parse(blob)
    assert [(place + p, b) for p, b, _, _ in members] == [(int(t["place"]), int(t["bytes"])) for t in mine]
    assert gzip.decompress(blob) == plain and sum(isize for _, _, _, isize in members) == len(plain)
    at = 0
    for _, _, _, isize in members:  # a member starts where a record starts: at 0 or behind a newline, on a header line
        assert isize > 0 and (at == 0 or plain[at - 1:at] == b"\n") and plain[at:at + 1] in (b">", b"@"), at
        at += isize
    return counts, len(members)


@pytest.mark.parametrize("kind", ["fasta", "fastq", "named_fastq", "named_fasta"])
def test_decode_formats(decoder, kind):
    ctx, enc = decoder
    plain = decode(ctx, enc, kind, False)
    assert plain.count(b"\n") == N_READS * (4 if "fastq" in kind else 2)
    blob = decode(ctx, enc, kind, True)
    counts, n_members = check_decode(ctx, plain, blob)
    assert (counts["members"], counts["text_bytes"], counts["bytes"]) == (n_members, len(plain), len(blob))
    assert len(blob) < len(plain)
    # the members are the library's own for that text and its records
    starts = [0] + [i + 1 for i in range(len(plain)) if plain[i] == 10][(4 if "fastq" in kind else 2) - 1::(4 if "fastq" in kind else 2)]
    assert blob == nt.bgzf_compress(plain, np.array(starts, dtype=np.uint64))[0]
    assert decode(ctx, enc, kind, False) == plain  # and the option leaves nothing behind


def test_decode_pairs(decoder):
    ctx, enc = decoder
    ctx.paired = "nocheck"
    try:
        for kind in ("named_fastq", "fasta"):
            plain = decode(ctx, enc, kind, False)
            first = ctx.pair_split()
            parts = (plain[:first], plain[first:])
            assert parts[0].count(b"\n") == parts[1].count(b"\n") > 0
            blob = decode(ctx, enc, kind, True)
            cfirst = ctx.pair_split()
            assert 0 < cfirst < len(blob)
            c1, m1 = check_decode(ctx, parts[0], blob[:cfirst], 0)
            c2, m2 = check_decode(ctx, parts[1], blob[cfirst:], cfirst)
            assert c1["members"] == m1 + m2 and c1["text_bytes"] == len(plain) and c1["bytes"] == len(blob)
    finally:
        ctx.paired = "off"


@pytest.mark.parametrize("kind", ["named_fastq", "fasta"])
def test_decode_a_window_that_cuts_both_ends(decoder, kind):
    ctx, enc = decoder
    for window in [(700, 900), (1, N_READS - 2), (1999, 1)]:
        plain = decode(ctx, enc, kind, False, window)
        assert plain.count(b"\n") == window[1] * (4 if "fastq" in kind else 2)
        blob = decode(ctx, enc, kind, True, window)
        check_decode(ctx, plain, blob)


def test_discard_text_wins(decoder):
    ctx, enc = decoder
    metas, payload = enc[0], enc[1]
    arr = (nt.BlockMeta * len(metas))(*metas)
    ctx.unpack(arr, payload, len(metas))
    ctx.set_option("discard_text", 1)
    try:
        ctx.decode_fasta_unpacked(bgzf=True)
        assert ctx.bgzf_last()[0]["members"] == 0
    finally:
        ctx.set_option("discard_text", 0)
