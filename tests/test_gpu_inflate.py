"""Inflate of gzip members on the GPU (inflate.hip, ntc_inflate_members with a context,
ntc_inflate_members_device): bytes, statuses and CRCs are those of the decoder's host restatement
(the same calls without a context, itself checked against zlib in test_inflate.py)."""
import zlib

import numpy as np
import pytest

import ntcomp_amd as nt
import inflate_lib as il
from test_codec_golden import CASES, recs_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = nt.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    """the sound and the damaged members, mixed, with the host restatement's answer, computed once"""
    good, bad = il.all_sound(), il.damaged()
    members, claimed, names = [], [], []
    for i in range(max(len(good), len(bad))):
        if i < len(good):
            members.append(good[i][1]), claimed.append(len(good[i][2])), names.append(good[i][0])
        if i < len(bad):
            members.append(bad[i][1]), claimed.append(bad[i][2]), names.append(bad[i][0])
    outs, res = il.run_all(None, members, claimed)
    return names, members, claimed, outs, res


def same(res, want):
    return all((res[f] == want[f]).all() for f in ("status", "out_bytes", "crc", "reserved"))


def test_the_corpus_in_one_call(ctx, corpus):
    """sound and damaged members side by side: the host's bytes, statuses and CRCs, and (run_all)
    not a byte written between the outputs or inside a failed member's place"""
    names, members, claimed, outs, res = corpus
    got, gres = il.run_all(ctx, members, claimed)
    for n, a, b, ra, rb in zip(names, got, outs, gres, res):
        assert ra["status"] == rb["status"], (n, nt.INFLATE_STATUS[int(ra["status"])], nt.INFLATE_STATUS[int(rb["status"])])
        assert a == b and ra["crc"] == rb["crc"] and ra["out_bytes"] == rb["out_bytes"], n
    for n, m, d in il.all_sound():
        i = names.index(n)
        assert got[i] == d and gres[i]["crc"] == zlib.crc32(d)
    assert {int(s) for s in gres["status"]} == set(range(10))


def test_calls_of_one_member(ctx, corpus):
    names, members, claimed, outs, res = corpus
    for n, m, c, o, r in zip(names, members, claimed, outs, res):
        out = np.full(c + 64, 0x5A, dtype=np.uint8)
        got, gres = nt.inflate_members(ctx, m, [(0, len(m), c, 32)], out=out)
        assert same(gres, res[names.index(n):names.index(n) + 1]), n
        if r["status"] == 0:
            assert got[32:32 + c].tobytes() == o, n
            got[32:32 + c] = 0x5A
        assert (got == 0x5A).all(), n


def test_mutants_get_the_hosts_statuses(ctx):
    """a fixed subset of 256 mutants in one call, then the same context again with sound members
    alone: the tables, queues and windows of a failed member are not carried over"""
    ms = il.mutants()[::7][:256]
    assert len(ms) == 256
    members, claimed = [m for _, m in ms], [il.claimed_of(m) for _, m in ms]
    outs, res = il.run_all(None, members, claimed)
    got, gres = il.run_all(ctx, members, claimed)
    assert same(gres, res) and got == outs
    assert (res["status"] != 0).sum() > 150
    good = il.all_sound()[:40]
    g2, r2 = il.run_all(ctx, [m for _, m, _ in good], [len(d) for _, _, d in good])
    assert (r2["status"] == 0).all() and g2 == [d for _, _, d in good]


def test_device_to_device(ctx, corpus):
    names, members, claimed, outs, res = corpus
    blob, m, cap = il.layout(members, claimed)
    d_comp, d_dst = ctx.alloc(len(blob)), ctx.alloc(cap)
    try:
        ctx.h2d(d_comp, np.frombuffer(blob, dtype=np.uint8))
        ctx.h2d(d_dst, np.full(cap, 0x3C, dtype=np.uint8))
        gres = ctx.inflate_members_device(d_comp, len(blob), m, d_dst, cap)
        out = ctx.d2h(np.zeros(cap, dtype=np.uint8), d_dst)
        with pytest.raises(nt.NtcError) as e:  # the refusals hold on this path too: nothing is launched
            ctx.inflate_members_device(d_comp, 100, [(0, 50, 10, 0), (50, 50, 10, 9)], d_dst, 100)
        assert e.value.code == 1
        assert (ctx.d2h(np.zeros(cap, dtype=np.uint8), d_dst) == out).all()
    finally:
        ctx.free(d_comp)
        ctx.free(d_dst)
    assert same(gres, res)
    mask = np.ones(cap, dtype=bool)
    for d, r, o in zip(m, res, outs):
        a, b = int(d["dst_off"]), int(d["dst_off"]) + int(d["out_bytes"])
        if r["status"] == 0:
            assert out[a:b].tobytes() == o
            mask[a:b] = False
    assert (out[mask] == 0x3C).all()


def test_round_trip_behind_the_device_deflate(ctx):
    """the streams of the codec fixtures' blocks through ntc_deflate_blocks_device and, without
    leaving the device, through this inflater: back come the streams (those of at most 64 KiB)"""
    seen = 0
    for name in sorted(n for n in CASES if not CASES[n]["dropped"]):
        c = CASES[name]
        meta, payload = nt.pack_block(recs_of(c), c["num_records"])
        raw = nt.stream_payloads(meta, payload)
        cap = sum(18 + len(r) + 5 * -(-len(r) // 32768) + 5 for r in raw)
        d_pay, d_mem, d_out = ctx.alloc(max(64, len(payload))), ctx.alloc(cap), ctx.alloc(max(64, len(payload)))
        try:
            ctx.h2d(d_pay, np.frombuffer(payload, dtype=np.uint8))
            off_len, used = ctx.deflate_device(d_pay, [meta], d_mem, cap)
            pick = [s for s in range(4) if len(raw[s]) <= il.MAX_OUT]
            descs = [(int(off_len[0, s, 0]), int(off_len[0, s, 1]), len(raw[s]), int(meta.stream[s].offset)) for s in pick]
            res = ctx.inflate_members_device(d_mem, used, descs, d_out, len(payload))
            back = ctx.d2h(np.zeros(max(64, len(payload)), dtype=np.uint8), d_out)
        finally:
            for p in (d_pay, d_mem, d_out):
                ctx.free(p)
        assert (res["status"] == 0).all(), name
        for s, r in zip(pick, res):
            o = int(meta.stream[s].offset)
            assert back[o:o + len(raw[s])].tobytes() == raw[s] and r["crc"] == zlib.crc32(raw[s]), (name, s)
            seen += 1
    assert seen >= 4 * 10
