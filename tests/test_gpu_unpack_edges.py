"""GPU block unpacker (unpack.hip) on the edge cases of tests/codec_edge_lib.py: Rice streams
that are simple, not-simple (codes through whole segments, past the 8-segment limit, past a
512-segment walk chunk, over a tile edge) and never synchronising; minimal-binary streams of
1 .. 64-bit codes; zips with flags past 255, values wider than their fields, long flags with
length bits, short records of up to 63 bases; damaged streams.  Every case gives the records
of the Python restatement of src/decode.rs:51-149 (tests/test_unpack_edges.py pins the host
decoder to the same), and the path counters (ntc_ctx_get_option "unpack_rice_not_simple",
"unpack_rice_serial", "unpack_rice_through") equal the CPU model of the segment rules, so a
case is known to reach the path it was built for.

ntc_decode_fasta_unpacked needs an uploaded index (NTC_ERR_NO_INDEX without one), and records
with random colex values decode through none, so the 600,000-record block is checked by its
records alone; tests/test_gpu_unpack.py covers the FASTA text of real blocks."""
import random

import numpy as np
import pytest

import ntcomp_amd as nt
from codec_edge_lib import (CASES, MB_TILE_BITS, REJECTED, RICE_TILE_BITS, VALID, large_block_records, lrec,
                            model_counters, packer_streams, srec, Case, Stream)
from test_unpack_edges import block_of_case

pytestmark = pytest.mark.gpu

KEYS = ("unpack_rice_not_simple", "unpack_rice_serial", "unpack_rice_through")


@pytest.fixture(scope="module")
def ctx():
    c = nt.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def large():
    """the 600,000-record block: (records, (meta, payload), the model's counters)"""
    recs = large_block_records()
    meta, pay = nt.pack_block(recs, 1)
    assert meta.status == 0
    streams = [Stream([], m.num_u64, m.param, m.encoded_size) for m in meta.stream]
    for st, b in zip(streams, nt.stream_payloads(meta, pay)):
        st.payload = b
    return recs, (meta, pay), model_counters(streams)


def unpack(ctx, blocks):
    """-> (blocks ok, reads, bases, records, the three path counters)"""
    metas, payload = nt.concat_streams(blocks)
    ok, nr, nb = ctx.unpack(metas, payload, len(blocks))
    return ok, nr, nb, ctx.unpacked_records(), tuple(ctx.get_option(k) for k in KEYS)


def check_alone(ctx, c):
    ok, nr, nb, got, counters = unpack(ctx, [block_of_case(c)])
    assert counters == c.counters, (c.name, counters)
    if c.rejected:
        assert (ok, nr, nb, len(got)) == (0, 0, 0, 0), c.name
        return
    assert ok == 1 and np.array_equal(got, c.expected), c.name
    assert (nr, nb) == c.reads_bases(), c.name


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_unpack_edge_case_alone(ctx, name):
    c = CASES[name]
    check_alone(ctx, c)
    if c.host_rows:  # past 32 bases the host decoder defines the value
        host, _, _ = nt.read_block(nt.deflate_block(*block_of_case(c)))
        assert np.array_equal(ctx.unpacked_records(), host)


def test_gpu_unpack_counters_reach_every_class(ctx):
    """at least one case each: simple, not-simple with run-through segments, serial"""
    seen = set()
    for name in ("rice_p3_small", "rice_walk_chunk_middle", "rice_all_ones_p20"):
        _, _, _, _, counters = unpack(ctx, [block_of_case(CASES[name])])
        seen.add(counters[:2] + (counters[2] > 0,))
    assert seen == {(0, 0, False), (1, 0, True), (1, 1, False)}


def shuffled_valid():
    names = sorted(VALID)
    random.Random(7).shuffle(names)
    return names


def test_gpu_unpack_all_valid_cases_in_one_call(ctx):
    """blocks of 41 .. 10,213 records side by side: the output is the concatenation, the
    counters are the sums"""
    names = shuffled_valid()
    ok, nr, nb, got, counters = unpack(ctx, [block_of_case(CASES[n]) for n in names])
    assert ok == len(names)
    assert np.array_equal(got, np.concatenate([CASES[n].expected for n in names]))
    assert (nr, nb) == tuple(sum(CASES[n].reads_bases()[k] for n in names) for k in range(2))
    assert counters == tuple(sum(CASES[n].counters[k] for n in names) for k in range(3))


@pytest.mark.parametrize("bad", sorted(REJECTED))
def test_gpu_unpack_damaged_case_in_the_middle_ends_output(ctx, bad):
    names = shuffled_valid()
    mid = len(names) // 2
    order = names[:mid] + [bad] + names[mid:]
    ok, nr, nb, got, counters = unpack(ctx, [block_of_case(CASES[n]) for n in order])
    assert ok == mid
    assert np.array_equal(got, np.concatenate([CASES[n].expected for n in names[:mid]]))
    assert (nr, nb) == tuple(sum(CASES[n].reads_bases()[k] for n in names[:mid]) for k in range(2))
    assert counters == tuple(sum(CASES[n].counters[k] for n in order) for k in range(3))  # (of the whole call)


def test_gpu_unpack_workspace_reuse(ctx, large):
    """One context, streams of different classes in turn: the marks and the E / Y tables are
    reused without clearing, so a stale entry would show in the records or the counters."""
    for name in ("rice_walk_chunk_first", "rice_p3_small", "rice_all_ones_p20", "rice_p0_zeros",
                 "rice_through_16_segments", "rice_ends_on_last_bit", "rice_walk_chunk_last", "rice_p63_wide"):
        check_alone(ctx, CASES[name])
    recs, block, counters = large
    two = [lrec(7, 12, 1), srec([2], False)]
    tiny = Case("two_records", packer_streams(two), intended=two)
    for _ in range(2):
        ok, _, _, got, got_counters = unpack(ctx, [block])
        assert ok == 1 and np.array_equal(got, recs) and got_counters == counters
        check_alone(ctx, tiny)
        assert np.array_equal(ctx.unpacked_records(), np.array(two, dtype=np.uint64))


def test_gpu_unpack_large_block(ctx, large):
    """600,000 records in one block: more Rice tiles than one round of k_rice_scan's wave (64)
    and more minimal-binary tiles than two chunks of k_mb_walk (128 each), in a stream that is
    not serial -- the sizes restated here, not read from the code under test."""
    recs, (meta, pay), counters = large
    rice_tiles = -(-64 * meta.stream[1].encoded_size // RICE_TILE_BITS)
    mb_tiles = -(-64 * meta.stream[0].encoded_size // MB_TILE_BITS)
    print("large block: %d Rice tiles (s2), %d minimal-binary tiles (s1), counters %s" % (rice_tiles, mb_tiles, counters))
    assert rice_tiles > 64 and mb_tiles > 256 and counters[1] == 0
    ok, nr, nb, got, got_counters = unpack(ctx, [(meta, pay)])
    assert ok == 1 and np.array_equal(got, recs)
    fl = recs >> np.uint64(56)
    short = (fl & np.uint64(2)) != 0
    assert nr == int((fl & np.uint64(1)).sum())
    assert nb == int(np.where(short, fl >> np.uint64(2), (recs >> np.uint64(32)) & np.uint64(0xFFFFFF)).sum())
    assert got_counters == counters
    # between ordinary blocks in one call
    a, b = block_of_case(CASES["rice_p3_small"]), block_of_case(CASES["mb_all_long_64"])
    ok, _, _, got, got_counters = unpack(ctx, [a, (meta, pay), b])
    assert ok == 3
    assert np.array_equal(got, np.concatenate([CASES["rice_p3_small"].expected, recs, CASES["mb_all_long_64"].expected]))
    assert got_counters == counters
