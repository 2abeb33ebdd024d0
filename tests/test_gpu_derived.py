"""The index tables the upload builds on the device (k_walk_*, k_rank2, k_tab_level, k_tab_bits,
k_pair_words, k_win_words), read back through the "dev_*" test hooks, against the emulator's
host build of the same index -- whole arrays, bit for bit, the first difference decoded to
(level, key) or (block, c1) -- and, on the tables small enough to evaluate whole, against each
structure's definition (tests/derived_lib.py) directly."""
import numpy as np
import pytest

import ntcomp_amd as nt
from derived_lib import (CASES, check_equal, check_tables, filter_level, load_case, pair_words_count, rank2_blocks,
                         reference_tables, tab_base, tab_bits_words, win_words_count)

pytestmark = pytest.mark.gpu

KEYS = ("dev_walk", "dev_rank2", "dev_tab", "dev_tab_bits", "dev_filt_bits", "dev_pair_w", "dev_win_w")


@pytest.fixture(scope="module")
def ctx():
    c = nt.GpuContext(0)
    yield c
    c.close()


def upload(ctx, ix, tab_u, ext2=1, pair_bytes=1, win=-1, decode_only=0):
    for key, v in (("tab_u", tab_u), ("ext2", ext2), ("pair_bytes", pair_bytes), ("win", win), ("joint", 0),
                   ("decode_only", decode_only)):
        ctx.set_option(key, v)
    ctx.upload(ix)


def fetch(ctx, key, shape, dtype=np.uint32):
    p = ctx.get_option(key)
    assert p != 0, key
    return ctx.d2h(np.zeros(shape, dtype=dtype), p)


def device_tables(ctx, n, U):
    """the uploaded index's derived arrays, in derived_lib.host_build's layout"""
    F = filter_level(U)
    pair = fetch(ctx, "dev_pair_w", ((pair_words_count(U) + 1) // 2 * 2,), np.uint16)
    assert pair_words_count(U) % 2 == 0 or pair[-1] == 0  # an odd count: the last half word stays zero
    return dict(walk=fetch(ctx, "dev_walk", (n, 4), np.uint64), rank2=fetch(ctx, "dev_rank2", (4 * rank2_blocks(n), 16)),
                tab=fetch(ctx, "dev_tab", (tab_base(U + 1), 2)), bits=fetch(ctx, "dev_tab_bits", (tab_bits_words(U),)),
                fbits=fetch(ctx, "dev_filt_bits", (tab_bits_words(F),)) if F else np.zeros(0, dtype=np.uint32),
                pair=pair[:pair_words_count(U)],
                win=fetch(ctx, "dev_win_w", (win_words_count(U), 8)) if U >= 4 else np.zeros((0, 8), dtype=np.uint32))


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_tables_equal_host_build(ctx, name):
    ix, ref, hb = load_case(name)
    n, U = ref.n, ref.U
    upload(ctx, ix, CASES[name][2])
    assert ctx.get_option("tab_u") == U
    if U < 4:
        assert ctx.get_option("dev_win_w") == 0
    if not filter_level(U):
        assert ctx.get_option("dev_filt_bits") == 0
    dev = device_tables(ctx, n, U)
    check_tables(f"{name}, device against host build", dev, hb, n, U)
    if ref.full and U <= 8:
        check_tables(f"{name}, device against the definition", dev, reference_tables(ref), n, U)


def test_gpu_hooks_return_zero_for_what_was_not_built(ctx):
    ix, ref, hb = load_case("A-u8")
    empty = nt.GpuContext(0)
    for key in KEYS:
        with pytest.raises(nt.NtcError) as e:
            empty.get_option(key)
        assert e.value.code == 7  # NTC_ERR_NO_INDEX
    empty.close()
    upload(ctx, ix, 8, ext2=0, pair_bytes=0, win=0)
    for key in KEYS:
        assert (ctx.get_option(key) == 0) == (key in ("dev_rank2", "dev_pair_w", "dev_win_w", "dev_filt_bits")), key
    upload(ctx, ix, 8)
    full = fetch(ctx, "dev_walk", (ref.n, 4), np.uint64)
    upload(ctx, ix, 8, decode_only=1)
    for key in KEYS:
        assert (ctx.get_option(key) != 0) == (key == "dev_walk"), key
    check_equal("walk entry of node, decode_only against the full upload",
                fetch(ctx, "dev_walk", (ref.n, 4), np.uint64), full)
    check_equal("walk entry of node, decode_only against the definition", full, ref.walk())
    ctx.set_option("decode_only", 0)
