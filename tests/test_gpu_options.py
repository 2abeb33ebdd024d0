"""The context's option table (capi.cpp kOptions), on a fresh context without an index: every
settable key takes its minimum and its maximum and returns them, refuses the value below and
the value above with NTC_ERR_INVALID_ARG and its own message, and an unknown key is named in
the error.  The rows restate the table's keys, ranges and messages: a key added to one and not
the other shows up in the last test.  (A context needs a device, so the module is marked gpu;
no kernel runs.)"""
import ctypes

import pytest

import ntcomp_amd as nt

pytestmark = pytest.mark.gpu

INVALID_ARG, NO_INDEX = 1, 7
I64_MAX = 2 ** 63 - 1
# key, min, max, message; the values in between that the key's rule also refuses
PLAIN = [
    ("encode_variant", 1, 4, "encode_variant must be 4 (default) or 1 (A/B baseline)", [2, 3]),
    ("tab_u", 0, 15, "tab_u must be 0 (default) or 1..15", []),
    ("pair_bytes", 0, 1, "pair_bytes must be 0 or 1", []),
    ("filter", -1, 1, "filter must be -1 (auto), 0 or 1", []),
    ("joint", -1, 1, "joint must be -1 (auto), 0 or 1", []),
    ("path_link", 0, 1, "path_link must be 0 or 1", []),
    ("win", -1, 1, "win must be -1 (auto), 0 or 1", []),
    ("subst", -1, 0, "subst must be -1 (auto) or 0", []),
    ("decode_only", 0, 1, "decode_only must be 0 or 1", []),
    ("ext2", 0, 1, "ext2 must be 0 or 1", []),
    ("max_pass_bases", 1, I64_MAX, "max_pass_bases must be >= 1", []),
    ("qualities", 0, 2, "qualities must be 0 (drop), 1 (keep) or 2 (bin8)", []),
    ("quality_coder", 0, 1, "quality_coder must be 0 (pack) or 1 (rans)", []),
    ("names", 0, 2, "names must be 0 (drop), 1 (keep) or 2 (id)", []),
    ("discard_text", 0, 1, "discard_text must be 0 or 1", []),
    ("paired", 0, 2, "paired must be 0 (off), 1 (ids) or 2 (no check)", []),
    ("digests", 0, 1, "digests must be 0 or 1", []),
    ("non_acgt", 0, 2, "non_acgt must be 0 (error), 1 (mask) or 2 (keep)", []),
]
# settable keys whose getter is not the stored value: ent_slots returns what 0 (auto) stands
# for (4 without joint runs); the test hook pool_per_read and the action warm_dma have none
ENT_SLOTS = ("ent_slots", 0, 1024, "ent_slots must be 0 (auto) or a multiple of 4 up to 1024", [1, 2, 3, 1022])
WRITE_ONLY = [("pool_per_read", 0, I64_MAX, "pool_per_read must be >= 0"),
              ("warm_dma", 1, 1 << 30, "warm_dma: 1 .. 2^30 bytes")]
READ_ONLY = ["filter_density_ppm", "n_paths", "path_text_len", "upload_host_us", "upload_total_us", "tab_u_fallback",
             "pack_us", "spill_reruns", "nx_sub", "nx_runs", "nx_bases", "unpack_rice_not_simple", "unpack_rice_serial",
             "unpack_rice_through", "pool_entries", "pool_records", "workspace_bytes"]
NEED_INDEX = ["subst_hash", "path_hash", "dev_walk", "dev_rank2", "dev_tab", "dev_tab_bits", "dev_filt_bits", "dev_pair_w",
              "dev_win_w"]


@pytest.fixture()
def ctx():
    c = nt.GpuContext(0)
    yield c
    c.close()


def _set(ctx, key, value):
    rc = ctx.L.ntc_ctx_set_option(ctx.h, key.encode(), value)
    return rc, ctx.L.ntc_last_error(ctx.h).decode()


def _get(ctx, key):
    v = ctypes.c_int64(-12345)
    return ctx.L.ntc_ctx_get_option(ctx.h, key.encode(), ctypes.byref(v)), int(v.value)


def _refused(ctx, key, lo, hi, msg, inside):
    for bad in [lo - 1] + ([hi + 1] if hi < I64_MAX else []) + inside:
        assert _set(ctx, key, bad) == (INVALID_ARG, msg), (key, bad)


@pytest.mark.parametrize("key,lo,hi,msg,inside", PLAIN, ids=[r[0] for r in PLAIN])
def test_plain_option_takes_its_range_and_returns_it(ctx, key, lo, hi, msg, inside):
    for v in (lo, hi):
        assert _set(ctx, key, v)[0] == 0, (key, v)
        assert _get(ctx, key) == (0, v)
    _refused(ctx, key, lo, hi, msg, inside)
    assert _get(ctx, key) == (0, hi)  # a refused value changes nothing


def test_ent_slots(ctx):
    key, lo, hi, msg, inside = ENT_SLOTS
    assert _set(ctx, key, hi)[0] == 0 and _get(ctx, key) == (0, hi)
    _refused(ctx, key, lo, hi, msg, inside)
    assert _set(ctx, key, lo)[0] == 0 and _get(ctx, key) == (0, 4)  # auto, no index: 4


def test_write_only_keys(ctx):
    for key, lo, hi, msg in WRITE_ONLY:
        assert _set(ctx, key, lo)[0] == 0, key
        if key != "warm_dma":  # (its maximum would pin and copy 1 GiB)
            assert _set(ctx, key, hi)[0] == 0, key
        _refused(ctx, key, lo, hi, msg, [])
        assert _get(ctx, key)[0] == INVALID_ARG


def test_read_only_keys_and_unknown_keys(ctx):
    for key in READ_ONLY:
        assert _get(ctx, key)[0] == 0, key
        assert _set(ctx, key, 0) == (INVALID_ARG, "unknown option " + key)
    for key in NEED_INDEX:
        assert _get(ctx, key)[0] == NO_INDEX, key
        assert _set(ctx, key, 0) == (INVALID_ARG, "unknown option " + key)
    for key in ("no_such_option", "dev_", "dev_nothing", ""):
        assert _set(ctx, key, 0) == (INVALID_ARG, "unknown option " + key)
        assert _get(ctx, key)[0] == INVALID_ARG
