"""The run-length code in colex_at's spare bits on the GPU (kernels.hip k_path_hint writes it
at upload, k_parse4 reads it instead of puniq; ctx option "uniq_hint"): the device records
and record offsets with the code on and off are identical to each other and to the oracle's on
the CPU tests' cases (tests/uniq_hint_lib.py), decode returns the reads, and the option reports
what the index in use was built with."""
import numpy as np
import pytest

import ntcomp_amd as nt
import uniq_hint_lib as ul

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = nt.GpuContext(0)
    yield c
    c.close()


def _device_records(ctx, bases, offs, n_exp):
    n, total = len(offs) - 1, int(offs[-1])
    db, do = ctx.alloc(bases.nbytes), ctx.alloc(offs.nbytes)
    dr, dro = ctx.alloc(total * 8 + 64), ctx.alloc(offs.nbytes)
    dout, doffs = ctx.alloc(total + 64), ctx.alloc((n + 1) * 8)
    try:
        ctx.h2d(db, bases)
        ctx.h2d(do, offs)
        ctx.encode_device(db, do, n, 0, dr, total + 8, dro)
        nrec = ctx.encode_status()
        assert nrec == n_exp
        got = ctx.d2h(np.zeros(nrec, dtype=np.uint64), dr)
        gro = ctx.d2h(np.zeros(n + 1, dtype=np.uint64), dro)
        ctx.decode_device(dr, nrec, dout, total, doffs, n + 1)
        assert ctx.decode_status() == (n, total)
        out = ctx.d2h(np.zeros(total, dtype=np.uint8), dout)
        oo = ctx.d2h(np.zeros(n + 1, dtype=np.uint64), doffs)
        return got, gro, out, oo
    finally:
        for p in (db, do, dr, dro, dout, doffs):
            ctx.free(p)


def _parity(ctx, ix, k, reads):
    bases, offs, exp, eoff = ul.oracle_records(ix, k, reads)
    try:
        for hint in (-1, 0):
            ctx.set_option("uniq_hint", hint)
            ctx.upload(ix)
            assert ctx.get_option("uniq_hint") == (1 if hint else 0)
            got, gro, out, oo = _device_records(ctx, bases, offs, len(exp))
            assert np.array_equal(gro, eoff), hint
            assert np.array_equal(got, exp), hint
            assert np.array_equal(out, bases) and np.array_equal(oo, offs), hint
    finally:
        ctx.set_option("uniq_hint", -1)


@pytest.mark.parametrize("k", [15, 31])
def test_gpu_repeats_at_the_threshold_edges(ctx, k):
    seqs, ix, reads, probes = ul.repeat_case(k)
    assert {t for _, t in probes} == set(ul.EDGES)
    _parity(ctx, ix, k, reads)


@pytest.mark.parametrize("k", [31, 91])
def test_gpu_benchmark_shapes(ctx, k):
    seqs, ix, reads = ul.random_case(k)
    _parity(ctx, ix, k, reads)


def test_gpu_long_reads(ctx):
    seqs, ix, reads = ul.long_case()
    _parity(ctx, ix, 31, reads)


def test_gpu_strain_collection(ctx):
    seqs, ix, reads = ul.strain_case()
    _parity(ctx, ix, 23, reads)


def test_gpu_option_reports_the_index_in_use(ctx):
    seqs, ix, reads = ul.random_case(31)
    try:
        ctx.set_option("uniq_hint", 0)
        ctx.upload(ix)
        assert ctx.get_option("uniq_hint") == 0
        ctx.set_option("uniq_hint", -1)       # for the next upload: the index in use has no code
        assert ctx.get_option("uniq_hint") == 0
        other = nt.GpuContext(0)
        try:
            assert other.get_option("uniq_hint") == -1   # no index: the setting
            other.share_index(ctx)
            assert other.get_option("uniq_hint") == 0
            ctx.upload(ix)
            assert ctx.get_option("uniq_hint") == 1
            assert other.get_option("uniq_hint") == 0    # still the index it shares
            other.share_index(ctx)
            assert other.get_option("uniq_hint") == 1
        finally:
            other.close()
    finally:
        ctx.set_option("uniq_hint", -1)
