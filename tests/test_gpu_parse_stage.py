"""k_parse4's query stage on the GPU (kernels.hip NTC_PARSE_QLDS: a block copies the words of
the 2-bit query stream its 256 reads cover into LDS and parses from there, or parses from global
memory when they do not fit): encode_device's records and record offsets equal the oracle's on
the batches of tests/parse_stage_lib.py -- staged and unstaged blocks in one launch, a block's
first and last word at every alignment, a batch that does not start at offset 0 of an aligned
buffer, the read counts around one block -- and a batch with an invalid base still returns its
error (every block reaches the barrier before it looks at the status)."""
import numpy as np
import pytest

import ntcomp_amd as nt
import parse_stage_lib as pl
from oracle_lib import OracleIndex, pack_reads

pytestmark = pytest.mark.gpu

INVALID_BASE = 2


@pytest.fixture(scope="module", params=[31, 91])
def env(request):
    k = request.param
    ix = pl.index(k)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    yield k, ix, ctx, OracleIndex(ix.n, k, ix.rows, ix.C, ix.lcs)
    ctx.close()


def _device_records(ctx, bases, offs):
    """encode_device over bases / offs as given (offs[0] may be > 0) -> (records, record offsets)"""
    n, total = len(offs) - 1, int(offs[-1] - offs[0])
    db, do = ctx.alloc(bases.nbytes + 64), ctx.alloc(offs.nbytes)
    dr, dro = ctx.alloc(total * 8 + 64), ctx.alloc(offs.nbytes)
    try:
        ctx.h2d(db, bases)
        ctx.h2d(do, offs)
        ctx.encode_device(db, do, n, 0, dr, total + 8, dro)
        nrec = ctx.encode_status()
        got = ctx.d2h(np.zeros(nrec, dtype=np.uint64), dr)
        gro = ctx.d2h(np.zeros(n + 1, dtype=np.uint64), dro)
        return got, gro
    finally:
        for p in (db, do, dr, dro):
            ctx.free(p)


@pytest.mark.parametrize("name", sorted(pl.cases()))
def test_gpu_records_equal_the_oracle(env, name):
    k, ix, ctx, orc = env
    reads, lead = pl.cases()[name]
    b0, o0 = pack_reads(reads)
    exp, eoff = orc.encode(b0, o0)
    bases, offs = pl.batch(reads, lead)
    got, gro = _device_records(ctx, bases, offs)
    assert np.array_equal(gro, eoff)
    assert np.array_equal(got, exp)


def test_gpu_invalid_base_still_reports_its_read(env):
    """*status is set by the pack kernel: every block of the parse takes the early-out after the
    barrier and the call returns the error as before; the next call on the context is clean"""
    k, ix, ctx, orc = env
    reads, _ = pl.cases()["bench_1000x150"]
    bases, offs = pack_reads(reads)
    bad = bases.copy()
    bad[int(offs[700]) + 3] = ord("N")
    with pytest.raises(nt.NtcError) as e:
        ctx.encode(bad, offs)
    assert e.value.code == INVALID_BASE and e.value.bad_read == 700
    recs, roff = ctx.encode(bases, offs)
    exp, eoff = orc.encode(bases, offs)
    assert np.array_equal(roff, eoff) and np.array_equal(recs, exp)
