"""Substitution words on the GPU: the uploaded words against the host build (bit for bit,
by hash), the `subst` option, and encode parity with the shortcut on, off and against the
oracle on the read shapes of tests/test_subst.py."""
import numpy as np
import pytest

import ntcomp_amd as nt
from oracle_lib import OracleIndex, pack_reads
from subst_lib import host_words, lone_reads, repeat_genome, shape_reads

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = nt.GpuContext(0)
    c.set_option("joint", 0)  # the build the words are for, whatever the path cover looks like
    yield c
    c.close()


@pytest.mark.parametrize("k", [10, 11, 31, 91])  # U = 10 here: k = U, U + 1, 31, 91
def test_gpu_subst_hash_equals_host(ctx, k):
    genome = nt.synth_genome(900 + k, 20_000).tobytes()
    ix = nt.Index.build([genome], k)
    ctx.set_option("subst", -1)
    ctx.upload(ix)
    hw = host_words(ix, k, 0)
    assert hw["U"] == 10 and ctx.get_option("tab_u") == 10
    assert hw["word"].sum() > 1000
    assert ctx.get_option("subst") == 1
    assert ctx.get_option("subst_hash") & U64 == hw["hash"]
    ctx.set_option("subst", 0)
    ctx.upload(ix)
    assert ctx.get_option("subst") == 0
    assert ctx.get_option("subst_hash") & U64 == host_words(ix, k, 0, subst=0)["hash"] != hw["hash"]
    ctx.set_option("subst", -1)


def test_gpu_subst_is_off_with_joint_runs(ctx):
    ix = nt.Index.build([nt.synth_genome(5, 20_000).tobytes()], 31)
    ctx.set_option("joint", 1)
    ctx.upload(ix)
    assert ctx.get_option("subst") == 0
    ctx.set_option("joint", 0)
    ctx.upload(ix)
    assert ctx.get_option("subst") == 1


@pytest.mark.parametrize("k", [31, 91])
def test_gpu_encode_parity_subst_on_and_off(ctx, k):
    genome = repeat_genome(500 + k, k)
    ix = nt.Index.build([genome.encode()], k)
    hw = host_words(ix, k, 0)
    L = 150
    shapes = shape_reads(genome, k, hw["U"], L, 4096, 3 * k)
    reads = (lone_reads(hw, k, L)[0] + shapes[4096:] + shapes)[:4096]  # lone, over path ends, the other shapes
    assert len(reads) == 4096  # more than one 64-read pool chunk per wave queue
    bases, offs = pack_reads(reads)
    exp, eoff = OracleIndex(ix.n, k, ix.rows, ix.C, ix.lcs).encode(bases, offs)
    ctx.set_option("subst", -1)
    ctx.upload(ix)
    assert ctx.get_option("subst") == 1
    on, on_off = ctx.encode(bases, offs)
    assert np.array_equal(on_off, eoff) and np.array_equal(on, exp)
    ctx.set_option("subst", 0)
    ctx.upload(ix)
    assert ctx.get_option("subst") == 0
    off, off_off = ctx.encode(bases, offs)
    assert np.array_equal(off_off, on_off) and np.array_equal(off, on)
    ctx.set_option("subst", -1)
