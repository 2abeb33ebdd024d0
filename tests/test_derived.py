"""The index tables the upload derives -- walk table, two-character rank chunks, suffix table,
presence bitmaps, pair words, window words -- as the emulator's host build makes them
(tests/derived_cpu over tests/emu's load()), against each structure's definition evaluated
from the node set in numpy (tests/derived_lib.py), array by array and whole.  The host build
calls the same per-entry functions as the kernels, so this is what says what an entry should
be; tests/test_gpu_derived.py holds the device arrays against the host build."""
import numpy as np
import pytest

from derived_lib import (CASES, K_TAB_SHORT, check_equal, check_tables, filter_level, load_case, pair_words_count,
                         rank2_blocks, reference_tables, tab_base, tab_bits_words, win_words_count)


def check_sizes(hb, n, U):
    """the arrays have the sizes the count functions give"""
    F = filter_level(U)
    assert hb["walk"].shape == (n, 4) and hb["rank2"].shape == (4 * rank2_blocks(n), 16)
    assert hb["tab"].shape == (tab_base(U + 1), 2) and hb["bits"].shape == (tab_bits_words(U),)
    assert hb["fbits"].shape == ((tab_bits_words(F),) if F else (0,))
    assert hb["pair"].shape == (pair_words_count(U),)
    assert hb["win"].shape == ((win_words_count(U), 8) if U >= 4 else (0, 8))


@pytest.mark.parametrize("name", list(CASES))
def test_host_build_equals_the_definition(name):
    ix, ref, hb = load_case(name)
    n, U = ref.n, ref.U
    check_sizes(hb, n, U)
    what = f"{name}, host build against the definition"
    if ref.full:
        check_tables(what, hb, reference_tables(ref), n, U)
        return
    # a deep table: every array but the suffix table whole; of the table, at every level which
    # entries are long, and every present entry by definition
    F = filter_level(U)
    exp = dict(hb, walk=ref.walk(), rank2=ref.rank2(), bits=ref.bitmap(U), fbits=ref.bitmap(F),
               pair=ref.pair_words(), win=ref.win_words())
    check_tables(what, hb, exp, n, U)
    for u in range(1, U + 1):
        keys, x, y = ref.levels[u]
        lv = hb["tab"][tab_base(u):tab_base(u + 1)]
        long_exp = np.zeros(4 ** u, dtype=bool)
        long_exp[keys] = True
        check_equal(f"{what}: level {u}, long entries, key", lv[:, 1] < K_TAB_SHORT, long_exp)
        ent = np.stack([x, ref.top_y(x, y) if u == U else y], axis=1).astype(np.uint32)
        i = np.flatnonzero((lv[keys] != ent).any(axis=1))
        assert len(i) == 0, f"{what}: level {u}, key {keys[i[0]]}: got {lv[keys[i[0]]]}, expected {ent[i[0]]}"
    for u, bits in ((U, hb["bits"]), (F, hb["fbits"])):  # as many bits as distinct u-mers end a label
        distinct = len(np.unique(ref.nd.keys(u)[ref.nd.ln >= u]))
        assert int(np.unpackbits(bits.view(np.uint8)).sum()) == distinct


def test_k_equals_u_has_single_real_nodes_only():
    """at k = U a U-mer is one k-mer node: no interval of several nodes, no dummy"""
    kinds = load_case("B-k8")[1].kinds()
    assert kinds["multi"] == 0 and kinds["single_nopos"] == 0 and kinds["single_pos"] == kinds["bits_set"]


def test_cg_genome_has_absent_characters():
    ix, ref, hb = load_case("D-cg")
    assert hb["absent"] == 0b1001
    assert np.array_equal(hb["tab"][[0, 3]], np.array([[0, K_TAB_SHORT]] * 2, dtype=np.uint32))  # u = 1: A, T


def test_small_index_walks_end_at_the_root():
    ix, ref, hb = load_case("F-n<112")
    assert ref.n < 112
    assert not (ref.walk()[:, 3] >> np.uint64(32)).any()
