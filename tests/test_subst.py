"""Substitution words (encode_core.h subst_clean) and the SCAN shortcut they feed in
MsLaneT<false>::step, on the CPU: the host-built word against a direct evaluation of its
definition from the k-mer set, and the non-joint emulation with the word on and zeroed --
same records, same (d, S) per position, bit-exact against the oracle -- with the NTC_STAT
counters showing that the shortcut and its fallback both ran."""
import numpy as np
import pytest

import ntcomp_amd as nt
from oracle_lib import OracleIndex, pack_reads
from subst_lib import brute_words, emu_run, host_words, lone_reads, repeat_genome, shape_reads

# (k, tab_u, genome length): k over U, U + 1, 15, 31.  Depths 4 .. 7 lie below t_jump =
# ceil(log4 n) + 2 >= 8 for every genome of 2 kbp and more, so the table carries no path
# positions there (tab_pos = 0) and the definition gives an all-zero word; depths 8 and 9
# carry them where the genome is small enough, and there both kinds of bit have a floor.
CASES = [(4, 4, 2000), (5, 4, 3000), (15, 5, 2000), (6, 6, 5000), (31, 6, 2000), (7, 7, 20000), (8, 7, 2000),
         (15, 7, 3000), (31, 7, 8000),
         (8, 8, 2000), (9, 8, 2500), (15, 8, 3000), (31, 8, 2000), (9, 9, 6000), (10, 9, 7000), (15, 9, 8000),
         (31, 9, 6000)]


@pytest.mark.parametrize("k,tab_u,glen", CASES)
def test_host_word_equals_the_definition(k, tab_u, glen):
    genome = nt.synth_genome(7000 + 31 * k + tab_u, glen).tobytes().decode()
    ix = nt.Index.build([genome.encode()], k)
    hw = host_words(ix, k, tab_u)
    assert hw["U"] == tab_u
    exp = brute_words(genome, k, hw)
    assert np.array_equal(hw["word"], exp), np.flatnonzero(hw["word"] != exp)[:10]
    # within U + 1 of a path end (and before a path's first k-mer end) every bit is 0
    end, U = hw["end"], tab_u
    last = np.flatnonzero((end[:-1] == 1) & (end[1:] == 0))  # last k-mer end of each path
    assert len(last) >= 2
    for e in last:  # the path's text ends at e + 1: positions from e + 1 - (U + 1) on, its pad, the next path's start
        assert not hw["word"][max(0, e - U):e + k + 1].any()
    n_set, n_clear = int(hw["word"].sum()), int((hw["word"][: hw["tlen"]] == 0).sum())
    print(f"k={k} U={tab_u} genome={glen}: {n_set} set, {n_clear} cleared of {hw['tlen']}")
    if tab_u >= hw["t_jump"]:
        assert n_set >= 200 and n_clear >= 200
    else:
        assert n_set == 0
    # zeroed on request
    assert host_words(ix, k, tab_u, subst=0)["word"].sum() == 0


def test_both_kinds_of_bit_are_tested():
    """the cases above reach the table depths that carry path positions"""
    live = 0
    for k, tab_u, glen in CASES:
        genome = nt.synth_genome(7000 + 31 * k + tab_u, glen).tobytes()
        live += tab_u >= host_words(nt.Index.build([genome], k), k, tab_u)["t_jump"]
    assert live >= 4


# --------------------------------------------------------------------------------------
# same lanes with the word on and zeroed
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[31, 91, 11])
def lanes(request):
    """index (default table depth), its host words and the oracle, shared by the lane tests"""
    k = request.param
    genome = repeat_genome(500 + k, k)
    ix = nt.Index.build([genome.encode()], k)
    hw = host_words(ix, k, 0)
    assert hw["tab_pos"] == 1 and hw["word"].sum() > 1000
    return k, genome, ix, hw, OracleIndex(ix.n, k, ix.rows, ix.C, ix.lcs)


def check_both_ways(lanes, reads):
    k, genome, ix, hw, orc = lanes
    bases, offs = pack_reads(reads)
    exp, eoff = orc.encode(bases, offs)
    on = emu_run(ix, k, reads, 1)
    off = emu_run(ix, k, reads, 0)
    assert off[4] == 0 and off[5] == 0  # a zero word: the shortcut is off
    for got in (on, off):
        assert np.array_equal(got[1], eoff) and np.array_equal(got[0], exp)
    assert np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])
    for r in range(len(reads)):
        od, olo = orc.ms(reads[r].encode())
        a, b = int(offs[r]), int(offs[r + 1])
        assert np.array_equal(on[2][a:b], od) and np.array_equal(on[3][a:b].astype(np.uint64), olo), r
    return on[4], on[5]


def test_lone_substitutions_take_the_shortcut(lanes):
    k, genome, ix, hw, orc = lanes
    reads, clean = lone_reads(hw, k, 150 if k < 60 else 260)
    assert len(reads) >= 200
    taken, fell = check_both_ways(lanes, reads)
    print(f"k={k}: {len(reads)} lone substitutions, {clean} at a clean position, shortcut taken {taken}, fell back {fell}")
    # Every lone substitution at a clean position takes the shortcut and keeps it (the read
    # equals the path around it).  At these indexes' U-mer density (20 kbp + reverse
    # complement, U = 10: 4 %) each of the six U-mers the definition wants absent is absent
    # with probability 0.96, so it holds for about three substitutions in four: at least half.
    # (A substitution at a position that is not clean leaves a chance U-mer behind; a run on
    # that chance match may break at a clean position of its own, take the shortcut and fall back.)
    assert taken - fell >= clean
    assert clean >= len(reads) // 2


def test_shapes_same_lanes_both_ways(lanes):
    k, genome, ix, hw, orc = lanes
    reads = shape_reads(genome, k, hw["U"], 150 if k < 60 else 260, 260, 17 * k)
    taken, fell = check_both_ways(lanes, reads)
    print(f"k={k}: {len(reads)} reads, shortcut taken {taken}, fell back {fell}")
    assert taken >= 40
    assert fell >= 1  # an unconfirmed guess was rejected and the lane went back to its break
