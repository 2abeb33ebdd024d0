"""The fixtures and models of big_batch_lib.py, pinned on the host so that the reference alone
decides them: the period's shape and every condition its tiling relies on, the oracle's records of
one period and that tiling them is what the oracle itself says of repeated periods, the text and
region models, the FASTQ generator against the host parser, and the three scan sizes against a
restatement of the scan's tile.  test_gpu_big_batch.py takes the same fixtures through the kernels."""
import time

import numpy as np
import pytest

import big_batch_lib as bb
import ntcomp_amd as nt
from big_batch_lib import BLOCK, K, TWO32
from oracle_lib import OracleIndex
from test_grid_cap import host_parse


@pytest.fixture(scope="module")
def per():
    return bb.period()


@pytest.fixture(scope="module")
def oracle(per):
    ix = nt.Index.build([per.genome], K)
    return OracleIndex(ix.n, K, ix.rows, ix.C, ix.lcs)


@pytest.fixture(scope="module")
def period_records(per, oracle):
    t0 = time.perf_counter()
    recs, roffs = oracle.encode(per.bases, per.offs)
    print(f"oracle on one period of {per.B} bases: {time.perf_counter() - t0:.2f} s")
    return recs, roffs


# ---- Part A: the period ---------------------------------------------------------------------------
def test_the_period_is_ragged_reads_of_the_genome(per):
    lens = np.diff(per.offs.astype(np.int64))
    assert per.P == len(per.reads) == bb.N_READS and per.B == int(lens.sum()) == len(per.bases)
    assert lens.min() == 1 and 39_000 < lens.max() <= 40_000 and 13_000 < lens.mean() < 17_000
    assert sorted(lens[lens < K].tolist())[:3] == [1, 7, 30] and 3_000_000 < per.B < 5_000_000
    assert per.bases.tobytes() == b"".join(per.reads) and set(per.bases.tolist()) == set(b"ACGT")
    strands, n_subs = set(), set()
    for read, (start, rev, subs) in zip(per.reads, per.origin):
        src = per.genome[start:start + len(read)]
        assert len(src) == len(read)
        src = bb.revcomp(src) if rev else src
        differ = [i for i, (a, b) in enumerate(zip(read, src)) if a != b]
        assert differ == list(subs) and len(subs) <= 4
        strands.add(rev)
        n_subs.add(len(subs))
    assert strands == {False, True} and n_subs == {0, 1, 2, 3, 4}
    assert bb.period() is per  # one fixture for every test of the session


def test_the_conditions_the_tiling_relies_on(per):
    c = bb.conditions(per.reads)
    figures = c.pop("_")
    assert all(c.values()), c
    B, P, R = per.B, per.P, per.R
    assert figures == dict(figures, P=P, B=B, R=R) and R == -(-(TWO32 + 2 * B) // B)
    # B odd: no power of two is a multiple of it, so a position truncated to any number of bits
    # lands in other content, and the repetitions start at every alignment modulo 16 and 32
    assert B % 2 == 1 and all((1 << b) % B for b in range(1, 64))
    assert {(i * B) % 32 for i in range(32)} == set(range(32)) and {(i * B) % 16 for i in range(16)} == set(range(16))
    for bits in (24, 31, 32):  # the content at a truncated position differs from the true one
        at = TWO32 + 12345
        assert per.bases[at % B:at % B + 64].tobytes() != per.bases[(at & ((1 << bits) - 1)) % B:][:64].tobytes()
    # base 2^32 strictly inside a read of at least 2 k bases
    offs = bb.tiled_offsets(per.offs, B, R)
    assert int(offs[-1]) == R * B >= TWO32 + 2 * B > (R - 1) * B and len(offs) == R * P + 1
    r = int(np.searchsorted(offs, TWO32, side="right")) - 1
    assert int(offs[r]) < TWO32 < int(offs[r + 1]) and int(offs[r + 1] - offs[r]) >= 2 * K
    assert r % P == figures["read_at_2_32"]
    # byte 2^32 of the FASTA text inside a sequence line
    lens = np.diff(offs.astype(np.int64))
    head, toffs = bb.text_layout(lens)
    t = figures["text_read_at_2_32"]
    assert int(toffs[t]) + int(head[t]) <= TWO32 < int(toffs[t + 1]) - 1
    # ragged grids and blocks
    assert (R * P) % 64 and (R * P) % 256
    assert all((b * BLOCK) % P for b in range(1, -(-R * P // BLOCK)))
    assert int(offs[R * P - 2 * P]) > TWO32  # the last two periods: offsets past 2^32 (the far-offsets test)


def test_tiled_offsets_are_the_cumulative_sums(per):
    R = 5
    lens = np.tile(np.diff(per.offs.astype(np.int64)), R)
    assert np.array_equal(bb.tiled_offsets(per.offs, per.B, R), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))


def test_the_oracle_on_one_period(per, oracle, period_records):
    recs, roffs = period_records
    n_rec = np.diff(roffs.astype(np.int64))
    ln, short = bb.record_lengths(recs)
    assert int(ln.sum()) == per.B and short.any() and (~short).any()
    assert (n_rec == 1).any() and (n_rec > bb.REC_SLOT).any() and n_rec.min() >= 1
    out, o2 = oracle.decode(recs)
    assert np.array_equal(out, per.bases) and np.array_equal(o2, per.offs)


def test_tiling_is_what_the_oracle_says_of_repeated_periods(per, oracle, period_records):
    """a read's records do not depend on where it lies in the batch: three periods through the
    oracle, at three alignments (B is odd), are the period's records tiled"""
    recs, roffs = period_records
    R = 3
    got, goffs = oracle.encode(np.tile(per.bases, R), bb.tiled_offsets(per.offs, per.B, R))
    want, woffs = bb.tiled_records(recs, roffs, R)
    assert np.array_equal(got, want) and np.array_equal(goffs, woffs)
    assert np.array_equal(woffs[per.P:2 * per.P + 1], roffs + roffs[-1])


# ---- Part A: the models ---------------------------------------------------------------------------
@pytest.mark.parametrize("first_id", [1, 95, 99_990])
def test_the_text_model_counts_what_python_prints(per, first_id):
    n = 2 * per.P + 5
    lens = np.array([len(per.reads[i % per.P]) for i in range(n)])
    head, toffs = bb.text_layout(lens, first_id)
    text = bb.fasta_text(per.reads, 0, n, first_id)
    assert int(toffs[-1]) == len(text)
    for i in (0, 4, 5, 9, 10, per.P, n - 1):
        rec = b">seq.%d\n%s\n" % (first_id + i, per.reads[i % per.P])
        assert text[int(toffs[i]):int(toffs[i + 1])] == rec and int(head[i]) == rec.index(b"\n") + 1
    assert bb.fasta_text(per.reads, per.P + 2, per.P + 4, first_id) == text[int(toffs[per.P + 2]):int(toffs[per.P + 4])]


def test_the_regions_that_are_compared(per):
    B, R = per.B, per.R
    regions = bb.check_regions(B, R)
    assert regions[0] == (0, 3 * B) and regions[-1] == (TWO32 - B, R * B) and regions[1] == (16 * B, 17 * B)
    assert all(lo % B == 0 and hi - lo == B and (lo // B) % 16 == 0 for lo, hi in regions[1:-1])
    assert len(regions) - 2 == ((TWO32 - B) // B - 1) // 16  # every 16th period below the tail
    assert sum(hi - lo for lo, hi in regions) < 80 * B
    small = np.tile(per.bases[:1001], 7)
    for lo, hi in [(0, 1001), (999, 3003), (1001 * 6 - 1, 1001 * 7)]:
        assert np.array_equal(bb.expected_bases(per.bases[:1001], lo, hi), small[lo:hi])
    lens = np.tile(np.diff(per.offs.astype(np.int64)), R)
    _, toffs = bb.text_layout(lens)
    pers = bb.check_periods(per.P, R, toffs, B)
    assert pers[0] == (0, 3 * per.P) and pers[-1][1] == R * per.P
    assert int(toffs[pers[-1][0]]) >= TWO32 - B > int(toffs[pers[-1][0] - 1])
    assert all(a[1] <= b[0] for a, b in zip(pers, pers[1:])) and all(f % (16 * per.P) == 0 for f, _ in pers[1:-1])


# ---- Part B: the scan's level edges and the generator ----------------------------------------------
def test_the_three_sizes_are_the_level_edges():
    tile = 256 * 16  # kScanThreads x kScanItems, restated
    assert bb.SCAN_TILE == tile and bb.SCAN_CASES == (tile ** 2, tile ** 2 + 1, tile ** 2 + tile + 1)
    assert bb.scan_levels(tile) == (1, [tile]) and bb.scan_levels(tile + 1) == (2, [tile + 1, 2])
    assert bb.scan_levels(bb.N_TWO_LEVELS) == (2, [tile ** 2, tile])             # level 2: exactly one full tile
    assert bb.scan_levels(bb.N_TWO_LEVELS - 1)[0] == 2
    assert bb.scan_levels(bb.N_THREE_LEVELS) == (3, [tile ** 2 + 1, tile + 1, 2])  # the smallest three-level scan
    assert bb.scan_levels(bb.N_LEVEL2_TAIL) == (3, [tile ** 2 + tile + 1, tile + 2, 2])  # level 2: a tail of two items
    # the parser scans n + 1 outputs from n kept counts: it is n that decides the levels
    from grid_cap_lib import N
    assert bb.scan_levels(N)[0] == 2  # the largest n any other test reaches


def test_the_generator_against_the_host_parser(tmp_path):
    t0 = time.perf_counter()
    t = bb.tiny_fastq(10_000, 3)
    assert time.perf_counter() - t0 < 1
    lens = np.diff(t.offs.astype(np.int64))
    assert set(lens.tolist()) == {1, 2, 3} and len(set(np.diff(lens).tolist())) > 2  # no arithmetic sequence
    assert set(t.bases.tolist()) == set(b"ACGT") and len(t.text) == int(t.starts[-1]) == 6 * 10_000 + 2 * len(t.bases)
    (tmp_path / "t.fq").write_bytes(t.text.tobytes())
    bases, offs = host_parse(tmp_path / "t.fq")
    assert np.array_equal(offs, t.offs) and np.array_equal(bases, t.bases)
    whole = t.text.tobytes()
    recs = [whole[a:b].split(b"\n") for a, b in zip(t.starts[:-1].tolist(), t.starts[1:].tolist())]
    assert all(len(r) == 5 and r[0] == b"@" and r[2] == b"+" and r[4] == b"" for r in recs)
    assert all(len(r[1]) == len(r[3]) == int(n) for r, n in zip(recs, lens))
    assert b"".join(r[1] for r in recs) == t.bases.tobytes()
    # a cut at a record boundary is the generator's own prefix
    c = bb.tiny_cut(t, 777)
    (tmp_path / "c.fq").write_bytes(c.text.tobytes())
    bases, offs = host_parse(tmp_path / "c.fq")
    assert len(offs) == 778 and np.array_equal(offs, t.offs[:778]) and np.array_equal(bases, t.bases[:int(t.offs[777])])
    # the damage: one quality byte less in one record, every line still there
    d = bb.tiny_damage(t, 9_990)
    assert len(d) == len(t.text) - 1 and d.tobytes().count(b"\n") == 40_000
    rec = d.tobytes()[int(t.starts[9_990]):int(t.starts[9_991]) - 1].split(b"\n")
    assert len(rec[1]) == len(rec[3]) + 1 and d.tobytes()[:int(t.starts[9_990])] == t.text.tobytes()[:int(t.starts[9_990])]
