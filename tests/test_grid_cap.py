"""The batches of grid_cap_lib.py, pinned on the host before any GPU sees them: the host parser
(fastx.cpp) reads out of the big texts the bases and offsets the makers intended, the Python
models the GPU tests compare with (names_lib, qual_lib, pair_lib) round-trip the makers' lists at
this size, and no record equals the one CAP before it.  test_gpu_grid_cap.py takes the same
batches through the kernels."""
import numpy as np
import pytest

import grid_cap_lib as gc
import names_lib as nl
import ntcomp_amd as nt
import pair_lib as pl
import qual_lib as ql
from grid_cap_lib import CAP, N, N_PAIRS


def long_read():
    """64 bases of the genome the GPU tests index: a long record for every block (grid_cap_lib.py)"""
    return nt.synth_genome(7, 20_000).tobytes()[500:564]


def host_parse(path):
    """every batch of the host parser, joined -> (bases, offsets)"""
    rd = nt.FastxReader(str(path))
    bs, os_, base = [], [np.zeros(1, np.uint64)], 0
    try:
        for b, o in rd:
            bs.append(b[int(o[0]):int(o[-1])])
            os_.append((o[1:] - o[0] + base).astype(np.uint64))
            base += int(o[-1] - o[0])
    finally:
        rd.close()
    return (np.concatenate(bs) if bs else np.zeros(0, np.uint8)), np.concatenate(os_)


def flat(reads):
    """reads as the parser leaves them -> (bases, offsets)"""
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), offs


def parse_shapes(names, reads, quals):
    """the three texts of the parse tests -> {shape: (text, reads the parser must find)}"""
    lines, qs = gc.messy(reads, quals)
    return {"lf": (nl.make_fastq(names, reads, quals), reads),
            "crlf_messy": (nl.make_fastq(names, lines, qs, eol=b"\r\n"), [ql.normalise(s) for s in lines]),
            "no_last_newline": (nl.make_fastq(names, reads, quals, last_newline=False), reads)}


@pytest.fixture(scope="module")
def plain():
    return gc.batch(long_read=long_read())


def test_the_sizes_leave_a_ragged_second_trip():
    assert CAP == 262144 and N > CAP and N_PAIRS > CAP
    assert all(N % m for m in (4, 64, 256)) and (N - 1) // CAP == 1  # the last record: a second-trip wave's


@pytest.mark.parametrize("shape", ["lf", "crlf_messy", "no_last_newline"])
def test_host_parser_reads_what_the_makers_meant(plain, tmp_path, shape):
    text, want = parse_shapes(*plain)[shape]
    if shape == "crlf_messy":  # beyond the cap the parser has work to do on every line: fold, replace or drop
        lines = gc.messy(plain[1], plain[2])[0]
        assert lines[:CAP] == want[:CAP] and all(s != w for s, w in zip(lines[CAP:], want[CAP:]))
        assert any(len(w) < len(s) for s, w in zip(lines[CAP:], want[CAP:])) and b"N" in b"".join(want[CAP:])
    assert (text[-1:] == b"\n") == (shape != "no_last_newline") and (b"\r" in text) == (shape == "crlf_messy")
    (tmp_path / "x.fq").write_bytes(text)
    bases, offs = host_parse(tmp_path / "x.fq")
    exp_b, exp_o = flat(want)
    assert len(offs) == N + 1 and np.array_equal(offs, exp_o) and np.array_equal(bases, exp_b)


@pytest.mark.parametrize("blanks", [False, True])
def test_the_models_round_trip_the_batch(blanks):
    names, reads, quals = gc.batch(blanks=blanks, long_read=long_read())
    assert len(names) == N and {len(r) for r in reads} == {1, 2, 3, gc.LONG}
    assert [i for i, r in enumerate(reads) if len(r) == gc.LONG] == [b * gc.BLOCK + 1 for b in range(5)]  # one per block
    assert all(names[i] == b"r%d" % i for i in range(CAP)) and all(n.startswith(b"r%d" % (CAP + i)) for i, n in enumerate(names[CAP:]))
    text = nl.make_fastq(names, reads, quals)
    assert b"".join(gc.records(names, reads, quals)) == text
    assert nl.names_of(text) == names
    assert ql.records(text) == list(zip(reads, quals))
    ids = nl.names_of(text, "id")
    if blanks:  # a space and a tab cut beyond the cap, and nowhere else
        assert [i for i in range(N) if ids[i] != names[i]] == [i for i in range(CAP, N) if i % 3 != 2]
        assert ids == [b"r%d" % i for i in range(N)]
    else:
        assert ids == names
    metas, pay = nl.sections(names, 65536)
    assert [m["n_reads"] for m in metas] == [65536] * 4 + [5]
    assert [n for m in metas for n in nl.expand(m, pay[m["payload_off"]:m["payload_off"] + m["payload_bytes"]])] == names


def test_the_models_round_trip_the_pairs():
    s1, s2 = gc.pairs(long_read=long_read())
    assert len(s1[0]) == len(s2[0]) == N_PAIRS
    assert [p for p, r in enumerate(s1[1]) if len(r) == gc.LONG] == [b * gc.BLOCK // 2 + 1 for b in range(9)]
    t1, t2 = nl.make_fastq(*s1), nl.make_fastq(*s2)
    woven = pl.weave(t1, t2)
    assert pl.split(woven, 4) == (t1, t2)
    assert nl.names_of(woven) == [n for mates in zip(s1[0], s2[0]) for n in mates]
    assert pl.first_bad_pair(s1[0], s2[0]) is None
    beyond = s1[0][CAP:] + s2[0][CAP:]  # both strip rules on the second trip
    assert any(n.endswith(b"/1") for n in beyond) and any(n.endswith(b" 1:N") for n in beyond) and any(b"\t2:N" in n for n in beyond)
    assert pl.weave(t1[:-1], t2) == woven == pl.weave(t1, t2[:-1])


def test_no_record_equals_the_one_a_cap_before_it(plain):
    gc.assert_trips_differ(*plain)
    gc.assert_trips_differ(*gc.batch(blanks=True, long_read=long_read()))
    lines, qs = gc.messy(plain[1], plain[2])
    gc.assert_trips_differ(plain[0], lines, qs)
    gc.assert_trips_differ(plain[0], [ql.normalise(s) for s in lines], qs)
    for side in gc.pairs(long_read=long_read()):
        gc.assert_trips_differ(*side)
    with pytest.raises(AssertionError):  # and the check can fail
        gc.assert_trips_differ(plain[0], plain[1][:CAP] + plain[1][:5], plain[2])
