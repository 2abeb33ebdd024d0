"""The order-1 rANS coder of the quality sections, the parts that need no GPU: the kernels' row
and lane logic compiled for the CPU under ASan + UBSan (tests/qrans_cpu), the checker's own
self-test, the version-2 "NTCQ" side file (ntc_q_write_* / ntc_q_read), the size it is for, and
the Python and command-line surface.

The checker is qrans_lib.py (numpy and plain Python)."""
import ctypes
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import ntcomp_amd as nt
import qrans_lib as qr
import qual_lib as ql

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT = 1, 8


# ---- row and lane logic on the CPU, under ASan + UBSan ----------------------------------------
@pytest.fixture(scope="module")
def lane_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qrans_cpu") / "qrans_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "qrans_cpu", "qrans_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _lanes(exe, tmp_path, syms, n_syms):
    """the body the CPU program makes of a block's symbols; it also decodes it back, checks the
    slot-stride bound and that every adjusted frequency is >= 1, and exits non-zero otherwise"""
    syms = np.asarray(syms, dtype=np.uint8)
    (tmp_path / "in.bin").write_bytes(struct.pack("<IIQ", n_syms, 0, len(syms)) + syms.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    return (tmp_path / "out.bin").read_bytes()


def _same(got, syms, n_syms):
    exp = qr.body(syms, n_syms)
    assert qr.split_body(got, len(syms), n_syms) == qr.split_body(exp, len(syms), n_syms)  # which part, if any
    assert got == exp
    _, sizes, _ = qr.split_body(exp, len(syms), n_syms)
    for j, size in enumerate(sizes):
        assert 4 <= size <= qr.span_bound(min(qr.SPAN, len(syms) - j * qr.SPAN))
    assert qr.decode_body(exp, len(syms), n_syms, bytes(range(40, 40 + n_syms))) == \
        (bytes(40 + int(s) for s in syms), True)


@pytest.mark.parametrize("n_syms", [1, 2, 3, 4, 5, 16, 17, 40, 94])
def test_lane_logic_alphabets_and_span_boundaries(lane_exe, tmp_path, n_syms):
    rng = np.random.default_rng(500 + n_syms)
    for nq in (1, 2047, 2048, 2049, 4097):
        syms = rng.integers(0, n_syms, nq)
        if nq >= n_syms:
            syms[rng.permutation(nq)[:n_syms]] = np.arange(n_syms)  # every symbol occurs
        _same(_lanes(lane_exe, tmp_path, syms, n_syms), syms, n_syms)


def test_lane_logic_rows_at_the_edges(lane_exe, tmp_path):
    # a row with a single symbol: f = 4096, no byte leaves the state
    syms = np.array(([0] * 9 + [1]) * 300)[:2900]
    syms[9::10] = 1  # after 1 always 0; after 0 mostly 0
    tab = qr.table(qr.counts(syms, 2))
    assert tab[1] == [4096, 0]
    _same(_lanes(lane_exe, tmp_path, syms, 2), syms, 2)
    # a symbol seen once among more than 4096 is raised to 1, and with enough of them the
    # difference to 4096 is negative: 40 symbols once each after symbol 0, which follows itself
    # 100,000 times
    n = 41
    syms = np.zeros(100_000 + 2 * 40, dtype=np.int64)
    syms[1000:1000 + 80:2] = np.arange(1, 41)  # 0 s 0 s' 0 ...: each s once after 0, 0 after each s
    c = qr.counts(syms, n)
    floors = [0 if v == 0 else max(1, int(v) * 4096 // int(c[0].sum())) for v in c[0]]
    assert sorted(set(c[0][1:].tolist())) == [1] and c[0].sum() > 4096 and 4096 - sum(floors) < 0
    f = qr.normalise(c[0])
    assert f[1:] == [1] * 40 and f[0] == 4096 - 40
    _same(_lanes(lane_exe, tmp_path, syms, n), syms, n)
    # 94 symbols, each present in one row only: symbol s is always followed by s + 1
    syms = np.arange(3 * 2048 + 5) % 94
    c = qr.counts(syms, 94)
    assert all(np.count_nonzero(c[:94, s]) == 1 for s in range(94))
    _same(_lanes(lane_exe, tmp_path, syms, 94), syms, 94)
    # the worst case of the normalisation: 93 symbols raised to 1, one takes the rest
    worst = [10 ** 6] + [1] * 93
    assert qr.normalise(worst) == [4096 - 93] + [1] * 93


# ---- the checker itself -----------------------------------------------------------------------
def test_checker_on_a_hand_written_case():
    # "ABAB" over {A, B}: rows A: (0, 2) -> B always, B: (1, 0) -> A always, start: (1, 0)
    syms = [0, 1, 0, 1]
    c = qr.counts(syms, 2)
    assert c.tolist() == [[0, 2], [1, 0], [1, 0]]
    tab = qr.table(c)
    assert tab == [[0, 4096], [4096, 0], [4096, 0]]
    # every frequency is 4096: x = ((x / 4096) << 12) + x % 4096 + 0 = x, and no byte leaves
    st = qr.encode_span(syms, tab, 2)
    assert st == struct.pack("<I", 1 << 23)
    assert qr.decode_span(st, 4, tab, 2) == (syms, True)
    assert qr.body(syms, 2) == struct.pack("<6H", 0, 4096, 4096, 0, 4096, 0) + struct.pack("<I", 4) + st
    # normalisation by hand: 3 : 1 -> 3072 : 1024; 1 : 1 : 1 -> the first of the largest takes the rest
    assert qr.normalise([3, 1]) == [3072, 1024] and qr.normalise([1, 1, 1]) == [1366, 1365, 1365]
    assert qr.normalise([0, 0]) == [0, 0] and qr.normalise([0, 7, 0]) == [0, 4096, 0]
    # one step by hand: x = L, symbol of start 3072 and frequency 1024: L >= 2^19 * 1024 = 2^29? no,
    # so x' = (L / 1024) << 12 + 0 + 3072
    tab = [[3072, 1024], [3072, 1024], [3072, 1024]]
    st = qr.encode_span([1], tab, 2)
    assert st == struct.pack("<I", ((1 << 23) // 1024 << 12) + 3072)
    # and a frequency of 1 pushes two bytes out: L >= 2^19, (L >> 8) = 2^15 < 2^19
    tab1 = [[4095, 1]] * 3
    st = qr.encode_span([1], tab1, 2)
    assert len(st) == 5 and st[4] == 0 and qr.decode_span(st, 1, tab1, 2) == ([1], True)
    # the decoder refuses: a missing byte, a byte too many, a zero row, another final state
    good = qr.encode_span([1, 0, 1, 1, 0, 0, 0, 1], tab, 2)
    assert qr.decode_span(good, 8, tab, 2) == ([1, 0, 1, 1, 0, 0, 0, 1], True)
    assert not qr.decode_span(good[:-1], 8, tab, 2)[1] and not qr.decode_span(good + b"\0", 8, tab, 2)[1]
    assert not qr.decode_span(good, 8, [[0, 0]] * 3, 2)[1]
    assert not qr.decode_span(good, 7, tab, 2)[1]
    assert qr.span_bound(2048) == 3076 and qr.n_spans(2049) == 2 and qr.n_spans(0) == 0
    q = qr.markov_quals(np.random.default_rng(1), b"#-<F", 20_000, 0.9)
    assert 0.88 < np.mean(q[1:] == q[:-1]) < 0.92 and set(q.tolist()) == set(b"#-<F")


# ---- the size condition -------------------------------------------------------------------------
def _v1_section(m, words):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    member = c.compress(words) + c.flush() if m["width"] else b""
    return struct.pack("<QQBBHI", m["n_reads"], m["n_quals"], m["width"], m["n_syms"], 0, len(member)) + \
        m["alphabet"] + member


def test_sections_of_a_markov_source_are_smaller_than_version_1():
    """Four symbols that stay with p = 0.9, blocks of 64 reads x 150: the version-2 section of
    every block is smaller than its version-1 section (zlib -6 on the packed words)."""
    text = qr.markov_fastq(21, 4 * 64, 150)
    m2, pay = qr.sections(text, 64)
    m1, words = ql.sections(text, 64)
    raw = words.astype("<u8").tobytes()
    for a, b in zip(m2, m1):
        v2 = len(qr.section_bytes(a, pay[a["payload_off"]:a["payload_off"] + a["payload_bytes"]]))
        v1 = len(_v1_section(b, raw[b["payload_off"]:b["payload_off"] + b["payload_bytes"]]))
        print("section bytes: version 2", v2, "version 1", v1)
        assert v2 < v1


# ---- side file ----------------------------------------------------------------------------------
def _qmetas(text, block_reads, mode="keep"):
    metas, pay = qr.sections(text, block_reads, mode)
    out = []
    for m in metas:
        q = nt.QualMeta()
        q.n_reads, q.n_quals, q.width, q.n_syms = m["n_reads"], m["n_quals"], m["width"], m["n_syms"]
        q.payload_off, q.payload_bytes, q.coder = m["payload_off"], m["payload_bytes"], 1
        ctypes.memmove(q.alphabet, m["alphabet"], len(m["alphabet"]))
        out.append(q)
    return out, pay


def _write(path, mode, metas, payload, **kw):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        nt.write_qualities(fd, mode, metas, payload, engine="zlib", **kw)
    finally:
        os.close(fd)


def _text(seed=1, syms=(4, 40, 1, 2), block_reads=64):
    reads, quals = ql.ragged_batch(np.random.default_rng(seed), list(syms), block_reads, block_reads * (len(syms) - 1) + 9)
    return ql.make_fastq(reads, quals)


def test_side_file_round_trip(tmp_path):
    text = _text()
    metas, payload = _qmetas(text, 64)
    p = tmp_path / "q.ntcq"
    _write(p, "keep", metas, payload, coder="rans")
    assert p.read_bytes() == qr.file_bytes(text, 64)  # the checker's file, byte for byte
    assert p.read_bytes()[:32] == b"NTCQ" + struct.pack("<IBB", 2, 1, 1) + bytes(22)
    mode, got, pay = nt.read_qualities(p)
    assert mode == 1 and pay == payload
    assert [qr.meta_dict(m) for m in got] == [qr.meta_dict(m) for m in metas]
    assert [m.coder for m in got] == [1, 1, 1, 1] and got[2].payload_bytes == 0
    # coder "pack" writes version 1, as ntc_q_write_header does
    for kw in ({}, {"coder": "pack"}):
        _write(tmp_path / "e.ntcq", "bin8", [], b"", **kw)
        assert (tmp_path / "e.ntcq").read_bytes() == b"NTCQ" + struct.pack("<IB", 1, 2) + bytes(23)
    _write(tmp_path / "e2.ntcq", "bin8", [], b"", coder="rans")
    assert nt.read_qualities(tmp_path / "e2.ntcq") == (2, [], b"")
    with pytest.raises(nt.NtcError) as e:
        _write(tmp_path / "e3.ntcq", "keep", [], b"", coder=2)
    assert e.value.code == INVALID_ARG


def test_side_file_writer_refuses_a_body_that_is_not_sound(tmp_path):
    metas, payload = _qmetas(_text(), 64)
    bad = bytearray(payload)
    bad[metas[0].payload_off] ^= 1  # a row that sums to 4095 or 4097
    with pytest.raises(nt.NtcError) as e:
        _write(tmp_path / "w.ntcq", "keep", metas, bytes(bad), coder="rans")
    assert e.value.code == INVALID_ARG


def _body(tab, streams):
    return np.asarray(tab, dtype="<u2").tobytes() + b"".join(struct.pack("<I", len(s)) for s in streams) + b"".join(streams)


def _section(n_reads, n_quals, alphabet, body, size=None):
    return struct.pack("<QQBBHI", n_reads, n_quals, ql.width(len(alphabet)), len(alphabet), 0,
                       len(body) if size is None else size) + alphabet + body


HEAD2 = qr.header("keep")
HEAD1 = b"NTCQ" + struct.pack("<IB", 1, 1) + bytes(23)
TAB = [[0, 4096], [4096, 0], [4096, 0]]  # "#I#I#": always the other one, "#" first
S5 = qr.encode_span([0, 1, 0, 1, 0], TAB, 2)
GOOD = _section(2, 5, b"#I", _body(TAB, [S5]))
TWO = [qr.encode_span(([0, 1] * 1024), TAB, 2), qr.encode_span([0, 1, 0], TAB, 2)]  # 2051 qualities: two spans
MALFORMED = {
    "row_sum_4095": HEAD2 + _section(2, 5, b"#I", _body([[0, 4095], [4096, 0], [4096, 0]], [S5])),
    "zero_start_row": HEAD2 + _section(2, 5, b"#I", _body([[0, 4096], [4096, 0], [0, 0]], [S5])),
    "span_size_3": HEAD2 + _section(2, 5, b"#I", _body(TAB, [S5[:3]])),
    "sizes_do_not_sum": HEAD2 + _section(2, 5, b"#I", _body(TAB, [S5]) + b"\0"),
    "sizes_past_the_body": HEAD2 + _section(3, 2051, b"#I", _body(TAB, TWO)[:-1]),
    "span_count": HEAD2 + _section(3, 2051, b"#I", _body(TAB, TWO[:1])),
    "body_at_one_symbol": HEAD2 + _section(2, 5, b"I", struct.pack("<I", 4) + S5),
    "truncated_table": HEAD2 + _section(2, 5, b"#I", _body(TAB, [S5])[:10]),
    "truncated_body": HEAD2 + GOOD[:-1],
    "no_body_at_two_symbols": HEAD2 + _section(2, 5, b"#I", b""),
    "coder_byte_2": HEAD2[:9] + b"\x02" + HEAD2[10:] + GOOD,
    "coder_byte_0": HEAD2[:9] + b"\x00" + HEAD2[10:] + GOOD,
    "header_pad": HEAD2[:31] + b"\x01" + GOOD,
    "version_3": HEAD2[:4] + struct.pack("<I", 3) + HEAD2[8:] + GOOD,
    "v1_header_over_a_v2_section": HEAD1 + GOOD,
    "width_too_large": HEAD2 + GOOD[:16] + b"\x02" + GOOD[17:],
}


def test_side_file_good_by_hand(tmp_path):
    p = tmp_path / "g.ntcq"
    p.write_bytes(HEAD2 + GOOD + _section(1, 3, b"I", b"") + _section(3, 2051, b"#I", _body(TAB, TWO)))
    mode, metas, pay = nt.read_qualities(p)
    b0, b2 = _body(TAB, [S5]), _body(TAB, TWO)
    assert mode == 1 and pay == b0 + bytes(-len(b0) % 8) + b2 + bytes(-len(b2) % 8)
    assert [(m.n_reads, m.n_quals, m.width, m.n_syms, m.payload_off, m.payload_bytes, m.coder) for m in metas] == \
        [(2, 5, 1, 2, 0, len(b0), 1), (1, 3, 0, 1, 24, 0, 1), (3, 2051, 1, 2, 24, len(b2), 1)]
    assert len(b0) == 12 + 4 + 4
    assert qr.decode_body(b0, 5, 2, b"#I") == (b"#I#I#", True)


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_side_file_malformed_is_refused(tmp_path, what):
    p = tmp_path / "bad.ntcq"
    p.write_bytes(MALFORMED[what])
    with pytest.raises(nt.NtcError) as e:
        nt.read_qualities(p)
    assert e.value.code == FORMAT


# ---- exports and the Python surface -------------------------------------------------------------
def test_exports_and_python_surface():
    L = nt.lib()
    assert "ntc_q_write_header2" in nt.EXPORTED and hasattr(L, "ntc_q_write_header2")
    assert nt.QUALITY_CODERS == {"pack": 0, "rans": 1}
    assert ctypes.sizeof(nt.QualMeta) == 136 and nt.QualMeta.alphabet.offset == 40 and nt.QualMeta.reserved.offset == 34
    m = nt.QualMeta()
    assert m.coder == 0
    m.coder = 1
    assert bytes(m.reserved) == b"\x01" + bytes(5)
    import inspect
    for fn, arg in ((nt.GpuContext.encode_pack_fastq, "quality_coder"), (nt.write_qualities, "coder")):
        assert arg in inspect.signature(fn).parameters, (fn.__name__, arg)
    assert isinstance(nt.GpuContext.quality_coder, property)
    assert L.ntc_q_write_header2(-1, 1, 1) == INVALID_ARG and L.ntc_q_write_header2(-1, 1, 0) == INVALID_ARG


# ---- both command lines -------------------------------------------------------------------------
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")


def _cli(which, *args, cwd):
    cmd = [NATIVE] if which == "native" else [sys.executable, "-m", "ntcomp_amd"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + list(args), cwd=cwd, capture_output=True, env=env, timeout=120)


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_argument_rules(tmp_path, which):
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    common = ["encode", "-i", str(tmp_path / "noindex"), str(tmp_path / "r.fq")]
    for mode in (["--qualities", "drop"], []):
        r = _cli(which, *common, *mode, "--quality-coder", "rans", cwd=tmp_path)
        assert r.returncode == 2 and r.stdout == b"", r.stderr
        assert r.stderr.strip() == b"ntcomp: encode: --quality-coder needs --qualities keep or bin8"
    r = _cli(which, *common, "--qualities", "keep", "--quality-file", str(tmp_path / "q.ntcq"), "--quality-coder", "huff",
             cwd=tmp_path)
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.strip() == b"ntcomp: encode: --quality-coder: pack or rans"
    assert not (tmp_path / "q.ntcq").exists()  # nothing is written


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_help_lists_the_flag(tmp_path, which):
    r = _cli(which, "encode", "--help", cwd=tmp_path)
    assert r.returncode == 0 and b"--quality-coder" in r.stdout and b"rans" in r.stdout
