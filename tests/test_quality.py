"""FASTQ quality scores, the parts that need no GPU: the "NTCQ" side file (ntc_q_write_* /
ntc_q_read), the kernels' lane logic compiled for the CPU under ASan + UBSan
(tests/quality_cpu), the checker's own self-test, and the Python surface.

The checker is qual_lib.py (numpy): mode tables, alphabet, width rule, bit packing."""
import ctypes
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import ntcomp_amd as nt
import qual_lib as ql

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT = 1, 8
ENGINE = "libdeflate" if nt.libdeflate_available() else "zlib"


def _qmetas(text, block_reads, mode="keep"):
    """qual_lib's sections as (list of nt.QualMeta, payload bytes)"""
    metas, words = ql.sections(text, block_reads, mode)
    out = []
    for m in metas:
        q = nt.QualMeta()
        q.n_reads, q.n_quals, q.width, q.n_syms = m["n_reads"], m["n_quals"], m["width"], m["n_syms"]
        q.payload_off, q.payload_bytes = m["payload_off"], m["payload_bytes"]
        ctypes.memmove(q.alphabet, m["alphabet"], len(m["alphabet"]))
        out.append(q)
    return out, words.astype("<u8").tobytes()


def _write(path, mode, metas, payload, header=True):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        nt.write_qualities(fd, mode, metas, payload, header=header, engine=ENGINE)
    finally:
        os.close(fd)


def _text(seed=1, syms=(4, 40, 1, 2), block_reads=64):
    reads, quals = ql.ragged_batch(np.random.default_rng(seed), list(syms), block_reads, block_reads * (len(syms) - 1) + 9)
    return ql.make_fastq(reads, quals)


# ---- side file --------------------------------------------------------------------------------
def test_side_file_round_trip(tmp_path):
    metas, payload = _qmetas(_text(), 64)
    assert [m.width for m in metas] == [2, 8, 0, 1]
    p = tmp_path / "q.ntcq"
    _write(p, "keep", metas, payload)
    mode, got, pay = nt.read_qualities(p)
    assert mode == 1 and pay == payload
    assert [ql.meta_dict(m) for m in got] == [ql.meta_dict(m) for m in metas]
    raw = p.read_bytes()
    assert raw[:32] == b"NTCQ" + struct.pack("<IB", 1, 1) + bytes(23)
    n_reads, n_quals, w, n_syms, zero, gz = struct.unpack_from("<QQBBHI", raw, 32)  # the first section, by hand
    assert (n_reads, n_quals, w, n_syms, zero) == (64, metas[0].n_quals, 2, 4, 0)
    assert raw[56:60] == bytes(metas[0].alphabet)[:4]
    assert gzip.decompress(raw[60:60 + gz]) == payload[:metas[0].payload_bytes]
    sec2 = 60 + gz + 24 + 40  # the width-0 section: header + 1 alphabet byte, no member
    gz2, = struct.unpack_from("<I", raw, 60 + gz + 20)
    assert struct.unpack_from("<QQBBHI", raw, sec2 + gz2)[2:] == (0, 1, 0, 0)


def test_side_file_of_an_empty_input_is_the_header_alone(tmp_path):
    p = tmp_path / "e.ntcq"
    _write(p, "bin8", [], b"")
    assert p.read_bytes() == b"NTCQ" + struct.pack("<IB", 1, 2) + bytes(23)
    assert nt.read_qualities(p) == (2, [], b"")


def _member(words):
    import zlib
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(words) + c.flush()


def _section(n_reads, n_quals, w, alphabet, words, gz=None, pad=0):
    body = _member(words) if w else b""
    return struct.pack("<QQBBHI", n_reads, n_quals, w, len(alphabet), pad, len(body) if gz is None else gz) + alphabet + body


HEAD = b"NTCQ" + struct.pack("<IB", 1, 1) + bytes(23)
GOOD = _section(2, 5, 1, b"#I", struct.pack("<Q", 0b10110))
MALFORMED = {
    "magic": b"NTCX" + HEAD[4:] + GOOD,
    "version": HEAD[:4] + struct.pack("<I", 2) + HEAD[8:] + GOOD,
    "mode_0": HEAD[:8] + b"\x00" + HEAD[9:] + GOOD,
    "mode_3": HEAD[:8] + b"\x03" + HEAD[9:] + GOOD,
    "header_pad": HEAD[:31] + b"\x01" + GOOD,
    "truncated_file_header": HEAD[:20],
    "truncated_section_header": HEAD + GOOD[:23],
    "truncated_alphabet": HEAD + GOOD[:25],
    "truncated_member": HEAD + GOOD[:-1],
    "width_too_small": HEAD + _section(2, 5, 1, b"#+I", struct.pack("<Q", 0b10110)),
    "width_too_large": HEAD + _section(2, 5, 2, b"#I", struct.pack("<Q", 0b0100010100)),
    "width_3": HEAD + _section(2, 5, 3, b"#$%&I", struct.pack("<Q", 0)),
    "alphabet_descending": HEAD + _section(2, 5, 1, b"I#", struct.pack("<Q", 0b10110)),
    "alphabet_repeats": HEAD + _section(2, 5, 1, b"II", struct.pack("<Q", 0b10110)),
    "alphabet_space": HEAD + _section(2, 5, 1, b" I", struct.pack("<Q", 0b10110)),
    "alphabet_del": HEAD + _section(2, 5, 1, b"I\x7f", struct.pack("<Q", 0b10110)),
    "member_too_long": HEAD + _section(2, 5, 1, b"#I", struct.pack("<QQ", 0b10110, 0)),
    "member_too_short": HEAD + _section(2, 65, 1, b"#I", struct.pack("<Q", 0b10110)),
    "member_not_gzip": HEAD + GOOD[:26] + b"\x00" * (len(GOOD) - 26),
    "padding_bits": HEAD + _section(2, 5, 1, b"#I", struct.pack("<Q", 0b110110)),
    "section_pad": HEAD + _section(2, 5, 1, b"#I", struct.pack("<Q", 0b10110), pad=1),
    "member_at_width_0": HEAD + struct.pack("<QQBBHI", 2, 5, 0, 1, 0, 4) + b"I" + b"\x00" * 4,
    "no_member_at_width_1": HEAD + struct.pack("<QQBBHI", 2, 5, 1, 2, 0, 0) + b"#I",
}


def test_side_file_good_by_hand(tmp_path):
    p = tmp_path / "g.ntcq"
    p.write_bytes(HEAD + GOOD + _section(1, 3, 0, b"I", b""))
    mode, metas, pay = nt.read_qualities(p)
    assert mode == 1 and pay == struct.pack("<Q", 0b10110)
    assert [(m.n_reads, m.n_quals, m.width, m.n_syms, m.payload_off, m.payload_bytes) for m in metas] == \
        [(2, 5, 1, 2, 0, 8), (1, 3, 0, 1, 8, 0)]


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_side_file_malformed_is_refused(tmp_path, what):
    p = tmp_path / "bad.ntcq"
    p.write_bytes(MALFORMED[what])
    with pytest.raises(nt.NtcError) as e:
        nt.read_qualities(p)
    assert e.value.code == FORMAT


def test_side_file_writer_refuses_a_meta_that_is_not_canonical(tmp_path):
    metas, payload = _qmetas(_text(), 64)
    metas[0].width = 4
    with pytest.raises(nt.NtcError) as e:
        _write(tmp_path / "w.ntcq", "keep", metas, payload)
    assert e.value.code == INVALID_ARG
    with pytest.raises(nt.NtcError) as e:
        _write(tmp_path / "w.ntcq", "drop", [], b"")
    assert e.value.code == INVALID_ARG


# ---- lane logic on the CPU, under ASan + UBSan ------------------------------------------------
@pytest.fixture(scope="module")
def lane_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quality_cpu") / "quality_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "quality_cpu", "quality_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _lanes(exe, tmp_path, text, block_reads, mode):
    recs = ql.records(text)
    kept = np.array([len(s) for s, _ in recs], dtype="<u8")
    qoff = np.zeros(len(recs) + 1, dtype="<u8")
    qoff[1:] = np.cumsum([len(q) for _, q in recs])
    blob = struct.pack("<IIQ", ql.MODES[mode], block_reads, len(recs)) + kept.tobytes() + qoff.tobytes() + \
        b"".join(q for _, q in recs)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    out = (tmp_path / "out.bin").read_bytes()
    status, nb = struct.unpack_from("<QQ", out, 0)
    at, metas, words = 16, [], []
    if status != 2 ** 64 - 1:
        return status, metas, np.zeros(0, dtype=np.uint64)
    off = 0
    for _ in range(nb):
        nq, w, ns = struct.unpack_from("<QQQ", out, at)
        alphabet = out[at + 24:at + 24 + ns]
        assert out[at + 24 + ns:at + 120] == bytes(96 - ns)
        nw, = struct.unpack_from("<Q", out, at + 120)
        words.append(np.frombuffer(out, dtype="<u8", count=nw, offset=at + 128))
        metas.append(dict(n_quals=nq, width=w, n_syms=ns, alphabet=alphabet, payload_off=8 * off, payload_bytes=8 * nw))
        off += nw
        at += 128 + 8 * nw
    assert at == len(out)
    return status, metas, np.concatenate(words)


def _same(got, exp):
    strip = lambda ms: [{k: v for k, v in m.items() if k != "n_reads"} for m in ms]
    assert strip(got[1]) == strip(exp[0]) and np.array_equal(got[2], exp[1])


@pytest.mark.parametrize("n_syms", [1, 2, 3, 4, 5, 16, 17, 94])
def test_lane_logic_widths_and_word_boundaries(lane_exe, tmp_path, n_syms):
    """The shapes of GPU test 1: ragged reads of 1..300 in three and a half blocks that hold
    63, 1, 0 qualities modulo 64."""
    reads, quals = ql.ragged_batch(np.random.default_rng(100 + n_syms), [n_syms] * 4, 1024, 3 * 1024 + 512)
    text = ql.make_fastq(reads, quals)
    got = _lanes(lane_exe, tmp_path, text, 1024, "keep")
    assert got[0] == 2 ** 64 - 1 and [m["n_quals"] % 64 for m in got[1][:3]] == [63, 1, 0]
    _same(got, ql.sections(text, 1024))


def test_lane_logic_per_block_alphabets_bin8_and_errors(lane_exe, tmp_path):
    reads, quals = ql.ragged_batch(np.random.default_rng(2), [2, 17, 1], 1024, 3 * 1024)
    text = ql.make_fastq(reads, quals)
    got = _lanes(lane_exe, tmp_path, text, 1024, "keep")
    assert [(m["n_syms"], m["width"]) for m in got[1]] == [(2, 1), (17, 8), (1, 0)]
    _same(got, ql.sections(text, 1024))
    reads, quals = ql.ragged_batch(np.random.default_rng(4), [94], 512, 300, ends=())
    text = ql.make_fastq(reads, quals)
    got = _lanes(lane_exe, tmp_path, text, 512, "bin8")
    assert got[1][0]["n_syms"] == 9
    _same(got, ql.sections(text, 512, "bin8"))
    for bad in (b"II\x1fI", b"II\x7fI", b"III"):
        t = ql.make_fastq([b"ACGT"] * 3, [b"IIII", b"IIII", bad])
        assert _lanes(lane_exe, tmp_path, t, 2, "keep")[0] == (2 << 8 | FORMAT)


# ---- the checker itself -----------------------------------------------------------------------
def test_checker_on_a_hand_written_case():
    text = b"@a\nACGTA\n+\nI#II#\n@b\nAC GT\r\n+\r\n#I#I\r\n@c\nacgu\n+\n5555"
    assert ql.records(text) == [(b"ACGTA", b"I#II#"), (b"ACGT", b"#I#I"), (b"ACGT", b"5555")]
    metas, words = ql.sections(text, 2)
    # block 0: "I#II#" "#I#I" over {#, I}: codes 1 0 1 1 0  0 1 0 1, one bit each, first lowest
    assert metas[0] == dict(n_reads=2, n_quals=9, width=1, n_syms=2, alphabet=b"#I", payload_off=0, payload_bytes=8)
    assert metas[1] == dict(n_reads=1, n_quals=4, width=0, n_syms=1, alphabet=b"5", payload_off=8, payload_bytes=0)
    assert words.tolist() == [0b101001101]
    # three symbols take two bits: # = 0, 5 = 1, I = 2
    _, w3 = ql.sections(b"@a\nACGTA\n+\nI#5I#\n", 4)
    assert w3.tolist() == [0b00_10_01_00_10]
    # 17 symbols take a byte each: nine qualities spill into a second word
    q = bytes(range(40, 57))
    m, w = ql.sections(b"@a\n" + b"A" * 17 + b"\n+\n" + q + b"\n", 1)
    assert m[0]["width"] == 8 and w.tolist() == [0x0706050403020100, 0x0F0E0D0C0B0A0908, 0x10]
    assert [ql.width(n) for n in (1, 2, 3, 4, 5, 16, 17, 94)] == [0, 1, 2, 2, 4, 4, 8, 8]
    assert ql.unpack(w, 17, 8).tolist() == list(range(17))
    tab = ql.mode_table("bin8")
    assert bytes(tab[33:75]) == bytes(33 + v for v in [0, 1] + [6] * 8 + [15] * 10 + [22] * 5 + [27] * 5 + [33] * 5 +
                                      [37] * 5 + [40] * 2)
    assert not tab[:33].any() and not tab[127:].any() and (tab[74:127] == 73).all()
    assert ql.fastq_text([(b"AC", b"I#")], 9) == b"@seq.9\nAC\n+\nI#\n"


# ---- exports and the Python surface -----------------------------------------------------------
def test_exports_and_python_surface():
    L = nt.lib()
    for name in ("ntc_encode_qualities", "ntc_decode_set_qualities", "ntc_q_write_header", "ntc_q_write_section",
                 "ntc_q_deflate_section", "ntc_q_read"):
        assert name in nt.EXPORTED and hasattr(L, name), name
    assert ctypes.sizeof(nt.QualMeta) == 136 and nt.QualMeta.alphabet.offset == 40
    assert nt.QUALITIES == {"drop": 0, "keep": 1, "bin8": 2}
    import inspect
    for fn, arg in ((nt.GpuContext.encode_pack_fastq, "qualities"), (nt.GpuContext.set_qualities, "metas"),
                    (nt.read_qualities, "path"), (nt.write_qualities, "fd")):
        assert arg in inspect.signature(fn).parameters, (fn.__name__, arg)
    assert callable(nt.GpuContext.qualities)
    n, b = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.ntc_encode_qualities(None, None, 0, None, 0, ctypes.byref(n), ctypes.byref(b)) == 1
    assert L.ntc_decode_set_qualities(None, None, 0, None, 0) == 1


# ---- both command lines -----------------------------------------------------------------------
import sys  # noqa: E402

NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")


def _cli(which, *args, cwd):
    cmd = [NATIVE] if which == "native" else [sys.executable, "-m", "ntcomp_amd"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + list(args), cwd=cwd, capture_output=True, env=env, timeout=120)


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_argument_rules(tmp_path, which):
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    common = ["encode", "-i", str(tmp_path / "noindex"), str(tmp_path / "r.fq")]
    for mode in ("keep", "bin8"):
        r = _cli(which, *common, "--qualities", mode, cwd=tmp_path)
        assert r.returncode == 2 and r.stdout == b"", r.stderr
        assert b"ntcomp: encode: --qualities " + mode.encode() + b" requires --quality-file PATH" in r.stderr
    for mode in (["--qualities", "drop"], []):
        r = _cli(which, *common, *mode, "--quality-file", str(tmp_path / "q.ntcq"), cwd=tmp_path)
        assert r.returncode == 2 and r.stdout == b"", r.stderr
        assert b"ntcomp: encode: --quality-file is only written under --qualities keep or bin8" in r.stderr
    r = _cli(which, *common, "--qualities", "bin4", cwd=tmp_path)
    assert r.returncode == 2 and b"ntcomp: encode: --qualities: drop, keep or bin8" in r.stderr
    assert not (tmp_path / "q.ntcq").exists()  # nothing is written


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_help_lists_both_flags(tmp_path, which):
    for command in ("encode", "decode"):
        r = _cli(which, command, "--help", cwd=tmp_path)
        assert r.returncode == 0
        assert b"--quality-file" in r.stdout, command
        if command == "encode" or which == "native":
            assert b"--qualities" in r.stdout


def test_pipeline_surface():
    L = nt.lib()
    for name in ("ntc_encode_file_ex", "ntc_decode_file_ex"):
        assert name in nt.EXPORTED and hasattr(L, name), name
    assert ctypes.sizeof(nt.FileOpts) == 32 and ctypes.sizeof(nt.QStats) == 32
    import inspect
    for fn, arg in ((nt.encode_file, "qualities"), (nt.encode_file, "q_fd"), (nt.decode_file, "q_path")):
        assert arg in inspect.signature(fn).parameters, (fn.__name__, arg)
    assert L.ntc_encode_file_ex(None, 0, b"x", 1, None, None, None, None, None) == 1
    assert L.ntc_decode_file_ex(None, 0, b"x", 1, None, None, None) == 1
