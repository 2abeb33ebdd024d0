"""FASTQ read names, the parts that need no GPU: the "NTCN" side file (ntc_n_write_* /
ntc_n_read), the kernels' per-name logic compiled for the CPU under ASan + UBSan
(tests/names_cpu), and the Python and command-line surface.

The checker is names_lib.py (plain Python / numpy); it tests itself on import."""
import ctypes
import gzip
import inspect
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import names_lib as nl
import ntcomp_amd as nt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT = 1, 8
ENGINE = "libdeflate" if nt.libdeflate_available() else "zlib"


def _nmetas(names, block_reads):
    """names_lib's sections as (list of nt.NameMeta, payload bytes)"""
    metas, pay = nl.sections(names, block_reads)
    return [nt.NameMeta(m["n_reads"], m["name_bytes"], m["mid_bytes"], m["payload_off"], m["payload_bytes"])
            for m in metas], pay


def _write(path, mode, metas, payload, header=True):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        nt.write_names(fd, mode, metas, payload, header=header, engine=ENGINE)
    finally:
        os.close(fd)


def _names(seed=1, n=300):
    rng = np.random.default_rng(seed)
    return nl.illumina_names(rng, n // 2) + nl.sra_names(n - n // 2)


# ---- side file --------------------------------------------------------------------------------
def test_side_file_round_trip(tmp_path):
    names = _names()
    metas, payload = _nmetas(names, 128)
    assert [m.n_reads for m in metas] == [128, 128, 44]
    p = tmp_path / "n.ntcn"
    _write(p, "keep", metas, payload)
    mode, got, pay = nt.read_names(p)
    assert mode == 1 and pay == payload
    assert [nl.meta_dict(m) for m in got] == [nl.meta_dict(m) for m in metas]
    raw = p.read_bytes()
    assert raw[:32] == b"NTCN" + struct.pack("<IB", 1, 1) + bytes(23)
    n_reads, name_bytes, mid_bytes, gz, zero = struct.unpack_from("<QQQII", raw, 32)  # the first section, by hand
    assert (n_reads, name_bytes, mid_bytes, zero) == (128, metas[0].name_bytes, metas[0].mid_bytes, 0)
    body = gzip.decompress(raw[64:64 + gz])
    assert body == payload[:metas[0].payload_bytes]
    assert nl.expand(nl.meta_dict(metas[0]), body) == names[:128]


def test_side_file_of_an_empty_input_is_the_header_alone(tmp_path):
    p = tmp_path / "e.ntcn"
    _write(p, "id", [], b"")
    assert p.read_bytes() == b"NTCN" + struct.pack("<IB", 1, 2) + bytes(23)
    assert nt.read_names(p) == (2, [], b"")


def _member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def _body(lens, pres, sufs, mid, pad=None):
    b = np.array(lens, dtype="<u2").tobytes() + bytes(pres) + bytes(sufs) + mid
    return b + (bytes(-len(b) % 8) if pad is None else pad)


def _section(n_reads, name_bytes, mid_bytes, body, gz=None, pad=0):
    m = _member(body)
    return struct.pack("<QQQII", n_reads, name_bytes, mid_bytes, len(m) if gz is None else gz, pad) + m


HEAD = b"NTCN" + struct.pack("<IB", 1, 1) + bytes(23)
# the worked example: r1/ab r2/ab r2/ab r
GOOD_BODY = _body([5, 5, 5, 1], [0, 1, 5, 1], [0, 3, 0, 0], b"r1/ab2")
GOOD = _section(4, 16, 6, GOOD_BODY)
# 65 names "ab": read 64 restarts the chain
RESTART = _body([2] * 65, [0] + [2] * 63 + [1], [0] * 65, b"ab" + b"b")
MALFORMED = {
    "magic": b"NTCQ" + HEAD[4:] + GOOD,
    "version": HEAD[:4] + struct.pack("<I", 2) + HEAD[8:] + GOOD,
    "mode_0": HEAD[:8] + b"\x00" + HEAD[9:] + GOOD,
    "mode_3": HEAD[:8] + b"\x03" + HEAD[9:] + GOOD,
    "header_pad": HEAD[:31] + b"\x01" + GOOD,
    "truncated_file_header": HEAD[:20],
    "truncated_section_header": HEAD + GOOD[:31],
    "truncated_member": HEAD + GOOD[:-1],
    "section_pad": HEAD + _section(4, 16, 6, GOOD_BODY, pad=1),
    "member_too_long": HEAD + _section(4, 16, 6, GOOD_BODY + bytes(8)),
    "member_too_short": HEAD + _section(4, 16, 6, GOOD_BODY[:16]),
    "member_not_gzip": HEAD + GOOD[:34] + b"\x00" * (len(GOOD) - 34),
    "len_4096": HEAD + _section(2, 4096, 4096, _body([4096, 0], [0, 0], [0, 0], b"x" * 4096)),
    "pre_plus_suf_past_len": HEAD + _section(2, 4, 3, _body([3, 1], [0, 1], [0, 1], b"abc")),
    "pre_past_previous": HEAD + _section(2, 4, 2, _body([1, 3], [0, 2], [0, 0], b"a" + b"c")),
    "suf_past_previous": HEAD + _section(2, 4, 2, _body([1, 3], [0, 0], [0, 2], b"a" + b"c")),
    "restart_pre": HEAD + _section(1, 2, 1, _body([2], [1], [0], b"a")),
    "restart_suf": HEAD + _section(1, 2, 1, _body([2], [0], [1], b"a")),
    "restart_pre_at_64": HEAD + _section(65, 130, 3, RESTART),
    "mids_do_not_sum": HEAD + _section(4, 16, 7, _body([5, 5, 5, 1], [0, 1, 5, 1], [0, 3, 0, 0], b"r1/ab2x")),
    "names_do_not_sum": HEAD + _section(4, 17, 6, GOOD_BODY),
    "padding_bytes": HEAD + _section(4, 16, 6, _body([5, 5, 5, 1], [0, 1, 5, 1], [0, 3, 0, 0], b"r1/ab2", pad=b"\x00\x01")),
    "mid_bytes_past_name_bytes": HEAD + _section(1, 1, 4, _body([1], [0], [0], b"abcd")),
}


def test_side_file_good_by_hand(tmp_path):
    p = tmp_path / "g.ntcn"
    ok65 = _body([2] * 65, [0] + [2] * 63 + [0], [0] * 65, b"ab" + b"ab")
    p.write_bytes(HEAD + GOOD + _section(65, 130, 4, ok65) + _section(1, 0, 0, _body([0], [0], [0], b"")))
    mode, metas, pay = nt.read_names(p)
    assert mode == 1 and pay == GOOD_BODY + ok65 + _body([0], [0], [0], b"")
    assert [(m.n_reads, m.name_bytes, m.mid_bytes, m.payload_off, m.payload_bytes) for m in metas] == \
        [(4, 16, 6, 0, 24), (65, 130, 4, 24, 264), (1, 0, 0, 288, 8)]
    assert nl.expand(nl.meta_dict(metas[0]), pay[:24]) == [b"r1/ab", b"r2/ab", b"r2/ab", b"r"]
    assert nl.expand(nl.meta_dict(metas[1]), pay[24:288]) == [b"ab"] * 65


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_side_file_malformed_is_refused(tmp_path, what):
    p = tmp_path / "bad.ntcn"
    p.write_bytes(MALFORMED[what])
    with pytest.raises(nt.NtcError) as e:
        nt.read_names(p)
    assert e.value.code == FORMAT


def test_side_file_writer_refuses_a_meta_that_is_not_canonical(tmp_path):
    names = _names()
    for field, delta in (("payload_bytes", 8), ("mid_bytes", 1), ("name_bytes", 1)):
        metas, payload = _nmetas(names, 128)
        setattr(metas[1], field, getattr(metas[1], field) + delta)
        with pytest.raises(nt.NtcError) as e:
            _write(tmp_path / "w.ntcn", "keep", metas, payload + bytes(8))
        assert e.value.code == INVALID_ARG, field
    with pytest.raises(nt.NtcError) as e:
        _write(tmp_path / "w.ntcn", "drop", [], b"")
    assert e.value.code == INVALID_ARG


# ---- per-name logic on the CPU, under ASan + UBSan --------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("names_cpu") / "names_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "names_cpu", "names_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _core(exe, tmp_path, headers, block_reads, mode):
    blob = struct.pack("<IIQ", nl.MODES[mode], block_reads, len(headers)) + \
        b"".join(struct.pack("<I", len(h)) + h for h in headers)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    out = (tmp_path / "out.bin").read_bytes()
    status, nb = struct.unpack_from("<QQ", out, 0)
    at, metas, pay = 16, [], b""
    for _ in range(nb):
        m = dict(zip(("n_reads", "name_bytes", "mid_bytes", "payload_off", "payload_bytes"), struct.unpack_from("<5Q", out, at)))
        metas.append(m)
        pay += out[at + 40:at + 40 + m["payload_bytes"]]
        at += 40 + m["payload_bytes"]
    assert at == len(out)
    return status, metas, pay


def test_core_on_edge_names_and_both_modes(core_exe, tmp_path):
    names = nl.edge_names()
    names = names + nl.illumina_names(np.random.default_rng(3), 448 - 29 - len(names)) + [b"dup"] * 29
    assert len(names) == 448
    names[63] = names[64] = b"across:the:group"     # 63 -> 64 restarts
    names[127] = names[128] = b"across:the:block"   # the block boundary
    for mode in ("keep", "id"):
        for eol in (b"", b"\r"):
            status, metas, pay = _core(core_exe, tmp_path, [b"@" + n + eol for n in names], 128, mode)
            exp = [nl.name_of(b"@" + n, mode) for n in names]
            assert status == 2 ** 64 - 1
            assert (metas, pay) == nl.sections(exp, 128), (mode, eol)
    m, pay = nl.sections(names, 128)
    assert {x["payload_bytes"] - 4 * x["n_reads"] - x["mid_bytes"] for x in m} != {0}  # some section is padded


def test_core_id_cut_and_errors(core_exe, tmp_path):
    hs = [b"@a b c", b"@a\tb", b"@nowhitespace", b"@ leading", b"@" + b"x" * 70 + b" y", b"@" + b"x" * 70 + b" z"]
    status, metas, pay = _core(core_exe, tmp_path, hs, 128, "id")
    assert status == 2 ** 64 - 1 and (metas, pay) == nl.sections([b"a", b"a", b"nowhitespace", b"", b"x" * 70, b"x" * 70], 128)
    long = b"@" + b"n" * 4096
    assert _core(core_exe, tmp_path, [b"@ok", long, b"@ok", long], 128, "keep")[0] == (1 << 8 | FORMAT)
    assert _core(core_exe, tmp_path, [b"@ok", b"@" + b"n" * 4095 + b"\r"], 128, "keep")[0] == 2 ** 64 - 1
    assert _core(core_exe, tmp_path, [b"@ok", b"@" + b"n" * 4095 + b" " + b"c" * 50], 128, "id")[0] == 2 ** 64 - 1


# ---- exports and the Python surface -----------------------------------------------------------
def test_exports_and_python_surface():
    L = nt.lib()
    for name in ("ntc_encode_names", "ntc_decode_set_names", "ntc_n_write_header", "ntc_n_write_section",
                 "ntc_n_deflate_section", "ntc_n_read", "ntc_encode_file_ex2", "ntc_decode_file_ex2"):
        assert name in nt.EXPORTED and hasattr(L, name), name
    assert ctypes.sizeof(nt.NameMeta) == 40
    assert [f for f, _ in nt.NameMeta._fields_] == ["n_reads", "name_bytes", "mid_bytes", "payload_off", "payload_bytes"]
    assert nt.NAMES == {"drop": 0, "keep": 1, "id": 2} and (nt.NAME_MAX, nt.NAME_GROUP) == (4095, 64)
    for fn, arg in ((nt.GpuContext.encode_pack_fastq, "names"), (nt.GpuContext.set_names, "metas"),
                    (nt.read_names, "path"), (nt.write_names, "fd"), (nt.encode_file, "names"), (nt.encode_file, "n_fd"),
                    (nt.decode_file, "n_path")):
        assert arg in inspect.signature(fn).parameters, (fn.__name__, arg)
    assert callable(nt.GpuContext.names)
    n, b = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.ntc_encode_names(None, None, 0, None, 0, ctypes.byref(n), ctypes.byref(b)) == 1
    assert L.ntc_decode_set_names(None, None, 0, None, 0) == 1


def test_pipeline_structs_and_entry_points():
    L = nt.lib()
    F = nt.FileOpts2
    assert ctypes.sizeof(F) == 56 and ctypes.sizeof(nt.NStats) == 40 and ctypes.sizeof(nt.FileOpts) == 32
    assert [(f, getattr(F, f).offset) for f, _ in F._fields_] == \
        [("struct_bytes", 0), ("nx_policy", 4), ("nx_fd", 8), ("q_mode", 12), ("q_fd", 16), ("nx_path", 24),
         ("q_path", 32), ("n_mode", 40), ("n_fd", 44), ("n_path", 48)]
    assert [f for f, _ in nt.NStats._fields_] == ["sections", "names", "name_bytes", "payload_bytes", "deflated_bytes"]
    assert L.ntc_encode_file_ex2(None, 0, b"x", 1, None, None, None, None, None, None) == 1
    assert L.ntc_decode_file_ex2(None, 0, b"x", 1, None, None, None) == 1
    # a struct that says it is shorter than this library's is refused before anything else is read
    fo = F(ctypes.sizeof(F) - 8, 0, -1, 0, -1, None, None, 1, 1, None)
    arr = (ctypes.c_void_p * 1)(None)
    assert L.ntc_encode_file_ex2(arr, 1, b"x", 1, ctypes.byref(fo), None, None, None, None, None) == 1
    assert L.ntc_decode_file_ex2(arr, 1, b"x", 1, ctypes.byref(fo), None, None) == 1


# ---- both command lines -----------------------------------------------------------------------
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")


def _cli(which, *args, cwd):
    cmd = [NATIVE] if which == "native" else [sys.executable, "-m", "ntcomp_amd"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + list(args), cwd=cwd, capture_output=True, env=env, timeout=120)


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_argument_rules(tmp_path, which):
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    common = ["encode", "-i", str(tmp_path / "noindex"), str(tmp_path / "r.fq")]
    for mode in ("keep", "id"):
        r = _cli(which, *common, "--names", mode, cwd=tmp_path)
        assert r.returncode == 2 and r.stdout == b"", r.stderr
        assert b"ntcomp: encode: --names " + mode.encode() + b" requires --name-file PATH" in r.stderr
    for mode in (["--names", "drop"], []):
        r = _cli(which, *common, *mode, "--name-file", str(tmp_path / "n.ntcn"), cwd=tmp_path)
        assert r.returncode == 2 and r.stdout == b"", r.stderr
        assert b"ntcomp: encode: --name-file is only written under --names keep or id" in r.stderr
    r = _cli(which, *common, "--names", "all", cwd=tmp_path)
    assert r.returncode == 2 and b"ntcomp: encode: --names: drop, keep or id" in r.stderr
    assert not (tmp_path / "n.ntcn").exists()  # nothing is written


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_help_lists_both_flags(tmp_path, which):
    for command in ("encode", "decode"):
        r = _cli(which, command, "--help", cwd=tmp_path)
        assert r.returncode == 0
        assert b"--name-file" in r.stdout, command
        if command == "encode" or which == "native":
            assert b"--names" in r.stdout
