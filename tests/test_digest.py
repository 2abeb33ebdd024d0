"""Per-block content digests without a GPU: the definition (pinned values, what the digest is
sensitive to), digest_core.h walked the kernels' way under ASan + UBSan (tests/digest_cpu), the
"NTCD" side file's writer and reader, and the argument checks of the pipelines and both command
lines.

The checker is independent of the code under test: digest_lib.py (plain Python)."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import digest_lib as dl
import ntcomp_amd as nt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
INVALID_ARG, FORMAT, UNSUPPORTED, DIGEST = 1, 8, 10, 12

PINNED_H = [(b"", 0xb55a8fa067537a73), (b"A", 0x17fbe03c9924f9f4), (b"A\0", 0xd5b33c276aee02e9),
            (b"ACGT", 0x4b141c047736ab3e), (b"ACGTACGT", 0xe6e951f43f1ea5e3), (b"ACGTACGTA", 0x9cca506ba38f9281),
            (b"ACGT" * 40, 0x7ea4201fefdcce41)]
PINNED_D = [([], 0), ([b""], 0xda88981a7cad61f1), ([b"ACGT", b"A"], 0x65f1adcc15f45fae),
            ([b"A", b"ACGT"], 0x755b7c2310c3a606), ([b"ACG", b"TA"], 0x5e2aea6c9dafad28),
            ([b"ACGT" * 40] * 3, 0x2244f7ebc8672972)]


# ---- the definition ------------------------------------------------------------------------------
def test_pinned_values():
    for s, v in PINNED_H:
        assert dl.h(s) == v, s
    for strings, v in PINNED_D:
        assert dl.D(strings) == v, strings


def test_long_strings_take_the_same_sum():
    """digest_lib's vectorised form of h (strings past 4096 bytes) is the plain one"""
    s = bytes(np.random.default_rng(1).integers(0, 256, 4097 + 13, dtype=np.uint8))
    inner = sum(dl.mix(int.from_bytes(s[8 * j:8 * j + 8], "little") + (j + 1) * dl.K1) for j in range((len(s) + 7) // 8))
    assert dl.h(s) == dl.mix((len(s) + 1) * dl.K0 + inner)


def test_sensitivities():
    a, b, c = b"ACGTTGCA", b"TTTT", b"GATTACA"
    assert dl.D([a, b, c]) != dl.D([b, a, c])               # two reads of a block swapped
    assert dl.D([b"ACG", b"TA"]) != dl.D([b"ACGT", b"A"])   # a byte moved across a read boundary
    assert dl.D([b"A"]) != dl.D([b"A\0"])                   # a trailing NUL
    assert dl.h(b"ACGTACGT") != dl.h(b"ACGTACGT" + b"\0" * 8)  # and a whole word of them
    one = [m["d_seq"] for m in dl.metas(3, [a, b, c])]
    two = [m["d_seq"] for m in dl.metas(2, [a, b, c])]
    assert one == [dl.D([a, b, c])] and two == [dl.D([a, b]), dl.D([c])]
    assert sum(one) & dl.M != sum(two) & dl.M               # the same reads in another block split


# ---- digest_core.h on the CPU, under ASan + UBSan ------------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("digest_cpu") / "digest_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "digest_cpu", "digest_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _core(exe, strings, block_reads, lead):
    blob = struct.pack("<IIQ", block_reads, lead, len(strings)) + b"".join(struct.pack("<I", len(s)) + s for s in strings)
    r = subprocess.run([exe], input=blob, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    lines = r.stdout.decode().split()
    hs = [int(v, 16) for k, v in zip(lines[::2], lines[1::2]) if k == "h"]
    ds = [int(v, 16) for k, v in zip(lines[::2], lines[1::2]) if k == "D"]
    return hs, ds


def test_core_pinned(core_exe):
    hs, ds = _core(core_exe, [s for s, _ in PINNED_H], 100, 0)
    assert hs == [v for _, v in PINNED_H]
    for strings, v in PINNED_D:
        assert _core(core_exe, strings, 100, 3)[1] == ([v] if strings else [])


@pytest.mark.parametrize("lead", range(8))
def test_core_equals_the_restatement(core_exe, lead):
    """every length class around the word, the quarter-wave's 16 words and the long threshold, at
    every misalignment of the first string (the others follow back to back, so they start
    anywhere); bytes of every value"""
    rng = np.random.default_rng(lead)
    lens = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 135, 136, 137, 511, 512, 513, 2047, 2048, 2049,
            2056, 4095, 0, 70_000, 3]
    strings = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lens]
    strings[3] = b"\0" * 8
    for br in (1, 5, len(strings)):
        hs, ds = _core(core_exe, strings, br, lead)
        assert hs == [dl.h(s) for s in strings]
        assert ds == [dl.D(strings[i:i + br]) for i in range(0, len(strings), br)]


# ---- the "NTCD" file ---------------------------------------------------------------------------
def _metas(rng, n, components):
    ms = []
    for _ in range(n):
        m = {"n_reads": int(rng.integers(1, 70_000)), "n_bases": int(rng.integers(1, 1 << 40)), "components": components}
        for c, key in enumerate(dl.COMPONENTS):
            m["d_" + key] = int(rng.integers(1, 1 << 63)) * 2 + 1 if components >> c & 1 else 0
        ms.append(m)
    return ms


def _struct(m):
    return nt.DigestMeta(m["n_reads"], m["n_bases"], m["d_seq"], m["d_sym"], m["d_qual"], m["d_name"], m["components"], 0)


def _write(path, components, k, n_nodes, ms):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        nt.write_digests(fd, components, k, n_nodes, [_struct(m) for m in ms])
    finally:
        os.close(fd)


@pytest.mark.parametrize("components", [1, 3, 5, 9, 15])
def test_file_round_trip(tmp_path, components):
    rng = np.random.default_rng(components)
    ms = _metas(rng, 4, components)
    ms[2]["components"] = 1  # a section may have fewer components than the header
    for key in dl.COMPONENTS[1:]:
        ms[2]["d_" + key] = 0
    p = str(tmp_path / "a.ntcd")
    _write(p, components, 31, (1 << 40) + 12345, ms)
    data = open(p, "rb").read()
    assert data == dl.file_bytes(components, 31, (1 << 40) + 12345, ms)
    assert len(data) == 32 + 56 * 4 and ctypes.sizeof(nt.DigestMeta) == 56
    c, k, n, back = nt.read_digests(p)
    assert (c, k, n) == (components, 31, (1 << 40) + 12345)
    assert [m.as_dict() for m in back] == ms == dl.parse_file(data)[3]
    _write(p, 1, 5, 7, [])  # no block at all: the header alone
    assert open(p, "rb").read() == dl.file_bytes(1, 5, 7, []) and nt.read_digests(p) == (1, 5, 7, [])


def _damage(data, what):
    b = bytearray(data)
    if what == "magic":
        b[3] = ord("N")
    elif what == "version":
        b[4] = 2
    elif what == "header_pad":
        b[10] = 1
    elif what == "header_tail":
        b[31] = 1
    elif what == "length":
        b = b[:-1]
    elif what == "length_extra":
        b += b"\0" * 8
    elif what == "short":
        b = b[:20]
    elif what == "bit_outside_header":   # block 1 claims qual, the header has seq and sym only
        b[32 + 56 + 48] |= 4
    elif what == "unknown_bit":
        b[8] |= 16
    elif what == "header_without_seq":
        b[8] &= ~1
    elif what == "value_of_absent":      # d_name of block 0, whose components have no name
        b[32 + 40] = 1
    elif what == "section_pad":
        b[32 + 52] = 1
    return bytes(b)


@pytest.mark.parametrize("what", ["magic", "version", "header_pad", "header_tail", "length", "length_extra", "short",
                                  "bit_outside_header", "unknown_bit", "header_without_seq", "value_of_absent",
                                  "section_pad"])
def test_reader_refuses(tmp_path, what):
    good = dl.file_bytes(3, 31, 1000, _metas(np.random.default_rng(0), 3, 3))
    p = tmp_path / "d.ntcd"
    p.write_bytes(good)
    assert len(nt.read_digests(str(p))[3]) == 3
    bad = _damage(good, what)
    assert bad != good
    p.write_bytes(bad)
    with pytest.raises(nt.NtcError) as e:
        nt.read_digests(str(p))
    assert e.value.code == FORMAT


def test_writer_refuses(tmp_path):
    p = str(tmp_path / "w.ntcd")
    ok = _metas(np.random.default_rng(2), 1, 3)[0]
    for components in (0, 2, 16, 17):  # without seq, or a bit outside the four
        with pytest.raises(nt.NtcError) as e:
            _write(p, components, 31, 9, [])
        assert e.value.code == INVALID_ARG
    for change in ({"components": 2}, {"components": 19}, {"d_qual": 5}, {"d_name": 1}):
        with pytest.raises(nt.NtcError) as e:
            _write(p, 3, 31, 9, [dict(ok, **change)])
        assert e.value.code == INVALID_ARG
    bad = _struct(ok)
    bad.reserved = 1
    fd = os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        assert nt.lib().ntc_d_write_section(fd, ctypes.byref(bad)) == INVALID_ARG
        assert nt.lib().ntc_d_write_section(-1, ctypes.byref(_struct(ok))) == INVALID_ARG
        assert nt.lib().ntc_d_write_header(-1, 1, 31, 9) == INVALID_ARG
    finally:
        os.close(fd)
    with pytest.raises(nt.NtcError) as e:
        nt.read_digests(str(tmp_path / "absent.ntcd"))
    assert e.value.code == 9  # NTC_ERR_IO


# ---- exports, structs and the pipelines' argument checks ----------------------------------------
def test_exports_and_python_surface():
    L = nt.lib()
    for name in ("ntc_encode_digests", "ntc_decode_set_digests", "ntc_decode_digests", "ntc_d_write_header",
                 "ntc_d_write_section", "ntc_d_read", "ntc_encode_file_ex3", "ntc_decode_file_ex3"):
        assert name in nt.EXPORTED and hasattr(L, name), name
    assert nt.STATUS[DIGEST] == "NTC_ERR_DIGEST" and L.ntc_abi_version() == 1
    assert [f for f, _ in nt.DigestMeta._fields_] == ["n_reads", "n_bases", "d_seq", "d_sym", "d_qual", "d_name",
                                                      "components", "reserved"]
    assert (nt.DIGEST_SEQ, nt.DIGEST_SYM, nt.DIGEST_QUAL, nt.DIGEST_NAME) == (dl.SEQ, dl.SYM, dl.QUAL, dl.NAME) == (1, 2, 4, 8)
    import inspect
    for fn, arg in ((nt.GpuContext.encode_pack_fastq, "digests"), (nt.GpuContext.encode_pack, "digests"),
                    (nt.GpuContext.decode_set_digests, "metas"), (nt.read_digests, "path"), (nt.write_digests, "fd"),
                    (nt.encode_file, "d_fd"), (nt.decode_file, "d_path")):
        assert arg in inspect.signature(fn).parameters, (fn.__name__, arg)
    assert isinstance(nt.GpuContext.digests, property)
    assert callable(nt.GpuContext.encode_digests) and callable(nt.GpuContext.decode_digests)
    n = ctypes.c_uint64()
    assert L.ntc_encode_digests(None, None, 0, ctypes.byref(n)) == INVALID_ARG
    assert L.ntc_decode_digests(None, None, 0, ctypes.byref(n)) == INVALID_ARG
    assert L.ntc_decode_set_digests(None, None, 0) == INVALID_ARG


def test_pipeline_structs_and_argument_checks():
    L = nt.lib()
    F = nt.FileOpts3
    assert ctypes.sizeof(F) == 72 and ctypes.sizeof(nt.DStats) == 48 and ctypes.sizeof(nt.FileOpts2) == 56
    assert [(f, getattr(F, f).offset) for f, _ in F._fields_] == \
        [("struct_bytes", 0), ("nx_policy", 4), ("nx_fd", 8), ("q_mode", 12), ("q_fd", 16), ("nx_path", 24),
         ("q_path", 32), ("n_mode", 40), ("n_fd", 44), ("n_path", 48), ("d_mode", 56), ("d_fd", 60), ("d_path", 64)]
    assert L.ntc_encode_file_ex3(None, 0, b"x", 1, None, None, None, None, None, None, None) == INVALID_ARG
    assert L.ntc_decode_file_ex3(None, 0, b"x", 1, None, None, None, None) == INVALID_ARG
    # a context that is never looked at: every call below is refused on its arguments alone
    fake = ctypes.create_string_buffer(4096)
    arr = (ctypes.c_void_p * 1)(ctypes.addressof(fake))
    short = F(ctypes.sizeof(nt.FileOpts2), 0, -1, 0, -1, None, None, 0, -1, None, 0, -1, None)
    assert L.ntc_encode_file_ex3(arr, 1, b"x", 1, ctypes.byref(short), None, None, None, None, None, None) == INVALID_ARG
    assert L.ntc_decode_file_ex3(arr, 1, b"x", 1, ctypes.byref(short), None, None, None) == INVALID_ARG
    for d_mode, d_fd in ((1, -1), (0, 5), (0, 0), (2, 5), (-1, -1), (1, -2)):
        fo = F(ctypes.sizeof(F), 0, -1, 0, -1, None, None, 0, -1, None, d_mode, d_fd, None)
        rc = L.ntc_encode_file_ex3(arr, 1, b"x", 1, ctypes.byref(fo), None, None, None, None, None, None)
        assert rc == INVALID_ARG, (d_mode, d_fd)
    # out_fd -1 is ntc_decode_file_ex3's alone; any other negative descriptor is refused there too
    fo2 = nt.FileOpts2(ctypes.sizeof(nt.FileOpts2), 0, -1, 0, -1, None, None, 0, -1, None)
    assert L.ntc_decode_file_ex2(arr, 1, b"x", -1, ctypes.byref(fo2), None, None) == INVALID_ARG
    fo = F(ctypes.sizeof(F), 0, -1, 0, -1, None, None, 0, -1, None, 0, -1, None)
    assert L.ntc_decode_file_ex3(arr, 1, b"x", -2, ctypes.byref(fo), None, None, None) == INVALID_ARG


def test_decode_pipeline_refuses_a_malformed_digest_file(tmp_path):
    """the digest file is read before anything else is touched: a bad one fails without a GPU"""
    L = nt.lib()
    F = nt.FileOpts3
    fake = ctypes.create_string_buffer(4096)
    arr = (ctypes.c_void_p * 1)(ctypes.addressof(fake))
    bad = tmp_path / "bad.ntcd"
    bad.write_bytes(b"NTCX" + bytes(28))
    st = nt.PipelineStats()
    for path, code in ((bad, FORMAT), (tmp_path / "absent.ntcd", 9)):
        fo = F(ctypes.sizeof(F), 0, -1, 0, -1, None, None, 0, -1, None, 0, -1, os.fsencode(str(path)))
        assert L.ntc_decode_file_ex3(arr, 1, b"x", 1, ctypes.byref(fo), None, ctypes.byref(st), None) == code
        assert st.error.startswith(b"digests: ")


# ---- both command lines ------------------------------------------------------------------------
def _cli(which, *args, cwd):
    cmd = [NATIVE] if which == "native" else [sys.executable, "-m", "ntcomp_amd"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + list(args), cwd=cwd, capture_output=True, env=env, timeout=120)


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_argument_rules(tmp_path, which):
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    (tmp_path / "e.dat").write_bytes(b"")
    ix, fq, enc, d = (str(tmp_path / n) for n in ("noindex", "r.fq", "e.dat", "d.ntcd"))
    r = _cli(which, "verify", "-i", ix, enc, cwd=tmp_path)
    assert r.returncode == 2 and r.stdout == b"" and b"ntcomp: verify: --digest-file PATH is required" in r.stderr
    for command, target in (("encode", fq), ("decode", enc), ("verify", enc)):
        r = _cli(which, command, "-i", ix, "--digest-file", "", target, cwd=tmp_path)
        assert r.returncode == 2 and r.stdout == b"", (command, r.stderr)
        assert b"ntcomp: " + command.encode() + b": --digest-file needs a path" in r.stderr
        r = _cli(which, command, "-i", ix, "--digest-file", target, target, cwd=tmp_path)  # the input itself
        assert r.returncode == 2 and b"--digest-file names a file this call uses already" in r.stderr, (command, r.stderr)
    r = _cli(which, "encode", "-i", ix, "--names", "keep", "--name-file", d, "--digest-file", d, fq, cwd=tmp_path)
    assert r.returncode == 2 and b"--digest-file names a file this call uses already" in r.stderr
    r = _cli(which, "decode", "-i", ix, "--quality-file", d, "--digest-file", d, enc, cwd=tmp_path)
    assert r.returncode == 2 and b"--digest-file names a file this call uses already" in r.stderr
    assert not (tmp_path / "d.ntcd").exists()  # nothing is written
    assert (tmp_path / "r.fq").read_text() == "@r\nACGT\n+\nIIII\n"


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_help_lists_the_flag_and_verify(tmp_path, which):
    for command in ("encode", "decode", "verify"):
        r = _cli(which, command, "--help", cwd=tmp_path)
        assert r.returncode == 0 and b"--digest-file" in r.stdout, command
    assert b"verify" in _cli(which, "--help", cwd=tmp_path).stdout
