"""Reads with N and IUPAC symbols, the parts that need no GPU: the "NTCX" side file
(ntc_nx_write / ntc_nx_read), the kernels' lane logic compiled for the CPU under ASan + UBSan
(tests/nonacgt_cpu), the two command lines' argument rules, and the Python surface.

The checker is nx_lib.py: a few lines of numpy that mask with the substitute base and list
the canonical runs."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import ntcomp_amd as nt
from nx_lib import SYMS, hand_batch, mask, ragged_batch, runs_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
FORMAT = 8


def _runs(rows):
    a = np.zeros(len(rows), dtype=nt.NX_RUN)
    for i, (r, p, n, s) in enumerate(rows):
        a[i] = (r, p, n, ord(s), 0)
    return a


def _write(path, sections, sub="A", header=True):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        nt.write_exceptions(fd, np.zeros(0, dtype=nt.NX_RUN), sub, header=header)
        for s in sections:
            nt.write_exceptions(fd, s, sub, header=False)
    finally:
        os.close(fd)


# ---- side file ------------------------------------------------------------------------------
def test_side_file_round_trip(tmp_path):
    a = _runs([(0, 0, 2, "N"), (0, 2, 2, "R"), (0, 4, 1, "N"), (3, 7, 5000, "-")])
    b = _runs([(3, 5007, 1, "M"), (70000, 0, 1, "N"), (2 ** 33, 2 ** 32 - 2, 2, "Y")])
    p = tmp_path / "x.ntcx"
    _write(p, [a, b], sub="C")
    raw = p.read_bytes()
    assert raw[:32] == b"NTCX" + struct.pack("<I", 1) + b"C" + bytes(23)
    assert raw[32:48] == struct.pack("<QQ", 4, 0) and len(raw) == 32 + 2 * 16 + 7 * 24
    assert raw[48:72] == struct.pack("<QIIII", 0, 0, 2, ord("N"), 0)
    runs, sub = nt.read_exceptions(p)
    assert sub == ord("C") and np.array_equal(runs, np.concatenate([a, b]))


def test_side_file_without_runs_is_the_header_alone(tmp_path):
    p = tmp_path / "e.ntcx"
    _write(p, [], sub="G")
    assert p.stat().st_size == 32
    runs, sub = nt.read_exceptions(p)
    assert len(runs) == 0 and runs.dtype == nt.NX_RUN and sub == ord("G")


def _good(tmp_path):
    p = tmp_path / "good.ntcx"
    _write(p, [_runs([(0, 0, 2, "N"), (0, 5, 1, "R")]), _runs([(1, 0, 3, "N")])])
    return p.read_bytes()


def _patched(raw, at, data):
    return raw[:at] + data + raw[at + len(data):]


MALFORMED = {
    "magic": lambda r: b"NTCY" + r[4:],
    "version": lambda r: _patched(r, 4, struct.pack("<I", 2)),
    "truncated header": lambda r: r[:20],
    "reserved header byte": lambda r: _patched(r, 20, b"\x01"),
    "reserved last header byte": lambda r: _patched(r, 31, b"\x01"),
    "truncated section header": lambda r: r[:32 + 8],
    "truncated run": lambda r: r[:-5],
    "section longer than the file": lambda r: _patched(r, 32, struct.pack("<Q", 3)),
    "len 0": lambda r: _patched(r, 48 + 12, struct.pack("<I", 0)),
    "sym A": lambda r: _patched(r, 48 + 16, struct.pack("<I", ord("A"))),
    "sym lower case": lambda r: _patched(r, 48 + 16, struct.pack("<I", ord("n"))),
    "unsorted reads": lambda r: _patched(r, 48, struct.pack("<Q", 2)),
    "unsorted positions": lambda r: _patched(r, 48 + 24 + 8, struct.pack("<I", 0)),
    "overlapping": lambda r: _patched(r, 48 + 24 + 8, struct.pack("<I", 1)),
    "sub N": lambda r: _patched(r, 8, b"N"),
    "sub 0": lambda r: _patched(r, 8, b"\0"),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_side_file_malformed_is_rejected(tmp_path, what):
    raw = _good(tmp_path)
    runs, _ = nt.read_exceptions(tmp_path / "good.ntcx")
    assert len(runs) == 3
    p = tmp_path / "bad.ntcx"
    p.write_bytes(MALFORMED[what](raw))
    with pytest.raises(nt.NtcError) as e:
        nt.read_exceptions(p)
    assert e.value.code == FORMAT


def test_side_file_writer_rejects_a_bad_substitute(tmp_path):
    fd = os.open(tmp_path / "w", os.O_WRONLY | os.O_CREAT)
    try:
        with pytest.raises(nt.NtcError) as e:
            nt.write_exceptions(fd, np.zeros(0, dtype=nt.NX_RUN), "N")
        assert e.value.code == 1
    finally:
        os.close(fd)
    assert (tmp_path / "w").stat().st_size == 0


# ---- lane logic on the CPU -------------------------------------------------------------------
@pytest.fixture(scope="module")
def lane_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nonacgt_cpu") / "nonacgt_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "nonacgt_cpu", "nonacgt_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _lanes(exe, tmp_path, bases, offs, sub):
    np.asarray(bases, dtype=np.uint8).tofile(tmp_path / "b.bin")
    np.asarray(offs, dtype="<u8").tofile(tmp_path / "o.bin")
    r = subprocess.run([exe, str(tmp_path / "b.bin"), str(tmp_path / "o.bin"), sub], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    lines = r.stdout.split(b"\n")
    at = next(i for i, l in enumerate(lines) if l.startswith(b"masked "))
    rows = np.array([[int(x) for x in l.split()] for l in lines[:at]], dtype=np.uint64).reshape(-1, 4)
    runs = np.zeros(len(rows), dtype=nt.NX_RUN)
    for k, f in enumerate(("read", "pos", "len", "sym")):
        runs[f] = rows[:, k]
    return runs, np.frombuffer(lines[at][len(b"masked "):], dtype=np.uint8)


@pytest.mark.parametrize("lead,shift", [(0, 0), (5, 1), (16, 2)])
@pytest.mark.parametrize("tail", [0, 1, 16])
def test_lane_logic_on_the_hand_built_shapes(lane_exe, tmp_path, lead, shift, tail):
    """The shapes of the GPU test's first case (nx_lib.hand_batch): runs starting and ending
    at positions 15, 16, 17, 63, 64, 65; totals that are no multiple of 16 or of 64; reads of
    one N and all-N reads of 1, 150 and 5000; NN at a read's end against NN at the next one's
    start; NNRRN; all twelve symbols; offsets that start past 0."""
    bases, offs = hand_batch(lead=lead, tail=tail, shift=shift)
    total = int(offs[-1] - offs[0])
    assert total % 64 == tail and int(offs[0]) == lead
    runs, masked = _lanes(lane_exe, tmp_path, bases, offs, "C")
    exp = runs_of(bases, offs)
    p0 = exp[exp["read"] == 0]  # the first read's runs: batch positions = positions in the read
    assert {15, 16, 17, 63, 64, 65} & set((p0["pos"]).tolist()) and len(p0) == 8
    assert len(exp) > 40 and set(exp["sym"].tolist()) == set(SYMS)
    assert np.array_equal(runs, exp)
    assert np.array_equal(masked, mask(bases, "C")[int(offs[0]):int(offs[-1])])


def test_lane_logic_on_ragged_and_dense_batches(lane_exe, tmp_path):
    bases, offs = ragged_batch(np.random.default_rng(5), 3000)
    runs, masked = _lanes(lane_exe, tmp_path, bases, offs, "A")
    assert np.array_equal(runs, runs_of(bases, offs)) and len(runs) > 500
    assert np.array_equal(masked, mask(bases, "A"))
    dense = np.frombuffer(b"NA" * 4800, dtype=np.uint8)
    offs = np.arange(0, 9601, 150, dtype=np.uint64)
    runs, masked = _lanes(lane_exe, tmp_path, dense, offs, "T")
    assert len(runs) == 4800 and np.array_equal(runs, runs_of(dense, offs))
    assert bytes(masked) == b"TA" * 4800


def test_lane_logic_on_a_clean_batch_and_a_single_base(lane_exe, tmp_path):
    g = nt.synth_genome(3, 1000)
    runs, masked = _lanes(lane_exe, tmp_path, g, np.array([0, 333, 1000], dtype=np.uint64), "A")
    assert len(runs) == 0 and np.array_equal(masked, g)
    one = np.frombuffer(b"N", dtype=np.uint8)
    runs, masked = _lanes(lane_exe, tmp_path, one, np.array([0, 1], dtype=np.uint64), "G")
    assert runs.tolist() == [(0, 0, 1, ord("N"), 0)] and bytes(masked) == b"G"


def test_checker_lists_canonical_runs():
    """The numpy checker itself, on the issue's own examples."""
    bases, offs = nt.pack_reads([b"ACNNRRNAC", b"GTNN", b"NNAC", b"N"])
    got = [(int(r["read"]), int(r["pos"]), int(r["len"]), chr(r["sym"])) for r in runs_of(bases, offs)]
    assert got == [(0, 2, 2, "N"), (0, 4, 2, "R"), (0, 6, 1, "N"), (1, 2, 2, "N"), (2, 0, 2, "N"), (3, 0, 1, "N")]
    assert bytes(mask(bases, "C")) == b"ACCCCCCACGTCCCCACC"


# ---- both command lines -----------------------------------------------------------------------
def _cli(which, *args, cwd):
    cmd = [NATIVE] if which == "native" else [sys.executable, "-m", "ntcomp_amd"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + list(args), cwd=cwd, capture_output=True, env=env, timeout=120)


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_argument_rules(tmp_path, which):
    (tmp_path / "r.fq").write_text("@r\nACGN\n+\nIIII\n")
    common = ["encode", "-i", str(tmp_path / "noindex"), str(tmp_path / "r.fq")]
    r = _cli(which, *common, "--non-acgt", "keep", cwd=tmp_path)
    assert r.returncode == 2 and r.stdout == b"", r.stderr
    assert b"ntcomp: encode: --non-acgt keep requires --exceptions PATH" in r.stderr
    for policy in (["--non-acgt", "mask"], []):
        r = _cli(which, *common, *policy, "--exceptions", str(tmp_path / "x.ntcx"), cwd=tmp_path)
        assert r.returncode == 2 and r.stdout == b"", r.stderr
        assert b"ntcomp: encode: --exceptions is only written under --non-acgt keep" in r.stderr
    r = _cli(which, *common, "--non-acgt", "drop", cwd=tmp_path)
    assert r.returncode == 2 and b"ntcomp: encode: --non-acgt: error, mask or keep" in r.stderr
    assert not (tmp_path / "x.ntcx").exists()  # nothing is written


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_help_lists_both_flags(tmp_path, which):
    for command in ("encode", "decode"):
        r = _cli(which, command, "--help", cwd=tmp_path)
        assert r.returncode == 0
        assert b"--exceptions" in r.stdout, command
        if command == "encode" or which == "native":
            assert b"--non-acgt" in r.stdout


# ---- exports and the Python surface -------------------------------------------------------------
def test_exports_and_python_surface():
    L = nt.lib()
    for name in ("ntc_encode_exceptions", "ntc_decode_set_exceptions", "ntc_nx_read", "ntc_nx_write",
                 "ntc_encode_file_nx", "ntc_decode_file_nx"):
        assert name in nt.EXPORTED and hasattr(L, name), name
    assert nt.NX_RUN.itemsize == 24 and nt.NX_RUN.names == ("read", "pos", "len", "sym", "reserved")
    assert ctypes.sizeof(nt.NxStats) == 32
    assert nt.NON_ACGT == {"error": 0, "mask": 1, "keep": 2}
    for name in ("exceptions", "set_exceptions", "encode", "encode_pack", "encode_pack_fastq"):
        assert callable(getattr(nt.GpuContext, name)), name
    import inspect
    for fn, arg in ((nt.GpuContext.encode, "non_acgt"), (nt.GpuContext.encode_pack, "non_acgt"),
                    (nt.GpuContext.encode_pack_fastq, "non_acgt"), (nt.encode_file, "non_acgt"),
                    (nt.encode_file, "nx_fd"), (nt.decode_file, "nx_path"), (nt.read_exceptions, "path")):
        assert arg in inspect.signature(fn).parameters, (fn.__name__, arg)
    # the null-argument paths of the two context entry points need no GPU
    n = ctypes.c_uint64()
    assert L.ntc_encode_exceptions(None, None, 0, ctypes.byref(n)) == 1
    assert L.ntc_decode_set_exceptions(None, None, 0, ord("A")) == 1
    assert L.ntc_encode_file_nx(None, 0, b"x", 1, 2, -1, None, None, None) == 1
