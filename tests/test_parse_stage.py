"""k_parse4's staged query reader (encode_core.h QStaged, stage_word_count) on the CPU.  The
stand-alone program tests/parse_stage_cpu, built with the address and undefined-behaviour
sanitizers and run directly, parses every block of every case of tests/parse_stage_lib.py twice:
from the 2-bit stream itself and from a heap copy of exactly the words the kernel claims a block
can touch.  A query access outside that range is a heap overflow the sanitizer reports, so a
clean run proves the stage's slack; the records of the two parses must be equal, and their count
must be the oracle's."""
import os
import subprocess

import numpy as np
import pytest

import parse_stage_lib as pl
from oracle_lib import REPO, OracleIndex, pack_reads


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    src = os.path.join(REPO, "tests", "parse_stage_cpu", "parse_stage_cpu.cpp")
    out = str(tmp_path_factory.mktemp("parse_stage") / "parse_stage_cpu")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-g", "-std=c++17",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), src,
                    os.path.join(REPO, "ntcomp_amd", "csrc", "derived.cpp"), "-o", out],
                   check=True, capture_output=True, text=True)
    return out


@pytest.fixture(scope="module")
def index_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("parse_stage_ix")
    paths = {}
    for k in (31, 91):
        ix = pl.index(k)
        paths[k] = str(d / f"ix_{k}.bin")
        with open(paths[k], "wb") as f:
            f.write(np.array([ix.n, k] + [int(c) for c in ix.C[:4]], dtype=np.uint64).tobytes())
            for c in range(4):
                f.write(np.ascontiguousarray(ix.rows[c], dtype=np.uint64)[: (ix.n + 63) // 64].tobytes())
            f.write(np.ascontiguousarray(ix.lcs, dtype=np.uint8)[: ix.n].tobytes())
    return paths


def test_the_cases_hold_what_they_claim():
    pl.check_shapes()


BLOCKS = (64, 256)


@pytest.mark.parametrize("k", [31, 91])
def test_staged_parse_equals_plain_parse_inside_the_claimed_words(exe, index_files, tmp_path, k):
    ix = pl.index(k)
    orc = OracleIndex(ix.n, k, ix.rows, ix.C, ix.lcs)
    paths, want = [], []
    for name, (reads, lead) in pl.cases().items():
        # in blocks of 64 and 256 reads: more block edges (first and last word at every alignment,
        # short and long reads at both ends) from the same reads
        bases, offs = pl.batch(reads, lead)
        paths.append(str(tmp_path / f"{name}.bin"))
        with open(paths[-1], "wb") as f:
            f.write(np.array([len(reads)], dtype=np.uint64).tobytes())
            f.write(offs.tobytes())
            f.write(bases.tobytes())
        b0, o0 = pack_reads(reads)
        _, eoff = orc.encode(b0, o0)
        want += [(len(reads), (len(reads) + b - 1) // b, int(eoff[-1])) for b in BLOCKS]
    r = subprocess.run([exe, index_files[k], ",".join(map(str, BLOCKS))] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("staged:")]
    got = [(int(w[1]), int(w[3]), int(w[7])) for w in lines]
    assert got == want
    assert sum(b for _, b, _ in got) > 50
