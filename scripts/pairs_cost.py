#!/usr/bin/env python3
"""What paired-end reads cost (DESIGN.md "Paired-end reads", profiles/pairs/).

  cost   one context: ntc_encode_pack_fastq_paired on two mate texts against
         ntc_encode_pack_fastq on the same reads interleaved beforehand, under paired 1 (ids
         checked) and 2 (not checked), and the paired decode call against the unsplit one.  The
         variants alternate inside one process: --rounds after --warmup, median and range.
  trace  one paired encode and one paired decode call, for `rocprofv3 --kernel-trace --stats --
         python scripts/pairs_cost.py trace` (the weave, check and split kernels' own times);
         prints the bytes each of them must move.
  e2e    the native command line: --mate-file R1 R2 against the same reads interleaved into one
         file; pipeline and process Gbases/s of each, and the NTCN bytes of Illumina-style mate
         names encoded as pairs against two separate single-file encodes.

Results go to stdout as one JSON line per figure; --out FILE also writes them there."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import ntcomp_amd as nt  # noqa: E402

NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")


def mates(genome, n_pairs, length, seed):
    """two FASTQ texts of n_pairs records: Illumina-style names ("... 1:N:0:..." / "... 2:N:0:...")"""
    rng = np.random.default_rng(seed)
    x = 1000 + np.cumsum(rng.integers(0, 30, n_pairs))
    y = rng.integers(1000, 40000, n_pairs)
    out = []
    for k in (1, 2):
        flat = nt.synth_reads(genome, seed + k, 0, n_pairs, length, 10_000).tobytes()
        q = bytes(rng.integers(35, 74, length, dtype=np.uint8))
        recs = [b"@A00123:45:HXXXXDSXX:1:1101:%d:%d %d:N:0:ATCACGTT+AGGCTATA\n%s\n+\n%s\n"
                % (x[p], y[p], k, flat[p * length:(p + 1) * length], q) for p in range(n_pairs)]
        out.append(recs)
    return b"".join(out[0]), b"".join(out[1]), b"".join(a + b for a, b in zip(*out))


def summary(name, secs, bases):
    med = statistics.median(secs)
    return dict(figure=name, median_ms=round(1e3 * med, 3), min_ms=round(1e3 * min(secs), 3),
                max_ms=round(1e3 * max(secs), 3), gbases_s=round(bases / med / 1e9, 2), rounds=len(secs))


def cmd_cost(a, emit):
    genome = nt.synth_genome(1, a.genome)
    ix = nt.Index.build([genome.tobytes()], a.k)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    t1, t2, both = mates(genome, a.pairs, a.length, 5)
    bases = 2 * a.pairs * a.length
    kw = dict(block_reads=65536, qualities="keep", names="keep") if a.sides else dict(block_reads=65536)

    def enc(mode, two):
        ctx.paired = mode
        t0 = time.perf_counter()
        out = ctx.encode_pack_fastq_paired(t1, t2, a.pairs, **kw) if two else ctx.encode_pack_fastq(both, 2 * a.pairs, **kw)
        return time.perf_counter() - t0, out

    ref = enc(0, False)[1]
    assert enc(1, True)[1][1] == ref[1], "the paired call's payload differs from the interleaved call's"
    arr = (nt.BlockMeta * len(ref[0]))(*ref[0])

    need = ctypes.c_uint64()
    ctx.unpack(arr, ref[1], len(ref[0]))
    ctx.L.ntc_decode_fasta_unpacked(ctx.h, 1, None, 0, ctypes.byref(need))
    text = np.zeros(need.value + 64, dtype=np.uint8)  # one touched buffer for every round: the C call alone is timed

    def dec(mode):
        ctx.paired = mode
        ctx.unpack(arr, ref[1], len(ref[0]))
        t0 = time.perf_counter()
        rc = ctx.L.ntc_decode_fasta_unpacked(ctx.h, 1, text.ctypes.data, len(text), ctypes.byref(need))
        dt = time.perf_counter() - t0
        assert rc == 0 and (not mode or 0 < ctx.pair_split() < need.value)
        return dt

    variants = [("encode interleaved text, paired 0", lambda: enc(0, False)[0]),
                ("encode interleaved text, paired 1", lambda: enc(1, False)[0]),
                ("encode two texts, paired 1", lambda: enc(1, True)[0]),
                ("encode two texts, paired 2", lambda: enc(2, True)[0]),
                ("decode, paired 0", lambda: dec(0)), ("decode, paired 1", lambda: dec(1))]
    times = {n: [] for n, _ in variants}
    for r in range(a.warmup + a.rounds):
        for n, f in variants:
            t = f()
            if r >= a.warmup:
                times[n].append(t)
    ctx.paired = 0
    for n, _ in variants:
        emit(dict(summary(n, times[n], bases), pairs=a.pairs, length=a.length, side_files=bool(a.sides)))
    ctx.close()


def cmd_trace(a, emit):
    genome = nt.synth_genome(1, a.genome)
    ix = nt.Index.build([genome.tobytes()], a.k)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    t1, t2, both = mates(genome, a.pairs, a.length, 5)
    ctx.paired = 1
    for _ in range(3):
        metas, payload, _ = ctx.encode_pack_fastq_paired(t1, t2, a.pairs)
        arr = (nt.BlockMeta * len(metas))(*metas)
        ctx.unpack(arr, payload, len(metas))
        p1, p2 = ctx.decode_fasta_unpacked(first_id=1)
    emit(dict(figure="bytes the kernels move", k_pw_copy=2 * len(both), k_pw_sizes=2 * 16 * a.pairs + 4 * a.pairs,
              k_pm_check="the header lines twice: about %d" % (2 * both.count(b"\n@") * 60),
              k_ps_copy=2 * (len(p1) + len(p2)), pairs=a.pairs))
    ctx.close()


def cmd_e2e(a, emit):
    d = a.dir
    os.makedirs(d, exist_ok=True)
    genome = nt.synth_genome(1, a.genome)
    nt.Index.build([genome.tobytes()], a.k).save(os.path.join(d, "idx"))
    t1, t2, both = mates(genome, a.pairs, a.length, 5)
    for name, t in (("r1.fq", t1), ("r2.fq", t2), ("both.fq", both)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(t)
    bases = 2 * a.pairs * a.length

    def run(tag, args, n_bases):
        best = None
        for _ in range(a.runs):
            t0 = time.perf_counter()
            with open(os.path.join(d, tag + ".dat"), "wb") as f:
                r = subprocess.run([NATIVE, "encode", "-i", os.path.join(d, "idx"), "--threads", "16", "--stats",
                                    "--names", "keep", "--name-file", os.path.join(d, tag + ".ntcn"), *args],
                                   stdout=f, stderr=subprocess.PIPE, check=True, timeout=1200)
            wall = time.perf_counter() - t0
            st = json.loads(r.stderr.decode().strip().splitlines()[-1])
            row = dict(figure="e2e " + tag, pipeline_gbases_s=round(n_bases / st["pipeline_wall_s"] / 1e9, 2),
                       process_gbases_s=round(n_bases / wall / 1e9, 2), parse_s=st["stats"]["parse"], gpu_s=st["stats"]["gpu"],
                       ntcn_bytes=os.path.getsize(os.path.join(d, tag + ".ntcn")), threads=st["threads"])
            if best is None or row["pipeline_gbases_s"] > best["pipeline_gbases_s"]:
                best = row
        emit(best)
        return best

    run("interleaved", ["--interleaved", os.path.join(d, "both.fq")], bases)
    run("mate_file", ["--mate-file", os.path.join(d, "r2.fq"), os.path.join(d, "r1.fq")], bases)
    s1 = run("single_r1", [os.path.join(d, "r1.fq")], bases // 2)
    s2 = run("single_r2", [os.path.join(d, "r2.fq")], bases // 2)
    emit(dict(figure="NTCN of two separate encodes", ntcn_bytes=s1["ntcn_bytes"] + s2["ntcn_bytes"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", choices=["cost", "trace", "e2e"])
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--genome", type=int, default=2_000_000)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2, help="e2e: runs of each command line, the best is reported")
    ap.add_argument("--sides", action="store_true", help="cost: with --qualities keep and --names keep")
    ap.add_argument("--dir", default="out/pairs_e2e", help="e2e: scratch directory")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    {"cost": cmd_cost, "trace": cmd_trace, "e2e": cmd_e2e}[a.command](a, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
