"""What the per-block content digests cost (DESIGN.md "Content digests"), on one GPU:

  cost    ntc_encode_pack_fastq on 1 M x 150 bp reads with "digests" 0 and 1, interleaved in one
          process, medians and ranges over --rounds after --warmups, once with no side file and
          once with all three (non_acgt keep, qualities keep, names keep); then the same for the
          decode of those blocks (ntc_unpack_streams + ntc_decode_fasta_unpacked) with and
          without expected digests; and the bytes each digest pass has to read (computed from
          the shapes, to set against kernel times from a `rocprofv3 --kernel-trace --stats` run
          of --trace)
  e2e     the native command line on a plain FASTQ file: encode with and without --digest-file
          (alternating), decode with and without it, and verify against decode > /dev/null
  trace   a few calls with digests on and one verified decode and nothing else, for the profiler

Prints one JSON object per part."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
import ntcomp_amd as nt  # noqa: E402
from names_cost import fastq_text, names_blob  # noqa: E402

NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
ALL = dict(non_acgt="keep", qualities="keep", names="keep")


def setup(args, n):
    genome = nt.synth_genome(1, args.genome_bp)
    ix = nt.Index.build([genome.tobytes()], args.k)
    reads = nt.synth_reads(genome, 2, 0, n, args.read_len, 10_000)
    blob, lens = names_blob("illumina", n, args.read_len)
    quals = np.random.default_rng(3).integers(ord("#"), ord("J"), n * args.read_len).astype(np.uint8)
    # (bytes: the wrapper then takes the text as it is, with no copy inside the timed calls)
    return ix, fastq_text(blob, lens, reads, args.read_len, quals).tobytes(), int(lens.sum())


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def encode_call(ctx, text, n, digests, **modes):
    t0 = time.perf_counter()
    out = ctx.encode_pack_fastq(text, n, digests=digests, **modes)
    return 1e3 * (time.perf_counter() - t0), out


def decode_call(ctx, out, modes, dg):
    arr = (nt.BlockMeta * len(out[0]))(*out[0])
    t0 = time.perf_counter()
    ctx.unpack(arr, out[1], len(out[0]))
    if modes:
        ctx.set_exceptions(out[3], ctx.substitute)
        ctx.set_qualities(*out[4])
        ctx.set_names(*out[5])
    if dg is not None:
        ctx.decode_set_digests(dg)
    need = ctypes.c_uint64()
    ctx.L.ntc_decode_fasta_unpacked(ctx.h, 1, None, 0, ctypes.byref(need))
    text = np.empty(need.value + 64, np.uint8)
    rc = ctx.L.ntc_decode_fasta_unpacked(ctx.h, 1, text.ctypes.data_as(ctypes.c_void_p), len(text), ctypes.byref(need))
    assert rc == 0, ctx.L.ntc_last_error(ctx.h)
    return 1e3 * (time.perf_counter() - t0)


def part_cost(args):
    ix, text, name_bytes = setup(args, args.reads)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    n, bases = args.reads, args.reads * args.read_len
    res = {"reads": n, "read_len": args.read_len,
           "bytes_read": {"seq": bases, "sym": bases, "qual": bases, "name": name_bytes, "offsets_per_pass": 8 * (n + 1)}}
    for label, modes in (("no_side_file", {}), ("all_three", ALL)):
        enc = {0: [], 1: []}
        dec = {0: [], 1: []}
        for i in range(args.warmups + args.rounds):
            for on in (0, 1):
                ms, out = encode_call(ctx, text, n, bool(on), **modes)
                dms = decode_call(ctx, out, modes, out[-1] if on else None)
                if i >= args.warmups:
                    enc[on].append(ms)
                    dec[on].append(dms)
        res[label] = {"encode_off": spread(enc[0]), "encode_on": spread(enc[1]), "decode_off": spread(dec[0]),
                      "decode_on": spread(dec[1])}
    print(json.dumps({"cost": res}))


def part_trace(args):
    ix, text, _ = setup(args, args.reads)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    for _ in range(3):
        _, out = encode_call(ctx, text, args.reads, True, **ALL)
    decode_call(ctx, out, ALL, out[-1])
    print(json.dumps({"trace": {"reads": args.reads, "encode_calls": 3, "decode_calls": 1}}))


def part_e2e(args):
    ix, text, _ = setup(args, args.e2e_reads)
    with tempfile.TemporaryDirectory(dir=args.tmp) as d:
        p = lambda name: os.path.join(d, name)
        ix.save(p("ix"))
        with open(p("r.fq"), "wb") as f:
            f.write(text)

        def run(argv, out):
            t0 = time.perf_counter()
            with open(out, "wb") as f:
                subprocess.run([NATIVE] + argv, stdout=f, stderr=subprocess.DEVNULL, check=True)
            return round(time.perf_counter() - t0, 3)

        r = {k: [] for k in ("encode_plain", "encode_digests", "decode_plain", "decode_digests", "verify", "decode_devnull")}
        enc = ["encode", "-i", p("ix"), p("r.fq")]
        for _ in range(args.e2e_runs):
            r["encode_plain"].append(run(enc, p("plain.dat")))
            r["encode_digests"].append(run(enc[:-1] + ["--digest-file", p("d.ntcd"), p("r.fq")], p("e.dat")))
        dec = ["-i", p("ix"), p("e.dat")]
        for _ in range(args.e2e_runs):
            r["decode_plain"].append(run(["decode"] + dec, p("o.fa")))
            r["decode_digests"].append(run(["decode", "--digest-file", p("d.ntcd")] + dec, p("o2.fa")))
            r["verify"].append(run(["verify", "--digest-file", p("d.ntcd")] + dec, p("v.txt")))
            r["decode_devnull"].append(run(["decode"] + dec, os.devnull))
        r["digest_file_bytes"] = os.path.getsize(p("d.ntcd"))
        r["reads"] = args.e2e_reads
    print(json.dumps({"e2e": r}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["cost", "trace", "e2e"])
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--e2e-reads", type=int, default=5_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=91)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--e2e-runs", type=int, default=2)
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    {"cost": part_cost, "trace": part_trace, "e2e": part_e2e}[args.part](args)


if __name__ == "__main__":
    main()
