"""What keeping FASTQ quality scores costs (DESIGN.md "Quality scores"), on one GPU:

  cost    ntc_encode_pack_fastq on 1 M x 150 bp reads under qualities drop and keep,
          interleaved in one process, medians over --rounds after --warmups, for a 4-symbol
          and a ~40-symbol quality alphabet; the sections' raw, packed and deflated bytes;
          the bytes each quality kernel has to move (computed from the shapes, to set
          against kernel times from a `rocprofv3 --kernel-trace --stats` run of --trace)
  e2e     the native command line on a plain FASTQ file: encode with and without
          --qualities keep (alternating), decode to FASTQ against decode to FASTA
  trace   a few keep calls and one FASTQ decode and nothing else, for the profiler

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
import ntcomp_amd as nt  # noqa: E402

ALPHABETS = {"4_symbols": b"#-<F", "40_symbols": bytes(range(35, 75))}


def fastq_text(reads, quals, L):
    n = len(reads) // L
    nl = np.full((n, 1), 10, np.uint8)
    rec = np.concatenate([np.frombuffer(b"@r\n", np.uint8)[None, :].repeat(n, 0), reads.reshape(n, L), nl,
                          np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0), quals.reshape(n, L), nl], axis=1)
    return rec.reshape(-1)


def qualities(rng, alphabet, n):
    """Skewed towards the high scores, as an instrument's are."""
    a = np.frombuffer(alphabet, np.uint8)
    p = np.arange(1, len(a) + 1, dtype=np.float64) ** 3
    return a[rng.choice(len(a), n, p=p / p.sum())]


def raw_call(ctx, text, n, block_reads, mode):
    """One ntc_encode_pack_fastq under the mode, wall ms (the payload is freed, not copied)."""
    nb = (n + block_reads - 1) // block_reads
    metas = (nt.BlockMeta * nb)()
    out, used, nbases, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int64(-1)
    ctx.set_option("qualities", mode)
    t0 = time.perf_counter()
    rc = ctx.L.ntc_encode_pack_fastq(ctx.h, text.ctypes.data_as(ctypes.c_void_p), len(text), n, block_reads, metas,
                                     ctypes.byref(out), ctypes.byref(used), ctypes.byref(nbases), ctypes.byref(bad))
    ms = 1e3 * (time.perf_counter() - t0)
    ctx.L.ntc_buffer_free(out)
    ctx.set_option("qualities", 0)
    if rc:
        raise nt.NtcError(rc, ctx.L.ntc_last_error(ctx.h).decode())
    return ms


def setup(args):
    genome = nt.synth_genome(1, args.genome_bp)
    ix = nt.Index.build([genome.tobytes()], args.k)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    reads = nt.synth_reads(genome, 2, 0, args.reads, args.read_len, 10_000)
    return genome, ix, ctx, reads


def part_cost(args):
    _, _, ctx, reads = setup(args)
    n, L, BR = args.reads, args.read_len, 65536
    res = {"what": "ntc_encode_pack_fastq wall ms, %d x %d bp, k = %d, %d interleaved rounds after %d warm-ups"
                   % (n, L, args.k, args.rounds, args.warmups)}
    engine = "libdeflate" if nt.libdeflate_available() else "zlib"
    for name, alphabet in ALPHABETS.items():
        text = fastq_text(reads, qualities(np.random.default_rng(5), alphabet, n * L), L)
        t = {0: [], 1: []}
        for i in range(args.warmups + args.rounds):
            for mode in (0, 1):
                ms = raw_call(ctx, text, n, BR, mode)
                if i >= args.warmups:
                    t[mode].append(ms)
        raw_call(ctx, text, n, BR, 1)
        t0 = time.perf_counter()
        qm, qp = ctx.qualities()
        fetch_ms = 1e3 * (time.perf_counter() - t0)
        deflated = 0
        buf = np.frombuffer(qp, np.uint8)
        for m in qm:
            out, ln = ctypes.c_void_p(), ctypes.c_uint64()
            rc = nt.lib().ntc_q_deflate_section(ctypes.byref(m), ctypes.c_void_p(buf.ctypes.data + m.payload_off),
                                                nt.DEFLATE_ENGINES[engine], ctypes.byref(out), ctypes.byref(ln))
            assert rc == 0
            nt.lib().ntc_buffer_free(out)
            deflated += ln.value
        w = qm[0].width
        nq = n * L
        res[name] = {
            "drop": {"median_ms": statistics.median(t[0]), "min_ms": min(t[0]), "max_ms": max(t[0])},
            "keep": {"median_ms": statistics.median(t[1]), "min_ms": min(t[1]), "max_ms": max(t[1])},
            "fetch_sections_ms": fetch_ms, "width": w, "n_syms": qm[0].n_syms,
            "raw_quality_bytes": nq, "packed_bytes": len(qp), "deflated_bytes": deflated, "deflate_engine": engine,
            # what each kernel must move: gather reads the quality lines, 2 newline positions and 2
            # offsets per read and writes the bytes; pack reads them and writes the words
            "bytes_moved": {"k_q_gather": 2 * nq + n * (2 * 4 + 2 * 8), "k_q_pack": nq + len(qp)},
        }
    ctx.close()
    print(json.dumps({"cost": res}))


def part_trace(args):
    _, _, ctx, reads = setup(args)
    n, L = args.reads, args.read_len
    text = fastq_text(reads, qualities(np.random.default_rng(5), ALPHABETS["4_symbols"], n * L), L)
    for _ in range(4):
        metas, payload, nb, (qm, qp) = ctx.encode_pack_fastq(text.tobytes(), n, qualities="keep")
    arr = (nt.BlockMeta * len(metas))(*metas)
    ctx.unpack(arr, payload, len(metas))
    ctx.set_qualities(qm, qp)
    out = ctx.decode_fasta_unpacked(first_id=1)
    ctx.close()
    print(json.dumps({"trace": {"reads": n, "read_len": L, "fastq_bytes": len(out),
                                "bytes_moved": {"k_q_unpack": len(qp) + n * L, "k_fastq": 2 * n * L + len(out)}}}))


def part_e2e(args):
    genome = nt.synth_genome(1, args.genome_bp)
    ix = nt.Index.build([genome.tobytes()], args.k)
    n, L = args.e2e_reads, args.read_len
    exe = os.path.join(REPO, "ntcomp_amd", "ntcomp")
    res = {"what": "native command line, %d x %d bp plain FASTQ, %d alternating runs each" % (n, L, args.e2e_runs),
           "bases": n * L}
    reads = nt.synth_reads(genome, 2, 0, n, L, 10_000)
    for name, alphabet in ALPHABETS.items():
        with tempfile.TemporaryDirectory(dir=args.tmp) as d:
            ix.save(os.path.join(d, "ix"))
            fastq_text(reads, qualities(np.random.default_rng(5), alphabet, n * L), L).tofile(os.path.join(d, "r.fq"))

            def run(cmd, out):
                with open(os.path.join(d, out), "wb") as f:
                    r = subprocess.run([exe] + cmd + ["--stats"], stdout=f, stderr=subprocess.PIPE, timeout=600)
                assert r.returncode == 0, r.stderr[-2000:]
                s = json.loads(r.stderr.decode().strip().split("\n")[-1])
                return {"pipeline_gbases_s": round(n * L / s["pipeline_wall_s"] / 1e9, 3),
                        "process_gbases_s": round(n * L / s["process_s"] / 1e9, 3),
                        "pipeline_wall_s": s["pipeline_wall_s"], "process_s": s["process_s"],
                        "deflate_thread_s": s["stats"].get("deflate"), "gpu_thread_s": s["stats"].get("gpu"),
                        "out_bytes": os.path.getsize(os.path.join(d, out)),
                        **{k: v for k, v in s.items() if k.startswith("q_")}}

            r = {"encode_drop": [], "encode_keep": [], "decode_fasta": [], "decode_fastq": []}
            enc = ["encode", "-i", os.path.join(d, "ix"), os.path.join(d, "r.fq")]
            for _ in range(args.e2e_runs):
                r["encode_drop"].append(run(enc, "drop.dat"))
                r["encode_keep"].append(run(enc + ["--qualities", "keep", "--quality-file", os.path.join(d, "q.ntcq")],
                                            "keep.dat"))
            r["quality_file_bytes"] = os.path.getsize(os.path.join(d, "q.ntcq"))
            dec = ["decode", "-i", os.path.join(d, "ix"), os.path.join(d, "keep.dat")]
            for _ in range(args.e2e_runs):
                r["decode_fasta"].append(run(dec, "out.fa"))
                r["decode_fastq"].append(run(dec + ["--quality-file", os.path.join(d, "q.ntcq")], "out.fq"))
            res[name] = r
    print(json.dumps({"e2e": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["cost", "trace", "e2e"])
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--e2e-reads", type=int, default=5_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=91)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--e2e-runs", type=int, default=2)
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    {"cost": part_cost, "trace": part_trace, "e2e": part_e2e}[args.part](args)


if __name__ == "__main__":
    main()
