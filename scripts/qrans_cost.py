"""What the order-1 rANS coder of the quality sections costs and saves, on
one GPU, beside the pack coder of scripts/quality_cost.py:

  cost    ntc_encode_pack_fastq on 1 M x 150 bp reads under qualities drop, keep + pack and
          keep + rans, interleaved in one process, medians over --rounds after --warmups, for
          three quality sources: iid over 4 symbols, iid over ~40 symbols (both as
          quality_cost.py draws them) and an order-1 Markov source over 4 symbols (stay
          probability 0.9); the sections' bytes under both coders, the pack ones deflated too;
          the decode call (unpacked blocks -> FASTQ text) under both
  e2e     the native command line on a plain FASTQ file: encode --qualities keep with
          --quality-coder pack and rans (alternating), and the decode of each to FASTQ,
          process time included (it holds the side file's read)
  trace   a few rans calls and one FASTQ decode and nothing else, for the profiler

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
from quality_cost import ALPHABETS, fastq_text, qualities, setup  # noqa: E402


def markov(rng, alphabet, n, p=0.9):
    """Order-1 Markov qualities: the symbol stays with probability p, otherwise another one is
    drawn uniformly (tests/qrans_lib.py markov_quals, vectorised)."""
    a = np.frombuffer(alphabet, np.uint8)
    out = np.empty(n, np.uint8)
    cur = int(rng.integers(0, len(a)))
    for at in range(0, n, 1 << 24):  # in pieces: the 5 M x 150 file has 750 M qualities
        m = min(1 << 24, n - at)
        jump = np.where(rng.random(m) < p, 0, rng.integers(1, len(a), m))
        s = (cur + np.cumsum(jump)) % len(a)
        out[at:at + m] = a[s]
        cur = int(s[-1])
    return out


SOURCES = {
    "iid_4_symbols": lambda rng, n: qualities(rng, ALPHABETS["4_symbols"], n),
    "iid_40_symbols": lambda rng, n: qualities(rng, ALPHABETS["40_symbols"], n),
    "markov_4_symbols": lambda rng, n: markov(rng, ALPHABETS["4_symbols"], n),
}


def raw_call(ctx, text, n, block_reads, mode, coder):
    """One ntc_encode_pack_fastq under the mode and coder, wall ms (the payload is freed, not copied)."""
    nb = (n + block_reads - 1) // block_reads
    metas = (nt.BlockMeta * nb)()
    out, used, nbases, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int64(-1)
    ctx.set_option("qualities", mode)
    ctx.set_option("quality_coder", coder)
    t0 = time.perf_counter()
    rc = ctx.L.ntc_encode_pack_fastq(ctx.h, text.ctypes.data_as(ctypes.c_void_p), len(text), n, block_reads, metas,
                                     ctypes.byref(out), ctypes.byref(used), ctypes.byref(nbases), ctypes.byref(bad))
    ms = 1e3 * (time.perf_counter() - t0)
    ctx.L.ntc_buffer_free(out)
    ctx.set_option("qualities", 0)
    ctx.set_option("quality_coder", 0)
    if rc:
        raise nt.NtcError(rc, ctx.L.ntc_last_error(ctx.h).decode())
    return ms


def med(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def part_cost(args):
    _, _, ctx, reads = setup(args)
    n, L, BR = args.reads, args.read_len, 65536
    res = {"what": "ntc_encode_pack_fastq wall ms, %d x %d bp, k = %d, %d interleaved rounds after %d warm-ups"
                   % (n, L, args.k, args.rounds, args.warmups)}
    engine = "libdeflate" if nt.libdeflate_available() else "zlib"
    variants = {"drop": (0, 0), "keep_pack": (1, 0), "keep_rans": (1, 1)}
    for name, draw in SOURCES.items():
        text = fastq_text(reads, draw(np.random.default_rng(5), n * L), L)
        t = {v: [] for v in variants}
        for i in range(args.warmups + args.rounds):
            for v, (mode, coder) in variants.items():
                ms = raw_call(ctx, text, n, BR, mode, coder)
                if i >= args.warmups:
                    t[v].append(ms)
        out = {v: med(t[v]) for v in variants}
        out["raw_quality_bytes"] = n * L
        for v, coder in (("pack", "pack"), ("rans", "rans")):
            metas, payload, nb, (qm, qp) = ctx.encode_pack_fastq(text.tobytes(), n, block_reads=BR, qualities="keep",
                                                                 quality_coder=coder)
            section = 0
            buf = np.frombuffer(qp, np.uint8)
            t0 = time.perf_counter()
            for m in qm:
                o, ln = ctypes.c_void_p(), ctypes.c_uint64()
                rc = nt.lib().ntc_q_deflate_section(ctypes.byref(m), ctypes.c_void_p(buf.ctypes.data + m.payload_off),
                                                    nt.DEFLATE_ENGINES[engine], ctypes.byref(o), ctypes.byref(ln))
                assert rc == 0
                nt.lib().ntc_buffer_free(o)
                section += ln.value
            host_ms = 1e3 * (time.perf_counter() - t0)
            arr = (nt.BlockMeta * len(metas))(*metas)
            dec = []
            for i in range(args.warmups + args.rounds):
                ctx.unpack(arr, payload, len(metas))
                ctx.set_qualities(qm, qp)
                t0 = time.perf_counter()
                text_out = ctx.decode_fasta_unpacked(first_id=1)
                if i >= args.warmups:
                    dec.append(1e3 * (time.perf_counter() - t0))
            out["sections_" + v] = {"payload_bytes": len(qp), "section_bytes": section, "host_section_ms_one_thread": host_ms,
                                    "deflate_engine": engine if v == "pack" else None,
                                    "decode_fastq_call": med(dec), "fastq_bytes": len(text_out)}
        res[name] = out
    ctx.close()
    print(json.dumps({"cost": res}))


def part_trace(args):
    _, _, ctx, reads = setup(args)
    n, L = args.reads, args.read_len
    text = fastq_text(reads, SOURCES[args.source](np.random.default_rng(5), n * L), L)
    for _ in range(4):
        metas, payload, nb, (qm, qp) = ctx.encode_pack_fastq(text.tobytes(), n, qualities="keep", quality_coder="rans")
    arr = (nt.BlockMeta * len(metas))(*metas)
    ctx.unpack(arr, payload, len(metas))
    ctx.set_qualities(qm, qp)
    out = ctx.decode_fasta_unpacked(first_id=1)
    ctx.close()
    print(json.dumps({"trace": {"reads": n, "read_len": L, "source": args.source, "fastq_bytes": len(out),
                                "payload_bytes": len(qp)}}))


def part_e2e(args):
    genome = nt.synth_genome(1, args.genome_bp)
    ix = nt.Index.build([genome.tobytes()], args.k)
    n, L = args.e2e_reads, args.read_len
    exe = os.path.join(REPO, "ntcomp_amd", "ntcomp")
    res = {"what": "native command line, %d x %d bp plain FASTQ, %d alternating runs each" % (n, L, args.e2e_runs),
           "bases": n * L}
    reads = nt.synth_reads(genome, 2, 0, n, L, 10_000)
    for name in args.sources.split(","):
        with tempfile.TemporaryDirectory(dir=args.tmp) as d:
            ix.save(os.path.join(d, "ix"))
            fastq_text(reads, SOURCES[name](np.random.default_rng(5), n * L), L).tofile(os.path.join(d, "r.fq"))

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

            r = {}
            enc = ["encode", "-i", os.path.join(d, "ix"), os.path.join(d, "r.fq"), "--qualities", "keep"]
            for _ in range(args.e2e_runs):
                for coder in ("pack", "rans"):
                    q = os.path.join(d, coder + ".ntcq")
                    r.setdefault("encode_" + coder, []).append(
                        run(enc + ["--quality-file", q, "--quality-coder", coder], coder + ".dat"))
            for coder in ("pack", "rans"):
                r["quality_file_bytes_" + coder] = os.path.getsize(os.path.join(d, coder + ".ntcq"))
            for _ in range(args.e2e_runs):
                for coder in ("pack", "rans"):
                    dec = ["decode", "-i", os.path.join(d, "ix"), os.path.join(d, coder + ".dat"), "--quality-file",
                           os.path.join(d, coder + ".ntcq")]
                    r.setdefault("decode_" + coder, []).append(run(dec, coder + ".fq"))
            with open(os.path.join(d, "pack.fq"), "rb") as a, open(os.path.join(d, "rans.fq"), "rb") as b:
                same = True
                while same:
                    x, y = a.read(1 << 24), b.read(1 << 24)
                    same = x == y
                    if not x:
                        break
            r["decoded_texts_equal"] = same
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
    ap.add_argument("--source", default="markov_4_symbols", choices=sorted(SOURCES))
    ap.add_argument("--sources", default=",".join(SOURCES))
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    {"cost": part_cost, "trace": part_trace, "e2e": part_e2e}[args.part](args)


if __name__ == "__main__":
    main()
