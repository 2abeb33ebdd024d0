"""What keeping FASTQ read names costs (DESIGN.md "Read names"), on one GPU:

  cost    ntc_encode_pack_fastq on 1 M x 150 bp reads under names drop and keep, interleaved
          in one process, medians over --rounds after --warmups, for Illumina-style and
          SRA-style names; the bytes each names kernel has to move (computed from the
          shapes, to set against kernel times from a `rocprofv3 --kernel-trace --stats` run
          of --trace)
  sizes   raw name bytes, section payload bytes and deflated bytes with the pipeline's engine,
          and the deflate seconds of one thread for the sections against the raw names
          (newline-separated) on the same engine: what the GPU coding buys the host pool
  e2e     the native command line on a plain FASTQ file: encode with and without
          --names keep (alternating), decode with and without --name-file
  trace   a few keep calls and one named decode and nothing else, for the profiler

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

STYLES = ("illumina", "sra")


def names_blob(style, n, L, seed=5):
    """-> (name bytes back to back, their lengths)"""
    S = lambda a: a.astype("S")
    if style == "illumina":  # A00123:45:HXXXXDSXX:1:1101:x:y 1:N:0:ATCACGTT+AGGCTATA, x ascending, y random
        rng = np.random.default_rng(seed)
        x = 1000 + np.cumsum(rng.integers(0, 2, n)) // 8
        y = rng.integers(1000, 40000, n)
        a = np.char.add(np.char.add(np.char.add(np.char.add(b"A00123:45:HXXXXDSXX:1:1101:", S(x)), b":"), S(y)),
                        b" 1:N:0:ATCACGTT+AGGCTATA")
    else:  # SRR1234567.N N length=L
        i = np.arange(1, n + 1)
        a = np.char.add(np.char.add(np.char.add(np.char.add(b"SRR1234567.", S(i)), b" "), S(i)), b" length=%d" % L)
    mat = a.view(np.uint8).reshape(n, a.dtype.itemsize)
    return mat[mat != 0], np.char.str_len(a).astype(np.int64)


def fastq_text(blob, lens, reads, L, quals=None):
    """"@name\\nread\\n+\\nquals\\n" per read, assembled without a Python loop"""
    n = len(lens)
    tail = 2 * L + 5
    nl = np.full((n, 1), 10, np.uint8)
    q = np.full((n, L), ord("I"), np.uint8) if quals is None else quals.reshape(n, L)
    fixed = np.concatenate([nl, reads.reshape(n, L), nl, np.full((n, 1), ord("+"), np.uint8), nl, q, nl], axis=1)
    rec = np.concatenate([[0], np.cumsum(lens + 1 + tail)])
    noff = np.concatenate([[0], np.cumsum(lens)])
    out = np.empty(rec[-1], np.uint8)
    out[rec[:-1]] = ord("@")
    out[np.repeat(rec[:-1] + 1 - noff[:-1], lens) + np.arange(noff[-1])] = blob
    out[((rec[:-1] + 1 + lens)[:, None] + np.arange(tail)[None, :]).reshape(-1)] = fixed.reshape(-1)
    return out


def raw_call(ctx, text, n, block_reads, mode):
    """One ntc_encode_pack_fastq under the mode, wall ms (the payload is freed, not copied)."""
    nb = (n + block_reads - 1) // block_reads
    metas = (nt.BlockMeta * nb)()
    out, used, nbases, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int64(-1)
    ctx.set_option("names", mode)
    t0 = time.perf_counter()
    rc = ctx.L.ntc_encode_pack_fastq(ctx.h, text.ctypes.data_as(ctypes.c_void_p), len(text), n, block_reads, metas,
                                     ctypes.byref(out), ctypes.byref(used), ctypes.byref(nbases), ctypes.byref(bad))
    ms = 1e3 * (time.perf_counter() - t0)
    ctx.L.ntc_buffer_free(out)
    ctx.set_option("names", 0)
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


def deflate_sections(nm, npay, engine):
    """-> (deflated bytes, seconds of this one thread)"""
    buf = np.frombuffer(npay, np.uint8)
    total, t0 = 0, time.perf_counter()
    for m in nm:
        out, ln = ctypes.c_void_p(), ctypes.c_uint64()
        rc = nt.lib().ntc_n_deflate_section(ctypes.byref(m), ctypes.c_void_p(buf.ctypes.data + m.payload_off),
                                            nt.DEFLATE_ENGINES[engine], ctypes.byref(out), ctypes.byref(ln))
        assert rc == 0
        nt.lib().ntc_buffer_free(out)
        total += ln.value - 32
    return total, time.perf_counter() - t0


def deflate_raw(chunks, engine):
    """The same engine over raw bytes: ntc_q_deflate_section does not look at the words of a
    width-8 section, so each chunk goes through it as one (zero-padded to whole words)."""
    total, secs = 0, 0.0
    for c in chunks:
        m = nt.QualMeta()
        m.n_reads, m.n_quals, m.width, m.n_syms = 1, len(c), 8, 94
        m.payload_bytes = (len(c) + 7) // 8 * 8
        ctypes.memmove(m.alphabet, bytes(range(33, 127)), 94)
        buf = np.zeros(m.payload_bytes, np.uint8)
        buf[:len(c)] = c
        out, ln = ctypes.c_void_p(), ctypes.c_uint64()
        t0 = time.perf_counter()
        rc = nt.lib().ntc_q_deflate_section(ctypes.byref(m), buf.ctypes.data_as(ctypes.c_void_p), nt.DEFLATE_ENGINES[engine],
                                            ctypes.byref(out), ctypes.byref(ln))
        secs += time.perf_counter() - t0
        assert rc == 0
        nt.lib().ntc_buffer_free(out)
        total += ln.value - 24 - 94
    return total, secs


def part_cost(args):
    _, _, ctx, reads = setup(args)
    n, L, BR = args.reads, args.read_len, 65536
    res = {"what": "ntc_encode_pack_fastq wall ms, %d x %d bp, k = %d, %d interleaved rounds after %d warm-ups"
                   % (n, L, args.k, args.rounds, args.warmups)}
    for style in STYLES:
        blob, lens = names_blob(style, n, L)
        text = fastq_text(blob, lens, reads, L)
        t = {0: [], 1: []}
        for i in range(args.warmups + args.rounds):
            for mode in (0, 1):
                ms = raw_call(ctx, text, n, BR, mode)
                if i >= args.warmups:
                    t[mode].append(ms)
        raw_call(ctx, text, n, BR, 1)
        t0 = time.perf_counter()
        nm, npay = ctx.names()
        fetch_ms = 1e3 * (time.perf_counter() - t0)
        name_bytes, mid_bytes = sum(m.name_bytes for m in nm), sum(m.mid_bytes for m in nm)
        res[style] = {
            "drop": {"median_ms": statistics.median(t[0]), "min_ms": min(t[0]), "max_ms": max(t[0])},
            "keep": {"median_ms": statistics.median(t[1]), "min_ms": min(t[1]), "max_ms": max(t[1])},
            "fetch_sections_ms": fetch_ms, "text_bytes": len(text), "name_bytes": name_bytes, "mid_bytes": mid_bytes,
            "payload_bytes": len(npay),
            # what each kernel must move: measure reads every name and its predecessor's head and tail
            # (at most all of it again), 3 newline positions per read, and writes 14 bytes per read; emit
            # reads those 14 bytes, two offsets and the mids and writes the payload
            "bytes_moved": {"k_n_measure": 2 * name_bytes + n * (3 * 4 + 14), "k_n_emit": n * (14 + 16) + mid_bytes + len(npay)},
        }
    ctx.close()
    print(json.dumps({"cost": res}))


def part_sizes(args):
    _, _, ctx, reads = setup(args)
    n, L, BR = args.reads, args.read_len, 65536
    engine = "libdeflate" if nt.libdeflate_available() else "zlib"
    res = {"what": "%d names, sections of %d reads, engine %s, one thread" % (n, BR, engine)}
    for style in STYLES:
        blob, lens = names_blob(style, n, L)
        metas, payload, nb, (nm, npay) = ctx.encode_pack_fastq(fastq_text(blob, lens, reads, L).tobytes(), n, names="keep")
        sec = [deflate_sections(nm, npay, engine) for _ in range(3)]
        noff = np.concatenate([[0], np.cumsum(lens + 1)])
        lines = np.full(noff[-1], 10, np.uint8)  # the names, a newline after each
        lines[np.repeat(noff[:-1] - np.concatenate([[0], np.cumsum(lens)])[:-1], lens) + np.arange(len(blob))] = blob
        chunks = [lines[noff[a]:noff[min(a + BR, n)]] for a in range(0, n, BR)]
        raw = [deflate_raw(chunks, engine) for _ in range(3)]
        res[style] = {"raw_name_bytes": int(lens.sum()), "raw_with_newlines": len(lines), "payload_bytes": len(npay),
                      "mid_bytes": sum(m.mid_bytes for m in nm), "deflated_sections": sec[0][0], "deflated_raw": raw[0][0],
                      "deflate_s_sections": min(s for _, s in sec), "deflate_s_raw": min(s for _, s in raw)}
    ctx.close()
    print(json.dumps({"sizes": res}))


def part_trace(args):
    _, _, ctx, reads = setup(args)
    n, L = args.reads, args.read_len
    blob, lens = names_blob("illumina", n, L)
    text = fastq_text(blob, lens, reads, L).tobytes()
    for _ in range(4):
        metas, payload, nb, (nm, npay) = ctx.encode_pack_fastq(text, n, names="keep")
    arr = (nt.BlockMeta * len(metas))(*metas)
    ctx.unpack(arr, payload, len(metas))
    ctx.set_names(nm, npay)
    out = ctx.decode_fasta_unpacked(first_id=1)
    ctx.close()
    name_bytes = int(lens.sum())
    print(json.dumps({"trace": {"reads": n, "read_len": L, "fasta_bytes": len(out), "name_bytes": name_bytes,
                                "payload_bytes": len(npay),
                                "bytes_moved": {"k_n_expand": len(npay) + name_bytes, "k_named": name_bytes + n * L + len(out)}}}))


def part_e2e(args):
    genome = nt.synth_genome(1, args.genome_bp)
    ix = nt.Index.build([genome.tobytes()], args.k)
    n, L = args.e2e_reads, args.read_len
    exe = os.path.join(REPO, "ntcomp_amd", "ntcomp")
    res = {"what": "native command line, %d x %d bp plain FASTQ, %d alternating runs each" % (n, L, args.e2e_runs),
           "bases": n * L}
    reads = nt.synth_reads(genome, 2, 0, n, L, 10_000)
    for style in args.styles.split(","):
        with tempfile.TemporaryDirectory(dir=args.tmp) as d:
            ix.save(os.path.join(d, "ix"))
            blob, lens = names_blob(style, n, L)
            fastq_text(blob, lens, reads, L).tofile(os.path.join(d, "r.fq"))

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
                        **{k: v for k, v in s.items() if k.startswith("n_")}}

            r = {"encode_drop": [], "encode_keep": [], "decode_numbered": [], "decode_named": []}
            enc = ["encode", "-i", os.path.join(d, "ix"), os.path.join(d, "r.fq")]
            for _ in range(args.e2e_runs):
                r["encode_drop"].append(run(enc, "drop.dat"))
                r["encode_keep"].append(run(enc + ["--names", "keep", "--name-file", os.path.join(d, "n.ntcn")], "keep.dat"))
            r["name_file_bytes"] = os.path.getsize(os.path.join(d, "n.ntcn"))
            dec = ["decode", "-i", os.path.join(d, "ix"), os.path.join(d, "keep.dat")]
            for _ in range(args.e2e_runs):
                r["decode_numbered"].append(run(dec, "out.fa"))
                r["decode_named"].append(run(dec + ["--name-file", os.path.join(d, "n.ntcn")], "named.fa"))
            res[style] = r
    print(json.dumps({"e2e": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["cost", "sizes", "trace", "e2e"])
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--e2e-reads", type=int, default=5_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=91)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--e2e-runs", type=int, default=2)
    ap.add_argument("--styles", default="illumina,sra")
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    {"cost": part_cost, "sizes": part_sizes, "trace": part_trace, "e2e": part_e2e}[args.part](args)


if __name__ == "__main__":
    main()
