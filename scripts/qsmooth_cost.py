"""What smoothing qualities inside long matches costs and gains (DESIGN.md "Smoothing qualities
inside long matches"), on one GPU:

  cost    ntc_encode_pack_fastq on 1 M x 150 bp reads (k = 91, 1 % substituted bases) under
          qualities keep against keep + quality_smooth 32, interleaved in one process, medians
          over --rounds after --warmups; the side data's bytes under both coders with and
          without smoothing (pack: packed and deflated; rans: the bodies); the share of
          positions smoothed and the share of substituted bases among them (parity); the
          bytes k_q_smooth has to move, computed from the shapes, to set against its time in a
          `rocprofv3 --kernel-trace --stats` run of --trace
  trace   a few smoothed calls and nothing else, for the profiler

The quality model is not uniform noise.  A read's scores follow a two-state chain: "good"
draws from : F I (mostly I), "poor" from + , 5 < ; a good position turns poor with probability
0.01 in the body of the read and rising linearly to 0.25 over its last 40 positions, a poor
one recovers with probability 0.3; a substituted base and its right neighbour are poor.

Prints one JSON object per part."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import ntcomp_amd as nt  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
GOOD, POOR = np.frombuffer(b"FFFI:IIIIIIIIIII", np.uint8), np.frombuffer(b"+,5<", np.uint8)


def make_reads(genome, rng, n, L, rate):
    """-> (bases n x L, bool n x L: the substituted positions)"""
    starts = rng.integers(0, len(genome) - L, n)
    reads = genome[starts[:, None] + np.arange(L)[None, :]]
    err = rng.random((n, L)) < rate
    code = np.searchsorted(ACGT, reads)
    reads = np.where(err, ACGT[(code + rng.integers(1, 4, (n, L))) % 4], reads).astype(np.uint8)
    return reads, err


def make_quals(rng, err):
    n, L = err.shape
    down = np.full(L, 0.01)
    down[L - 40:] = np.linspace(0.01, 0.25, 40)
    poor = np.zeros((n, L), dtype=bool)
    u = rng.random((n, L))
    state = np.zeros(n, dtype=bool)
    for i in range(L):  # (columns: the chain runs along the read)
        state = np.where(state, u[:, i] >= 0.3, u[:, i] < down[i]) | err[:, i] | (err[:, i - 1] if i else False)
        poor[:, i] = state
    return np.where(poor, POOR[rng.integers(0, len(POOR), (n, L))], GOOD[rng.integers(0, len(GOOD), (n, L))]).astype(np.uint8)


def fastq_text(reads, quals):
    n, L = reads.shape
    nl = np.full((n, 1), 10, np.uint8)
    rec = np.concatenate([np.frombuffer(b"@r\n", np.uint8)[None, :].repeat(n, 0), reads, nl,
                          np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0), quals, nl], axis=1)
    return rec.reshape(-1)


def raw_call(ctx, text, n, block_reads, smooth, coder=0, to=ord("I")):
    """One ntc_encode_pack_fastq under qualities keep, wall ms (the payload is freed, not copied)."""
    nb = (n + block_reads - 1) // block_reads
    metas = (nt.BlockMeta * nb)()
    out, used, nbases, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int64(-1)
    for key, v in (("qualities", 1), ("quality_coder", coder), ("quality_smooth", smooth), ("quality_smooth_to", to)):
        ctx.set_option(key, v)
    t0 = time.perf_counter()
    rc = ctx.L.ntc_encode_pack_fastq(ctx.h, text.ctypes.data_as(ctypes.c_void_p), len(text), n, block_reads, metas,
                                     ctypes.byref(out), ctypes.byref(used), ctypes.byref(nbases), ctypes.byref(bad))
    ms = 1e3 * (time.perf_counter() - t0)
    ctx.L.ntc_buffer_free(out)
    for key, v in (("qualities", 0), ("quality_coder", 0), ("quality_smooth", 0), ("quality_smooth_to", ord("I"))):
        ctx.set_option(key, v)
    if rc:
        raise nt.NtcError(rc, ctx.L.ntc_last_error(ctx.h).decode())
    return ms


def records_of(ctx):
    """records of the last encode (the status box of the call holds them)"""
    try:
        return ctx.encode_status()
    except nt.NtcError:
        return 0


def setup(args):
    rng = np.random.default_rng(9)
    genome = nt.synth_genome(1, args.genome_bp)
    ix = nt.Index.build([genome.tobytes()], args.k)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    reads, err = make_reads(genome, rng, args.reads, args.read_len, args.error_rate)
    quals = make_quals(rng, err)
    return ctx, reads, err, quals, fastq_text(reads, quals)


def deflated_bytes(qm, qp):
    engine = "libdeflate" if nt.libdeflate_available() else "zlib"
    buf, total = np.frombuffer(qp, np.uint8), 0
    for m in qm:
        out, ln = ctypes.c_void_p(), ctypes.c_uint64()
        rc = nt.lib().ntc_q_deflate_section(ctypes.byref(m), ctypes.c_void_p(buf.ctypes.data + m.payload_off),
                                            nt.DEFLATE_ENGINES[engine], ctypes.byref(out), ctypes.byref(ln))
        assert rc == 0
        nt.lib().ntc_buffer_free(out)
        total += ln.value
    return total, engine


def part_cost(args):
    ctx, reads, err, quals, text = setup(args)
    n, L, BR, M = args.reads, args.read_len, 65536, args.m
    nq = n * L
    res = {"what": "ntc_encode_pack_fastq wall ms, %d x %d bp, k = %d, %.3g substituted, M = %d, %d interleaved rounds "
                   "after %d warm-ups" % (n, L, args.k, args.error_rate, M, args.rounds, args.warmups)}
    for coder, name in ((0, "pack"), (1, "rans")):
        t = {0: [], M: []}
        for i in range(args.warmups + args.rounds):
            for smooth in (0, M):
                ms = raw_call(ctx, text, n, BR, smooth, coder)
                if i >= args.warmups:
                    t[smooth].append(ms)
        side = {}
        for smooth in (0, M):
            raw_call(ctx, text, n, BR, smooth, coder)
            qm, qp = ctx.qualities()
            side[smooth] = {"payload_bytes": len(qp), "widths": sorted({m.width for m in qm})}
            if coder == 0:
                side[smooth]["deflated_bytes"], side[smooth]["deflate_engine"] = deflated_bytes(qm, qp)
        res[name] = {"keep": {"median_ms": statistics.median(t[0]), "min_ms": min(t[0]), "max_ms": max(t[0]), **side[0]},
                     "keep_smooth": {"median_ms": statistics.median(t[M]), "min_ms": min(t[M]), "max_ms": max(t[M]), **side[M]}}
    # parity: to a byte the model never draws, so the smoothed positions can be read off the decoded text
    metas, payload, _, (qm, qp) = ctx.encode_pack_fastq(text.tobytes(), n, qualities="keep", quality_smooth=M,
                                                         quality_smooth_to=b"~")
    smoothed = ctx.quality_smoothed
    n_rec = records_of(ctx)
    arr = (nt.BlockMeta * len(metas))(*metas)
    assert ctx.unpack(arr, payload, len(metas))[0] == len(metas)
    ctx.set_qualities(qm, qp)
    out = np.frombuffer(ctx.decode_fasta_unpacked(first_id=1), np.uint8)
    lines = [l for l in out.tobytes().split(b"\n")[3::4]]
    got = np.frombuffer(b"".join(lines), np.uint8).reshape(n, L)
    hit = got == ord("~")
    assert int(hit.sum()) == smoothed and np.array_equal(got[~hit], quals[~hit])
    res["parity"] = {"positions": nq, "smoothed": smoothed, "share_smoothed": smoothed / nq,
                     "trusted_at_or_below_floor_not_counted": True,
                     "substituted_bases": int(err.sum()), "substituted_bases_smoothed": int((hit & err).sum())}
    # what k_q_smooth must move: the qualities once, a record and two offsets pairs per read in;
    # out at most the qualities again (whole words where it replaced a byte), at least the bytes replaced
    res["k_q_smooth_bytes"] = {"read": nq + 8 * n_rec + 4 * 8 * n, "written_at_least": smoothed, "written_at_most": nq,
                               "records": n_rec}
    ctx.close()
    print(json.dumps({"cost": res}))


def part_trace(args):
    ctx, reads, err, quals, text = setup(args)
    for _ in range(4):
        raw_call(ctx, text, args.reads, 65536, args.m, 0)
    n_rec = records_of(ctx)
    smoothed = ctx.quality_smoothed
    ctx.close()
    print(json.dumps({"trace": {"reads": args.reads, "read_len": args.read_len, "calls": 4, "records": n_rec,
                                "smoothed": smoothed}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["cost", "trace"])
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=91)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--genome-bp", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmups", type=int, default=3)
    args = ap.parse_args()
    {"cost": part_cost, "trace": part_trace}[args.part](args)


if __name__ == "__main__":
    main()
