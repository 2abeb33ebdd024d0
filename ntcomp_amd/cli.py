"""ntcomp command line: `python -m ntcomp_amd build | encode | decode | verify | info`.

Mirrors the reference CLI (src/cli.rs:27-93, src/main.rs:91-211) with the hot path on
the GPU: FASTX ingest in C++ (needletail parse + normalize(true) restated), encode /
decode through libntcomp_gpu.so, blocks of 65,536 reads (main.rs:152) in the encoded.dat
layout (file header lib.rs:52-67, write_block_to lib.rs:232-252), decode output
">seq.N" (main.rs:203-209).  Encode runs the native pipeline (ntc_encode_file,
include/ntcomp_pipeline.h): FASTX batches into pinned buffers, GPU encode + block packer
per context, deflate on the host pool, blocks in file order.  Decode: blocks unzip on a
thread pool (ctypes releases the GIL), batches decode on the GPU contexts, FASTA
formatting on the pool, output in file order.

Index files: <prefix>.sbwt / <prefix>.lcs written by default in a recalled restatement of
the sbwt 0.3.11 / kbo 0.5.1 layout the reference always writes (kbo::index::serialize_sbwt,
main.rs:138), with the -p prefix lookup table (unpinned offline -- DESIGN.md section 8);
--index-format own writes this library's own layout.  encode/decode read either.
"""
import argparse
import sys


BLOCK_READS = 65536  # main.rs:152
# contexts per device (--contexts-per-gpu): encode 2 (one call's H2D of FASTQ text overlaps
# the other's kernels), decode 1 -- as the native CLI (ntcomp_main.cpp)
ENCODE_CONTEXTS_PER_GPU, DECODE_CONTEXTS_PER_GPU = 2, 1


def log(*a):
    print(*a, file=sys.stderr, flush=True)


class _Stats:
    """--stats: seconds spent per pipeline stage (summed over threads) and wall clock."""

    def __init__(self, on):
        import threading
        import time
        self.on, self.time, self.lock = on, time.perf_counter, threading.Lock()
        self.t0 = self.time()
        self.acc = {}

    def wrap(self, name, fn):
        if not self.on:
            return fn

        def run(*a, **k):
            t = self.time()
            try:
                return fn(*a, **k)
            finally:
                with self.lock:
                    self.acc[name] = self.acc.get(name, 0.0) + self.time() - t
        return run

    def report(self, **extra):
        if self.on:
            import json
            d = {k: round(v, 3) for k, v in self.acc.items()}
            try:  # interpreter start -> now, imports included
                import psutil
                import time
                extra["process_s"] = round(time.time() - psutil.Process().create_time(), 3)
            except Exception:
                pass
            log(json.dumps({"stats": d, "wall_s": round(self.time() - self.t0, 3), **extra}))


SMOOTH_MIN, SMOOTH_MAX, SMOOTH_DEFAULT = 12, 16777215, 32  # --quality-smooth [M]


def _smooth_default(argv):
    """--quality-smooth may stand without a value: it takes the next argument only when that is
    a number (as the native CLI does), else M = 32."""
    out = []
    for i, a in enumerate(argv):
        bare = a == "--quality-smooth" and not (i + 1 < len(argv) and argv[i + 1].isascii() and argv[i + 1].isdigit())
        out.append(f"--quality-smooth={SMOOTH_DEFAULT}" if bare else a)
    return out


def _bad_args(msg):
    """An argument error found after parsing: status 2, before anything is loaded or written
    (the native CLI's bad_args, same messages)."""
    log(f"ntcomp: {msg}")
    raise SystemExit(2)


def _check_nx_args(args):
    """encode: --non-acgt error|mask|keep and --exceptions PATH go together only under keep."""
    if args.non_acgt not in ("error", "mask", "keep"):
        _bad_args("encode: --non-acgt: error, mask or keep")
    if args.non_acgt == "keep" and not args.exceptions:
        _bad_args("encode: --non-acgt keep requires --exceptions PATH")
    if args.non_acgt != "keep" and args.exceptions is not None:
        _bad_args("encode: --exceptions is only written under --non-acgt keep")


def _read_list(path):
    """--input-list: one path, or tab-separated name and path, per line (main.rs:64-89)."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if not line:
                continue
            parts = line.split("\t")
            out.append(parts[1] if len(parts) > 1 else parts[0])
    return out


def cmd_build(args):
    import ntcomp_amd as nt
    files = list(args.seq_files or [])
    if args.input_list:
        files += _read_list(args.input_list)
    if not files:
        raise SystemExit("build: no input files")
    log(f"Building SBWT index from {len(files)} files...")
    seqs = []
    for path in files:
        rd = nt.FastxReader(path)
        for bases, offs in rd:
            for i in range(len(offs) - 1):
                seqs.append(bases[int(offs[i]):int(offs[i + 1])].tobytes())
        rd.close()
    builder = args.builder
    ctx = None
    if builder in ("auto", "gpu"):
        try:
            ctx = nt.GpuContext(args.device)
            builder = "gpu"
        except Exception as e:  # auto without a usable GPU: the host builder
            if builder == "gpu":
                raise SystemExit(f"build: --builder gpu: {e}")
            builder = "host"
    if builder == "gpu":
        # the same index built on the GPU (build.hip; tests/test_gpu_build.py: equal to the host
        # build).  kbo's BuildOpts (main.rs:111-134; cli.rs:55-60: --temp-dir builds "on temporary
        # disk space instead of in-memory", -m is the memory for that): -m given bounds the device
        # memory of a pass (else 85 % of the free HBM); with --temp-dir, sorted partitions past -m GB
        # of host memory go to files there, without it nothing spills.
        mem = int((args.mem_gb if args.mem_gb is not None else 4) * (1 << 30))
        stats = {}
        try:
            ix = nt.Index.build_gpu(ctx, seqs, args.kmer_size, add_revcomp=True,
                                    device_budget=mem if args.mem_gb is not None else 0,
                                    host_budget=mem if args.temp_dir else 0, temp_dir=args.temp_dir, stats=stats)
        finally:
            ctx.close()
        if args.verbose:
            log("build: " + ", ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}"
                                      for k, v in stats.items()))
    else:
        ix = nt.Index.build(seqs, args.kmer_size, add_revcomp=True, threads=args.num_threads)
    if args.index_format == "sbwt-rs" and args.prefix_precalc:
        ix.set_prefix_precalc(min(args.prefix_precalc, args.kmer_size, 12))
    log(f"Serializing SBWT index to {args.output_prefix}.sbwt ...")
    log(f"Serializing LCS array to {args.output_prefix}.lcs ...")
    ix.save(args.output_prefix, layout=args.index_format)


def _open_gpus(index, devices, st=None, per_gpu=1, decode_only=False):
    """per_gpu contexts per entry of devices; an int n means devices
    0..n-1.  The first context of a device uploads the index, the others on that device share
    it (ntc_index_share): calls alternate over the contexts, so one call's copies and host
    work overlap another's kernels.  decode_only: the upload builds only the walk table
    (ctx option decode_only)."""
    import ntcomp_amd as nt
    ctxs, first = [], {}
    for d in (range(devices) if isinstance(devices, int) else devices):
        for _ in range(max(1, per_gpu)):
            c = (st.wrap("gpu_init", nt.GpuContext) if st else nt.GpuContext)(d)
            if d in first:
                c.share_index(first[d])
            else:
                if decode_only:
                    c.set_option("decode_only", 1)
                (st.wrap("index_upload", c.upload) if st else c.upload)(index)
                first[d] = c
                if st and st.on:
                    st.acc["upload_host_derive"] = (st.acc.get("upload_host_derive", 0.0) +
                                                    c.get_option("upload_host_us") / 1e6)
            ctxs.append(c)
    return ctxs


def _devices(args):
    """--devices 0,0,1 (contexts, several may share a GPU) or --gpus N (devices 0..N-1)."""
    if getattr(args, "devices", None):
        return [int(x) for x in args.devices.split(",") if x.strip() != ""]
    return list(range(args.gpus))


def _check_q_args(args):
    """encode: --qualities drop|keep|bin8 and --quality-file PATH go together under keep and bin8."""
    if args.qualities not in ("drop", "keep", "bin8"):
        _bad_args("encode: --qualities: drop, keep or bin8")
    if args.qualities != "drop" and not args.quality_file:
        _bad_args(f"encode: --qualities {args.qualities} requires --quality-file PATH")
    if args.qualities == "drop" and args.quality_file is not None:
        _bad_args("encode: --quality-file is only written under --qualities keep or bin8")
    if args.quality_coder is not None and args.quality_coder not in ("pack", "rans"):
        _bad_args("encode: --quality-coder: pack or rans")
    if args.quality_coder is not None and args.qualities == "drop":
        _bad_args("encode: --quality-coder needs --qualities keep or bin8")
    # smoothing inside long matches: --quality-smooth [M] and --quality-smooth-to C
    for flag, value in (("--quality-smooth", args.quality_smooth), ("--quality-smooth-to", args.quality_smooth_to)):
        if value is not None and args.qualities == "drop":
            _bad_args(f"encode: {flag} needs --qualities keep or bin8")
    if args.quality_smooth is not None:
        m = args.quality_smooth
        if not (m.isascii() and m.isdigit() and len(m) <= 8 and SMOOTH_MIN <= int(m) <= SMOOTH_MAX):
            _bad_args(f"encode: --quality-smooth: M must be {SMOOTH_MIN}..{SMOOTH_MAX}")
        args.quality_smooth = int(m)
    if args.quality_smooth_to is not None:
        c = args.quality_smooth_to.encode("utf-8", errors="surrogateescape")
        if len(c) != 1 or not ord("$") <= c[0] <= ord("~"):
            _bad_args("encode: --quality-smooth-to: one printable byte in '$'..'~'")
        if args.qualities == "bin8" and c[0] <= ord("*"):
            _bad_args("encode: --quality-smooth-to: under bin8 the byte must lie above '*', or its level is that of '#'")
        args.quality_smooth_to = c


def _check_n_args(args):
    """encode: --names drop|keep|id and --name-file PATH go together under keep and id."""
    if args.names not in ("drop", "keep", "id"):
        _bad_args("encode: --names: drop, keep or id")
    if args.names != "drop" and not args.name_file:
        _bad_args(f"encode: --names {args.names} requires --name-file PATH")
    if args.names == "drop" and args.name_file is not None:
        _bad_args("encode: --name-file is only written under --names keep or id")


def _check_d_args(args, command, others):
    """--digest-file PATH: not empty, and no file the same call reads or writes."""
    d = args.digest_file
    if d is None:
        if command == "verify":
            _bad_args("verify: --digest-file PATH is required")
        return
    if d == "":
        _bad_args(f"{command}: --digest-file needs a path")
    if any(o is not None and o == d for o in others):
        _bad_args(f"{command}: --digest-file names a file this call uses already: {d}")


def _check_p_args(args):
    """encode: --mate-file R2 or --interleaved make the reads pairs; --mate-check ids|off goes with either."""
    if args.mate_file is not None and args.interleaved:
        _bad_args("encode: --mate-file and --interleaved exclude each other")
    if args.mate_file == "":
        _bad_args("encode: --mate-file needs a path")
    pairs = args.mate_file is not None or args.interleaved
    if args.mate_check is not None and not pairs:
        _bad_args("encode: --mate-check needs --mate-file or --interleaved")
    if args.mate_check not in (None, "ids", "off"):
        _bad_args("encode: --mate-check: ids or off")
    if pairs and args.host_parse:
        _bad_args("encode: pairs are woven and checked on the GPU: not with --host-parse")
    return None if not pairs else "nocheck" if args.mate_check == "off" else "ids"


def _check_i_args(args):
    """encode: --inflate gpu takes BGZF inputs alone (their first 18 bytes decide) and feeds the GPU parser."""
    if args.inflate not in ("host", "gpu"):
        _bad_args("encode: --inflate: host or gpu")
    if args.inflate != "gpu":
        return
    if args.host_parse:
        _bad_args("encode: --inflate gpu feeds the GPU parser: not with --host-parse")
    for p in (args.query_file, args.mate_file):
        if not p:
            continue
        try:
            with open(p, "rb") as f:
                h = f.read(18)
        except OSError:
            h = b""
        if not (len(h) == 18 and h[:3] == b"\x1f\x8b\x08" and h[3] & 4 and h[10] | h[11] << 8 >= 6 and h[12:14] == b"BC"
                and (h[16] | h[17] << 8) + 1 >= 26):
            _bad_args(f"encode: --inflate gpu: {p} does not start with a BGZF member")


def parse_reads(spec):
    """--reads A-B, 1-based and inclusive as decode prints seq.N; also A, A- and -B.  Returns
    (a, b) with b None for "to the last read"; ValueError for anything else."""
    s = spec
    a, sep, b = s.partition("-")
    if not s or (sep and "-" in b) or not all(x == "" or (x.isascii() and x.isdigit()) for x in (a, b)):
        raise ValueError(f"--reads {spec}: want A-B, A, A- or -B (1-based, inclusive)")
    if not sep:
        lo, hi = a, a
    else:
        lo, hi = a or "1", b or None
    if (not a and not b) or int(lo) < 1 or (hi is not None and int(hi) < int(lo)):
        raise ValueError(f"--reads {spec}: want 1 <= A <= B")
    return int(lo), None if hi is None else int(hi)


def parse_shard(spec):
    """--shard I/N with 1 <= I <= N; ValueError otherwise."""
    i, sep, n = spec.partition("/")
    if not sep or not (i.isascii() and i.isdigit() and n.isascii() and n.isdigit()) or not 1 <= int(i) <= int(n):
        raise ValueError(f"--shard {spec}: want I/N with 1 <= I <= N")
    return int(i), int(n)


def _check_r_args(args, command):
    """--reads and --shard, from the arguments alone (before anything is loaded): the parsed
    (a, b) or (i, n), or None."""
    reads, shard = getattr(args, "reads", None), getattr(args, "shard", None)
    if reads is not None and shard is not None:
        _bad_args(f"{command}: --reads and --shard exclude each other")
    try:
        if reads is not None:
            a, b = parse_reads(reads)
            if getattr(args, "mate_out", None) is not None and (a % 2 == 0 or (b is not None and b % 2 == 1)):
                _bad_args(f"{command}: --reads {reads} with --mate-out: whole pairs start at an odd read and end at an even one")
            return ("reads", a, b)
        if shard is not None:
            return ("shard",) + parse_shard(shard)
    except ValueError as e:
        _bad_args(f"{command}: {e}")
    return None


def _place_range(args, command, asked):
    """The asked --reads / --shard against the archive's block headers (host only): (first,
    count) from 0 for decode_file, or None for an empty shard.  Status 2 for a range the
    archive does not hold."""
    import ntcomp_amd as nt
    try:
        info = nt.archive_info(args.input_path)
    except nt.NtcError:
        raise SystemExit(f"ntcomp: {command}: cannot read {args.input_path}")
    total = info["n_reads"]
    if asked[0] == "reads":
        a, b = asked[1], asked[2] if asked[2] is not None else total
        if a > total or b > total:
            _bad_args(f"{command}: --reads {args.reads}: the archive holds {total} reads")
        if getattr(args, "mate_out", None) is not None and b % 2:
            _bad_args(f"{command}: --reads {args.reads} with --mate-out: the range ends inside a pair")
        return a - 1, b - a + 1
    lo, hi = nt.shard_blocks(asked[1], asked[2], info["n_blocks"])
    first = sum(blk["reads"] for blk in info["blocks"][:lo])
    count = sum(blk["reads"] for blk in info["blocks"][lo:hi])
    if count and getattr(args, "mate_out", None) is not None and first % 2:
        _bad_args(f"{command}: --shard {args.shard} with --mate-out: the slice starts inside a pair")
    return (first, count) if count else None


def _component_names(mask):
    return ",".join(n for c, n in enumerate(("seq", "sym", "qual", "name")) if mask >> c & 1) or "-"


def cmd_encode(args):
    """main.rs:141-181 through the native pipeline (ntc_encode_file): plain FASTQ parsed
    on the GPU (--host-parse: on the host pool, as every other input is), GPU encode +
    block packer per context, deflate on the host pool (--deflate gpu: on the GPU, behind the
    packer), blocks written in file order."""
    _check_nx_args(args)
    _check_q_args(args)
    _check_n_args(args)
    _check_d_args(args, "encode", (args.exceptions, args.quality_file, args.name_file, args.query_file))
    pair_mode = _check_p_args(args)
    _check_i_args(args)
    import ntcomp_amd as nt
    st = _Stats(args.stats)
    log("Loading SBWT index...")
    index = st.wrap("index_load", nt.Index.load)(args.index_prefix)
    ctxs = _open_gpus(index, _devices(args), st, args.contexts_per_gpu)
    log("Encoding fastX data...")
    if args.deflate == "auto":
        args.deflate = "adaptive" if nt.libdeflate_available() else "zlib"
    out = sys.stdout.buffer
    out.flush()
    nx_file = q_file = n_file = d_file = None
    try:
        if args.digest_file is not None:
            try:
                d_file = open(args.digest_file, "wb")
            except OSError:
                raise SystemExit(f"ntcomp: encode: cannot write {args.digest_file}")
        if args.names != "drop":
            try:
                n_file = open(args.name_file, "wb")
            except OSError:
                raise SystemExit(f"ntcomp: encode: cannot write {args.name_file}")
        if args.qualities != "drop":
            try:
                q_file = open(args.quality_file, "wb")
            except OSError:
                raise SystemExit(f"ntcomp: encode: cannot write {args.quality_file}")
        if args.non_acgt == "keep":
            try:
                nx_file = open(args.exceptions, "wb")
            except OSError:
                raise SystemExit(f"ntcomp: encode: cannot write {args.exceptions}")
        nx_args = {} if args.non_acgt == "error" else {"non_acgt": args.non_acgt,
                                                       "nx_fd": nx_file.fileno() if nx_file else -1}
        if q_file:
            nx_args.update(qualities=args.qualities, q_fd=q_file.fileno())
            for c in ctxs:  # the pipeline takes the coder and the smoothing from its contexts
                c.quality_coder = args.quality_coder or "pack"
                c.quality_smooth = args.quality_smooth or 0
                if args.quality_smooth_to is not None:
                    c.quality_smooth_to = args.quality_smooth_to
        if n_file:
            nx_args.update(names=args.names, n_fd=n_file.fileno())
        if d_file:
            nx_args.update(d_fd=d_file.fileno())
        if pair_mode:
            nx_args.update(pair_mode=pair_mode, mate_path=args.mate_file)
        if args.inflate == "gpu":
            nx_args.update(inflate="gpu")
        res =st.wrap("pipeline", nt.encode_file)(ctxs, args.query_file, out.fileno(), threads=args.threads,
                                                  blocks_per_batch=args.blocks_per_batch, deflate=args.deflate,
                                                  host_parse=args.host_parse, **nx_args)
    except nt.NtcError as e:
        bad = getattr(e, "bad_read", -1)
        raise SystemExit(f"ntcomp encode: {e}" + (f" (read {bad + 1})" if bad is not None and bad >= 0 else ""))
    finally:
        if nx_file:
            nx_file.close()
        if q_file:
            q_file.close()
        if n_file:
            n_file.close()
        if d_file:
            d_file.close()
        smoothed = sum(c.get_option("quality_smoothed_total") for c in ctxs) if args.quality_smooth else 0
        for c in ctxs:
            c.close()
    if res["dropped_blocks"]:
        log(f"warning: {res['dropped_blocks']} block(s) dropped (no long or no short records; "
            "main.rs:170 ignores write_block_to's error, SURVEY App. B.3)")
    if st.on:
        for k in ("parse_s", "gpu_s", "deflate_s", "write_s"):
            st.acc[k[:-2]] = res[k]
    st.report(command="encode", gpus=len(ctxs), threads=res["threads"], reads=res["reads"], blocks=res["blocks"],
              dropped_blocks=res["dropped_blocks"], pipeline_wall_s=round(res["wall_s"], 3), deflate=args.deflate,
              gpu_parsed_batches=res["gpu_parsed"], non_acgt=args.non_acgt,
              **{"nx_" + k: v for k, v in res.get("nx", dict.fromkeys(("runs", "bases", "reads",
                                                                        "runs_in_dropped_blocks"), 0)).items()},
              **({"qualities": args.qualities, "quality_coder": args.quality_coder or "pack",
                  **{"q_" + k: v for k, v in res["q"].items()}} if "q" in res else {}),
              **({"quality_smooth": args.quality_smooth, "quality_smooth_to": (args.quality_smooth_to or b"I").decode(),
                  "q_smoothed": smoothed} if args.quality_smooth else {}),
              **({"names": args.names, **{"n_" + k: v for k, v in res["n"].items()}} if "n" in res else {}),
              **({"d_" + k: v for k, v in res["d"].items() if k != "not_checkable"} if "d" in res else {}),
              **({"pairs": res["p"]["pairs"], "mate_check": "off" if pair_mode == "nocheck" else "ids",
                  "mate1_bytes": res["p"]["bytes1"], "mate2_bytes": res["p"]["bytes2"]} if "p" in res else {}),
              inflate=args.inflate,
              **{"inflate_" + k: v for k, v in res.get("i", dict.fromkeys(("members", "bytes", "runs", "fallback_runs"), 0)).items()
                 if k not in ("engine", "seconds")},
              inflate_s=round(res.get("i", {}).get("seconds", 0.0), 3))


def cmd_decode(args, verify=False):
    """main.rs:183-211 through the native pipeline (ntc_decode_file): blocks inflated and
    stream-decoded on the host pool, inverse-SBWT walk + FASTA formatting per context on the
    GPU, ">seq.N" text written in file order.  verify: the same with every block checked against
    the --digest-file and no text copied off the device or written; one line on stdout."""
    command = "verify" if verify else "decode"
    bgzf = bool(getattr(args, "bgzf", False))
    if verify and bgzf:
        _bad_args("verify: writes no text: not with --bgzf")
    _check_d_args(args, command, (args.exceptions, args.quality_file, args.name_file, args.input_path))
    asked = _check_r_args(args, command)
    import ntcomp_amd as nt
    st = _Stats(args.stats)
    r_args = {}
    if asked is not None:  # placed from the block headers, before any GPU is opened
        placed = _place_range(args, command, asked)
        if placed is None:  # an empty slice: nothing to write
            if verify:
                print(f"verify: OK: 0 blocks of the archive's, 0 reads (--shard {args.shard} is empty)", flush=True)
            if bgzf:  # an empty BGZF file is its EOF member
                sys.stdout.buffer.write(nt.BGZF_EOF)
                sys.stdout.buffer.flush()
                if getattr(args, "mate_out", None) is not None:
                    with open(args.mate_out, "wb") as f:
                        f.write(nt.BGZF_EOF)
            st.report(command=command, reads=0, blocks=0)
            return
        r_args = dict(reads=placed)
    index = st.wrap("index_load", nt.Index.load)(args.index_prefix)
    ctxs = _open_gpus(index, _devices(args), st, args.contexts_per_gpu, decode_only=True)
    log("Verifying encoded data..." if verify else "Decoding encoded data...")
    out = sys.stdout.buffer
    out.flush()
    mate_out = None  # a paired archive: the mate-1 records to stdout, the mate-2 records to --mate-out
    if getattr(args, "mate_out", None) is not None:
        try:
            mate_out = open(args.mate_out, "wb")
        except OSError:
            raise SystemExit(f"ntcomp: decode: cannot write {args.mate_out}")
    p_args = dict(out_fd2=mate_out.fileno(), pair_mode="nocheck") if mate_out else {}
    if bgzf:  # the text as BGZF members, compressed on the GPU that formatted it
        p_args["out_format"] = "bgzf"
    try:
        res = st.wrap("pipeline", nt.decode_file)(ctxs, args.input_path, -1 if verify else out.fileno(),
                                                  threads=args.threads, blocks_per_batch=args.blocks_per_batch,
                                                  nx_path=args.exceptions, q_path=args.quality_file,
                                                  n_path=args.name_file, d_path=args.digest_file, **p_args, **r_args)
    except nt.NtcError as e:
        bad = getattr(e, "bad_read", -1)
        raise SystemExit(f"ntcomp {command}: {e}" + (f" (read {bad + 1})" if e.code == 12 and bad is not None and bad >= 0
                                                     else ""))
    finally:
        if mate_out:
            mate_out.close()
        for c in ctxs:
            c.close()
    if res["dropped_blocks"]:
        # the reference's `while let Ok(..) = decode_block` just ends here (main.rs:202)
        log(f"warning: {res['error']}; {res['dropped_blocks']} block(s) not decoded")
    if st.on:
        for k, name in (("parse_s", "unzip"), ("gpu_s", "gpu"), ("write_s", "write")):
            st.acc[name] = res[k]
    if verify:
        d = res["d"]
        checked = sum(1 << c for c, k in enumerate(("blocks_seq", "blocks_sym", "blocks_qual", "blocks_name")) if d[k])
        of = f" of {res['r']['blocks_total']}" if "r" in res else ""
        print(f"verify: OK: {d['sections']}{of} blocks, {res['reads']} reads, checked {_component_names(checked)}, "
              f"not checkable {_component_names(d['not_checkable'])}", flush=True)
    st.report(command=command, gpus=len(ctxs), threads=res["threads"], reads=res["reads"], blocks=res["blocks"],
              pipeline_wall_s=round(res["wall_s"], 3),
              **({**{"d_" + k: v for k, v in res["d"].items() if k != "not_checkable"},
                  "d_not_checkable": _component_names(res["d"]["not_checkable"])} if "d" in res else {}),
              **({"pairs": res["p"]["pairs"], "mate1_bytes": res["p"]["bytes1"], "mate2_bytes": res["p"]["bytes2"]}
                 if "p" in res else {}),
              **({"r_" + k: v for k, v in res["r"].items()} if "r" in res else {}),
              **({} if verify else _bgzf_stats(bgzf, res.get("z", {}))))


def _bgzf_stats(on, z):
    """the --stats fields of decode --bgzf (ntc_z_stats); zeros without the flag"""
    return dict(bgzf=on, bgzf_members=z.get("members", 0), bgzf_text_bytes=z.get("text_bytes", 0), bgzf_bytes=z.get("bytes", 0),
                bgzf_chunks_stored=z.get("chunks_stored", 0), bgzf_chunks_huffman=z.get("chunks_huffman", 0),
                bgzf_chunks_matches=z.get("chunks_matches", 0), bgzf_s=round(z.get("seconds", 0.0), 3))


def cmd_info(args):
    """`ntcomp info encoded.dat [--blocks]`: what the archive holds, from its block headers
    alone (ntc_archive_info): no index, no GPU.  Status 1 when a block's headers are damaged."""
    import ntcomp_amd as nt
    try:
        info = nt.archive_info(args.input_path)
    except nt.NtcError:
        raise SystemExit(f"ntcomp: info: cannot read {args.input_path}")
    size = sum(b["bytes"] for b in info["blocks"])
    bad = sum(b["bad"] for b in info["blocks"])
    print(f"blocks {info['n_blocks']} reads {info['n_reads']} records {info['n_records']} bytes {size} "
          f"trailing_bytes {info['tail_bytes']}" + (f" damaged_blocks {bad}" if bad else ""))
    if args.blocks:
        first = 1
        for i, b in enumerate(info["blocks"]):
            print(f"block {i} offset {b['offset']} bytes {b['bytes']} reads {b['reads']} records {b['records']} "
                  + ("damaged" if b["bad"] else f"first_read {first}"))
            first += b["reads"]
    sys.stdout.flush()
    if bad:
        raise SystemExit(1)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="ntcomp", description="Sequencing data compression with SBWT + k-bounded "
                                 "matching statistics; encode/decode hot path on MI355X.")
    ap.add_argument("-V", "--version", action="version", version="ntcomp 0.1.0")  # Cargo.toml:3, clap's `version`
    sub = ap.add_subparsers(dest="command")
    b = sub.add_parser("build", help="Build the compression dictionary")
    b.add_argument("seq_files", nargs="*", help="Sequence data file(s).")
    b.add_argument("-l", "--input-list", help="File with paths or tab separated name and path on each line.")
    b.add_argument("-o", "--output-prefix", required=True, help="Prefix for output files <prefix>.sbwt and <prefix>.lcs.")
    b.add_argument("-k", dest="kmer_size", type=int, default=31, help="k-mer size.")
    b.add_argument("-p", "--prefix-precalc", type=int, default=8,
                   help="Prefix lookup table length (written with --index-format sbwt-rs).")
    b.add_argument("-d", "--dedup-batches", action="store_true",
                   help="Deduplicate k-mers per batch (the GPU build always deduplicates a full pass in place).")
    b.add_argument("-t", "--threads", dest="num_threads", type=int, default=1)
    b.add_argument("-m", "--mem-gb", type=float, default=None,
                   help="Memory budget in GB (default 4 for --temp-dir): device memory per GPU build pass when given "
                        "(else 85%% of the free HBM), and with --temp-dir the host memory for sorted partitions.")
    b.add_argument("--temp-dir", help="Build on temporary disk space at this path: sorted partitions past -m GB of "
                                      "host memory spill there (without it nothing spills).")
    b.add_argument("--verbose", action="store_true")
    b.add_argument("--builder", choices=["auto", "host", "gpu"], default="auto",
                   help="auto (default): the GPU when one is usable, else the host; host: threaded C++ builder "
                        "(in memory); gpu: k-mer sort, dummies, LCS and labels on the GPU in memory-bounded "
                        "passes (same index)")
    b.add_argument("--device", type=int, default=0, help="GPU for --builder gpu")
    b.add_argument("--index-format", choices=["own", "sbwt-rs"], default="sbwt-rs",
                   help="sbwt-rs (default): a restatement of the sbwt 0.3.11/kbo 0.5.1 files the reference writes "
                        "(parity unpinned); own: this library's layout. encode/decode read either")
    e = sub.add_parser("encode", help="Encode fastX data using an SBWT index")
    e.add_argument("query_file", help="Query file with sequence data.")
    e.add_argument("-i", "--index", dest="index_prefix", required=True, help="Prefix for prebuilt <prefix>.sbwt and <prefix>.lcs")
    e.add_argument("--gpus", type=int, default=1, help="GPUs to encode on (batches dealt round-robin).")
    e.add_argument("--devices", help="comma-separated device list, one context each (e.g. 0,0 shares GPU 0); "
                                     "overrides --gpus")
    e.add_argument("--threads", type=int, default=0,
                   help="host pool for FASTQ parse and deflate (0: CPUs available to the process)")
    e.add_argument("--contexts-per-gpu", type=int, default=ENCODE_CONTEXTS_PER_GPU,
                   help="contexts per device sharing one index copy; calls alternate over them")
    e.add_argument("--blocks-per-batch", type=int, default=4, help="65,536-read blocks per GPU call")
    e.add_argument("--deflate", choices=["auto", "zlib", "libdeflate", "adaptive", "gpu"], default="auto",
                   help="gzip engine for the block streams, level 6 (the reference's Compression::default()): "
                        "adaptive (auto, when libdeflate.so.0 loads: libdeflate, with streams of >= 7.9 bits of "
                        "entropy per byte stored), libdeflate (~3x faster than zlib) or zlib.  The deflate bytes "
                        "differ, the inflated streams do not; no engine reproduces the reference's zlib-rs bytes.  gpu: the "
                        "streams are deflated on the GPU behind the packer (32 KiB chunks, greedy in-chunk matches; about "
                        "2 %% larger) and the host only copies the members; side files are deflated as under auto")
    e.add_argument("--inflate", default="host", metavar="ENGINE",
                   help="who inflates a BGZF input: host (default; libdeflate on the reader's threads) or gpu (runs of "
                        "members inflated on the first GPU; every input must be BGZF; the output is byte for byte the host "
                        "engine's; not with --host-parse)")
    e.add_argument("--stats", action="store_true", help="print per-stage seconds to stderr")
    e.add_argument("--host-parse", action="store_true",
                   help="parse a plain FASTQ on the host pool instead of the GPU")
    e.add_argument("--non-acgt", default="error", metavar="POLICY",
                   help="reads with N or IUPAC symbols: error (default) stops at the first, mask replaces each symbol "
                        "by the substitute base (lossy), keep also writes the replaced symbols to the --exceptions "
                        "file (lossless)")
    e.add_argument("--exceptions", metavar="PATH", help="with --non-acgt keep: the side file to write")
    e.add_argument("--qualities", default="drop", metavar="MODE",
                   help="FASTQ quality scores: drop (default), keep (lossless) or bin8 (Phred scores binned to 8 levels, "
                        "lossy); keep and bin8 write them, packed on the GPU, to the --quality-file")
    e.add_argument("--quality-file", metavar="PATH", help="with --qualities keep or bin8: the side file to write")
    e.add_argument("--quality-coder", default=None, metavar="CODER",
                   help="with --qualities keep or bin8: pack (default; packed codes, deflated on the host) or rans "
                        "(order-1 rANS coded on the GPU, no host deflate)")
    e.add_argument("--quality-smooth", default=None, metavar="M",
                   help="with --qualities keep or bin8: smooth the scores inside long matches to the index (lossy): a "
                        "score above '#' that lies in a long record of at least M bases (12..16777215; 32 when M is "
                        "left out) becomes the --quality-smooth-to byte")
    e.add_argument("--quality-smooth-to", default=None, metavar="C",
                   help="the byte --quality-smooth writes: one of '$'..'~' (default I; under bin8 above '*')")
    e.add_argument("--names", default="drop", metavar="MODE",
                   help="FASTQ read names: drop (default), keep (lossless: the header line after '@') or id (the name up "
                        "to its first space or tab, lossy); keep and id write them, front-coded on the GPU, to the "
                        "--name-file")
    e.add_argument("--name-file", metavar="PATH", help="with --names keep or id: the side file to write")
    e.add_argument("--digest-file", metavar="PATH",
                   help="also write per-block content digests, computed on the GPU, for decode / verify --digest-file")
    e.add_argument("--mate-file", metavar="R2",
                   help="paired-end reads: the query file holds the mate-1 records, R2 the mate-2 records (any supported "
                        "compression each); the GPU weaves them, reads 2p and 2p+1 of the archive are a pair")
    e.add_argument("--interleaved", action="store_true", help="paired-end reads: the query file already alternates the mates")
    e.add_argument("--mate-check", default=None, metavar="CHECK",
                   help="ids (default): the mates' ids (cut at the first blank, /1 and /2 stripped) are compared on the "
                        "GPU; off: they are not")
    d = sub.add_parser("decode", help="Decode data written with Encode")
    d.add_argument("input_path", help="File with encoded fastX data.")
    d.add_argument("-i", "--index", dest="index_prefix", required=True, help="Prefix for prebuilt <prefix>.sbwt and <prefix>.lcs")
    d.add_argument("--gpus", type=int, default=1, help="GPUs to decode on (batches dealt round-robin).")
    d.add_argument("--devices", help="comma-separated device list, one context each; overrides --gpus")
    d.add_argument("--threads", type=int, default=0, help="block unzip / format threads (0: CPUs available)")
    d.add_argument("--contexts-per-gpu", type=int, default=DECODE_CONTEXTS_PER_GPU,
                   help="contexts per device sharing one index copy; calls alternate over them")
    d.add_argument("--blocks-per-batch", type=int, default=2, help="blocks per GPU call")
    d.add_argument("--stats", action="store_true", help="print per-stage seconds to stderr")
    d.add_argument("--quality-file", metavar="PATH",
                   help="the side file of encode --qualities keep or bin8: the output is then FASTQ")
    d.add_argument("--name-file", metavar="PATH",
                   help="the side file of encode --names keep or id: the reads carry their names instead of seq.N")
    d.add_argument("--exceptions", metavar="PATH",
                   help="the side file of encode --non-acgt keep, whose symbols are put back")
    d.add_argument("--digest-file", metavar="PATH",
                   help="the digest file of encode --digest-file: every block is checked against it on the GPU; another "
                        "index, a damaged or truncated file or a side file of another run is an error that names the "
                        "block and the component")
    d.add_argument("--mate-out", metavar="R2.out",
                   help="the archive holds pairs: the mate-1 records go to stdout, the mate-2 records to R2.out")
    r_help = ("only reads A-B of the archive, 1-based and inclusive as decode numbers them (seq.N); also A, A- and -B. "
              "Only the blocks that hold them are read; the reads keep their numbers, names and qualities")
    s_help = ("only the I-th of N contiguous slices of whole blocks; the N outputs concatenated in order are the full "
              "decode (one process per GPU or node)")
    d.add_argument("--bgzf", action="store_true",
                   help="write the text as BGZF (.gz: bgzip's blocked gzip), cut at record boundaries and compressed on the "
                        "GPU; with --mate-out both outputs.  The EOF member is written only when the decode succeeds; the "
                        "--shard outputs concatenated are one BGZF file")
    d.add_argument("--reads", metavar="A-B", help=r_help)
    d.add_argument("--shard", metavar="I/N", help=s_help)
    v = sub.add_parser("verify", help="Check encoded data against its digest file without writing the text")
    v.add_argument("input_path", help="File with encoded fastX data.")
    v.add_argument("-i", "--index", dest="index_prefix", required=True, help="Prefix for prebuilt <prefix>.sbwt and <prefix>.lcs")
    v.add_argument("--gpus", type=int, default=1, help="GPUs to decode on (batches dealt round-robin).")
    v.add_argument("--devices", help="comma-separated device list, one context each; overrides --gpus")
    v.add_argument("--threads", type=int, default=0, help="block unzip threads (0: CPUs available)")
    v.add_argument("--contexts-per-gpu", type=int, default=DECODE_CONTEXTS_PER_GPU,
                   help="contexts per device sharing one index copy; calls alternate over them")
    v.add_argument("--blocks-per-batch", type=int, default=2, help="blocks per GPU call")
    v.add_argument("--stats", action="store_true", help="print per-stage seconds to stderr")
    v.add_argument("--digest-file", metavar="PATH", help="the digest file of encode --digest-file (required)")
    v.add_argument("--quality-file", metavar="PATH", help="the side file of encode --qualities keep or bin8")
    v.add_argument("--name-file", metavar="PATH", help="the side file of encode --names keep or id")
    v.add_argument("--exceptions", metavar="PATH", help="the side file of encode --non-acgt keep")
    v.add_argument("--bgzf", action="store_true", help=argparse.SUPPRESS)  # (refused: verify writes no text)
    v.add_argument("--reads", metavar="A-B", help=r_help + "; the touched blocks are checked whole")
    v.add_argument("--shard", metavar="I/N", help=s_help)
    n = sub.add_parser("info", help="What an encoded file holds, from its block headers (no index, no GPU)")
    n.add_argument("input_path", help="File with encoded fastX data.")
    n.add_argument("--blocks", action="store_true", help="one line per block")
    args = ap.parse_args(_smooth_default(sys.argv[1:] if argv is None else list(argv)))
    if getattr(args, "threads", None) == 0:
        import ntcomp_amd as nt
        args.threads = nt.host_threads()
    if args.command == "build":
        cmd_build(args)
    elif args.command == "encode":
        cmd_encode(args)
    elif args.command == "decode":
        cmd_decode(args)
    elif args.command == "verify":
        cmd_decode(args, verify=True)
    elif args.command == "info":
        cmd_info(args)
    else:
        ap.print_help()
    return 0
