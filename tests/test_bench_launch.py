"""bench.py's multi-GPU launch on CPU (--dry-run stops at the GPU boundary): `bench.py
--gpus 2` outside torch.distributed.run starts a 2-rank child job itself, each rank takes its
shard (weak scaling, data independent of the sharding, main.rs:152,162-173), checks an
oracle sample of its own reads, and rank 0 prints one line carrying every rank's verdict."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True,
                       timeout=600, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout  # stdout: the JSON line alone
    return json.loads(lines[0]), p.stderr


def test_bench_spawns_ranks_without_torchrun():
    line, err = _run(["--gpus", "2", "--dry-run", "--full", "--configs", "encode", "--reads-per-gpu", "4000",
                      "--batch-reads", "1500", "--genome-bp", "200000"])
    assert "[launcher] 2 ranks" in err
    assert line["n_gpus"] == 2 and line["dry_run"] is True
    par = line["parity"]
    assert par["ranks"] == 2 and par["shards"] == [[0, 4000], [4000, 4000]]
    assert par["encode_bit_exact_all_ranks"] is True
    assert all(c > 0 for c in par["reads_checked_per_rank"])
    assert "[rank 1] C91: reads 4000..8000 in 3 batch(es)" in err


SMALL = ["--reads-per-gpu", "4000", "--batch-reads", "1500", "--genome-bp", "200000"]


def test_plain_run_is_the_headline_alone():
    """without --full: C91 encode only, no oracle sample, no other configs"""
    sys.path.insert(0, REPO)
    import bench
    for bad in (["--configs", "strains"], ["--mode", "decode"], ["--configs", "encode,c31"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    with pytest.raises(SystemExit):
        bench.parse_args(["--full", "--configs", "decode", "--dump-outputs", "x"])
    assert bench.parse_args([]).full is False and bench.parse_args(["--full", "--configs", "strains"]).full
    line, err = _run(["--gpus", "1", "--dry-run"] + SMALL)
    assert line["full"] is False and line["dry_run"] is True
    assert line["parity"]["encode_bit_exact_all_ranks"] is None and line["parity"]["reads_checked_per_rank"] is None
    assert "decode" not in line and "strains" not in line and "c31" not in line


class _FakeCtx:
    """device pointers are keys of a dict of host arrays"""

    def __init__(self):
        self.mem = {}

    def put(self, arr):
        self.mem[len(self.mem) + 1] = arr
        return len(self.mem)

    def d2h(self, arr, ptr):
        arr[:] = self.mem[ptr][:len(arr)]
        return arr


def test_dump_outputs_sample_and_totals(tmp_path):
    """dump_outputs on two batches whose latest outputs sit in different slots: the sampled
    reads' records are the right slices of the shard's output, the totals cover all of it,
    and a second dump of the same outputs is the same files"""
    sys.path.insert(0, REPO)
    import bench
    rng = np.random.default_rng(5)
    ctx, batches, all_recs, all_cnt = _FakeCtx(), [], [], []
    for n, last in ((700, 1), (300, 0)):
        cnt = rng.integers(0, 6, n)
        recs = rng.integers(0, 2 ** 63, int(cnt.sum()), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        roffs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        good = {"d_recs": ctx.put(np.concatenate([recs, np.zeros(8, np.uint64)])), "d_roffs": ctx.put(roffs)}
        stale = {"d_recs": ctx.put(np.zeros(len(recs) + 8, np.uint64)), "d_roffs": ctx.put(np.zeros(n + 1, np.uint64))}
        batches.append({"n": n, "n_recs": len(recs), "cap": len(recs) + 8, "last_out": last,
                        "out": [stale, good] if last else [good, stale]})
        all_recs.append(recs)
        all_cnt.append(cnt)
    recs, cnt = np.concatenate(all_recs), np.concatenate(all_cnt)
    starts = np.cumsum(cnt) - cnt

    class Sh:
        pass
    sh = Sh()
    sh.batches, sh.n, sh.first = batches, 1000, 5000
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(ctx, sh, str(a), 0, 1)
    bench.dump_outputs(ctx, sh, str(b), 0, 1)
    got = {p.name[:-4]: np.load(p) for p in a.iterdir()}
    assert set(got) == {"sample_reads", "sample_record_offsets", "sample_records", "totals"}
    assert all(v.dtype == np.float64 for v in got.values())
    for name, v in got.items():
        assert np.array_equal(v, np.load(b / (name + ".npy")))
    reads = got["sample_reads"].astype(np.int64) - 5000
    assert len(reads) == 1000 and np.array_equal(reads, np.arange(1000))  # fewer reads than the sample: all of them
    off = got["sample_record_offsets"].astype(np.int64)
    assert np.array_equal(off[:, 0], starts[reads]) and np.array_equal(off[:, 1], starts[reads] + cnt[reads])
    words = got["sample_records"].astype(np.uint64)
    assert np.array_equal((words[:, 0] << np.uint64(32)) | words[:, 1], recs)
    fold = np.bitwise_xor.reduce(recs)
    assert got["totals"].tolist() == [1000.0, float(len(recs)), float(fold >> np.uint64(32)),
                                      float(fold & np.uint64(0xFFFFFFFF))]


def test_dump_outputs_keeps_to_its_budget(tmp_path, monkeypatch):
    """more reads and records than the sample holds: a seeded subset, cut at the record budget"""
    sys.path.insert(0, REPO)
    import bench
    monkeypatch.setattr(bench, "DUMP_READS", 200)
    monkeypatch.setattr(bench, "DUMP_RECORDS", 500)
    n = 1000
    recs = np.arange(1, 4 * n + 1, dtype=np.uint64) << np.uint64(30)
    ctx = _FakeCtx()
    out = {"d_recs": ctx.put(recs), "d_roffs": ctx.put(np.arange(0, 4 * n + 1, 4, dtype=np.uint64))}

    class Sh:
        pass
    sh = Sh()
    sh.batches, sh.n, sh.first = [{"n": n, "n_recs": 4 * n, "cap": 4 * n, "last_out": 0, "out": [out]}], n, 0
    bench.dump_outputs(ctx, sh, str(tmp_path), 0, 1)
    reads = np.load(tmp_path / "sample_reads.npy").astype(np.int64)
    assert len(reads) == 125 and np.all(np.diff(reads) > 0)  # 500 records at 4 per read
    pick = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, size=200, replace=False))[:125]
    assert np.array_equal(reads, pick)
    words = np.load(tmp_path / "sample_records.npy").astype(np.uint64)
    want = recs.reshape(n, 4)[pick].ravel()
    assert np.array_equal((words[:, 0] << np.uint64(32)) | words[:, 1], want)


@pytest.mark.gpu
def test_plain_bench_dumps_the_oracles_records(tmp_path):
    """a plain run on the GPU at a small size: --steps sets the timed steps, ms_per_step is
    there, and the dumped records of the sampled reads are the oracle's records of those reads"""
    import ntcomp_amd as nt
    from oracle_lib import OracleIndex
    line, err = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)] + SMALL)
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["roofline"] is None and line["cpu_baseline"] is None
    # value and ms_per_step are one measurement: bases / step time, up to the rounding of ms_per_step to 1 us
    assert abs(line["value"] - 4000 * 150 / (line["ms_per_step"] / 1e3) / 1e6) <= \
        line["value"] * 0.0006 / line["ms_per_step"] + 0.01
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("sample_reads", "sample_record_offsets", "sample_records",
                                                         "totals")}
    assert all(v.dtype == np.float64 for v in got.values())
    genome = nt.synth_genome(1, 200_000)
    ix = nt.Index.build([genome.tobytes()], 91)
    reads = nt.synth_reads(genome, 2, 0, 4000, 150, 10_000)
    exp, eoff = OracleIndex(ix.n, 91, ix.rows, ix.C, ix.lcs).encode(reads, np.arange(0, 4000 * 150 + 1, 150,
                                                                                     dtype=np.uint64))
    assert np.array_equal(got["sample_reads"], np.arange(4000))
    assert np.array_equal(got["sample_record_offsets"][:, 0], eoff[:-1].astype(np.float64))
    assert np.array_equal(got["sample_record_offsets"][:, 1], eoff[1:].astype(np.float64))
    words = got["sample_records"].astype(np.uint64)
    assert np.array_equal((words[:, 0] << np.uint64(32)) | words[:, 1], exp)
    fold = np.bitwise_xor.reduce(exp)
    assert got["totals"].tolist() == [4000.0, float(len(exp)), float(fold >> np.uint64(32)),
                                      float(fold & np.uint64(0xFFFFFFFF))]


def test_bench_default_sizing_is_c91x8_per_gpu_at_n_gt_1():
    sys.path.insert(0, REPO)
    import bench
    a = bench.parse_args(["--gpus", "8"])
    assert a.reads_per_gpu is None  # resolved per world size in main(): 25M at N > 1, 10M at N = 1
    src = open(os.path.join(REPO, "bench.py")).read()
    assert "10_000_000 if world == 1 else 25_000_000" in src
