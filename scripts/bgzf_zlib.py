#!/usr/bin/env python3
"""The host alternative to `decode --bgzf`: a text cut into 65,280-byte BGZF members and deflated
by zlib, serially for the sizes and over a thread pool for the time (zlib releases the GIL).

    python scripts/bgzf_zlib.py TEXT [--levels 6,1] [--threads 16] [--gpu-file OUT.gz]

One JSON line: per level the bytes (28-byte EOF member included) and the wall seconds of the pool;
with --gpu-file the bytes of that `decode --bgzf` output and the ratios against each level
(DESIGN.md section 28)."""
import argparse
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

M = 65280
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")


def member(level, piece):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(piece) + c.flush()
    return len(HEAD) + 2 + len(body) + 8, struct.pack("<II", zlib.crc32(piece), len(piece))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("text")
    ap.add_argument("--levels", default="6,1")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--gpu-file")
    a = ap.parse_args()
    text = memoryview(open(a.text, "rb").read())
    out = {"text_bytes": len(text), "members": -(-len(text) // M), "threads": a.threads, "levels": {}}
    with ThreadPoolExecutor(a.threads) as pool:
        for level in (int(x) for x in a.levels.split(",")):
            t0 = time.time()
            sizes = list(pool.map(lambda at: member(level, text[at:at + M])[0], range(0, len(text), M)))
            out["levels"][str(level)] = {"bytes": sum(sizes) + 28, "pool_wall_s": round(time.time() - t0, 3)}
    if a.gpu_file:
        g = os.path.getsize(a.gpu_file)
        out["gpu_bytes"] = g
        out["gpu_over_level"] = {k: round(g / v["bytes"], 4) for k, v in out["levels"].items()}
        out["gpu_ratio"] = round(len(text) / g, 3)
    json.dump(out, sys.stdout)
    print()


if __name__ == "__main__":
    main()
