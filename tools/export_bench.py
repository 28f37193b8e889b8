"""Product-path rate of bench.py's workload (4K Main10 4:2:0 closed GOPs of 16, one pipeline per GOP stream) with and without
the pictures leaving the DPB:

    none          no output (bench.py's `value`)
    export_native every picture exported (de265hip_pipeline_submit_desc_export) into a two-deep ring of torch tensors, NATIVE planar
    export_f16    the same as F16 planar
    export_native_ring8, export_f16_ring8   the same with rings of 8, as deep as copy_out's
    copy_out      every picture copied out to pinned host memory (bench.py's with_copy_out: a ring of 8 per stream)

    python tools/export_bench.py [--steps K] [--warmup W] [--streams S] [--workers N]

Prints one JSON line: pictures/s per mode.  A ring entry is handed to the next picture once the ticket that used it has been
waited for, as an application's output queue would: a ring of n holds each stream's pipeline to n pictures in flight."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (before libde265_hip.so: tests/conftest.py)

import pysynth  # noqa: E402
from libde265_amd import backend, farm  # noqa: E402


def make_gop(w, h, bd, gop, seed):
    pics = []
    for k, (st, refs) in enumerate(farm.gop_plan(gop)):
        over = dict(ref_slots=refs, weighted_pred=1 if (k % 10) == 5 else 0) if refs else {}
        pics.append(pysynth.SynthPicture(pysynth.default_config(w, h, bd, st, seed=seed + k, **over)))
    return pics


def run_pass(pipes, gops, steps, rings, kind):
    """every picture of every stream submitted `steps` times; rings[s]: ExportSpecs / PinnedPlanes (kind 'export' / 'copy')"""
    def feed(s):
        ring = rings[s] if rings else None
        tickets = [None] * (len(ring) if ring else 0)
        n = 0
        for _ in range(steps):
            for k, sp in enumerate(gops[s]):
                if not ring:
                    pipes[s].submit_desc(k, sp.desc)
                    continue
                b = n % len(ring)
                if tickets[b] is not None:
                    pipes[s].wait(tickets[b])
                if kind == "export":
                    tickets[b] = pipes[s].submit_desc(k, sp.desc, export=ring[b])
                else:
                    tickets[b] = pipes[s].submit_desc(k, sp.desc, ring[b])
                n += 1
        for t in tickets:
            if t is not None:
                pipes[s].wait(t)

    with ThreadPoolExecutor(len(pipes)) as pool:
        list(pool.map(feed, range(len(pipes))))
    for p in pipes:
        p.drain()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--workers", type=int, default=3)
    ap.add_argument("--gop", type=int, default=16)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bit-depth", type=int, default=10)
    args = ap.parse_args()
    W, H, BD, S, GOP = args.width, args.height, args.bit_depth, args.streams, args.gop
    gops = [make_gop(W, H, BD, GOP, farm.gop_seed(4, 0, s)) for s in range(S)]
    decs = [backend.Decoder(device=0) for _ in range(S)]
    for d in decs:
        for k in range(GOP):
            d.dpb_alloc(k, W, H, BD)
    pipes = [backend.Pipeline(d, args.workers) for d in decs]
    def ring(dtype, n):
        return [[backend.ExportSpec(W, H, BD, BD, 1, dtype=dtype, device="cuda") for _ in range(n)] for _ in range(S)]

    modes = {
        "none": (None, None),
        "export_native": (ring("native", 2), "export"),
        "export_f16": (ring("f16", 2), "export"),
        "export_native_ring8": (ring("native", 8), "export"),
        "export_f16_ring8": (ring("f16", 8), "export"),
        "copy_out": ([[backend.PinnedPlanes(W, H, BD) for _ in range(8)] for _ in range(S)], "copy"),
    }
    res = {}
    for name, (rings, kind) in modes.items():
        run_pass(pipes, gops, max(1, args.warmup), rings, kind)
        t0 = time.perf_counter()
        run_pass(pipes, gops, args.steps, rings, kind)
        res[name] = round(S * GOP * args.steps / (time.perf_counter() - t0), 1)
    for p in pipes:
        p.close()
    for r in modes["copy_out"][0]:
        for pp in r:
            pp.free()
    for d in decs:
        d.close()
    print(json.dumps({"metric": "product-path pictures/s (%dx%d %d-bit 4:2:0, GOP %d, %d streams)" % (W, H, BD, GOP, S),
                      "steps": args.steps, "warmup": args.warmup, "workers": args.workers, **res}))


if __name__ == "__main__":
    main()
