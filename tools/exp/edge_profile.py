#!/usr/bin/env python3
"""Structured builds (the device derives the deblocking edge bits from the CU / TU structure) against plain builds, on the
bench's 4K Main10 I and B pictures.

    python tools/exp/edge_profile.py host
        host side, no GPU needed: de265hip_derive_edge_flags (what a host saves) against the structured build's extra host
        time (validation + staging the structure planes: a dry build with the device-side scan, with and without structure),
        and the extra bytes uploaded per picture
    python tools/exp/edge_profile.py device --kind B --structured 1 --streams 3 [--pictures 24]
        pictures built and run to the final stage on `streams` decoders (interleaved; 1 = alone); under
        `rocprofv3 --kernel-trace --stats -- python ...` the k_scan_tus line is the scan's first launch with (structured) and
        without the edge-bit workgroups"""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("DE265HIP_TUNING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import pysynth  # noqa: E402
from libde265_amd import _abi, backend, farm  # noqa: E402

W, H, BD = 3840, 2160, 10


def picture(kind):
    st, refs = farm.gop_plan(3)[0 if kind == "I" else 1]
    over = dict(ref_slots=refs) if refs else {}
    return pysynth.SynthPicture(pysynth.default_config(W, H, BD, st, seed=farm.gop_seed(4, 0) + (0 if kind == "I" else 1), **over))


def best_of(fn, reps):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def host(reps):
    L = backend.lib()
    for kind in ("I", "B"):
        sp = picture(kind)
        structure = sp.structure()
        cb_log2, cb_part, tu_split, noedge = structure
        d = sp.d
        flags = np.ascontiguousarray(noedge).copy()

        def helper():
            flags[:] = noedge
            backend.derive_edge_flags(d.params, d.slices, d.n_slices, d.ctbs, cb_log2, cb_part, tu_split, flags)
        t_helper = best_of(helper, reps)
        cs, keep = backend.cu_structure(structure)
        os.environ["DE265HIP_DRY_NO_HASH"] = "1"
        t = {}
        dev_bytes = {}
        for name, arg in (("plain", None), ("structured", C.byref(cs))):
            t[name] = best_of(lambda: L.de265hip_debug_build_host_only_structured(sp.desc, arg, 1, 1, None), reps)
            pic = C.c_void_p()
            assert L.de265hip_debug_build_host_only_structured(sp.desc, arg, 1, 1, C.byref(pic)) == 0
            s = _abi.PictureStats()
            L.de265hip_picture_get_stats(pic, C.byref(s))
            lay = (C.c_int64 * 32)()
            L.de265hip_debug_picture_layout(pic, lay)
            dev_bytes[name] = (s.device_bytes, lay[26])
            L.de265hip_picture_free(pic)
        print("4K10 %s: derive_edge_flags %.3f ms | dry host stage (device scan; a structured one runs the edge body on the host "
              "too) plain %.3f ms, structured %.3f ms | structure planes %d + %d + %d bytes, arena +%d bytes" % (
                  kind, 1e3 * t_helper, 1e3 * t["plain"], 1e3 * t["structured"],
                  cb_log2.size, cb_part.size, tu_split.size, dev_bytes["structured"][0] - dev_bytes["plain"][0]), flush=True)
        if backend.device_count() > 0:
            # the product's host stage (de265hip_picture_build_host[_structured]: validation, MC tasks, staging into pinned
            # memory, the upload issued); the edge bits are the device's.  Each picture is freed outside the timed region.
            dec = backend.Decoder()
            dec.dpb_alloc(3, W, H, BD)
            tb = {}
            for name in ("plain", "structured"):
                samples = []
                for _ in range(reps):
                    h = C.c_void_p()
                    t0 = time.perf_counter()
                    if name == "plain":
                        rc = L.de265hip_picture_build_host(dec._h, 3, sp.desc, C.byref(h))
                    else:
                        rc = L.de265hip_picture_build_host_structured(dec._h, 3, sp.desc, C.byref(cs), C.byref(h))
                    samples.append(time.perf_counter() - t0)
                    assert rc == 0, rc
                    dec.sync()
                    L.de265hip_picture_free(h)
                tb[name] = (min(samples), float(np.median(samples)))
            print("4K10 %s: build_host plain min %.3f / median %.3f ms, structured min %.3f / median %.3f ms: extra %.3f ms (min), "
                  "%.3f ms (median)" % (kind, 1e3 * tb["plain"][0], 1e3 * tb["plain"][1], 1e3 * tb["structured"][0], 1e3 * tb["structured"][1],
                                        1e3 * (tb["structured"][0] - tb["plain"][0]), 1e3 * (tb["structured"][1] - tb["plain"][1])), flush=True)
            dec.close()
        sp.close()


def device(kind, structured, streams, pictures):
    sp = picture(kind)
    structure = sp.structure() if structured else None
    decs = [backend.Decoder() for _ in range(streams)]
    for dec in decs:
        for s in (0, 1):
            dec.dpb_alloc(s, W, H, BD)
            dec.fill(s, 512, 512, 512)
        dec.dpb_alloc(2, W, H, BD)
    t0 = time.perf_counter()
    live = []
    for k in range(pictures):
        dec = decs[k % streams]
        pic = dec.build(2, sp.desc, structure=structure)
        dec.run(pic, _abi.STAGE_FINAL)
        live.append(pic)
        if len(live) >= 2 * streams:
            for dd in decs:
                dd.sync()
            for p in live:
                p.free()
            live = []
    for dd in decs:
        dd.sync()
    for p in live:
        p.free()
    dt = time.perf_counter() - t0
    print("4K10 %s structured=%d streams=%d: %d pictures in %.1f ms" % (kind, structured, streams, pictures, 1e3 * dt), flush=True)
    for dd in decs:
        dd.close()
    sp.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["host", "device"])
    ap.add_argument("--kind", choices=["I", "B"], default="B")
    ap.add_argument("--structured", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--pictures", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.what == "host":
        host(a.reps)
    else:
        device(a.kind, a.structured, a.streams, a.pictures)
