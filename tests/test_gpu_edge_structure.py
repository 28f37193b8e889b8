"""Structured builds on the GPU: the host hands over the CU / TU structure and garbage (or no) edge bits; the device derives
the edge bits (libde265_amd/csrc/edge_core.h, by workgroups of the scan's first launch or a launch of its own) before any
kernel reads them, and every stage of the picture equals what libde265 / the oracle compute from the true edge bits."""
import ctypes as C
import glob
import hashlib
import json
import os

import numpy as np
import pytest

import f1_stream
import pyoracle
import pysynth
import ref_cases
from libde265_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stream_*.npz")))
GOLD_P = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_pictures.json")))["cases"]


@pytest.fixture(scope="module")
def dec():
    from libde265_amd import backend
    assert backend.device_count() > 0, "no GPU visible: HIP path cannot run"
    d = backend.Decoder()
    yield d
    d.close()


def garbage_high_nibble(flags, seed):
    rng = np.random.default_rng(seed)
    return ((flags & 0x0F) | (rng.integers(0, 16, flags.size, dtype=np.uint8) << 4)).astype(np.uint8)


def with_flags(desc, flags, drop_motion=False):
    d = _abi.PictureDesc.from_buffer_copy(desc)
    d.blk_flags = C.cast(flags.ctypes.data, C.POINTER(C.c_uint8))
    if drop_motion:
        d.blk_motion = None
    return d


def md5(planes):
    m = hashlib.md5()
    for p in planes:
        m.update(np.ascontiguousarray(p).tobytes())
    return m.hexdigest()


@pytest.mark.parametrize("case", ref_cases.PICTURE_CASES, ids=[c["name"] for c in ref_cases.PICTURE_CASES])
def test_structured_pictures_reproduce_the_reference(dec, case):
    """every picture case of tests/golden/ref_pictures.json, edge bits of blk_flags replaced by garbage"""
    sp, refs, init = ref_cases.make_picture(case)
    w, h, bd, cf = case["w"], case["h"], case["bd"], 0 if case.get("monochrome") else case.get("chroma_format", 1)
    try:
        for s, pl in refs.items():
            dec.dpb_alloc(s, w, h, bd, chroma_format=cf)
            dec.upload(s, pl)
        dec.dpb_alloc(2, w, h, bd, chroma_format=cf)
        structure = sp.structure()
        flags = garbage_high_nibble(structure[3], case["seed"])
        pic = dec.build(2, with_flags(sp.d, flags), structure=structure)
        try:
            for stage, key in ref_cases.STAGES:
                dec.upload(2, init)
                dec.run(pic, stage)
                dec.sync()
                assert ref_cases.digest(dec.download(2, w, h, bd)) == GOLD_P[case["name"]][key], "%s: %s" % (case["name"], key)
        finally:
            pic.free()
    finally:
        sp.close()


def _stream_recorder(rp, n, strip):
    from libde265_amd import backend
    d = rp.to_desc()
    cb_log2, cb_part, tu_split, noedge = rp.structure()
    rp._flags[:] = noedge if strip else garbage_high_nibble(noedge, n)      # (the desc's blk_flags: the edges libde265 derived, replaced)
    sf = rp.a["scaling"] if rp.a["scaling"].size else None
    rec = backend.Recorder(rp.params, sf)
    rec.record_desc(d)
    rec.record_structure(cb_log2, cb_part, tu_split)
    return rec


@pytest.mark.parametrize("fx", FIXTURES, ids=[os.path.basename(f)[7:-4] for f in FIXTURES])
def test_stream_fixtures_through_a_structured_recorder(dec, fx):
    for n, (rp, dg) in enumerate(f1_stream.load_fixture(fx)):
        P = rp.params
        rec = _stream_recorder(rp, n, strip=n % 2 == 0)
        slot = rp.meta["dst_slot"]
        dec.dpb_alloc(slot, P.width, P.height, P.bit_depth_luma, chroma_format=P.chroma_format_idc)
        pic = rec.submit(dec, slot)
        try:
            for stage, key in ((_abi.STAGE_PREFILTER, "prefilter"), (_abi.STAGE_FINAL, "final")):
                dec.upload(slot, pyoracle.alloc_planes(P.width, P.height, P.bit_depth_luma, chroma_format=P.chroma_format_idc))
                dec.run(pic, stage)
                dec.sync()
                got = dec.download(slot, P.width, P.height, P.bit_depth_luma)
                assert md5(got) == dg[key], "%s picture %d: %s differs from libde265's decoder" % (os.path.basename(fx), n, key)
        finally:
            pic.free()
            rec.free()


@pytest.mark.parametrize("fx", FIXTURES, ids=[os.path.basename(f)[7:-4] for f in FIXTURES])
def test_stream_fixtures_through_a_pipeline_of_structured_recorders(fx):
    """the pipeline's `prepare` path: three workers build the structured recorders' pictures, copy-outs into pinned planes"""
    from libde265_amd import backend
    pics = f1_stream.load_fixture(fx)
    P = pics[0][0].params
    d = backend.Decoder()
    pipe = backend.Pipeline(d, 3)
    pins = [backend.PinnedPlanes(P.width, P.height, P.bit_depth_luma, P.chroma_format_idc) for _ in pics]
    try:
        for rp, _ in pics:
            d.dpb_alloc(rp.meta["dst_slot"], P.width, P.height, P.bit_depth_luma, chroma_format=P.chroma_format_idc)
        tickets = [pipe.submit(rp.meta["dst_slot"], (lambda rp=rp, n=n: _stream_recorder(rp, n, strip=n % 2 == 1)), pins[n])
                   for n, (rp, _) in enumerate(pics)]
        for n, (rp, dg) in enumerate(pics):
            pipe.wait(tickets[n])
            assert md5(pins[n].planes) == dg["final"], "%s picture %d" % (os.path.basename(fx), n)
        pipe.drain()
    finally:
        pipe.close()
        for p in pins:
            p.free()
        d.close()


def _run_structured(dec, w, h, bd, st, seed, drop_motion=False, stages=(0, 1, 2), **over):
    sp = pysynth.SynthPicture(pysynth.default_config(w, h, bd, st, seed=seed, **over))
    try:
        refs = {0: pysynth.fill_planes(w, h, bd, 100 + seed), 1: pysynth.fill_planes(w, h, bd, 200 + seed)}
        for slot, pl in refs.items():
            dec.dpb_alloc(slot, w, h, bd)
            dec.upload(slot, pl)
        dec.dpb_alloc(2, w, h, bd)
        structure = sp.structure()
        flags = garbage_high_nibble(structure[3], seed)
        pic = dec.build(2, with_flags(sp.d, flags, drop_motion), structure=structure)
        try:
            for stage in stages:
                init = pysynth.fill_planes(w, h, bd, 999)
                exp = [p.copy() for p in init]
                pyoracle.reconstruct(sp.desc, sp.order, refs, exp, last_stage=stage)      # (the generator's own edge bits)
                dec.upload(2, init)
                dec.run(pic, stage)
                dec.sync()
                got = dec.download(2, w, h, bd)
                for c in range(3):
                    bad = np.argwhere(got[c] != exp[c])
                    assert bad.size == 0, "seed %d stage %d comp %d: %d samples differ, first %s" % (seed, stage, c, len(bad), tuple(bad[0]))
        finally:
            pic.free()
    finally:
        sp.close()


@pytest.mark.parametrize("drop_motion", [False, True], ids=["motion_plane", "motion_from_pus"])
@pytest.mark.parametrize("seed", range(6))
def test_random_structured_pictures_equal_the_oracle(dec, seed, drop_motion):
    over = [dict(n_slices=3, lf_across_slices_pct=50), dict(tile_cols=3, tile_rows=2, slice_per_tile=1, lf_across_tiles=0,
            lf_across_slices_pct=50), dict(tile_cols=2, tile_rows=2, lf_across_tiles=0, n_slices=2), dict(log2_ctb_size=4, n_slices=4),
            dict(log2_ctb_size=5, tile_cols=2, lf_across_tiles=0, amp=1), dict(deblocking=0, n_slices=2)][seed]
    _run_structured(dec, 416, 240, 8 + 2 * (seed & 1), seed % 2, 7700 + seed, drop_motion, **over)


@pytest.mark.parametrize("env", [{"DE265HIP_SEPARATE_BS": "1"}, {"DE265HIP_TWO_PASS_DEBLOCK": "1"}, {"DE265HIP_HOST_SCAN": "1"}],
                         ids=["separate_bs", "two_pass_deblock", "host_scan"])
def test_structured_pictures_under_decoder_variants(env):
    """variables read when a decoder is created: the bS kernel, the two-pass deblocking, the host scan (the edge bits by a
    launch of their own)"""
    from libde265_amd import backend
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    d2 = backend.Decoder()
    try:
        _run_structured(d2, 416, 240, 10, 0, 7801, n_slices=2, tile_cols=2, lf_across_tiles=0, amp=1)
        _run_structured(d2, 352, 288, 8, 1, 7802, drop_motion=True, n_slices=3, lf_across_slices_pct=50)
    finally:
        d2.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
