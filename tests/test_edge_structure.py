"""Structured builds without a GPU: the host hands over the CU / TU structure (de265hip_cu_structure) instead of the
deblocking edge bits, and the edge-bit body the device runs (libde265_amd/csrc/edge_core.h) derives them.  A dry build
(de265hip_debug_build_host_only_structured) runs that same body on the host into the kept arena, where these tests read it:
  - against the host helper de265hip_derive_edge_flags on seeded synthetic pictures;
  - against libde265's own derive_edgeFlags: the edges the recording decoder dumped for the 15 real-bitstream fixtures, and
    the reference-generated edge_flags digests of every picture case in tests/golden/ref_pictures.json;
  - validation, garbage structures, and unstructured builds that stay byte-identical to what they were."""
import ctypes as C
import glob
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import f1_stream
import pysynth
import ref_cases
from libde265_amd import _abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stream_*.npz")))
GOLD_P = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_pictures.json")))["cases"]
EDGE_OFF = 25                      # de265hip_debug_picture_layout: offset of blk_flags in the arena; [26]: the EdgeJob


def garbage_high_nibble(flags, seed):
    """the host's low nibble kept, random edge bits: a structured build must ignore them"""
    rng = np.random.default_rng(seed)
    return ((flags & 0x0F) | (rng.integers(0, 16, flags.size, dtype=np.uint8) << 4)).astype(np.uint8)


def with_flags(desc, flags):
    """a copy of the description whose blk_flags point at `flags` (keep it alive)"""
    d = _abi.PictureDesc.from_buffer_copy(desc)
    d.blk_flags = C.cast(flags.ctypes.data, C.POINTER(C.c_uint8))
    return d


def dry_build(desc, structure, mode=0):
    """-> (rc, derived blk_flags plane or None, whole kept arena or None)"""
    L = backend.lib()
    pic = C.c_void_p()
    if structure is None:
        rc = L.de265hip_debug_build_host_only_structured(C.byref(desc), None, 1, mode, C.byref(pic))
    else:
        cs, keep = backend.cu_structure(structure)
        rc = L.de265hip_debug_build_host_only_structured(C.byref(desc), C.byref(cs), 1, mode, C.byref(pic))
    if rc:
        assert not pic.value
        return rc, None, None
    try:
        lay = (C.c_int64 * 32)()
        assert L.de265hip_debug_picture_layout(pic, lay) == 0
        P = desc.params
        nblk = ((P.width + 3) // 4) * ((P.height + 3) // 4)
        flags = np.empty(nblk, np.uint8)
        assert L.de265hip_debug_picture_read(pic, lay[EDGE_OFF], nblk, flags.ctypes.data) == 0
        # (what a dry build wrote: the uploaded part of the arena, which ends with the EdgeJob in a structured build)
        n = lay[EDGE_OFF + 1] + 256 if lay[EDGE_OFF + 1] >= 0 else lay[EDGE_OFF] + nblk
        arena = np.empty(n, np.uint8)
        assert L.de265hip_debug_picture_read(pic, 0, n, arena.ctypes.data) == 0
        return 0, flags, (arena, lay[EDGE_OFF], lay[EDGE_OFF + 1])
    finally:
        L.de265hip_picture_free(pic)


def helper_edges(desc, structure, noedge):
    cb_log2, cb_part, tu_split = structure[:3]
    ef = np.ascontiguousarray(noedge, dtype=np.uint8).copy()
    backend.derive_edge_flags(desc.params, desc.slices, desc.n_slices, desc.ctbs, cb_log2, cb_part, tu_split, ef)
    return ef


# ------------------------------------------------------------------ ABI
def test_cu_structure_layout_matches_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "de265_hip.h"\nint main(){\n'
           'printf("size %zu\\n", sizeof(de265hip_cu_structure));\n'
           'printf("cb_log2_size %zu\\n", offsetof(de265hip_cu_structure, cb_log2_size));\n'
           'printf("cb_part_mode %zu\\n", offsetof(de265hip_cu_structure, cb_part_mode));\n'
           'printf("tu_split %zu\\n", offsetof(de265hip_cu_structure, tu_split));\n'
           'return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        cfile, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(cfile, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
        out = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(_abi.CuStructure)
    for name, _ in _abi.CuStructure._fields_:
        assert int(out[name]) == getattr(_abi.CuStructure, name).offset, name


# ------------------------------------------------------------------ the body == the host helper
SYNTH = []
for _i, (_ctb, _over) in enumerate([
        (4, dict(n_slices=3, lf_across_slices_pct=50)),
        (5, dict(n_slices=4, lf_across_slices_pct=30)),
        (6, dict(n_slices=2, lf_across_slices_pct=0)),
        (4, dict(tile_cols=3, tile_rows=2, slice_per_tile=1, lf_across_tiles=0, lf_across_slices_pct=50)),
        (5, dict(tile_cols=2, tile_rows=2, lf_across_tiles=0)),
        (6, dict(tile_cols=3, tile_rows=1, slice_per_tile=1, lf_across_tiles=0, lf_across_slices_pct=100)),
        (5, dict(deblocking=0)),
        (6, dict(deblocking=0, n_slices=2)),
        (4, dict(amp=1, split_bias=20)),
        (5, dict(amp=1, split_bias=80)),
        (6, dict(amp=1, n_slices=3, lf_across_slices_pct=50)),
]):
    for _st in (0, 1, 2):
        SYNTH.append((_i, _ctb, _st, _over))
# picture sizes that are not CTB multiples
SIZES = [(416, 240), (328, 184), (360, 200), (200, 136)]


def _synth(i, ctb, st, over, size_idx=None):
    w, h = SIZES[(i + st) % len(SIZES)] if size_idx is None else SIZES[size_idx]
    return pysynth.SynthPicture(pysynth.default_config(w, h, 8 + 2 * (st & 1), st, seed=9100 + 10 * i + st, log2_ctb_size=ctb, **over))


@pytest.mark.parametrize("i,ctb,st,over", SYNTH, ids=["%d_ctb%d_st%d" % (i, 1 << c, st) for i, c, st, _ in SYNTH])
@pytest.mark.parametrize("mode", [0, 1], ids=["host_scan", "device_scan"])
def test_structured_build_derives_what_the_host_helper_derives(i, ctb, st, over, mode):
    sp = _synth(i, ctb, st, over)
    try:
        structure = sp.structure()
        noedge = structure[3]
        assert not (noedge & 0xF0).any()
        d = sp.d
        flags_in = garbage_high_nibble(noedge, i)
        rc, got, _ = dry_build(with_flags(d, flags_in), structure, mode)
        assert rc == 0
        exp = helper_edges(d, structure, noedge)
        assert np.array_equal(got & 0x0F, flags_in & 0x0F)
        assert np.array_equal(got, exp), "%d units differ" % int((got != exp).sum())
        assert bool((exp & 0xF0).any()) == bool(over.get("deblocking", 1))
    finally:
        sp.close()


@pytest.mark.parametrize("which", [0, 1])
def test_deblocking_on_in_one_slice_only(which):
    """slice_deblocking_filter_disabled_flag set on all slices but one of the generated description"""
    sp = pysynth.SynthPicture(pysynth.default_config(416, 240, 8, 0, seed=9300 + which, n_slices=2, lf_across_slices_pct=50, amp=1))
    try:
        d = sp.d
        assert d.n_slices == 2
        d.slices[which].slice_deblocking_filter_disabled_flag = 1
        d.slices[1 - which].slice_deblocking_filter_disabled_flag = 0
        structure = sp.structure()
        noedge = structure[3]
        flags_in = garbage_high_nibble(noedge, 77)
        rc, got, _ = dry_build(with_flags(d, flags_in), structure)
        assert rc == 0
        exp = helper_edges(d, structure, noedge)
        assert np.array_equal(got, exp)
        on = np.array([not d.slices[d.ctbs[a].slice_idx].slice_deblocking_filter_disabled_flag for a in range(d.n_ctbs)])
        assert on.any() and not on.all() and (exp & 0xF0).any()
    finally:
        sp.close()


def test_structured_build_keeps_any_edges_and_deblock_bytes():
    """alg_bytes_deblock of a structured build follows derive_edgeFlags' answer (some CTB in a slice with deblocking on):
    nothing to read in a dry build but the kept picture's stats, which equal the unstructured build's here"""
    L = backend.lib()
    for deb in (0, 1):
        sp = pysynth.SynthPicture(pysynth.default_config(416, 240, 8, 0, seed=9400 + deb, deblocking=deb))
        try:
            structure = sp.structure()
            noedge = structure[3]
            flags_plain = helper_edges(sp.d, structure, noedge)
            d_plain = with_flags(sp.d, flags_plain)
            flags_in = garbage_high_nibble(noedge, 5)
            d_struct = with_flags(sp.d, flags_in)
            stats = []
            for desc, st in ((d_plain, None), (d_struct, structure)):
                pic = C.c_void_p()
                cs, keep = backend.cu_structure(structure) if st is not None else (None, None)
                assert L.de265hip_debug_build_host_only_structured(C.byref(desc), C.byref(cs) if cs is not None else None, 1, 0,
                                                                   C.byref(pic)) == 0
                s = _abi.PictureStats()
                assert L.de265hip_picture_get_stats(pic, C.byref(s)) == 0
                stats.append(s.alg_bytes_deblock)
                L.de265hip_picture_free(pic)
            assert stats[0] == stats[1]
            assert (stats[1] > 0) == bool(deb)
        finally:
            sp.close()


# ------------------------------------------------------------------ the body == libde265
@pytest.mark.parametrize("fx", FIXTURES, ids=[os.path.basename(f)[7:-4] for f in FIXTURES])
def test_structured_build_derives_the_edges_libde265_derived(fx):
    for n, (rp, _) in enumerate(f1_stream.load_fixture(fx)):
        cb_log2, cb_part, tu_split, noedge = rp.structure()
        d = rp.to_desc()
        flags_in = garbage_high_nibble(noedge, n)
        rc, got, _ = dry_build(with_flags(d, flags_in), (cb_log2, cb_part, tu_split))
        assert rc == 0
        assert np.array_equal(got, noedge | rp.a["edges"]), "picture %d: %d units differ" % (n, int((got != (noedge | rp.a["edges"])).sum()))


@pytest.mark.parametrize("case", ref_cases.PICTURE_CASES, ids=[c["name"] for c in ref_cases.PICTURE_CASES])
def test_structured_build_matches_reference_edge_digest(case):
    """tests/golden/ref_pictures.json: the edge_flags digest the compiled reference's derive_edgeFlags produced"""
    sp, _, _ = ref_cases.make_picture(case)
    try:
        structure = sp.structure()
        flags_in = garbage_high_nibble(structure[3], 3)
        rc, got, _ = dry_build(with_flags(sp.d, flags_in), structure)
        assert rc == 0
        assert ref_cases.digest([got]) == GOLD_P[case["name"]]["edge_flags"]
    finally:
        sp.close()


# ------------------------------------------------------------------ validation and garbage
def _small():
    sp = pysynth.SynthPicture(pysynth.default_config(328, 184, 8, 0, seed=9500, log2_ctb_size=5, n_slices=2, amp=1))
    cb_log2, cb_part, tu_split, noedge = sp.structure()
    return sp, [cb_log2.copy(), cb_part.copy(), tu_split.copy()], noedge


def test_validation_refuses_what_the_body_cannot_use():
    L = backend.lib()
    sp, st, noedge = _small()
    try:
        d = sp.d
        assert dry_build(d, st)[0] == 0
        for k in range(3):                                          # a NULL plane
            cs, keep = backend.cu_structure(st)
            setattr(cs, _abi.CuStructure._fields_[k][0], None)
            pic = C.c_void_p()
            assert L.de265hip_debug_build_host_only_structured(C.byref(d), C.byref(cs), 1, 0, C.byref(pic)) == _abi.ERROR_PARAMETER_OUT_OF_RANGE
        for bad in (1, 2, 6, 7, 255):                               # log2 CB sizes outside {0} and [3, 5]
            s2 = [a.copy() for a in st]
            s2[0][17] = bad
            assert dry_build(d, s2)[0] == _abi.ERROR_PARAMETER_OUT_OF_RANGE, bad
        for bad in (8, 9, 255):                                     # part modes above 7
            s2 = [a.copy() for a in st]
            s2[1][s2[1].size - 1] = bad
            assert dry_build(d, s2)[0] == _abi.ERROR_PARAMETER_OUT_OF_RANGE, bad
        d2 = _abi.PictureDesc.from_buffer_copy(d)                   # log2_min_cb_size the body cannot index with
        for lmin in (2, 6):
            d2.params.log2_min_cb_size = lmin
            assert dry_build(d2, st)[0] == _abi.ERROR_PARAMETER_OUT_OF_RANGE, lmin
        # the public entry points: no structure, no structured build (and no decoder needed to say so)
        h = C.c_void_p()
        assert L.de265hip_picture_build_structured(None, 0, C.byref(d), None, C.byref(h)) == _abi.ERROR_PARAMETER_OUT_OF_RANGE
        assert L.de265hip_picture_build_host_structured(None, 0, C.byref(d), None, C.byref(h)) == _abi.ERROR_PARAMETER_OUT_OF_RANGE
        rec = backend.Recorder(d.params)
        assert L.de265hip_record_structure(rec._h, None, st[1].ctypes.data, st[2].ctypes.data) == _abi.ERROR_PARAMETER_OUT_OF_RANGE
        rec.record_structure(*st)
        rec.free()
    finally:
        sp.close()


@pytest.mark.parametrize("seed", range(6))
def test_garbage_structure_stays_inside_the_plane(seed):
    """valid-looking values in wrong places (a quadtree that does not tile) and random split bits: the build succeeds, the
    body terminates, and nothing but the edge bits of blk_flags differs from a build with the true structure"""
    sp, st, noedge = _small()
    rng = np.random.default_rng(seed)
    try:
        d = sp.d
        rc, good, (arena_g, o_flags, o_job) = dry_build(d, st)
        assert rc == 0
        g = [a.copy() for a in st]
        if seed % 2:
            g[0][:] = rng.choice(np.array([0, 3, 4, 5], np.uint8), g[0].size)
        g[1][:] = rng.integers(0, 8, g[1].size, dtype=np.uint8)
        g[2][:] = rng.integers(0, 256, g[2].size, dtype=np.uint8)
        rc, bad, (arena_b, o_flags_b, o_job_b) = dry_build(d, g)
        assert rc == 0 and (o_flags_b, o_job_b) == (o_flags, o_job) and arena_b.size == arena_g.size
        assert np.array_equal(bad & 0x0F, good & 0x0F)
        # the structure planes lie between blk_flags and the EdgeJob: their offset from the job's pointers (cb_log2 first, flags
        # seventh); everything else of the arena is the same in both builds
        ptrs = arena_g[o_job:o_job + 56].view(np.uint64)
        o_struct = o_flags + int(ptrs[0]) - int(ptrs[6])
        assert o_flags < o_struct < o_job
        mask = np.ones(arena_g.size, bool)
        mask[o_flags:o_flags + good.size] = False
        mask[o_struct:] = False
        assert np.array_equal(arena_b[mask], arena_g[mask])
    finally:
        sp.close()


# ------------------------------------------------------------------ no change for existing hosts
# de265hip_debug_last_build_hash of UNSTRUCTURED builds (host scan: everything the device would receive), as the parent commit
# of the structured builds computed them (tools/exp/build_hash.py is the long form of this net)
HASH_CASES = [
    (416, 240, 8, 0, 7101, dict(log2_ctb_size=4, n_slices=3, lf_across_slices_pct=50)),
    (416, 240, 10, 1, 7102, dict(log2_ctb_size=5, tile_cols=2, tile_rows=2, lf_across_tiles=0)),
    (416, 240, 8, 2, 7103, dict(log2_ctb_size=6, amp=1)),
    (360, 200, 8, 0, 7104, dict(log2_ctb_size=5, deblocking=0)),
    (328, 184, 10, 2, 7105, dict(log2_ctb_size=4, n_slices=2, tile_cols=3, lf_across_tiles=0, amp=1)),
    (832, 480, 8, 0, 7106, dict(n_slices=4, lf_across_slices_pct=30, amp=1)),
    (1920, 1080, 10, 2, 7107, {}),
    (1920, 1080, 8, 0, 7108, dict(weighted_pred=1, amp=1)),
]
HASHES = ['0:198f3bca486e0389', '0:052840aea5d9d106', '0:531dc89603c74d40', '0:3b7314c6c4a48b14',
          '0:dd7c540ff94d3991', '0:666a21d199c6df76', '0:9c9b1b8c3e699078', '0:0bd21d0284158dd7']


def test_unstructured_builds_are_byte_identical_to_before():
    L = backend.lib()
    got = []
    for (w, h, bd, st, seed, over) in HASH_CASES:
        sp = pysynth.SynthPicture(pysynth.default_config(w, h, bd, st, seed=seed, **over))
        rc = L.de265hip_debug_build_host_only(sp.desc, 1)
        got.append("%d:%016x" % (rc, L.de265hip_debug_last_build_hash()))
        sp.close()
    assert got == HASHES
    # and the structured entry point without a structure is the unstructured build
    sp = pysynth.SynthPicture(pysynth.default_config(*HASH_CASES[0][:4], seed=HASH_CASES[0][4], **HASH_CASES[0][5]))
    try:
        pic = C.c_void_p()
        assert L.de265hip_debug_build_host_only_structured(sp.desc, None, 1, 0, C.byref(pic)) == 0
        L.de265hip_picture_free(pic)
        assert "0:%016x" % L.de265hip_debug_last_build_hash() == HASHES[0]
    finally:
        sp.close()
