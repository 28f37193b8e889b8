"""The export of decoded pictures into device buffers (de265hip_dpb_export_async, Decoder.export, the pipeline's export) on the
GPU: bit for bit against the numpy restatement (tools/export_ref.py) of what de265hip_dpb_download hands out, against
libde265's decoded pictures, and ordered on the device without host waits."""
import glob
import hashlib
import os

import numpy as np
import pytest
import torch

import export_ref
import f1_stream
from libde265_amd import farm
import pyoracle
import pysynth
from libde265_amd import _abi, backend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stream_*.npz")))
TDT = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.float32): torch.float32,
       np.dtype(np.float16): torch.float16}


def host(t):
    return np.ascontiguousarray(t.cpu().numpy())


def random_planes(rng, w, h, bds, cf):
    sw, sh = export_ref.sub_wh(cf)
    cw, ch = (0, 0) if cf == 0 else (w // sw, h // sh)
    out = []
    for c, (pw, ph) in enumerate([(w, h), (cw, ch), (cw, ch)]):
        bd = bds[0] if c == 0 else bds[1]
        out.append(rng.integers(0, 1 << bd, size=(ph, pw)).astype(np.uint8 if bd <= 8 else np.uint16))
    return out


def padded_out(shapes_dtypes, pad, offset):
    """tensors of these shapes whose rows are `pad` elements longer (pitch not a multiple of 16 bytes) and whose storage starts
    `offset` elements into an allocation"""
    out = []
    for sh, dt in shapes_dtypes:
        row = int(np.prod(sh[1:])) + pad
        buf = torch.zeros(offset + sh[0] * row, dtype=dt, device="cuda")
        v = buf[offset:].view(sh[0], row)[:, :int(np.prod(sh[1:]))]
        out.append(v.view(sh) if len(sh) == 2 else v.unflatten(1, sh[1:]))
    return out


def assert_same(got, exp, what):
    assert len(got) == len(exp), what
    for c, (g, e) in enumerate(zip(got, exp)):
        g = host(g)
        assert g.dtype == e.dtype and g.shape == e.shape, (what, c, g.dtype, e.dtype, g.shape, e.shape)
        assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(e).view(np.uint8)), (what, c)


@pytest.mark.parametrize("cf", [0, 1, 2, 3])
def test_export_matrix_equals_the_restatement(cf):
    rng = np.random.default_rng(100 + cf)
    w, h = 72, 40
    sw, sh = export_ref.sub_wh(cf)
    crops = [(0, 0, 0, 0), (0, 2 * sw, 0, 4 * sh), (2 * sw, 4 * sw, 2 * sh, 2 * sh)]
    dec = backend.Decoder()
    try:
        for bds in [(8, 8), (10, 10), (12, 12), (10, 12)]:
            dec.dpb_alloc(3, w, h, bds[0], bds[1], chroma_format=cf)
            planes = random_planes(rng, w, h, bds, cf)
            dec.upload(3, planes)
            for layout in export_ref.LAYOUTS:
                if layout == "semiplanar" and cf == 0:
                    continue
                for fmt in export_ref.FORMATS:
                    for crop in crops:
                        exp = export_ref.restate(planes, bds, cf, layout, fmt, crop)
                        what = (cf, bds, layout, fmt, crop)
                        assert_same(dec.export(3, layout, fmt, crop), exp, what + ("tight",))
                        sd = [(e.shape, TDT[e.dtype]) for e in exp]
                        for pad, offset in ((3, 0), (5, 1)):
                            out = padded_out(sd, pad, offset)
                            res = dec.export(3, layout, fmt, crop, out=out)
                            assert all(a is b for a, b in zip(res, out))
                            assert_same(res, exp, what + (pad, offset))
    finally:
        dec.close()


def test_exhaustive_f32_f16():
    dec = backend.Decoder()
    try:
        for bd in range(8, 13):
            w, h = 64, 64                                          # 4096 samples: every value of 12 bits, the others repeated
            v = (np.arange(w * h) % (1 << bd)).astype(np.uint8 if bd <= 8 else np.uint16).reshape(h, w)
            dec.dpb_alloc(0, w, h, bd, bd, chroma_format=3)
            dec.upload(0, [v, v[:, ::-1].copy(), v[::-1].copy()])
            f32 = [host(t) for t in dec.export(0, dtype="f32")]
            f16 = [host(t) for t in dec.export(0, dtype="f16")]
            for c, p in enumerate([v, v[:, ::-1], v[::-1]]):
                e32 = p.astype(np.float32) / np.float32(2 ** bd - 1)
                assert np.array_equal(f32[c].view(np.uint32), e32.view(np.uint32)), (bd, c)
                assert np.array_equal(f16[c].view(np.uint16), e32.astype(np.float16).view(np.uint16)), (bd, c)
    finally:
        dec.close()


def md5(planes):
    m = hashlib.md5()
    for p in planes:
        m.update(np.ascontiguousarray(p).tobytes())
    return m.hexdigest()


@pytest.mark.parametrize("fx", FIXTURES, ids=[os.path.basename(f)[7:-4] for f in FIXTURES])
def test_decoded_pictures_export_as_libde265_decodes_them(fx):
    dec = backend.Decoder()
    try:
        for i, (rp, dg) in enumerate(f1_stream.load_fixture(fx)):
            P = rp.params
            sf = rp.a["scaling"] if rp.a["scaling"].size else None
            rec = backend.Recorder(P, sf)
            rec.record_desc(rp.to_desc())
            slot, cf = rp.meta["dst_slot"], P.chroma_format_idc
            dec.dpb_alloc(slot, P.width, P.height, P.bit_depth_luma, P.bit_depth_chroma, chroma_format=cf)
            pic = rec.submit(dec, slot)
            try:
                dec.upload(slot, pyoracle.alloc_planes(P.width, P.height, P.bit_depth_luma, chroma_format=cf))
                dec.run(pic, _abi.STAGE_FINAL)
                got = dec.export(slot)                               # no sync: the export follows the picture on the device
                torch.cuda.current_stream().synchronize()
                planes = [host(t) for t in got]
                if cf == 0:
                    planes += [np.zeros((0, 0), planes[0].dtype)] * 2
                assert md5(planes) == dg["final"], "%s picture %d" % (os.path.basename(fx), i)
                if cf:
                    bds = (P.bit_depth_luma, P.bit_depth_chroma)
                    assert_same(dec.export(slot, "semiplanar"), export_ref.restate(planes, bds, cf, "semiplanar"), (fx, i))
            finally:
                pic.free()
                rec.free()
    finally:
        dec.close()


def test_8bit_conformance_window_follows_pixels_confwin():
    """1920x1088 8-bit, conf_win_bottom_offset 4 (crop_bottom 8): libde265 hands out width_confwin x height_confwin samples from
    pixels_confwin = pixels + crop_left + crop_top * stride (image.cc:324-387), chroma with / SubWidthC, / SubHeightC"""
    rng = np.random.default_rng(7)
    w, h = 1920, 1088
    planes = random_planes(rng, w, h, (8, 8), 1)
    dec = backend.Decoder()
    try:
        dec.dpb_alloc(0, w, h, 8)
        dec.upload(0, planes)
        got = [host(t) for t in dec.export(0, crop=(0, 0, 0, 8))]
        for c, p in enumerate(planes):
            flat = p.ravel()
            stride, wc = p.shape[1], p.shape[1]
            hc = (h - 8) // (2 if c else 1)
            exp = np.stack([flat[0 + y * stride: 0 + y * stride + wc] for y in range(hc)])
            assert np.array_equal(got[c], exp), c
        assert got[0].shape == (1080, 1920) and got[1].shape == (540, 960)
    finally:
        dec.close()


def synth_gop(w, h, bd, n, seed):
    return [pysynth.SynthPicture(pysynth.default_config(w, h, bd, st, seed=seed + k, **(dict(ref_slots=refs) if refs else {})))
            for k, (st, refs) in enumerate(farm.gop_plan(n))]


def b_picture_into(dec, slot, w, h, bd, seed):
    """builds and runs (no wait) a B picture into `slot` that predicts from slots 0 and 1"""
    sp = pysynth.SynthPicture(pysynth.default_config(w, h, bd, 0, seed=seed, ref_slots=[0, 1]))
    pic = dec.build(slot, sp.desc)
    dec.run(pic, _abi.STAGE_FINAL)
    return pic, sp


@pytest.mark.parametrize("mode", ["one_lane", "two_lanes", "realloc"])
def test_the_slots_next_writer_waits_for_the_export(mode):
    w, h, bd, s = 352, 288, 10, 2
    dec = backend.Decoder()
    try:
        if mode == "two_lanes":
            dec.set_lanes(2)
        for k in range(3):
            dec.dpb_alloc(k, w, h, bd)
            dec.upload(k, pysynth.fill_planes(w, h, bd, 10 + k))
        a = pysynth.fill_planes(w, h, bd, 12)
        if mode == "two_lanes":                     # picture A itself decoded on a lane, then exported from its writer's stream
            pa, _ = b_picture_into(dec, s, w, h, bd, 77)
            dec.sync()
            a = dec.download(s, w, h, bd)
            pa.free()
        exp = dec.export(s)
        if mode == "realloc":
            dec.dpb_alloc(s, w + 64, h, bd)         # re-allocation of the slot right behind the export
        else:
            pb, _ = b_picture_into(dec, s, w, h, bd, 99)
        dec.wait_export(s, exp.export_id)
        assert_same(exp, a, mode)
        if mode != "realloc":
            dec.sync()
            assert not np.array_equal(dec.download(s, w, h, bd)[0], a[0])    # (B did overwrite the slot)
            pb.free()
    finally:
        dec.close()


def test_a_writer_on_the_other_lane_waits_for_a_delayed_export():
    """the export of picture A runs on lane 0 (A's writer) behind a slow consumer (AFTER_CONSUMER); picture B into the same slot
    goes to lane 1 (its references were uploaded: no predecessor, lane 1 has had no work).  Only the slot's export event orders B
    behind the export: without it B's kernels overwrite the slot long before the consumer's sleep ends."""
    w, h, bd, s = 352, 288, 10, 2
    dec = backend.Decoder()
    try:
        dec.set_lanes(2)
        for k in range(3):
            dec.dpb_alloc(k, w, h, bd)
            dec.upload(k, pysynth.fill_planes(w, h, bd, 30 + k))
        pa, _ = b_picture_into(dec, s, w, h, bd, 78)
        dec.sync()
        a = dec.download(s, w, h, bd)
        pa.free()
        out = dec.export_spec(s).tensors
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            torch.cuda._sleep(50_000_000)
        exp = dec.export(s, out=out, stream=side, after_consumer=True)
        pb, _ = b_picture_into(dec, s, w, h, bd, 98)
        side.synchronize()
        assert_same(exp, a, "delayed export")
        dec.sync()
        assert not np.array_equal(dec.download(s, w, h, bd)[0], a[0])        # (B did overwrite the slot)
        pb.free()
    finally:
        dec.close()


@pytest.mark.parametrize("consumer", ["current", "side"])
def test_fresh_exports_for_a_slow_consumer_keep_their_pictures(consumer):
    """a consumer loop that drops each picture's tensors while its own read of them is still queued (behind a slow op): the
    allocator hands their blocks to the next export at once, which must not write them before that read.  `side`: the loop runs
    on a stream of its own"""
    w, h, bd, n = 352, 288, 10, 6
    dec = backend.Decoder()
    side = torch.cuda.Stream() if consumer == "side" else torch.cuda.current_stream()
    try:
        pics = []
        for k in range(n):
            dec.dpb_alloc(k, w, h, bd)
            pics.append(pysynth.fill_planes(w, h, bd, 40 + k))
            dec.upload(k, pics[k])
        reads = []
        with torch.cuda.stream(side):
            for k in range(n):
                y = dec.export(k)
                torch.cuda._sleep(20_000_000)                  # the consumer is slower than the decoder
                reads.append([t.clone() for t in y])
                del y
        torch.cuda.synchronize()
        for k in range(n):
            assert_same(reads[k], pics[k], k)
    finally:
        dec.close()


def test_consumer_stream_sees_the_picture_without_host_waits():
    w, h, bd = 352, 288, 10
    dec = backend.Decoder()
    try:
        for k in range(3):
            dec.dpb_alloc(k, w, h, bd)
            dec.upload(k, pysynth.fill_planes(w, h, bd, 20 + k))
        pic, _ = b_picture_into(dec, 2, w, h, bd, 5)
        got = dec.export(2)
        first = [t.to(torch.int32) for t in got]                   # enqueued on the current stream right away
        dec.sync()
        exp = dec.download(2, w, h, bd)
        for c in range(3):
            assert np.array_equal(host(first[c]), exp[c].astype(np.int32)), c
        pic.free()
        side = torch.cuda.Stream()
        got2 = dec.export(2, dtype="f16", stream=side)
        with torch.cuda.stream(side):
            s2 = [t.float().clone() for t in got2]
        side.synchronize()
        for c in range(3):
            assert np.array_equal(host(s2[c]), export_ref.convert(exp[c], bd, "f16").astype(np.float32)), c
    finally:
        dec.close()


def test_after_consumer_ring_over_a_gop():
    w, h, bd, n = 256, 128, 10, 16
    gop = synth_gop(w, h, bd, n, 4242)
    dec = backend.Decoder()
    try:
        for k in range(n):
            dec.dpb_alloc(k, w, h, bd)
        ring = [dec.export_spec(0).tensors for _ in range(2)]
        clones, pics = [], []
        for k, sp in enumerate(gop):
            pic = dec.build(k, sp.desc)
            dec.run(pic, _abi.STAGE_FINAL)
            pics.append(pic)
            got = dec.export(k, out=ring[k % 2], after_consumer=True)
            clones.append([t.clone() for t in got])                  # the next export into this ring entry waits for the clone
        dec.sync()
        torch.cuda.synchronize()
        for k in range(n):
            assert_same(clones[k], dec.download(k, w, h, bd), k)
        for p in pics:
            p.free()
    finally:
        dec.close()


def test_pipeline_exports_to_a_torch_stream():
    w, h, bd, n = 256, 128, 10, 16
    gop = synth_gop(w, h, bd, n, 777)
    dec = backend.Decoder()
    pipe = backend.Pipeline(dec, 2)
    try:
        for k in range(n):
            dec.dpb_alloc(k, w, h, bd)
        specs = [backend.ExportSpec(w, h, bd, bd, 1, dtype=("native" if k % 2 else "f16"), device="cuda") for k in range(n)]
        tickets = [pipe.submit_desc(k, gop[k].desc, export=specs[k]) for k in range(n)]
        clones = []
        for k, t in enumerate(tickets):
            clones.append([x.clone() for x in pipe.export_to_stream(t)])
        for t in tickets:
            pipe.wait(t)                                            # raises unless de265hip_pipeline_wait returns 0
        pipe.drain()
        torch.cuda.synchronize()
        for k in range(n):
            ref = dec.download(k, w, h, bd)
            exp = ref if k % 2 else [export_ref.convert(p, bd, "f16") for p in ref]
            assert_same(clones[k], exp, k)
    finally:
        pipe.close()
        dec.close()


def test_device_entry_point_refusals_enqueue_nothing():
    import ctypes as C
    L = backend.lib()
    E = _abi.ERROR_PARAMETER_OUT_OF_RANGE
    w, h = 64, 32
    dec = backend.Decoder()
    try:
        dec.dpb_alloc(0, w, h, 10)
        dec.upload(0, pysynth.fill_planes(w, h, 10, 1))
        good = dec.export_spec(0)
        before = [t.clone() for t in good.tensors]
        eid = C.c_uint64(123)

        def call(d, slot=0, stream=None):
            return L.de265hip_dpb_export_async(dec._h, slot, C.byref(d), stream, C.byref(eid))

        for slot in (1, -1, _abi.MAX_DPB_SLOTS):
            assert call(good.desc, slot) == E and eid.value == 0
        bad = []
        for field, val in (("layout", 5), ("format", 9), ("crop_left", 1), ("crop_top", 32), ("flags", 4)):
            d = _abi.ExportDesc.from_buffer_copy(good.desc)
            setattr(d, field, val)
            bad.append(d)
        d = _abi.ExportDesc.from_buffer_copy(good.desc); d.pitch_bytes[0] = 2 * w - 2; bad.append(d)
        d = _abi.ExportDesc.from_buffer_copy(good.desc); d.pitch_bytes[1] = w + 1; bad.append(d)
        d = _abi.ExportDesc.from_buffer_copy(good.desc); d.dst[2] = None; bad.append(d)
        d = _abi.ExportDesc.from_buffer_copy(good.desc); d.dst[1] = good.desc.dst[1] + 1; bad.append(d)    # (misaligned uint16)
        d = _abi.ExportDesc.from_buffer_copy(good.desc)
        for c in range(3):
            d.dst[c] = None
        bad.append(d)
        d = _abi.ExportDesc.from_buffer_copy(good.desc); d.flags = _abi.EXPORT_AFTER_CONSUMER; bad.append(d)   # (no consumer)
        for d in bad:
            eid.value = 123
            assert call(d) == E and eid.value == 0
        assert L.de265hip_dpb_wait_export(dec._h, 1, 1) == E and L.de265hip_dpb_wait_export(dec._h, 0, 0) == E
        dec.sync()
        torch.cuda.synchronize()
        for a, b in zip(before, good.tensors):
            assert np.array_equal(host(a), host(b))                 # nothing was written
        assert call(good.desc) == 0 and eid.value == 1
        dec.wait_export(0, 1)
    finally:
        dec.close()
