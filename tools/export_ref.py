"""numpy restatement of the export of a decoded picture (de265hip_dpb_export_async, include/de265_hip.h "export"):
what k_export writes, from the planes de265hip_dpb_download hands out."""
import numpy as np

LAYOUTS = ("planar", "semiplanar")
FORMATS = ("native", "msb16", "f32", "f16")


def sub_wh(chroma_format):
    """(SubWidthC, SubHeightC) of table 6-1; monochrome 1, 1"""
    return {0: (1, 1), 1: (2, 2), 2: (2, 1), 3: (1, 1)}[chroma_format]


def convert(v, bd, fmt):
    """one component's samples (uint8 / uint16 array of bit depth bd) in a sample format"""
    if fmt == "native":
        return v.astype(np.uint8 if bd <= 8 else np.uint16)
    if fmt == "msb16":
        return (v.astype(np.uint32) << (16 - bd)).astype(np.uint16)
    f = v.astype(np.float32) / np.float32((1 << bd) - 1)          # float32 division: correctly rounded
    return f if fmt == "f32" else f.astype(np.float16)             # round to nearest-even


def restate(planes, bit_depths, chroma_format, layout="planar", fmt="native", crop=(0, 0, 0, 0)):
    """planes: [Y, Cb, Cr] as downloaded; bit_depths: (luma, chroma); crop: (left, right, top, bottom) in luma samples, offset
    by samples at every bit depth.  Planar: [Y, Cb, Cr] (monochrome: [Y]); semi-planar: [Y, CbCr (ch, cw, 2)], Cb first."""
    l, r, t, b = crop
    sw, sh = sub_wh(chroma_format)
    h, w = planes[0].shape
    out = [convert(planes[0][t:h - b, l:w - r], bit_depths[0], fmt)]
    if chroma_format == 0:
        return out
    ch, cw = planes[1].shape
    win = [convert(p[t // sh:ch - b // sh, l // sw:cw - r // sw], bit_depths[1], fmt) for p in planes[1:3]]
    if layout == "planar":
        return out + win
    return out + [np.stack(win, axis=-1)]
