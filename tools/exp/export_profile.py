"""k_export alone, for rocprofv3 --kernel-trace --stats: one 4K Main10 4:2:0 picture (random samples) exported 50 times as
NATIVE planar and 50 times as F16 planar into preallocated torch tensors.

    rocprofv3 --kernel-trace --stats -d OUT -o export -- python tools/exp/export_profile.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libde265_hip.so: tests/conftest.py)

from libde265_amd import backend  # noqa: E402

W, H, BD = 3840, 2160, 10
rng = np.random.default_rng(1)
dec = backend.Decoder(device=0)
dec.dpb_alloc(0, W, H, BD)
dec.upload(0, [rng.integers(0, 1 << BD, size=s).astype(np.uint16) for s in [(H, W), (H // 2, W // 2), (H // 2, W // 2)]])
for dtype in ("native", "f16"):
    spec = dec.export_spec(0, dtype=dtype)
    for _ in range(50):
        dec.export(0, dtype=dtype, out=spec.tensors)
    torch.cuda.synchronize()
dec.close()
print("export_profile done")
