"""Writes tests/golden/spatial_ref_case.bin: one small SpatialPannerNode case rendered by tests/_spatial_model.render, with the
descriptors the model's geometry gives, for tests/spatial_ref_main.cpp (form (a) of tests/spatial_ref.hpp against the model).

Little-endian: int32 magic, T, D, nblocks, stereo; float32 hrir[D][2][T]; float32 x[channels][N]; float32 history[512];
nblocks + 1 descriptors (int32 idx[4], float32 w[4], gb, dry, int32 seg, flags; entry 0 is not used); float64 expected[2][N].
spatialBlend is 1/2 or 1, so gb = g * beta and dry = g * (1 - beta) are exact in float32 and in the model's float64 alike.
Run from the repository root: python tests/golden/make_spatial_ref_case.py"""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import _spatial_model as M   # noqa: E402

T, A, E, NB = 7, 4, 2, 5
D = A * E
rng = np.random.default_rng(20261021)
hrir = rng.uniform(-1, 1, (D, 2, T)).astype(np.float32)
x = rng.uniform(-1, 1, (2, NB * 128)).astype(np.float32)
hist = rng.uniform(-1, 1, 512).astype(np.float32)
silent = [False, False, True, False, False]
params = [dict(positionX=1.0, positionY=0.5, positionZ=-2.0, spatialBlend=0.5),
          dict(positionX=1.5, positionY=0.25, positionZ=-1.0, spatialBlend=1.0),
          dict(positionX=1.5, positionY=0.25, positionZ=-1.0, spatialBlend=1.0),
          dict(positionX=-2.0, positionY=-1.0, positionZ=0.75, spatialBlend=0.5),
          dict(positionX=-2.0, positionY=-1.0, positionZ=0.75, spatialBlend=0.5)]
xs = x.astype(np.float64).copy()
for b, s in enumerate(silent):
    if s:
        xs[:, b * 128:(b + 1) * 128] = 0.0   # (the model mixes what it is given: a silent block's input is zeros)
want = M.render(xs, hrir, A, params, silent=silent, history=hist.astype(np.float64))

out = [struct.pack("<5i", 0x31415053, T, D, NB, 1), hrir.tobytes(), x.tobytes(), hist.tobytes()]
out.append(struct.pack("<4i4f2f2i", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0))
prev = None
for b in range(NB):
    if silent[b]:
        out.append(struct.pack("<4i4f2f2i", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0))
        prev = None
        continue
    direction, g = M.geometry(params[b])
    idx, w = M.select(direction, A, E)
    beta = np.float32(params[b]["spatialBlend"])
    cur = (idx, tuple(float(v) for v in w), float(g), float(beta))
    fade = prev is not None and prev != cur
    gb, dry = np.float32(g * beta), np.float32(g * np.float32(np.float32(1.0) - beta))
    assert float(gb) == float(g) * float(beta) and float(dry) == float(g) * (1.0 - float(beta))
    out.append(struct.pack("<4i4f2f2i", *idx, *[float(v) for v in w], float(gb), float(dry), 0, (1 if fade else 0) | 2))
    prev = cur
out.append(np.ascontiguousarray(want, dtype=np.float64).tobytes())
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spatial_ref_case.bin")
with open(path, "wb") as f:
    f.write(b"".join(out))
print(path, sum(len(o) for o in out), "bytes")
