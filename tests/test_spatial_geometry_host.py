"""The shared SpatialPannerNode geometry (graphaudio_amd/csrc/ga_spatial_geom.hpp) built with a plain host compiler, in both of its
instantiations -- the host's (the C library's float acos / pow) and the device's (rounded once from double) -- against the float32
restatement of tests/_spatial_model.py.

Indices and weights are equal: both sides take atan2 / asin from the same C library in double, from the same float32 direction.
g is within 1e-6 relative, the figure DESIGN.md section 2e states for the host's gain (acos / pow may differ in the last place between
numpy, the C library's float functions and a double rounded once).
"""
import math
import os
import struct
import subprocess

import numpy as np

from tests import _spatial_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphaudio_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "spatial_geometry_main.cpp")
NAMES = ["positionX", "positionY", "positionZ", "orientationX", "orientationY", "orientationZ", "refDistance", "maxDistance",
         "rolloffFactor", "coneInnerAngle", "coneOuterAngle", "coneOuterGain", "spatialBlend"]
f32 = np.float32

CONES = {   # the source-to-listener direction is set against `toward` below
    "off": lambda toward, side: dict(),
    "inside": lambda toward, side: dict(zip(NAMES[3:6], toward), coneInnerAngle=60.0, coneOuterAngle=120.0, coneOuterGain=0.25),
    "between": lambda toward, side: dict(zip(NAMES[3:6], [t + s for t, s in zip(toward, side)]), coneInnerAngle=60.0, coneOuterAngle=120.0, coneOuterGain=0.25),
    "outside": lambda toward, side: dict(zip(NAMES[3:6], [-t for t in toward]), coneInnerAngle=60.0, coneOuterAngle=120.0, coneOuterGain=0.25),
}
GRIDS = [(1, 1), (4, 3), (24, 7)]
LISTENERS = [M.IDENTITY, M.listener_from((0.5, -0.25, 0.125), (1.0, 0.5, 0.0), (0.0, 1.0, 0.0))]


def cases():
    rng = np.random.default_rng(2024)
    out = []
    for model in (M.LINEAR, M.INVERSE, M.EXPONENTIAL):
        for cone in CONES:
            for (A, E) in GRIDS:
                for li, listener in enumerate(LISTENERS):
                    origin = [float(c) for c in listener[0]]
                    i = int(rng.integers(0, A))
                    az = math.radians(360.0 * i / A)
                    r = float(rng.uniform(1.5, 6.0))
                    rel = [
                        (r * math.sin(az), 0.0, -r * math.cos(az)),                       # on a grid azimuth, elevation 0
                        (r * math.sin(az) * 0.8, r * 0.6, -r * math.cos(az) * 0.8),       # on a grid azimuth, raised
                        (0.0, r, 0.0), (0.0, -r, 0.0),                                    # the poles
                        (0.00003, 0.00002, -0.00001),                                     # distance <= 0.0001: straight ahead, distance 0
                        tuple(float(v) for v in rng.uniform(-4.0, 4.0, 3)),
                        tuple(float(v) for v in rng.uniform(-12.0, 12.0, 3)),
                    ]
                    for d in rel:
                        pos = [float(f32(o + c)) for o, c in zip(origin, d)]
                        w = np.array([float(f32(p) - f32(o)) for p, o in zip(pos, origin)])
                        n = np.linalg.norm(w)
                        toward = list(-w / n) if n > 1e-3 else [0.0, 0.0, 1.0]
                        side = np.cross(toward, [0.3, 0.5, 0.8])
                        side = list(side / np.linalg.norm(side))        # unit, perpendicular: toward + side is 45 degrees off
                        p = dict(zip(NAMES[:3], pos), refDistance=float(rng.uniform(0.5, 2.0)), maxDistance=float(rng.uniform(8.0, 20.0)),
                                 rolloffFactor=float(rng.uniform(0.3, 1.5)), spatialBlend=float(rng.uniform(0.0, 1.0)))
                        p.update(CONES[cone](toward, side))
                        p = {k: float(f32(v)) for k, v in p.items()}
                        out.append((model, A, E, listener, p, cone))
    return out


def program_input(cs):
    lines = []
    for model, A, E, listener, p, _ in cs:
        q = dict(M.PARAM_DEFAULTS)
        q.update(p)
        pv = [q[k] for k in NAMES] + [0.0, 1.0, 1.0, 1.0]
        L = [float(c) for v in listener for c in v]
        lines.append(" ".join([str(model), str(A), str(A * E)] + ["%.9g" % v for v in L + pv]))
    return "\n".join(lines) + "\n"


def parse(line):
    t = line.split()
    def one(u):
        unb = lambda h: struct.unpack("<f", struct.pack("<I", int(h, 16)))[0]
        return tuple(int(v) for v in u[:4]), tuple(f32(unb(h)) for h in u[4:8]), f32(unb(u[8])), f32(unb(u[9]))
    return one(t[:10]), one(t[10:20])


def build(tmp_path, extra=()):
    exe = tmp_path / "spatial_geometry"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC, MAIN, "-o", str(exe)])
    return exe


def test_both_instantiations_match_the_model(tmp_path):
    cs = cases()
    assert len(cs) >= 300
    exe = build(tmp_path)
    got = subprocess.run([str(exe)], input=program_input(cs), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(cs)
    worst = 0.0
    seen = set()
    for (model, A, E, listener, p, cone), line in zip(cs, got):
        direction, g = M.geometry(p, model, listener)
        idx, w = M.select(direction, A, E)
        for which, (gi, gw, gg, gbeta) in zip(("libm", "double"), parse(line)):
            what = (which, model, A, E, cone, p)
            assert gi == tuple(idx), what
            assert all(a == b for a, b in zip(gw, w)), what
            assert gbeta == f32(p["spatialBlend"]), what
            assert abs(float(gg) - float(g)) <= 1e-6 * abs(float(g)), (what, float(gg), float(g))
            if g != 0:
                worst = max(worst, abs(float(gg) - float(g)) / abs(float(g)))
        seen.add((model, cone, A))
    print(f"{len(cs)} parameter sets; worst relative difference of g {worst:.3e}")
    assert len(seen) == 3 * 4 * 3          # every distance model x cone case x grid


def test_cone_cases_are_what_they_are_called():
    """the generated orientations land inside, between and outside the cone (so every branch of the directivity is compared)"""
    hits = {}
    for model, A, E, listener, p, cone in cases():
        if cone == "off" or model != M.INVERSE:
            continue
        _, g = M.geometry(p, model, listener)
        _, g0 = M.geometry({k: v for k, v in p.items() if not k.startswith("cone")}, model, listener)
        origin = [float(c) for c in listener[0]]
        if math.dist([p["positionX"], p["positionY"], p["positionZ"]], origin) < 1e-3 or g0 == 0:
            continue
        hits.setdefault(cone, []).append(float(g) / float(g0))
    assert all(abs(r - 1.0) < 1e-6 for r in hits["inside"])
    assert all(abs(r - 0.25) < 1e-6 for r in hits["outside"])
    assert all(0.3 < r < 0.95 for r in hits["between"]), hits["between"]
