"""SpatialPannerNode: the public surface (Python host, C header, C# binding) and the geometry of the float64 model the GPU tests
compare against (tests/_spatial_model.py).  No GPU needed."""
import os
import re

import numpy as np

from tests import _spatial_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMAX = float(np.finfo(np.float32).max)

# GraphAudio.SteamAudio/Nodes/SpatialPannerNode.cs:94-110, transcribed: (name, default, min, max), all k-rate
REFERENCE_PARAMS = [
    ("positionX", 0.0, -FMAX, FMAX), ("positionY", 0.0, -FMAX, FMAX), ("positionZ", 0.0, -FMAX, FMAX),
    ("orientationX", 1.0, -1.0, 1.0), ("orientationY", 0.0, -1.0, 1.0), ("orientationZ", 0.0, -1.0, 1.0),
    ("refDistance", 1.0, 0.0, FMAX), ("maxDistance", 10000.0, 0.0, FMAX), ("rolloffFactor", 1.0, 0.0, FMAX),
    ("coneInnerAngle", 360.0, 0.0, 360.0), ("coneOuterAngle", 360.0, 0.0, 360.0), ("coneOuterGain", 0.0, 0.0, 1.0),
    ("spatialBlend", 1.0, 0.0, 1.0), ("occlusion", 0.0, 0.0, 1.0),
    ("transmissionLow", 0.0, 0.0, 1.0), ("transmissionMid", 0.0, 0.0, 1.0), ("transmissionHigh", 0.0, 0.0, 1.0),
]


def test_python_surface_matches_the_reference():
    from graphaudio_amd import DistanceModelType, SpatialPannerNode
    assert [tuple(p) for p in SpatialPannerNode.PARAMS] == REFERENCE_PARAMS
    assert [m.name for m in DistanceModelType] == ["Linear", "Inverse", "Exponential"]   # SpatialPannerNode.cs:42-47
    assert [int(m) for m in DistanceModelType] == [0, 1, 2]
    for prop in ("DistanceModel", "Hrir", "HrirAzimuths"):
        assert isinstance(getattr(SpatialPannerNode, prop), property)
    from graphaudio_amd import OfflineAudioContext
    for method in ("SetListener", "SetListenerTransform", "SetHrir"):
        assert callable(getattr(OfflineAudioContext, method))


def test_header_and_csharp_binding_carry_the_node_type():
    hdr = open(os.path.join(ROOT, "include", "graphaudio_hip.h")).read()
    m = re.search(r"GA_NODE_SPATIAL_PANNER\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 12
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GraphAudioHip.cs")).read()
    m = re.search(r"NodeSpatialPanner\s*=\s*(\d+)", cs)
    assert m and int(m.group(1)) == 12
    from graphaudio_amd import SpatialPannerNode, _capi
    assert SpatialPannerNode._node_type == _capi.NODE_SPATIAL_PANNER == 12
    wrapper = open(os.path.join(ROOT, "bindings", "csharp", "HipOfflineAudioContext.cs")).read()
    assert "class SpatialPannerNode" in wrapper


def test_model_source_on_the_right_is_azimuth_plus_90():
    direction, g = M.geometry(dict(positionX=1.0))
    az, el = M.azimuth_elevation(direction)
    assert az == 90.0 and el == 0.0
    assert g == np.float32(1.0)   # inverse model at the reference distance


def test_model_grid_point_has_unit_weight():
    A, E = 24, 7
    for i, j in [(0, 3), (5, 3), (23, 1), (7, 5), (12, 2)]:
        az, el = np.radians(360.0 * i / A), np.radians(-90.0 + 180.0 * j / (E - 1))
        # (float32 directions: the weight of the grid point is 1 to rounding; the exact cases follow)
        direction = (np.float32(np.sin(az) * np.cos(el)), np.float32(np.sin(el)), np.float32(-np.cos(az) * np.cos(el)))
        idx, w = M.select(direction, A, E)
        k = int(np.argmax(w))
        assert abs(float(w[k]) - 1.0) < 1e-5 and idx[k] == j * A + i
    idx, w = M.select((np.float32(1), np.float32(0), np.float32(0)), 4, 1)   # +x with A = 4: exactly direction 1
    assert idx[0] == 1 and tuple(w) == (1.0, 0.0, 0.0, 0.0)
    idx, w = M.select((np.float32(0), np.float32(0), np.float32(-1)), 24, 7)   # front, horizontal ring j = 3
    assert idx[0] == 3 * 24 and tuple(w) == (1.0, 0.0, 0.0, 0.0)


def test_model_azimuth_seam_wraps():
    az = np.radians(352.5)
    idx, w = M.select((np.float32(np.sin(az)), np.float32(0), np.float32(-np.cos(az))), 24, 1)
    assert idx[0] == 23 and idx[1] == 0
    assert abs(float(w[0]) - 0.5) < 1e-5 and abs(float(w[1]) - 0.5) < 1e-5


def test_model_poles_are_well_defined():
    for y, ring in [(1.0, 6), (-1.0, 0)]:
        idx, w = M.select((np.float32(0), np.float32(y), np.float32(0)), 24, 7)
        assert all(np.isfinite(float(v)) for v in w)
        assert abs(sum(float(v) for v in w) - 1.0) < 1e-6
        assert all(i // 24 == ring for i, v in zip(idx, w) if v > 0)
    direction, g = M.geometry(dict(positionY=5.0))
    assert direction == (0.0, 1.0, 0.0) and abs(float(g) - 0.2) < 1e-7
    direction, g = M.geometry({})   # source on the listener: the (0, 0, -1) fallback, distance 0
    assert direction == (0.0, 0.0, -1.0) and g == np.float32(1.0)


def test_model_listener_from_matches_the_reference_convention():
    lst = M.listener_from((1.0, 2.0, 3.0), (0.0, 0.0, -2.0), (0.0, 3.0, 0.0))
    assert lst[0] == (1.0, 2.0, 3.0)
    assert lst[1] == (1.0, 0.0, 0.0)      # right = forward x up
    assert lst[2] == (0.0, 1.0, 0.0)
    assert lst[3] == (0.0, 0.0, 1.0)      # ahead = -forward (SteamAudioContext.cs:161)
