"""Option "conv_migrate" (DESIGN.md 2b), the parts that need no GPU: the surface, the index arithmetic of the rebuild kernel and the
set builder it shares with the private-IR convolver stage (a stand-alone program under the address and undefined-behaviour
sanitizers), and -- on the oracle -- that every edit session of
tests/_migrate_scenes.py really exercises its sink after the edit.  A scene whose delay time does not move across sample boundaries
would pass on the device whatever formulation the convolver is on."""
import os
import subprocess

import numpy as np
import pytest

from graphaudio_amd import _capi
from tests import _graphs as G
from tests import _migrate_scenes as M
from tests._oracle import OracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_conv_migrations_is_the_last_field_of_the_statistics():
    assert _capi.Stats._fields_[-1][0] == "conv_migrations"
    header = _read("include", "graphaudio_hip.h")
    body = header[header.index("typedef struct ga_stats"):header.index("} ga_stats;")]
    last_decl = [ln for ln in body.splitlines() if ln.strip().startswith(("int64_t", "int32_t", "double", "char"))][-1]
    assert "conv_migrations" in last_decl
    cs = _read("bindings", "csharp", "GraphAudioHip.cs")
    stats = cs[cs.index("public unsafe struct Stats"):]
    stats = stats[:stats.index("}")]
    assert stats.strip().splitlines()[-1].strip() == "public long conv_migrations;"


def test_the_option_is_named_where_a_host_looks_for_it():
    assert '"conv_migrate"' in _read("include", "graphaudio_hip.h")
    cs = _read("bindings", "csharp", "HipOfflineAudioContext.cs")
    assert "public bool ConvMigrate" in cs and '"conv_migrate"' in cs
    assert "conv_migrate" in _read("INTEGRATION.md")
    assert "conv_migrate" in _read("DESIGN.md")


def test_rebuild_index_arithmetic_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "conv_rebuild")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "graphaudio_amd", "csrc"), os.path.join(ROOT, "tests", "conv_rebuild_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok")


@pytest.mark.parametrize("scene", M.ALL_SCENES, ids=lambda s: s.name)
def test_the_oracle_hears_the_scene_after_the_edit(scene):
    o = OracleContext(M.SR)
    out, _, _ = M.run(o, scene)
    o.Dispose()
    assert np.isfinite(out).all()
    assert G.rms(out[:, scene.pre_frames:]) > 1e-4


@pytest.mark.parametrize("scene", M.DELAY_SCENES, ids=lambda s: s.name)
def test_the_depth_signal_moves_the_delay_across_sample_boundaries(scene):
    o = OracleContext(M.SR)
    sig, _, _ = M.run(o, scene, probe=True)
    o.Dispose()
    idx = M.delay_indices(scene, sig)
    print(f"{scene.name}: depth signal rms {G.rms(sig[:, scene.pre_frames:]):.3e}, {len(np.unique(idx))} distinct sample delays "
          f"({idx.min()} .. {idx.max()})")
    assert len(np.unique(idx)) >= 8
