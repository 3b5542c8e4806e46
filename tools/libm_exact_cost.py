"""The price of option "libm_exact" (libm class): the crowd scenes of tests/_param_scenes.py -- 80 automated
biquads of all types, 80 automated panners -- lengthened to 2,000 blocks with their ramps stretched over the whole render, so that
most voices recompute their coefficients at (nearly) every sample from the first block to the last.  Each leg is a fresh context
that renders the scene in one call with option "profile" on; the figure is ga_stats.other_ms_total (the stage both kernels are
accounted under: it also holds the scene's source, mix and parameter-curve kernels, which are the same on both legs).  One warm-up
render per option, then five renders per option, alternating; the median is printed.

    python tools/libm_exact_cost.py [--blocks 2000] [--repeats 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from graphaudio_amd import ChannelMergerNode, GainNode, OfflineAudioContext   # noqa: E402
from tests import _graphs as G   # noqa: E402
from tests import _param_scenes as P   # noqa: E402

B, SR = P.B, P.SR


def bq_crowd(ctx, blocks):
    end = blocks * B / SR
    mg = ChannelMergerNode(ctx, 32)
    hold = [mg]
    for v in range(80):
        s = P.noise(ctx, 1, blocks, seed=100 + v)
        f = q = None
        if v % 3 == 0:     # steps: one update per block
            f = P.ftl().set(200.0 + 37.0 * v, 0.0).set(1000.0, end / 3).set(150.0 + 11 * v, 2 * end / 3)
        elif v % 3 == 1:   # a slow frequency ramp: an update every few samples
            f = P.ramp_f_timeline(300.0 + 50.0 * v, 0.0004 * (1 + v % 4), blocks)
        else:              # a Q ramp: an update at every sample
            q = P.qtl().set(0.5 + 0.05 * v, 0.0).lin(4.0, end)
        bq = P.biquad(ctx, P.CROWD_TYPES[v % 8], s, f=f, q=q, fv=None if f else 900.0 + 13 * v, gv=float(v % 13 - 6))
        bq.Inputs[0].SetChannelCount(1)
        bq.Connect(mg, 0, v % 32)
        hold += [s, bq]
    mg.Connect(ctx.Destination)
    return hold, 32


def pan_crowd(ctx, blocks):
    end = blocks * B / SR
    hold = []
    for v in range(80):
        s = P.noise(ctx, 1 + v % 2, blocks, seed=300 + v)
        tl = P.ptl().set(-1.0 + v / 40.0, 0.0)
        if v % 3:          # a ramp over the whole render: new gains at every sample
            tl.lin(1.0 - v / 40.0 + 0.01, end)
        else:              # two steps
            tl.set(0.9 - v / 50.0, end / 3).set(-0.3 + v / 200.0, 2 * end / 3)
        p = P.panner(ctx, s, tl, mono=v % 4 == 0)
        g = GainNode(ctx)
        g.Gain.Value = 0.125
        p.Connect(g).Connect(ctx.Destination)
        hold += [s, p, g]
    return hold, 2


def leg(build, blocks, exact):
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("profile", 1)
    ctx.SetOption("libm_exact", exact)
    hold, ch = build(ctx, blocks)
    ctx.Destination.SetChannelCount(ch)
    out = np.zeros((ch, blocks * B), np.float32)
    t0 = time.perf_counter()
    ctx.Render(out, blocks * B)
    wall = (time.perf_counter() - t0) * 1e3
    other = ctx.GetStats()["other_ms_total"]
    del hold
    ctx.Dispose()
    return other, wall, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for name, build in (("bq_crowd", bq_crowd), ("pan_crowd", pan_crowd)):
        outs = {}
        for exact in (0, 1):   # warm-up: code objects, first touch of the pools
            outs[exact] = leg(build, a.blocks, exact)[2]
        ms = {0: [], 1: []}
        walls = {0: [], 1: []}
        for _ in range(a.repeats):
            for exact in (0, 1):
                o, w, _ = leg(build, a.blocks, exact)
                ms[exact].append(o)
                walls[exact].append(w)
        differ = int((outs[0] != outs[1]).sum())
        print(f"{name}: {a.blocks} blocks, rms {G.rms(outs[0]):.3e}, {differ} of {outs[0].size} values differ between the options")
        for exact in (0, 1):
            print(f"  libm_exact = {exact}: other_ms_total median {statistics.median(ms[exact]):.3f} ms (min {min(ms[exact]):.3f}, max {max(ms[exact]):.3f}); "
                  f"render call median {statistics.median(walls[exact]):.1f} ms")
