"""The price of moving running convolvers to formulation R (option "conv_migrate").

64 voices x 65,536 taps (the size of bench.py's reference-order variant), 10 s in render calls of 1 s; after 2 s a resonant
biquad (peaking, 104 Hz, Q 2.1, +6 dB) is inserted between the bus and the destination, which makes every convolver sensitive.
Prints, per render call, the wall time of the call and the device time of its chunks (option "profile"), for three legs:
conv_migrate = 1 (the call behind the edit holds the migrating chunk), conv_migrate = 0 (the nodes stay on formulation D) and
conv_reference_order = 2 (formulation R from the first block).  With GA_TIMING=1 in the environment the library adds its own
per-chunk host phases on stderr.

    python tools/conv_migrate_scene.py [--voices 64] [--taps 65536] [--seconds 10]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphaudio_amd import (AudioBufferSourceNode, BiQuadFilterNode, ConvolverNode, FilterType, GainNode, OfflineAudioContext,  # noqa: E402
                            PlayableAudioBuffer)
from tests import _graphs as G  # noqa: E402

SR = 48000


def leg(name, voices, taps, seconds, **opts):
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("profile", 1)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    ctx.Destination.SetChannelCount(2)
    ir = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, taps) for c in range(2)], SR)
    bus = GainNode(ctx)
    bus.Gain.Value = 1.0 / 8.0
    frames = SR * seconds
    for v in range(voices):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, frames + 256), SR)
        cv = ConvolverNode(ctx)
        cv.Buffer = ir
        s.Connect(cv).Connect(bus)
        s.Start()
    bus.Connect(ctx.Destination)
    out = np.zeros((2, frames), np.float32)
    rows = []
    dev0 = 0.0
    for call in range(seconds):
        if call == 2:
            bq = BiQuadFilterNode(ctx)
            bq.Type = FilterType.Peaking
            bq.Frequency.Value = 104.0
            bq.Q.Value = 2.1
            bq.Gain.Value = 6.0
            bus.Disconnect()
            bus.Connect(bq).Connect(ctx.Destination)
        t0 = time.perf_counter()
        ctx.Render(out, SR, call * SR)
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx.GetStats()
        rows.append((call, wall, st["device_ms_total"] - dev0, st["conv_migrations"], st["ref_order_rows"]))
        dev0 = st["device_ms_total"]
    ctx.Dispose()
    print(f"-- {name}")
    for call, wall, dev, moved, rrows in rows:
        print(f"   call {call}: wall {wall:8.3f} ms  device {dev:8.3f} ms  moved {moved:3d}  reference-order rows {rrows}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=64)
    ap.add_argument("--taps", type=int, default=65536)
    ap.add_argument("--seconds", type=int, default=10)
    a = ap.parse_args()
    moved = leg("conv_migrate = 1", a.voices, a.taps, a.seconds, conv_migrate=1)
    leg("conv_migrate = 0", a.voices, a.taps, a.seconds, conv_migrate=0)
    twin = leg("conv_reference_order = 2", a.voices, a.taps, a.seconds, conv_reference_order=2)
    post = slice(2 * SR, None)
    print(f"behind the edit, conv_migrate = 1 against R from the start: {int((moved[:, post] != twin[:, post]).sum())} of {moved[:, post].size} values differ")


if __name__ == "__main__":
    main()
