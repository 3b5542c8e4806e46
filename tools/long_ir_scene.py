#!/usr/bin/env python3
"""Long impulse responses on the convolver (tools/long_ir_scene.py --case shared|private|one [--taps N] [--library PATH] [--opts k=v,..]):
what a 10 s step costs when the response is longer than 131,072 taps.  One JSON line per run.

  shared  : 1024 voices -> ConvolverNode (ONE shared stereo response, default 288,000 taps = 6 s) -> destination
  private : 64 voices, each with a stereo response of its own (288,000 taps)
  one     : one voice x a stereo response of 1,048,576 taps

`--taps 65536` builds the same graph on the headline's response (the anchor).  `--library` loads another build of the product
library (the parent commit's, for A/B runs: one process per library, runs interleaved by the caller); `--opts coarse_long=0` is the
same switch inside one build.  `--stages` adds the stage table of the last step (option profile = 1: not for timing)."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=["shared", "private", "one"], default="shared")
ap.add_argument("--taps", type=int, default=0)
ap.add_argument("--voices", type=int, default=0)
ap.add_argument("--library", default="")
ap.add_argument("--opts", default="")
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--stages", action="store_true")
ap.add_argument("--label", default="")
a = ap.parse_args()
from graphaudio_amd import _capi
if a.library:
    _capi.use_library(os.path.abspath(a.library))
from graphaudio_amd import AudioBufferSourceNode, ConvolverNode, OfflineAudioContext, PlayableAudioBuffer
from tests import _graphs as G
SR = 48000
taps = a.taps or (1048576 if a.case == "one" else 288000)
voices = a.voices or {"shared": 1024, "private": 64, "one": 1}[a.case]
frames = 10 * SR // 128 * 128
ctx = OfflineAudioContext(SR)
for kv in a.opts.split(","):
    if "=" in kv: ctx.SetOption(kv.split("=")[0], float(kv.split("=")[1]))
if a.stages: ctx.SetOption("profile", 1)
shared_ir = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, taps) for c in range(2)], SR)
ctx.Destination.SetChannelCount(2)
for v in range(voices):
    s = AudioBufferSourceNode(ctx); s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v % 64, frames), SR); s.Loop = True
    cv = ConvolverNode(ctx)
    cv.Buffer = shared_ir if a.case != "private" else PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, taps, seed0=7 + 100 * (v + 1)) for c in range(2)], SR)
    s.Connect(cv).Connect(ctx.Destination); s.Start()
out = np.zeros((2, frames), np.float32)
ms = []
for step in range(a.warmup + a.steps):
    t0 = time.perf_counter(); ctx.Render(out, frames); dt = time.perf_counter() - t0
    if step >= a.warmup: ms.append(dt * 1e3)
st = ctx.GetStats()
med = statistics.median(ms)
line = {"tool": "long_ir_scene", "label": a.label, "case": a.case, "voices": voices, "taps": taps, "opts": a.opts, "library": os.path.basename(os.path.dirname(a.library)) if a.library else "",
        "steps": a.steps, "warmup": a.warmup, "ms_per_10s_median": round(med, 3), "ms_per_10s_all": [round(x, 3) for x in ms],
        "frames_per_s": round(frames / (med * 1e-3), 1), "chunks": st["chunks"], "kernel_launches": st["kernel_launches"],
        "coarse_fwd_launches": st["stage_launches"][5], "direct_sum_launches": st["stage_launches"][3], "rms": float(G.rms(out))}
if a.stages:
    line["stages"] = [{"stage": i, "kernel": st["stage_kernel"][i], "launches": st["stage_launches"][i], "ms": round(st["stage_ms"][i], 4),
                       "GB": round(st["stage_bytes"][i] / 1e9, 4), "GFLOP": round(st["stage_flops"][i] / 1e9, 3)} for i in range(16) if st["stage_launches"][i]]
print(json.dumps(line), flush=True)
ctx.Dispose()
