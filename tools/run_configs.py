#!/usr/bin/env python3
"""Render the other BASELINE.json configurations at full size on the HIP path and report frames/s (not bench lines:
bench.py measures configs[2]; these are parity-test cases, timed here to find performance bugs)."""
import os, sys, time, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphaudio_amd import OfflineAudioContext, _capi
from tests import _graphs as G

if os.environ.get("GA_TOOL_LIBRARY"):   # a tools/build_variant.sh build (this tool only; the product reads no such variable)
    _capi.use_library(os.environ["GA_TOOL_LIBRARY"])

SR = 48000
which = sys.argv[1] if len(sys.argv) > 1 else "2"
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
frames = int(seconds * SR) // 128 * 128
ctx = OfflineAudioContext(SR)
ctx.SetOption("profile", 1)
for kv in os.environ.get("GA_OPTS", "").split(","):   # e.g. GA_OPTS=coarse_tail_private=0,async=1
    if "=" in kv:
        ctx.SetOption(kv.split("=")[0], float(kv.split("=")[1]))
t0 = time.time()
if which == "2":
    ch = G.config2_biquad(ctx, voices=256, frames=frames + 256)
elif which == "4":
    ch = G.config4_eq(ctx, voices=int(sys.argv[3]) if len(sys.argv) > 3 else 4096, frames=frames)
elif which == "3u":
    ch = G.config3_convolver(ctx, voices=int(sys.argv[3]) if len(sys.argv) > 3 else 64, taps=65536, frames=frames, shared=False)
elif which == "5":
    from graphaudio_amd import AudioBufferSourceNode, ConvolverNode, PlayableAudioBuffer
    nsrc = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    taps, C = 32768, 16
    ctx.Destination.SetChannelCount(C)
    n = np.arange(taps)
    env = np.exp(-6.9 * n / taps).astype(np.float32)
    for v in range(nsrc):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, frames + 256), SR)
        rng = np.random.default_rng(7 + 100 * v)
        irs = [(rng.standard_normal(taps, dtype=np.float32) * env) for c in range(C)]
        cv = ConvolverNode(ctx)
        cv.Buffer = PlayableAudioBuffer.FromChannelArrays(irs, SR)
        s.Connect(cv).Connect(ctx.Destination)
        s.Start()
    ch = C
elif which == "kit":   # buses + panners + post-mix reverb
    ch = G.kit_scene(ctx, voices=int(sys.argv[3]) if len(sys.argv) > 3 else 256, frames=frames + 256, taps=65536)
elif which == "osc":   # oscillators + panners (8(f) rank 1 nodes at scale)
    from graphaudio_amd import OscillatorNode, OscillatorType, StereoPannerNode, GainNode
    n_osc = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    for v in range(n_osc):
        o = OscillatorNode(ctx)
        o.Type = OscillatorType(v % 4)
        o.Frequency.Value = 55.0 * 2.0 ** (v / 128.0)
        p = StereoPannerNode(ctx)
        p.Inputs[0].SetChannelCount(1)
        p.Pan.Value = -1.0 + 2.0 * v / max(n_osc - 1, 1)
        g = GainNode(ctx)
        g.Gain.Value = 1.0 / 64.0
        o.Connect(p).Connect(g).Connect(ctx.Destination)
        o.Start()
    ch = 2
elif which in ("spatial", "spatial_occlusion", "spatial_builtin"):   # SpatialPannerNode at scale: every voice through its own node, moving, so that every block crossfades
    import math                                    # spatial_occlusion: every node behind a wall as well (option spatial_occlusion: spatial_direct_kernel)
    from graphaudio_amd import AudioBufferSourceNode, HrirSet, PlayableAudioBuffer, SpatialPannerNode
    n_voices = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    T, A, E = 256, 24, 7
    k = np.arange(T)
    hrir = (np.random.default_rng(5).standard_normal((A * E, 2, T)) * np.exp(-6.9 * k / T) * 0.1).astype(np.float32)
    if which == "spatial_builtin":   # no set assigned: every node on the built-in spherical-head set (T = 112 at 48 kHz, 72 x 25 directions)
        ctx.SetOption("spatial_builtin_hrir", 1)
    else:
        ctx.SetHrir(HrirSet.FromArray(hrir, SR), A)
    if which == "spatial_occlusion":
        ctx.SetOption("spatial_occlusion", 1)
    corners, period = 32, 5.0   # a circle as a 32-gon of linear ramps, one revolution per 5 s
    for v in range(n_voices):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, frames + 256, 1.0 / 64.0), SR)
        p = SpatialPannerNode(ctx)
        radius, phase = 1.5 + 2.0 * (v % 17) / 17.0, 2.0 * math.pi * v / n_voices
        p.PositionY.Value = -1.0 + 2.0 * (v % 5) / 4.0
        if which == "spatial_occlusion":
            p.Occlusion.Value = 1.0
            p.TransmissionLow.Value, p.TransmissionMid.Value, p.TransmissionHigh.Value = 0.9, 0.5, 0.1
        for c in range(int(math.ceil(seconds / period * corners)) + 1):
            a, t = phase + 2.0 * math.pi * c / corners, c * period / corners
            first = c == 0
            (p.PositionX.SetValueAtTime if first else p.PositionX.LinearRampToValueAtTime)(radius * math.sin(a), t)
            (p.PositionZ.SetValueAtTime if first else p.PositionZ.LinearRampToValueAtTime)(-radius * math.cos(a), t)
        s.Connect(p).Connect(ctx.Destination)
        s.Start()
    ch = 2
elif which == "spatial_head":   # what remaking the built-in set costs: one voice, one-block renders with and without a radius change in front
    import statistics
    from graphaudio_amd import AudioBufferSourceNode, PlayableAudioBuffer, SpatialPannerNode
    ctx.SetOption("spatial_builtin_hrir", 1)
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(0, 128 * 64), SR)
    p = SpatialPannerNode(ctx)
    p.PositionX.Value = 1.0
    s.Connect(p).Connect(ctx.Destination)
    s.Start()
    out = np.zeros((2, 128 * 64), np.float32)
    for b in range(4):
        ctx.Render(out, 128, b * 128)
    remake, plain = [], []
    for i in range(12):
        ctx.SetOption("spatial_head_radius", 0.08 if i % 2 == 0 else 0.0875)   # (sets of the same stored size)
        for times in (remake, plain):
            t0 = time.perf_counter()
            ctx.Render(out, 128, (4 + 2 * i + (times is plain)) * 128)
            times.append((time.perf_counter() - t0) * 1e3)
    print(f"one-block render behind a radius change: median {statistics.median(remake):.3f} ms (min {min(remake):.3f}); without: median "
          f"{statistics.median(plain):.3f} ms (min {min(plain):.3f}); a remake of the set (allocation, launch, spatial_head_kernel over 3600 x 112 "
          f"taps, release of the old copy) costs the difference, {statistics.median(remake) - statistics.median(plain):.3f} ms")
    raise SystemExit(0)
elif which == "spatial_signals":   # the scene above with every orbit driven by two oscillators (option spatial_param_signals): descriptors made on the device
    import math
    from graphaudio_amd import AudioBufferSourceNode, GainNode, HrirSet, OscillatorNode, PlayableAudioBuffer, SpatialPannerNode
    ctx.SetOption("spatial_param_signals", 1)
    n_voices = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    T, A, E = 256, 24, 7
    k = np.arange(T)
    hrir = (np.random.default_rng(5).standard_normal((A * E, 2, T)) * np.exp(-6.9 * k / T) * 0.1).astype(np.float32)
    ctx.SetHrir(HrirSet.FromArray(hrir, SR), A)
    period = 5.0
    for v in range(n_voices):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, frames + 256, 1.0 / 64.0), SR)
        p = SpatialPannerNode(ctx)
        radius, freq = 1.5 + 2.0 * (v % 17) / 17.0, (1.0 + (v % 7) / 50.0) / period
        p.PositionY.Value = -1.0 + 2.0 * (v % 5) / 4.0
        # x = r sin(w t); z = r sin(w (t - T / 4)) = -r cos(w t) from a quarter period on (0 before: the orbit opens along x).  A
        # GainNode's stereo output reaches the parameter as (L + R) / sqrt(2): its gain is r / sqrt(2).
        for param, when in ((p.PositionX, 0.0), (p.PositionZ, 0.25 / freq)):
            o = OscillatorNode(ctx)
            o.Frequency.Value = freq
            g = GainNode(ctx)
            g.Gain.Value = radius / math.sqrt(2.0)
            o.Connect(g)
            g.Connect(param)
            o.Start(when)
        s.Connect(p).Connect(ctx.Destination)
        s.Start()
    ch = 2
else:
    raise SystemExit("unknown config")
print(f"build {time.time() - t0:.1f} s")
out = np.zeros((ch, frames), np.float32)
piece = frames // 4 // 128 * 128
for rep in range(4):   # the first pieces carry one-time costs (formulation assignment, first touch of scratch memory): quote the last
    t0 = time.time()
    ctx.Render(out, piece, rep * piece)
    dt = time.time() - t0
    print(f"render piece {rep}: {dt * 1e3:.1f} ms -> {piece / dt / 1e6:.2f} M frames/s")
st = ctx.GetStats()
print(json.dumps({k: st[k] for k in ("chunks", "segments", "kernel_launches", "device_ms_total", "mac_ms_total", "fft_ms_total", "other_ms_total", "device_bytes_in_use")}))
print("rms", G.rms(out))
if which in ("spatial", "spatial_signals", "spatial_occlusion", "spatial_builtin"):   # spatial_panner_kernel is accounted under stage "other"; 157.3 TFLOPS fp32 vector peak = 78.65e12 fma/s
    ms, flops = st["stage_ms"][0], st["stage_flops"][0]
    print(f"stage other ({st['stage_kernel'][0]}): {ms:.2f} ms over {st['profiled_chunks']} chunks, {flops / 2 / 1e9:.1f} G fma, "
          f"{flops / 2 / max(ms, 1e-9) / 1e9:.2f} T fma/s = {flops / 2 / max(ms, 1e-9) / 1e9 / 78.65 * 100:.1f} % of the fp32 vector peak (all 'other' kernels in the time)")

if os.environ.get("GA_SIGPROF_OUT"):   # tools/prof/sigprof.c preloaded: write its samples before the process leaves through _exit
    import ctypes
    ctypes.CDLL(None).sigprof_dump()
