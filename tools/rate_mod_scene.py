"""Measurement: 1024 vibrato voices (a looping 44.1 kHz buffer each, its own 5 Hz-ish LFO through a gain into PlaybackRate) into the
destination -- the scene of DESIGN.md "Modulated playbackRate".

Reports the device path's frames/s with the source walk on the device (option rate_mod_walk=1) and on the host from the read-back
rates (=0), the host time per chunk of each (GA_TIMING=1: "chunk total on the host"), and the one-thread CPU oracle's frames/s on a
short form of the scene.  Every leg runs in a child process of its own (GA_TIMING is read when the library loads).

    python tools/rate_mod_scene.py [--seconds 4] [--oracle-seconds 0.5] [--voices 1024]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000


def scene(ctx, voices):
    import numpy as np
    from graphaudio_amd import AudioBufferSourceNode, GainNode, OscillatorNode, PlayableAudioBuffer
    rng = np.random.default_rng(11)
    hold = []
    for v in range(voices):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray((rng.standard_normal(22050) * 0.05).astype(np.float32), 44100)
        s.Loop = True
        lfo = OscillatorNode(ctx)
        lfo.Frequency.Value = 4.0 + 0.002 * v
        g = GainNode(ctx)
        g.Gain.Value = 0.03
        lfo.Connect(g)
        g.Connect(s.PlaybackRate)
        s.Connect(ctx.Destination)
        lfo.Start()
        s.Start()
        hold += [s, lfo, g]
    return hold


def leg(kind, seconds, voices, walk):
    """One measurement in this process: prints one JSON line."""
    sys.path.insert(0, ROOT)
    import numpy as np
    if kind == "oracle":
        from tests._oracle import OracleContext as Ctx
        ctx = Ctx(SR)
    else:
        from graphaudio_amd import OfflineAudioContext
        ctx = OfflineAudioContext(SR)
        ctx.SetOption("rate_mod_walk", walk)
    hold = scene(ctx, voices)
    frames = int(seconds * SR) // 128 * 128
    warm = 128 * 64
    out = np.zeros((2, warm + frames), np.float32)
    ctx.Render(out, warm, 0)   # (first chunks: allocations, code objects)
    if hasattr(ctx, "Synchronize"):
        ctx.Synchronize()
    sys.stderr.write("[scene] timed\n")
    t0 = time.perf_counter()
    ctx.Render(out, frames, warm)
    if hasattr(ctx, "Synchronize"):
        ctx.Synchronize()
    dt = time.perf_counter() - t0
    del hold
    print(json.dumps({"kind": kind, "walk": walk, "frames": frames, "seconds": dt, "frames_per_s": frames / dt,
                      "rms": float(np.sqrt(np.mean(out[:, warm:].astype(np.float64) ** 2)))}))


def run_leg(kind, seconds, voices, walk):
    env = dict(os.environ)
    env["GA_TIMING"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--seconds", str(seconds), "--voices", str(voices),
                        "--walk", str(walk)], env=env, capture_output=True, text=True, timeout=1800)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(f"leg {kind} walk={walk} failed with status {p.returncode}")
    res = json.loads(p.stdout.strip().splitlines()[-1])
    timed = p.stderr.split("[scene] timed", 1)[-1]
    host = [float(x) for x in re.findall(r"chunk total on the host \(incl\. destructors\): ([0-9.]+) ms", timed)]
    waits = [float(x) for x in re.findall(r"stage 1 wait ([0-9.]+) ms", timed)]
    if host:
        res["chunks"] = len(host)
        res["host_ms_per_chunk"] = sum(host) / len(host)
        res["host_ms_per_chunk_excl_stage1_wait"] = (sum(host) - sum(waits)) / len(host)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--oracle-seconds", type=float, default=0.5)
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--walk", type=int, default=1)
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.seconds, a.voices, a.walk)
        return
    out = {"voices": a.voices}
    out["device_walk"] = run_leg("device", a.seconds, a.voices, 1)
    out["host_replay"] = run_leg("device", a.seconds, a.voices, 0)
    out["oracle"] = run_leg("oracle", a.oracle_seconds, a.voices, 1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
