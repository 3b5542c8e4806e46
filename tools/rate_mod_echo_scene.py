"""Measurement: 1024 vibrato voices (tools/rate_mod_scene.py) on a master bus with a feedback loop -- the scene of DESIGN.md
"Modulated playbackRate", "... in a graph with feedback loops".

Legs, each in a child process of its own (GA_TIMING is read when the library loads):
  echo    the bus -> DelayNode(0.25 s) -> destination, DelayNode -> GainNode(0.5) -> DelayNode: the loop is cut at the DelayNode,
          93-block two-stage chunks
  uncut   the bus -> a -> b -> a, b -> destination (two GainNodes feeding each other): a loop that cannot be cut, one-block chunks
  oracle  the one-thread CPU oracle on a short form of the echo leg

Reports frames/s, the chunks of the timed render, the host time per chunk (GA_TIMING=1: "chunk total on the host") and the stage-1
wait per chunk ("two-stage chunk: stage 1 wait").

    python tools/rate_mod_echo_scene.py [--seconds 4] [--uncut-seconds 0.5] [--oracle-seconds 0.5] [--voices 1024]
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


def scene(ctx, voices, loop):
    import numpy as np
    from graphaudio_amd import AudioBufferSourceNode, DelayNode, GainNode, OscillatorNode, PlayableAudioBuffer
    rng = np.random.default_rng(11)
    bus = GainNode(ctx)
    bus.Gain.Value = 0.5
    bus.Connect(ctx.Destination)
    hold = [bus]
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
        s.Connect(bus)
        lfo.Start()
        s.Start()
        hold += [s, lfo, g]
    if loop == "echo":
        d = DelayNode(ctx, 1.0)
        d.DelayTime.Value = 0.25
        fb = GainNode(ctx)
        fb.Gain.Value = 0.5
        bus.Connect(d)
        d.Connect(fb).Connect(d)
        d.Connect(ctx.Destination)
        hold += [d, fb]
    else:
        a, b = GainNode(ctx), GainNode(ctx)
        a.Gain.Value = 0.5
        b.Gain.Value = 0.5
        bus.Connect(a).Connect(b).Connect(a)
        b.Connect(ctx.Destination)
        hold += [a, b]
    return hold


def leg(kind, seconds, voices):
    """One measurement in this process: prints one JSON line."""
    sys.path.insert(0, ROOT)
    import numpy as np
    if kind == "oracle":
        from tests._oracle import OracleContext as Ctx
        ctx = Ctx(SR)
    else:
        from graphaudio_amd import OfflineAudioContext
        ctx = OfflineAudioContext(SR)
    hold = scene(ctx, voices, "uncut" if kind == "uncut" else "echo")
    frames = int(seconds * SR) // 128 * 128
    warm = 128 * 200   # (first chunks: allocations, code objects; two full echo chunks)
    out = np.zeros((2, warm + frames), np.float32)
    ctx.Render(out, warm, 0)
    if hasattr(ctx, "Synchronize"):
        ctx.Synchronize()
    sys.stderr.write("[scene] timed\n")
    t0 = time.perf_counter()
    ctx.Render(out, frames, warm)
    if hasattr(ctx, "Synchronize"):
        ctx.Synchronize()
    dt = time.perf_counter() - t0
    del hold
    print(json.dumps({"kind": kind, "frames": frames, "seconds": dt, "frames_per_s": frames / dt,
                      "rms": float(np.sqrt(np.mean(out[:, warm:].astype(np.float64) ** 2))),
                      "finite": bool(np.isfinite(out).all())}))


def run_leg(kind, seconds, voices):
    env = dict(os.environ)
    env["GA_TIMING"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--seconds", str(seconds), "--voices", str(voices)],
                       env=env, capture_output=True, text=True, timeout=1800)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(f"leg {kind} failed with status {p.returncode}")
    res = json.loads(p.stdout.strip().splitlines()[-1])
    timed = p.stderr.split("[scene] timed", 1)[-1]
    host = [float(x) for x in re.findall(r"chunk total on the host \(incl\. destructors\): ([0-9.]+) ms", timed)]
    waits = [float(x) for x in re.findall(r"stage 1 wait ([0-9.]+) ms", timed)]
    if host:
        res["chunks"] = len(host)
        res["blocks_per_chunk"] = res["frames"] / 128 / len(host)
        res["host_ms_per_chunk"] = sum(host) / len(host)
        res["stage1_wait_ms_per_chunk"] = sum(waits) / len(host)
        res["host_ms_per_chunk_excl_stage1_wait"] = (sum(host) - sum(waits)) / len(host)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--uncut-seconds", type=float, default=0.5)
    ap.add_argument("--oracle-seconds", type=float, default=0.5)
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--leg", default=None)
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.seconds, a.voices)
        return
    out = {"voices": a.voices}
    out["echo"] = run_leg("echo", a.seconds, a.voices)
    out["uncut"] = run_leg("uncut", a.uncut_seconds, a.voices)
    out["oracle"] = run_leg("oracle", a.oracle_seconds, a.voices)
    out["echo_over_oracle"] = out["echo"]["frames_per_s"] / out["oracle"]["frames_per_s"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
