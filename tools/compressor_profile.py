"""Kernel times of compressor_kernel for DESIGN.md section 2g: (a) one stereo node over a 3,750-block chunk, (b) 1024 mono nodes
over the same chunk.  Run under `rocprofv3 --kernel-trace --stats --output-format csv`; the long dispatches of compressor_kernel are (a) then (b)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphaudio_amd import AudioBufferSourceNode, DynamicsCompressorNode, OfflineAudioContext, PlayableAudioBuffer  # noqa: E402

FS = 48000
BLOCKS = 3750
FRAMES = BLOCKS * 128


def run(nodes, channels):
    ctx = OfflineAudioContext(FS, device=0)
    rng = np.random.default_rng(5)
    # noise at about -12 dBFS: above the default threshold, so every frame takes the logarithm and the knee
    rows = [(rng.standard_normal(FRAMES + 4096) * 0.25).astype(np.float32) for _ in range(channels)]
    buf = PlayableAudioBuffer.FromChannelArrays(rows, FS)
    for v in range(nodes):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = buf
        cm = DynamicsCompressorNode(ctx)
        s.Connect(cm).Connect(ctx.Destination)
        s.Start(0.0, v / FS)   # (every node reads the buffer from another offset)
    out = np.zeros((2, FRAMES), dtype=np.float32)
    t0 = time.time()
    ctx.Render(out, FRAMES)
    st = ctx.GetStats()
    print(f"{nodes} node(s) x {channels} ch: render {1e3 * (time.time() - t0):.1f} ms wall, chunks {st['chunks']}, launches {st['kernel_launches']}, "
          f"peak {np.max(np.abs(out)):.3f}", flush=True)


run(1, 2)
run(1024, 1)
