"""What option "ir_resample" costs where it acts ("Impulse responses at another sample rate"): the time of
`ConvolverNode.Buffer = ir` for a 65,536-tap stereo impulse response, (a) at 44.1 kHz on a 48 kHz context with the option on --
upload, conversion on the device, copy back, spectra -- and (b) for a response of the converted length (71,332 taps) at 48 kHz,
as a caller who converted beforehand would assign it -- upload and spectra alone.  Every leg is a fresh context and a fresh buffer; one warm-up per leg
(code objects), then the median of the repeats, alternating.  The host-side figure of the same conversion (one thread running the
header) is `ir_resample_main time 44100 48000 2 65536` (tests/ir_resample_main.cpp).

    python tools/ir_resample_cost.py [--taps 65536] [--repeats 7]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from graphaudio_amd import ConvolverNode, OfflineAudioContext, PlayableAudioBuffer   # noqa: E402
from tests import _graphs as G   # noqa: E402
from tests import _ir_resample_model as model   # noqa: E402

SR = 48000


def leg(rows, rate, option):
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", option)
    cv = ConvolverNode(ctx)
    buf = PlayableAudioBuffer.FromChannelArrays(rows, rate)
    t0 = time.perf_counter()
    cv.Buffer = buf
    ms = (time.perf_counter() - t0) * 1e3
    n = ctx.GetStats()["ir_resamples"]
    ctx.Dispose()
    return ms, n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--taps", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    at_44 = [G.synth_ir(c, a.taps) for c in range(2)]
    # leg (b): a response of the converted length (its time does not depend on the values; the model's (M, 2W) matrices for 71,332
    # outputs are not worth their memory here)
    m = model.out_length(a.taps, model.plan(44100, SR))
    at_48 = [G.synth_ir(c, m) for c in range(2)]
    legs = {"44.1 kHz, ir_resample = 1": (at_44, 44100, 1), "48 kHz, converted beforehand": (at_48, SR, 0)}
    for rows, rate, opt in legs.values():
        leg(rows, rate, opt)
    ms = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, (rows, rate, opt) in legs.items():
            t, n = leg(rows, rate, opt)
            assert n == opt
            ms[k].append(t)
    for k, v in ms.items():
        print(f"ConvolverNode.Buffer = ({a.taps} taps x 2, {k}): median {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f}) of {len(v)}")
