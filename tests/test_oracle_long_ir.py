"""The CPU oracle against the float64 model on impulse responses longer than 131,072 taps -- the yardstick the GPU tests of
tests/test_gpu_long_ir.py lean on.  The oracle's float32 partition sum (PartitionedConvolver.cs:104-223: P partitions of 128 samples
accumulated in float) drifts from the float64 convolution about as sqrt(P).  Measured with tests/_f64model.config3_shared, two
voices, relative RMS over the whole render / over the part where every partition is populated:

    262,144 taps : 8.4e-7 / 1.10e-6          524,288 taps : 1.16e-6 / 1.55e-6

The figures are seed free (fixed generators); the 1.5 x margin covers another libm's last bits, the only thing that can move them.
"""
import pytest

from tests import _f64model as M
from tests import _graphs as G
from tests._oracle import OracleContext

SR = 48000


@pytest.mark.parametrize("taps,whole,steady", [(262144, 8.4e-7, 1.10e-6), (524288, 1.16e-6, 1.55e-6)])
def test_oracle_drift_from_float64_on_long_responses(taps, whole, steady):
    frames = 128 * ((taps + 128 * 64 + 127) // 128)   # every partition populated
    o = OracleContext(SR)
    G.config3_convolver(o, voices=2, taps=taps, frames=frames)
    ref = G.render(o, 2, frames)
    o.Dispose()
    model = M.config3_shared(2, taps, frames)
    w = M.rms(ref - model) / M.rms(model)
    s = M.rms(ref[:, taps:] - model[:, taps:]) / M.rms(model[:, taps:])
    print(f"oracle vs float64 at {taps} taps: whole render {w:.3e}, steady state {s:.3e}")
    assert w <= 1.5 * whole, w
    assert s <= 1.5 * steady, s
