"""What tests/test_gpu_libm_exact.py and tests/test_libmf_host.py share (option "libm_exact"): the context
class that switches the option on, and the pow scene -- no scene of tests/_param_scenes.py tells powf from the rounded-once double
(its gain ramps are bit-equal between the two oracles), so this one steps a k-rate gain through gains at which they differ."""
import numpy as np

from graphaudio_amd import FilterType, OfflineAudioContext
from tests import _param_scenes as P

B = P.B

# float32 bit patterns of 24 of the gains `libmf_main gains` prints: powf(10, g / 40) is one ulp above the rounded-once double
POW_GAIN_BITS = [0xC26EE666, 0xC26C7BE2, 0xC26B2198, 0xC26B15C2, 0xC2682312, 0xC266A239, 0xC2661A67, 0xC265DC69,
                 0xC2644C37, 0xC262E167, 0xC2625B39, 0xC2621651, 0xC2618141, 0xC25E6191, 0xC25DEE23, 0xC25CFADB,
                 0xC25B6617, 0xC25B4F01, 0xC25A8ED1, 0xC25861F1, 0xC2553322, 0xC2552E72, 0xC255294A, 0xC254CA7C]
POW_GAINS = np.array(POW_GAIN_BITS, np.uint32).view(np.float32)
POW_BLOCKS = 26


def exact_context(form="default"):
    """A context class for P.render: the device with libm_exact = 1 and the options of the render form (P.render sets those only
    on OfflineAudioContext itself)."""
    opts = P.FORMS[form][1]

    class LibmExactContext(OfflineAudioContext):
        def __init__(self, sampleRate=P.SR):
            super().__init__(sampleRate)
            self.SetOption("libm_exact", 1)
            for k, v in opts.items():
                self.SetOption(k, v)
    return LibmExactContext


def pow_gain_timeline():
    """k-rate: the value at a block's start holds for the block.  Gain 0 in block 0, gain k from block k + 1 on, the last one held."""
    tl = P.gtl(0.0)
    for k, g in enumerate(POW_GAINS):
        tl.set(float(g), P.at_frame((k + 1) * B))
    return tl


def pow_scene(ftype):
    """1200 Hz is off the 1000 Hz baseline every block starts from: one coefficient update, and so one powf, per block."""
    def build(ctx):
        s = P.noise(ctx, 2, POW_BLOCKS, scale=0.05)
        bq = P.biquad(ctx, ftype, s, fv=1200.0, qv=0.9, g=pow_gain_timeline())
        bq.Connect(ctx.Destination)
        return (s, bq)
    return P.Scene(f"bq_pow_gains_{ftype.name}", build, POW_BLOCKS)


POW_TYPES = [FilterType.Peaking, FilterType.Lowshelf]
