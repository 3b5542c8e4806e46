"""Option "conv_migrate" (DESIGN.md 2b): a ConvolverNode that is running on formulation D (coarse partitions) when an edit makes it
sensitive -- its output now reaches a DelayNode.delayTime, a resonant low biquad or a feedback loop with a gain near 1 -- moves to
the B / C state layout and is evaluated in the reference's own order (formulation R) from that chunk on.  Its spectra history and
overlap are rebuilt from D's input history (conv_rebuild_kernel, then block T-1 alone through R's partition sum and inverse
transform), so the guarantee is bit equality: from the migrating chunk on the output is that of a node that was on R from its first
block and was fed the same samples.  The twin of every session is therefore the same session with conv_reference_order = 2.

The sessions live in tests/_migrate_scenes.py; tests/test_conv_migrate_host.py shows on the oracle that each of them exercises its
sink.  Every render (oracle, migrating device, twin) is made once and shared by the tests that read it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import OfflineAudioContext
from tests import _graphs as G
from tests import _migrate_scenes as M
from tests._oracle import OracleContext

COARSE_FWD = 5   # GA_STAGE_COARSE_FWD
CHUNK = 37

_renders = {}


def oracle(scene):
    key = (scene.name, "oracle")
    if key not in _renders:
        o = OracleContext(M.SR)
        _renders[key] = M.run(o, scene)[0]
        o.Dispose()
        _renders[key].setflags(write=False)
    return _renders[key]


def device(scene, leg):
    """leg: "migrate" (conv_migrate = 1 on formulation D), "off" (the same without the option), "twin" (R from the first block)"""
    key = (scene.name, leg)
    if key not in _renders:
        h = OfflineAudioContext(M.SR)
        h.SetOption("max_chunk_blocks", CHUNK)
        for k, v in scene.opts.items():
            h.SetOption(k, v)
        if leg == "twin":
            h.SetOption("conv_reference_order", 2)
        else:
            h.SetOption("coarse_min_blocks", 1)
            h.SetOption("conv_migrate", 1 if leg == "migrate" else 0)
        out, st0, st1 = M.run(h, scene)
        h.Dispose()
        out.setflags(write=False)
        _renders[key] = (out, st0, st1)
    return _renders[key]


def flips(ref, got):
    return int((ref != got).sum())


def assert_reference_order_bounds(ref, got):
    """the bounds test_gpu_reforder's static test holds this kind of scene to"""
    n, err = flips(ref, got), G.rms(ref - got)
    print(f"  {n} of {ref.size} values differ, rms error {err:.3e}")
    assert n <= ref.size * 1e-4 and err <= 1e-7, (n, err)


def assert_moved_from_d(st0, st1, moved=1):
    assert st0["stage_launches"][COARSE_FWD] > 0 and st0["ref_order_rows"] == 0 and st0["conv_migrations"] == 0
    assert st1["conv_migrations"] == moved and st1["ref_order_rows"] > 0


def assert_equals_twin(scene):
    got, st0, st1 = device(scene, "migrate")
    twin, _, t1 = device(scene, "twin")
    assert t1["conv_migrations"] == 0 and t1["stage_launches"][COARSE_FWD] == 0
    pre = scene.pre_frames
    assert G.rms(got[:, pre:]) > 1e-4
    assert np.array_equal(got[:, pre:], twin[:, pre:]), (scene.name, flips(got[:, pre:], twin[:, pre:]), G.rms(got[:, pre:] - twin[:, pre:]))
    return got, st0, st1


# ---- case 1: the base scene --------------------------------------------------------------------------------------------------
def test_unknown_values_are_refused():
    h = OfflineAudioContext(M.SR)
    for bad in (2, -1, 0.5):
        with pytest.raises(Exception):
            h.SetOption("conv_migrate", bad)
    h.SetOption("conv_migrate", 1)
    h.SetOption("conv_migrate", 0)
    h.Dispose()


def test_base_scene_moves_once_and_keeps_off_the_coarse_path():
    _, st0, st1 = device(M.BASE, "migrate")
    assert_moved_from_d(st0, st1)
    assert st1["stage_launches"][COARSE_FWD] == st0["stage_launches"][COARSE_FWD]   # no coarse launch since the edit
    assert st1["stage_kernel"][2] == "conv_rebuild_kernel" and st0["stage_kernel"][2] == ""   # GA_STAGE_RFFT_FWD: the rebuild ran


def test_base_scene_is_bit_identical_to_reference_order_from_the_start():
    assert_equals_twin(M.BASE)


def test_base_scene_against_the_oracle():
    ref = oracle(M.BASE)
    got, _, _ = device(M.BASE, "migrate")
    pre = M.BASE.pre_frames
    assert_reference_order_bounds(ref[:, pre:], got[:, pre:])
    assert G.rms(ref[:, :pre] - got[:, :pre]) <= 1e-5   # (formulation D in front of the edit: the contract)


def test_base_scene_with_the_option_off_stays_on_d():
    ref = oracle(M.BASE)
    off, st0, st1 = device(M.BASE, "off")
    got, _, _ = device(M.BASE, "migrate")
    pre = M.BASE.pre_frames
    assert st0["conv_migrations"] == 0 and st1["conv_migrations"] == 0
    assert st0["ref_order_rows"] == 0 and st1["ref_order_rows"] == 0
    assert st1["stage_launches"][COARSE_FWD] > st0["stage_launches"][COARSE_FWD]
    e_on, e_off = G.rms(ref[:, pre:] - got[:, pre:]), G.rms(ref[:, pre:] - off[:, pre:])
    print(f"base scene, post-edit rms error against the oracle: conv_migrate = 1 {e_on:.3e}, conv_migrate = 0 {e_off:.3e}")


# ---- cases 2-4: what the input history can look like ----------------------------------------------------------------------------
@pytest.mark.parametrize("scene", M.HISTORY_SHAPES, ids=lambda s: s.name)
def test_history_shapes_equal_the_twin(scene):
    _, st0, st1 = assert_equals_twin(scene)
    assert_moved_from_d(st0, st1)


@pytest.mark.parametrize("scene", M.EMPTY_HISTORIES, ids=lambda s: s.name)
def test_empty_and_silent_histories_equal_the_twin(scene):
    got, st0, st1 = assert_equals_twin(scene)
    assert st1["conv_migrations"] == 1
    # in front of the onset the convolver adds exact zeros: the delay time is exactly its intrinsic value there and the delayed dry voice
    # -- a copy of samples -- is all there is, value for value
    ref = oracle(scene)
    pre, onset = scene.pre_frames, scene.pre_frames + 128 * 4
    assert np.array_equal(got[:, pre:onset], ref[:, pre:onset])


def test_more_than_1024_partitions_equal_the_twin():
    _, st0, st1 = assert_equals_twin(M.LONG_IR)
    assert_moved_from_d(st0, st1)


# ---- cases 5, 6: groups -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", M.GROUP_MEMBER, ids=lambda s: s.name)
def test_one_member_leaves_a_premixed_group(scene):
    ref = oracle(scene)
    got, st0, st1 = device(scene, "migrate")
    assert st0["coarse_premixed_signals"] > 0 and st0["conv_migrations"] == 0
    assert st1["conv_migrations"] == 1 and st1["ref_order_rows"] > 0
    # the other eight stay a pre-mixed group in every chunk behind the edit (37 + 3 + 20 blocks: three chunks)
    assert st1["coarse_premixed_signals"] - st0["coarse_premixed_signals"] == 8 * 3
    err = G.rms(ref - got)
    print(f"{scene.name}: rms error against the oracle {err:.3e} (bus rms {G.rms(ref):.3e})")
    assert err <= 1e-5


@pytest.mark.parametrize("scene", M.GROUP_MEMBER_ALONE, ids=lambda s: s.name)
def test_the_delayed_voice_alone_meets_the_reference_order_bounds(scene):
    ref = oracle(scene)
    got, st0, st1 = device(scene, "migrate")
    assert st1["conv_migrations"] == 1
    pre = scene.pre_frames
    assert G.rms(ref[:, pre:]) > 1e-4
    assert_reference_order_bounds(ref[:, pre:], got[:, pre:])


def test_all_members_move_at_once():
    got, st0, st1 = assert_equals_twin(M.GROUP_ALL)
    assert st0["coarse_premixed_signals"] > 0
    assert st1["conv_migrations"] == 9
    assert st1["stage_launches"][COARSE_FWD] == st0["stage_launches"][COARSE_FWD]


# ---- cases 7, 8: sensitivity without a new connection to a parameter ------------------------------------------------------------
def test_a_retuned_biquad_moves_the_node():
    ref = oracle(M.RETUNE)
    got, st0, st1 = device(M.RETUNE, "migrate")
    off, _, o1 = device(M.RETUNE, "off")
    assert_moved_from_d(st0, st1)
    assert o1["conv_migrations"] == 0 and o1["ref_order_rows"] == 0
    e_on, e_off = G.rms(ref - got), G.rms(ref - off)
    print(f"retuned biquad, rms error against the oracle: conv_migrate = 1 {e_on:.3e}, conv_migrate = 0 {e_off:.3e}")
    assert e_on <= 1e-5


def test_a_loop_closed_behind_a_running_convolver_moves_it():
    ref = oracle(M.LOOP)
    got, st0, st1 = device(M.LOOP, "migrate")
    assert_moved_from_d(st0, st1)
    err, scale = G.rms(ref - got), max(G.rms(ref), 1e-3)
    print(f"loop closed behind the convolver: rms error {err:.3e} at {scale:.3e}")
    assert err <= 1e-5 * max(1.0, scale) and err <= 2e-5 * scale   # the bounds of the generated sessions with feedback loops


# ---- case 9: formulation A ------------------------------------------------------------------------------------------------------
def test_formulation_a_member_moves_by_state_copy():
    """A's spectra history comes from float32 transforms: the P - 1 blocks behind the move are R's arithmetic over A's spectra (the
    convolver tolerance of the README, 2e-6), and from block P behind the move on -- the first block whose incoming overlap was made
    of R's spectra alone -- the output is that of the session in which voice 0 had its sink, and formulation R, from the first block."""
    P = (M.A_TAPS + 127) // 128
    scene = M.A_MEMBER
    ref = oracle(scene)
    got, st0, st1 = device(scene, "migrate")
    twin, _, t1 = device(M.A_MEMBER_TWIN, "off")
    assert st0["conv_migrations"] == 0 and st0["ref_order_rows"] == 0 and st0["n_conv_rows"] > 0
    assert st1["conv_migrations"] == 1 and st1["ref_order_rows"] > 0 and st1["stage_launches"][COARSE_FWD] == 0
    assert t1["conv_migrations"] == 0 and t1["ref_order_rows"] > 0
    pre = scene.pre_frames
    a, b = pre + 128 * (P - 1), pre + 128 * P
    err = G.rms(ref[:, pre:a] - got[:, pre:a])
    print(f"formulation A, the {P - 1} blocks behind the move: rms error against the oracle {err:.3e}; whole render {G.rms(ref - got):.3e}")
    assert err <= 2e-6
    assert G.rms(got[:, b:]) > 1e-4
    assert np.array_equal(got[:, b:], twin[:, b:]), (flips(got[:, b:], twin[:, b:]), G.rms(got[:, b:] - twin[:, b:]))


# ---- case 11: generated edit sessions -------------------------------------------------------------------------------------------
# The first twenty move a convolver (a rewiring or a parameter write puts a resonant biquad, a parameter or a loop behind one that was
# running on formulation D or A); the other ten do not.  Seeds >= 50000 have feedback loops.
MOVING_SESSIONS = [20025, 20196, 20210, 20225, 20293, 20313, 20408, 20720, 30058, 30118, 40099, 40169, 40171, 50085, 50154, 50222, 50257,
                   50258, 50459, 50523]
OTHER_SESSIONS = [20160, 20161, 20162, 20163, 20164, 50160, 50161, 50162, 50163, 50164]
_moved = {}


@pytest.mark.parametrize("seed", MOVING_SESSIONS + OTHER_SESSIONS)
def test_generated_edit_sessions(seed):
    """the bounds of tests/test_gpu_fuzz.py::test_random_edit_session_matches_oracle, with conv_migrate = 1 on formulation D"""
    from tests._fuzz import run_random_session
    o = OracleContext(48000)
    ref, ref_log = run_random_session(o, seed)
    h = OfflineAudioContext(48000)
    h.SetOption("max_chunk_blocks", 11)
    h.SetOption("coarse_min_blocks", 1)
    h.SetOption("conv_migrate", 1)
    got, got_log = run_random_session(h, seed)
    _moved[seed] = h.GetStats()["conv_migrations"]
    h.Dispose()
    o.Dispose()
    assert ref_log == got_log
    assert np.isfinite(ref).all() and G.rms(ref) <= 50.0   # (no loop of these sessions grows without bound)
    err = G.rms(ref - got)
    scale = max(G.rms(ref), 1e-3)
    print(f"session {seed}: {_moved[seed]} moved, rms error {err:.3e} at {scale:.3e}")
    assert err <= 1e-5 * max(1.0, scale if seed >= 50000 else 1.0) and err <= 2e-5 * scale, (seed, err, scale)
    if seed in MOVING_SESSIONS:
        assert _moved[seed] > 0


# ---- case 10: next to the other things a chunk can be ---------------------------------------------------------------------------
def test_next_to_a_voice_with_a_modulated_playback_rate():
    base, _, b1 = device(M.BASE, "migrate")
    got, st0, st1 = device(M.BASE_WITH_VIBRATO, "migrate")
    assert_moved_from_d(st0, st1)
    assert st1["kernel_launches"] > b1["kernel_launches"]   # (the modulator cone's stage runs in every chunk)
    assert np.array_equal(got, base)



def test_asynchronous_render_into_page_locked_rows():
    import torch
    base, _, _ = device(M.BASE, "migrate")
    h = OfflineAudioContext(M.SR)
    for k, v in (("max_chunk_blocks", CHUNK), ("coarse_min_blocks", 1), ("conv_migrate", 1), ("async", 1)):
        h.SetOption(k, v)
    ses = M.BASE.build(h)
    rows = torch.zeros((2, M.BASE.frames), dtype=torch.float32).pin_memory()
    out = rows.numpy()
    pos = 0
    for n in M.BASE.pre:
        h.Render(out, 128 * n, pos)
        pos += 128 * n
    ses.edit()
    for n in M.BASE.post:
        h.Render(out, 128 * n, pos)
        pos += 128 * n
    h.Synchronize()
    st = h.GetStats()
    got = out.copy()
    h.Dispose()
    assert st["conv_migrations"] == 1
    assert np.array_equal(got, base)
