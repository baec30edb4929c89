"""CPU suite: the host side of r3d_streams_peek (early poses for live streams of centred models: the window the reference builds when
a clip ends at the newest frame, read out of the rings without ending the streams) - header, binding and exports, the argument rules
(all checked before any device call: they run without a GPU), and the host hook r3d_debug_streams_peek_host, bit for bit, against
three things: the REFERENCE's own prefix windows (tests/golden/peek.npz: UnchunkedGenerator + Trainer.eval_data_prepare on
clip[:c]), a NumPy restatement of the rule tick by tick (tests/streams_peek_cases.py), and the drain - the window a DRAIN started at
that tick emits.  Everything inside guard bands (tests/buffers_util.py), the state compared byte for byte around every call.
tests/test_gpu_streams_peek.py runs the kernel on the same sequences."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, hooks_library

import streams_cases as sc
import streams_peek_cases as pc
import streams_repair_cases as rc_cases
from streams_cases import DRAIN, FILL, IDLE, NONE, PUSH, RESTART, same_bits
from streams_peek_cases import PeekRig
from ray3d_amd import _capi

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed


# ------------------------------------------------------------------------------------ header, binding, exports

def test_header_binding_and_exports_agree_and_the_abi_stays_6():
    assert "r3d_streams_peek" in _capi.EXPORTS and "r3d_debug_streams_peek_host" in _capi.HOOK_EXPORTS
    assert int(re.search(r"#define R3D_STREAMS_PEEK_MAX (\d+)", HDR).group(1)) == _capi.STREAMS_PEEK_MAX == 8
    assert re.search(r"\bint r3d_streams_peek\(const void \*state_dev", HDR)
    assert HDR.index("int r3d_debug_streams_peek_host(") > HDR.index("#ifdef R3D_TEST_HOOKS") > HDR.index("int r3d_streams_peek(")
    assert HDR.index("int r3d_streams_peek(") > HDR.index("int r3d_streams_step(")
    product = C.CDLL(_capi.LIB_PATH)
    assert hasattr(product, "r3d_streams_peek") and not hasattr(product, "r3d_debug_streams_peek_host")
    hooks = hooks_library()
    assert hasattr(hooks, "r3d_streams_peek") and hasattr(hooks, "r3d_debug_streams_peek_host")
    assert hooks.r3d_abi_version() == 6 == _capi.ABI_VERSION and int(re.search(r"#define R3D_ABI_VERSION (\d+)", HDR).group(1)) == 6


# ------------------------------------------------------------------------------------ 1. the reference's prefix windows

@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_previews_are_the_reference_windows_of_the_clip_prefix(case):
    """The six clips side by side on a state nobody zeroed, a peek with the looks 0, lag / 2 and lag - 1 behind every tick: after
    tick c - 1 stream k holds clip[:c], and its preview at look L is window c - 1 - L of the generator + eval_data_prepare on that
    prefix, straight and mirrored - or, where the fixture says c <= L, there is none."""
    clips, rf, lag, perm, _, _ = sc.golden_case(case, "centred")
    z = pc.golden()
    pairs, plain, mirror = z[case + "_pairs"], z[case + "_plain"], z[case + "_mirror"]
    looks = pc.looks_of(lag)
    assert sorted(set(pairs[:, 2].tolist())) == sorted(set(looks)) and (pairs[:, 3] < 0).any()
    J, F = clips[0].shape[1:]
    rig = PeekRig("cpu", len(clips), rf, lag, J, F, looks, NONE, perm)
    frames, actions = pc.clip_schedule(clips, lag)
    outs = pc.run(rig, frames, actions)
    seen = 0
    for k, c, L, row in pairs.tolist():
        out, kk = outs[c - 1], looks.index(L)
        assert actions[c - 1, k] in (PUSH, RESTART)
        if row < 0:
            assert c <= L and out["emit"][kk, k] == -1 and out["status"][kk, k] == 0 and (out["x"][kk, k] == FILL).all()
            continue
        assert out["emit"][kk, k] == c - 1 - L and out["status"][kk, k] == 0
        assert same_bits(out["x"][kk, k], plain[row]) and same_bits(out["x_mirror"][kk, k], mirror[row]), (k, c, L)
        seen += 1
    assert seen == plain.shape[0] == mirror.shape[0]
    # the prefixes the fixture has to cover: one frame, fewer frames than the look, exactly lag, exactly RF, a wrapped ring
    cs, Ls = pairs[:, 1], pairs[:, 2]
    assert (cs == 1).any() and (cs <= Ls).any() and (cs == lag).any() and (cs == rf).any() and (cs > rf).any()


# ------------------------------------------------------------------------------------ 2. the restatement, tick by tick

@pytest.mark.parametrize("looks", ["one", "three"])
@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_clips_side_by_side_equal_the_restatement(case, looks):
    """The clips' schedule (RESTART, PUSH ..., DRAIN x lag, IDLE), K = 1 (the last admissible look) and K = 3 (0 and lag - 1 among
    them): pc.run checks emit / peek_status of every (k, s), the previewing rows against the ring AND the frames the stream was
    given, every other row at its fill, the guards and the state's bytes."""
    clips, rf, lag, perm, _, _ = sc.golden_case(case, "centred")
    J, F = clips[0].shape[1:]
    lk = (lag - 1,) if looks == "one" else pc.looks_of(lag)
    rig = PeekRig("cpu", len(clips), rf, lag, J, F, lk, NONE, perm)
    frames, actions = pc.clip_schedule(clips, lag)
    outs = pc.run(rig, frames, actions)
    # a stream previews exactly while it PUSHes with more frames than the look; never during its drain or afterwards
    for t, out in enumerate(outs):
        for s, c in enumerate(clips):
            for k, L in enumerate(lk):
                assert out["emit"][k, s] == (t - L if t < c.shape[0] and t - L >= 0 else -1), (t, s, k)
        assert (out["status"] == 0).all()


@pytest.mark.parametrize("use_action", [True, False], ids=["actions", "no-actions"])
@pytest.mark.parametrize("mirror", [True, False], ids=["mirror", "plain"])
@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_mixed_actions_on_a_poisoned_state_equal_the_restatement(case, mirror, use_action):
    """IDLE, RESTART, DRAIN and refused streams mixed in, on a state of 0xA5 bytes; with action_dev NULL every stream whose head
    allows it counts as pushed (an IDLE stream then previews what it holds)."""
    clips, rf, lag, perm, _, _ = sc.golden_case(case, "centred")
    J, F = clips[0].shape[1:]
    rig = PeekRig("cpu", 6, rf, lag, J, F, pc.looks_of(lag), NONE, perm)
    frames, actions = pc.mixed_schedule(6, J, F, lag, rf, rf + 8)
    outs = pc.run(rig, frames, actions, use_action=use_action, mirror=mirror)
    st = np.stack([o["status"][0] for o in outs])
    assert (st[:, 4] == 1).all() and (st[:, 5] == 1).all()            # an untouched poisoned head; a stream the step refuses
    assert st[5, 3] == 1 and st[6, 3] == 0 and (st[:, 0] == 0).all()  # the unknown action word, once
    emit0 = np.stack([o["emit"][0] for o in outs])
    idle = actions[:, 1] == IDLE
    assert ((emit0[idle, 1] == -1) if use_action else (emit0[idle, 1] >= 0)).all()
    drains = actions[:, 2] == DRAIN
    assert (emit0[drains, 2] == -1).all() and emit0[np.nonzero(drains)[0][-1] + 1, 2] == 0          # the RESTART: frame 0 at once
    assert emit0[-1, 0] == len(actions) - 1 > rf                       # the ring of stream 0 has wrapped


def test_a_zeroed_state_and_fewer_looks_than_the_buffers_hold():
    """An all-zero state is freshly reset streams (count 0: nothing to preview until the first PUSH); a call with K = 2 on buffers
    for three looks writes the front two row blocks and word rows and nothing behind them."""
    J, F, rf, lag = 14, 2, 9, 4
    rig = PeekRig("cpu", 2, rf, lag, J, F, (0, 1, 3), NONE, None, zero_state=True)
    frame = np.random.RandomState(3).standard_normal((2, J, F)).astype(np.float32)
    rig.tick(frame, np.array([IDLE, IDLE], np.int32))
    out = rig.peek(use_action=False)
    assert out["rc"] == 0 and (out["emit"] == -1).all() and (out["status"] == 0).all() and (out["x"] == FILL).all()
    rig.tick(frame, np.array([PUSH, IDLE], np.int32))
    out = rig.peek(looks=(0, 3))
    assert out["emit"].tolist() == [[0, -1], [-1, -1]] and (out["emit_rest"] == pc.FILL_EMIT).all() and (out["status_rest"] == pc.FILL_STATUS).all()
    assert same_bits(out["x"][0, 0], np.broadcast_to(frame[0], (rf, J, F))) and (out["x"][0, 1] == FILL).all() and (out["x"][1:] == FILL).all()
    assert (out["x_mirror"] == FILL).all()


# ------------------------------------------------------------------------------------ 3. the drain

@pytest.mark.parametrize("frames_pushed", ["1", "3", "lag", "rf", "rf + 5"])
@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_a_peek_with_look_lag_minus_k_is_the_window_the_drain_emits_at_tick_k(case, frames_pushed):
    """Just before a drain, for every k in 1 .. lag: the peek at look lag - k (emit, window, mirrored window) is what DRAIN tick k
    writes - also where neither has a frame (a stream shorter than the look)."""
    clips, rf, lag, perm, _, _ = sc.golden_case(case, "centred")
    J, F = clips[0].shape[1:]
    N = {"1": 1, "3": 3, "lag": lag, "rf": rf, "rf + 5": rf + 5}[frames_pushed]
    S = 2
    src = np.random.RandomState(40 + N).standard_normal((N, S, J, F)).astype(np.float32)
    all_looks = list(range(lag))
    rig = PeekRig("cpu", S, rf, lag, J, F, all_looks[:_capi.STREAMS_PEEK_MAX], NONE, perm)
    for t in range(N):
        assert rig.tick(src[t], np.full(S, RESTART if t == 0 else PUSH, np.int32))["rc"] == 0
    peeked = {}
    for at in range(0, lag, _capi.STREAMS_PEEK_MAX):
        chunk = all_looks[at:at + _capi.STREAMS_PEEK_MAX]
        out = rig.peek(looks=chunk)
        assert out["rc"] == 0
        for i, L in enumerate(chunk):
            peeked[L] = (out["emit"][i].copy(), out["x"][i].copy(), out["x_mirror"][i].copy())
    for k in range(1, lag + 1):
        d = rig.tick(sc.garbage_frame(S, J, F), np.full(S, DRAIN, np.int32))
        emit, x, xm = peeked[lag - k]
        assert np.array_equal(d["emit"], emit) and (emit == (N - 1 - lag + k if N - 1 - lag + k >= 0 else -1)).all(), (k, d["emit"], emit)
        assert same_bits(d["x"], x) and same_bits(d["x_mirror"], xm), k


# ------------------------------------------------------------------------------------ the repaired ring

@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_behind_a_repair_the_previews_are_the_ring_as_it_stands(case):
    """r3d_debug_streams_repair_host in front of every step, gapped input (holes that are held, interpolated and back-filled): the
    previews are the windows of the ring at that tick - entries the repair rewrote included, which no caller-side history has."""
    scn = rc_cases.golden_scenario(case, "centred", "interp")
    rig = rc_cases.RepairRig("cpu", **scn["rig"])
    S, rf, lag, J, F, perm = rig.S, rig.rf, rig.lag, rig.J, rig.F, rig.perm
    looks = pc.looks_of(lag)
    K = len(looks)
    rewritten = previews = 0
    last_ring = None
    for t, (frame, act, conf) in enumerate(scn["ticks"]):
        tick = rig.tick(frame, act, conf)
        assert tick["rc"] == 0 and tick["rc_step"] == 0
        x, xm = np.full((K, S, rf, J, F), FILL, np.float32), np.full((K, S, rf, J, F), FILL, np.float32)
        emit, pst = np.full((K, S), pc.FILL_EMIT, np.int64), np.full((K, S), pc.FILL_STATUS, np.int32)
        before = rig._np("state")
        rc = _capi.debug_streams_peek_host(rig.t["state"].data_ptr(), S, rf, lag, J, F, looks, rig.t["action"].data_ptr(),
                                           rig.t["status"].data_ptr(), x.ctypes.data, xm.ctypes.data, perm, emit.ctypes.data, pst.ctypes.data)
        rig.arena.check()
        assert rc == 0 and np.array_equal(rig._np("state"), before)
        want_emit, want_pst = pc.expected(tick["heads"], act, tick["status"], looks, lag)
        assert np.array_equal(emit, want_emit) and np.array_equal(pst, want_pst), t
        ring = tick["ring"].view(np.float32)
        if last_ring is not None:          # ring entries other than the pushed slot that this tick's repair changed
            for s in range(S):
                c = int(tick["heads"]["count"][s])
                changed = np.nonzero((ring[s].view(np.uint32) != last_ring[s].view(np.uint32)).any(axis=(1, 2)))[0]
                rewritten += int(act[s] == PUSH and any(int(sl) != (c - 1) % rf for sl in changed))
        last_ring = ring.copy()
        for k in range(K):
            for s in range(S):
                p = int(emit[k, s])
                if p < 0:
                    assert (x[k, s] == FILL).all() and (xm[k, s] == FILL).all()
                    continue
                want = pc.window_of_ring(ring[s], p, int(tick["heads"]["count"][s]), rf, lag)
                assert same_bits(x[k, s], want) and same_bits(xm[k, s], pc.mirrored(want, perm)), (t, k, s)
                previews += 1
    assert rewritten > 0 and previews > 0


# ------------------------------------------------------------------------------------ the argument rules

def test_every_refusal_and_its_message():
    hooks = hooks_library()
    S, J, F, rf, lag, K = 3, 17, 3, 9, 4, 3
    state = np.zeros(S * 16 + S * rf * J * F * 4 + 8, np.uint8)
    state = state[(-state.ctypes.data) % 8:][:S * 16 + S * rf * J * F * 4]
    action, status = np.full(S, PUSH, np.int32), np.zeros(S, np.int32)
    x, xm = np.full((K, S, rf, J, F), FILL, np.float32), np.full((K, S, rf, J, F), FILL, np.float32)
    emit, pst = np.full((K, S), pc.FILL_EMIT, np.int64), np.full((K, S), pc.FILL_STATUS, np.int32)
    perm = sc.evaluate.mirror_permutation(J, [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16])
    base = dict(state=state.ctypes.data, S=S, rf=rf, lag=lag, J=J, F=F, looks=(0, 2, 3), n=None, action=action.ctypes.data,
                status=status.ctypes.data, x=x.ctypes.data, xm=xm.ctypes.data, perm=perm, emit=emit.ctypes.data, pst=pst.ctypes.data)

    def call(**kw):
        a = dict(base, **kw)
        return _capi.debug_streams_peek_host(a["state"], a["S"], a["rf"], a["lag"], a["J"], a["F"], a["looks"], a["action"], a["status"], a["x"],
                                             a["xm"], a["perm"], a["emit"], a["pst"], num_looks=a["n"])

    big = _capi.ENCODE_MAX_POINTS
    null, mir = "null pointer", "x_mirror_dev and mirror_perm go together"
    bad = [(dict(state=0), null), (dict(looks=None, n=1), null), (dict(status=0), null), (dict(x=0), null), (dict(emit=0), null), (dict(pst=0), null),
           (dict(S=0), "num_streams must be in 1..65535"), (dict(S=-1), "num_streams"), (dict(S=_capi.CLIPS_MAX + 1), "num_streams"),
           (dict(J=0, xm=0, perm=None), "num_joints must be in 1..17"), (dict(J=18, xm=0, perm=None), "num_joints"),
           (dict(rf=0, lag=0), "receptive_field must be >= 1"), (dict(rf=-3), "receptive_field"),
           (dict(lag=-1), "lag must be in 0..receptive_field - 1"), (dict(lag=rf), "lag must be"), (dict(F=1), "in_features must be 2 or 3"),
           (dict(F=4), "in_features"), (dict(lag=0, looks=(0,)), "lag is 0 (a causal model)"),
           (dict(looks=(), n=0), "num_looks must be in 1..8"), (dict(looks=tuple(range(9)), rf=27, lag=13), "num_looks must be in 1..8"),
           (dict(looks=(0,), n=-1), "num_looks"), (dict(looks=(0, 2, 4)), "looks[2] must be in 0..lag - 1 = 3 (got 4)"),
           (dict(looks=(-1, 2, 3)), "looks[0] must be in 0..lag - 1 = 3 (got -1)"), (dict(looks=(0, 2, 2)), "strictly increasing"),
           (dict(looks=(2, 0, 3)), "strictly increasing"), (dict(xm=0), mir), (dict(perm=None), mir), (dict(perm=[0] * J), "mirror_perm"),
           (dict(perm=[J] + perm[1:]), "mirror_perm"), (dict(rf=big // J + 1, lag=1, looks=(0,)), "must not exceed"),
           (dict(rf=2 ** 20, lag=1, S=200, looks=(0,)), "must not exceed"),
           (dict(rf=2 ** 20, lag=4, S=50), "num_looks * num_streams * receptive_field * num_joints"),      # 3 looks x 50 streams: too many
           (dict(state=state.ctypes.data + 4), "8-byte aligned"), (dict(emit=emit.ctypes.data + 4), "8-byte aligned")]
    for kw, message in bad:
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
        err = hooks.r3d_last_error().decode()
        assert err.startswith("r3d_debug_streams_peek_host: ") and message in err, (kw, err)
    assert (x == FILL).all() and (xm == FILL).all() and (emit == pc.FILL_EMIT).all() and (pst == pc.FILL_STATUS).all()      # nothing was written
    assert not state.any()
    assert call() == 0 and call(xm=0, perm=None) == 0 and call(action=0) == 0 and call(looks=(3,)) == 0 and call(looks=(0, 1, 2)) == 0
    with pytest.raises(_capi.Ray3DHipError):
        call(perm=perm[:-1])


def test_device_entry_point_refuses_before_any_device_call():
    """The same rules through r3d_streams_peek itself, on pointers that are never followed: R3D_ERR_ARG without a GPU."""
    lib = _capi.load()
    perm = (C.c_int32 * 17)(*range(17))
    three = (C.c_int32 * 3)(0, 6, 12)

    def call(state=BOGUS, S=6, rf=27, lag=13, J=17, F=3, looks=three, n=3, action=BOGUS, status=BOGUS, x=BOGUS, xm=BOGUS, perm=perm, emit=BOGUS,
             pst=BOGUS):
        return lib.r3d_streams_peek(state, S, rf, lag, J, F, looks, n, action, status, x, xm, perm, emit, pst, None)

    for kw in (dict(state=None), dict(looks=None), dict(status=None), dict(x=None), dict(emit=None), dict(pst=None), dict(S=0), dict(S=65536),
               dict(J=0), dict(J=18), dict(rf=0), dict(lag=-1), dict(lag=27), dict(lag=0), dict(F=4), dict(n=0), dict(n=9),
               dict(looks=(C.c_int32 * 3)(0, 6, 13)), dict(looks=(C.c_int32 * 3)(0, 6, 6)), dict(looks=(C.c_int32 * 3)(6, 0, 12)),
               dict(xm=None), dict(perm=None), dict(perm=(C.c_int32 * 17)(*([0] * 17))), dict(rf=2 ** 27, lag=1, n=1),
               dict(state=BOGUS + 4), dict(emit=BOGUS + 4)):
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
        assert lib.r3d_last_error().decode().startswith("r3d_streams_peek: ")
    with pytest.raises(_capi.Ray3DHipError, match="looks\\[1\\] must be in 0..lag - 1 = 12"):
        _capi.streams_peek(BOGUS, 6, 27, 13, 17, 3, (0, 13), BOGUS, BOGUS, BOGUS, None, None, BOGUS, BOGUS, 0)
