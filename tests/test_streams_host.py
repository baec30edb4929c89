"""CPU suite: the host side of r3d_streams_step (live streams lifted a frame at a time: a head and a ring of RF frames per stream) -
the layout of r3d_stream_head against the header, the exports, r3d_streams_state_bytes, the argument rules (all checked before any
device call: they run without a GPU), and the host hook r3d_debug_streams_step_host (the call's head rule, action step, slot index
and point routines on the CPU) against the REFERENCE's own windows (tests/golden/windows.npz: UnchunkedGenerator +
Trainer.eval_data_prepare), inside guard bands (tests/buffers_util.py).  tests/test_gpu_streams.py runs the kernel on the same
sequences."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, hooks_library

import streams_cases as sc
from streams_cases import DRAIN, FILL, IDLE, NONE, PUSH, RESTART, Rig, same_bits
from ray3d_amd import _capi

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed


# ------------------------------------------------------------------------------------ header, binding, exports

def test_struct_matches_header():
    body = re.search(r"typedef struct \{([^}]*)\} r3d_stream_head;\s*/\* 16 bytes", HDR).group(1)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", body)
    dt = _capi.stream_head_dtype()
    assert fields == [("int64_t", "count"), ("int64_t", "drained")] and [n for _, n in fields] == list(dt.names)
    assert [dt.fields[n][1] for n in dt.names] == [0, 8] and dt.itemsize == _capi.STREAM_HEAD_BYTES == 16
    for name, value in (("R3D_ENCODE_NONE", _capi.R3D_ENCODE_NONE), ("R3D_STREAM_IDLE", IDLE), ("R3D_STREAM_PUSH", PUSH),
                        ("R3D_STREAM_RESTART", RESTART), ("R3D_STREAM_DRAIN", DRAIN)):
        assert int(re.search(r"#define %s (\d+)" % name, HDR).group(1)) == value
    assert len({IDLE, PUSH, RESTART, DRAIN}) == 4
    assert _capi.R3D_ENCODE_NONE not in (_capi.R3D_ENCODE_RAY, _capi.R3D_ENCODE_INTRINSIC, _capi.R3D_ENCODE_SCREEN)


def test_exports_and_abi():
    assert {"r3d_streams_state_bytes", "r3d_streams_step"} <= set(_capi.EXPORTS) and "r3d_debug_streams_step_host" in _capi.HOOK_EXPORTS
    assert re.search(r"\bsize_t r3d_streams_state_bytes\(", HDR) and re.search(r"\bint r3d_streams_step\(", HDR)
    assert HDR.index("int r3d_debug_streams_step_host(") > HDR.index("#ifdef R3D_TEST_HOOKS") > HDR.index("int r3d_streams_step(")
    product = C.CDLL(_capi.LIB_PATH)
    assert hasattr(product, "r3d_streams_step") and hasattr(product, "r3d_streams_state_bytes")
    assert not hasattr(product, "r3d_debug_streams_step_host")
    hooks = hooks_library()
    assert hasattr(hooks, "r3d_streams_step") and hasattr(hooks, "r3d_streams_state_bytes") and hasattr(hooks, "r3d_debug_streams_step_host")
    assert hooks.r3d_abi_version() == 6 == _capi.ABI_VERSION and int(re.search(r"#define R3D_ABI_VERSION (\d+)", HDR).group(1)) == 6


def test_state_bytes_is_the_formula():
    for S, rf, J, F in ((1, 1, 1, 2), (6, 27, 17, 3), (6, 9, 14, 2), (1024, 243, 17, 3), (_capi.CLIPS_MAX, 243, 17, 3)):
        assert _capi.streams_state_bytes(S, rf, J, F) == S * 16 + S * rf * J * F * 4
    big = _capi.ENCODE_MAX_POINTS
    for bad in ((0, 27, 17, 3), (_capi.CLIPS_MAX + 1, 27, 17, 3), (6, 0, 17, 3), (6, 27, 0, 3), (6, 27, 18, 3), (6, 27, 17, 1), (6, 27, 17, 4),
                (1, big // 17 + 1, 17, 3), (200, 2 ** 20, 17, 3)):
        assert _capi.streams_state_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------------ the reference's windows

@pytest.mark.parametrize("shift", ["centred", "causal"])
@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_streams_reproduce_the_reference_windows(case, shift):
    """The six clips of windows.npz (1, 2, 5, 13, 14, 40 frames) as six streams side by side on a state nobody zeroed: RESTART,
    PUSH ..., DRAIN x lag, IDLE.  Every stream emits every frame 0 .. N - 1 once and in order; each emitted window is the
    reference's (UnchunkedGenerator's edge padding + eval_data_prepare) and its mirror the flipped sequence's, bit for bit; rows of
    streams that emit nothing keep their fill."""
    clips, rf, lag, perm, want, want_mirror = sc.golden_case(case, shift)
    J, F = clips[0].shape[1:]
    rig = Rig("cpu", len(clips), rf, lag, J, F, NONE, perm)
    ticks = sc.run_clips(rig, clips)
    assert len(ticks) - 1 == sc.TICKS[case, shift]
    nxt = [0] * len(clips)
    for t, out in enumerate(ticks):
        assert out["rc"] == 0 and (out["status"] == 0).all(), t
        for s in range(len(clips)):
            n = int(out["emit"][s])
            if n < 0:
                assert n == -1 and (out["x"][s] == FILL).all() and (out["x_mirror"][s] == FILL).all(), (t, s)
                continue
            assert n == nxt[s], (t, s, n)
            nxt[s] += 1
            assert same_bits(out["x"][s], want[s][n]) and same_bits(out["x_mirror"][s], want_mirror[s][n]), (t, s, n)
    assert nxt == [c.shape[0] for c in clips]
    assert (ticks[-1]["emit"] == -1).all() and np.array_equal(ticks[-1]["state"], ticks[-2]["state"])      # the all-IDLE tick
    heads = rig.state()[0]
    assert heads["count"].tolist() == nxt and (heads["drained"] == lag).all()


def test_without_a_mirror_and_on_a_zeroed_state():
    """x_mirror_dev / mirror_perm NULL: the same plain windows; an all-zero state is freshly reset streams: PUSH without RESTART."""
    clips, rf, lag, perm, want, _ = sc.golden_case("rf9", "centred")
    J, F = clips[0].shape[1:]
    rig = Rig("cpu", len(clips), rf, lag, J, F, NONE, None, zero_state=True)
    lengths = [c.shape[0] for c in clips]
    actions, frame_of = sc.schedule(lengths, lag)
    actions[0] = PUSH
    got = [[] for _ in clips]
    for t in range(actions.shape[0]):
        frame = sc.garbage_frame(len(clips), J, F)
        for s, c in enumerate(clips):
            if frame_of[t, s] >= 0:
                frame[s] = c[frame_of[t, s]]
        out = rig.tick(frame, actions[t])
        assert out["rc"] == 0 and (out["status"] == 0).all() and (out["x_mirror"] == FILL).all()
        for s in range(len(clips)):
            if out["emit"][s] >= 0:
                got[s].append(out["x"][s])
    for s in range(len(clips)):
        assert same_bits(np.stack(got[s]), want[s])


# ------------------------------------------------------------------------------------ refusals, restart, payloads

def _warm(rig, frames_per_stream, seed=3):
    """RESTART + PUSHes: stream s gets frames_per_stream[s] frames (0: it stays IDLE, its state as it was)."""
    rng = np.random.RandomState(seed)
    for t in range(max(frames_per_stream)):
        act = np.array([IDLE if t >= n else (RESTART if t == 0 else PUSH) for n in frames_per_stream], np.int32)
        out = rig.tick(rng.standard_normal((rig.S, rig.J, rig.width)).astype(np.float32), act)
        assert out["rc"] == 0 and (out["status"] == 0).all()


def _twin(J=14, F=2, rf=9, lag=4, frames=(6, 5, 7)):
    a, b = (Rig("cpu", 3, rf, lag, J, F, NONE, sc.evaluate.mirror_permutation(J, [4, 5, 6], [1, 2, 3])) for _ in range(2))
    _warm(a, frames), _warm(b, frames)
    assert np.array_equal(a.state()[2], b.state()[2])
    return a, b


def _refused_alone(a, b, s, action, frame_seed=9):
    """Stream s of rig `a` gets `action`, of rig `b` IDLE; the neighbours PUSH in both.  Stream s: status 1, emit -1, its state and
    rows untouched; the neighbours: what they are without it."""
    frame = np.random.RandomState(frame_seed).standard_normal((a.S, a.J, a.width)).astype(np.float32)
    act_a, act_b = np.full(a.S, PUSH, np.int32), np.full(a.S, PUSH, np.int32)
    act_a[s], act_b[s] = action, IDLE
    before = a.state()[2]
    ra, rb = a.tick(frame, act_a), b.tick(frame, act_b)
    assert ra["rc"] == 0 and ra["status"][s] == 1 and ra["emit"][s] == -1
    assert (ra["x"][s] == FILL).all() and (ra["x_mirror"][s] == FILL).all()
    others = [k for k in range(a.S) if k != s]
    assert (ra["status"][others] == 0).all() and np.array_equal(ra["emit"][others], rb["emit"][others])
    assert same_bits(ra["x"][others], rb["x"][others]) and same_bits(ra["x_mirror"][others], rb["x_mirror"][others])
    (ha, ringa, rawa), (hb, ringb, _) = a.state(), b.state()
    assert np.array_equal(rawa[s * 16:(s + 1) * 16], before[s * 16:(s + 1) * 16])                   # the head
    assert same_bits(ringa[s], before[a.S * 16:].view(np.float32).reshape(ringa.shape)[s])         # the ring
    assert np.array_equal(ha[others], hb[others]) and same_bits(ringa[others], ringb[others])


@pytest.mark.parametrize("action", [4, -1, 7, 2 ** 31 - 1, -2 ** 31])
def test_an_unknown_action_is_refused(action):
    a, b = _twin()
    _refused_alone(a, b, 1, action)


def test_push_after_a_drain_began_is_refused_until_restart():
    a, b = _twin()
    idle = np.full(3, IDLE, np.int32)
    drain1 = idle.copy()
    drain1[1] = DRAIN
    frame = sc.garbage_frame(3, a.J, a.width)
    for rig in (a, b):
        out = rig.tick(frame, drain1)
        assert out["status"].tolist() == [0, 0, 0] and out["emit"][1] == 5 - 1 - 4 + 1 and rig.state()[0]["drained"].tolist() == [0, 1, 0]
    _refused_alone(a, b, 1, PUSH)
    new = np.random.RandomState(4).standard_normal((3, a.J, a.width)).astype(np.float32)
    act = idle.copy()
    act[1] = RESTART
    out = a.tick(new, act)
    assert out["status"].tolist() == [0, 0, 0] and out["emit"].tolist() == [-1, -1, -1]
    assert a.state()[0][1].tolist() == (1, 0) and same_bits(a.state()[1][1, 0], new[1])


@pytest.mark.parametrize("action", [PUSH, DRAIN])
@pytest.mark.parametrize("head", ["count -1", "drained lag + 1", "count 2^62 + 1", "drained -1", "count INT64_MIN"])
def test_a_corrupted_head_is_refused(head, action):
    a, b = _twin()
    lag = a.lag
    count, drained = {"count -1": (-1, 0), "drained lag + 1": (5, lag + 1), "count 2^62 + 1": (2 ** 62 + 1, 0), "drained -1": (5, -1),
                      "count INT64_MIN": (-2 ** 63, 0)}[head]
    for rig in (a, b):
        rig.set_head(1, count, drained)
    _refused_alone(a, b, 1, action)
    assert a.state()[0][1].tolist() == (count, drained)


def test_a_full_counter_refuses_push_and_the_last_count_still_works():
    a, b = _twin()
    for rig in (a, b):
        rig.set_head(1, 2 ** 62, 0)
    _refused_alone(a, b, 1, PUSH)
    for rig in (a, b):
        rig.set_head(1, 2 ** 62 - 1, 0)
    frame = np.random.RandomState(2).standard_normal((3, a.J, a.width)).astype(np.float32)
    out = a.tick(frame, np.full(3, PUSH, np.int32))
    assert out["status"].tolist() == [0, 0, 0] and out["emit"][1] == 2 ** 62 - 1 - a.lag and a.state()[0][1].tolist() == (2 ** 62, 0)
    assert same_bits(a.state()[1][1, (2 ** 62 - 1) % a.rf], frame[1])


@pytest.mark.parametrize("lag", [0, 4])
def test_restart_mid_stream_forgets_the_old_frames(lag):
    """RESTART after six frames: the first window afterwards - at once for a causal stream, after the drain for a centred one - is RF
    copies of the new frame."""
    J, F, rf = 14, 2, 9
    rig = Rig("cpu", 2, rf, lag, J, F, NONE, None)
    _warm(rig, (6, 6))
    new = np.random.RandomState(8).standard_normal((2, J, F)).astype(np.float32)
    out = rig.tick(new, np.array([RESTART, IDLE], np.int32))
    assert out["status"].tolist() == [0, 0] and rig.state()[0][0].tolist() == (1, 0)
    for _ in range(lag):
        assert out["emit"].tolist() == [-1, -1] and (out["x"] == FILL).all()
        out = rig.tick(sc.garbage_frame(2, J, F), np.array([DRAIN, IDLE], np.int32))
    assert out["emit"].tolist() == [0, -1] and (out["x"][1] == FILL).all()
    assert same_bits(out["x"][0], np.broadcast_to(new[0], (rf, J, F)))
    out = rig.tick(sc.garbage_frame(2, J, F), np.array([DRAIN, DRAIN], np.int32))      # stream 0 has nothing left; stream 1 drains
    assert out["status"].tolist() == [0, 0] and out["emit"][0] == -1 and (out["emit"][1] == 6 - lag if lag else out["emit"][1] == -1)


def test_nan_and_inf_bit_patterns_travel_unchanged():
    J, F, rf, lag = 17, 3, 27, 0
    perm = sc.evaluate.mirror_permutation(J, [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16])
    rig = Rig("cpu", 1, rf, lag, J, F, NONE, perm)
    frames = np.random.RandomState(1).standard_normal((3, 1, J, F)).astype(np.float32)
    fb = frames.view(np.uint32)
    fb[1, 0, 2, 0], fb[1, 0, 16, 1], fb[2, 0, 0, 0], fb[2, 0, 5, 2], fb[0, 0, 4, 0] = 0x7FC12345, 0xFFC00001, 0x7F800001, 0xFF800000, 0x7F800000
    for t in range(3):
        out = rig.tick(frames[t], np.array([RESTART if t == 0 else PUSH], np.int32))
    want = np.concatenate([np.repeat(frames[:1, 0], rf - 2, axis=0), frames[1:, 0]], axis=0)
    assert out["emit"].tolist() == [2] and same_bits(out["x"][0], want)
    wm = want[:, perm, :].copy()
    wm.view(np.uint32)[:, :, 0] ^= np.uint32(0x80000000)
    assert same_bits(out["x_mirror"][0], wm)
    xb, mb = out["x"].view(np.uint32), out["x_mirror"].view(np.uint32)
    for bits in (0x7FC12345, 0xFFC00001, 0x7F800001, 0xFF800000, 0x7F800000):
        assert (xb == bits).any()
    assert (mb == 0xFFC12345).any() and (mb == 0xFF800001).any() and (mb == 0xFF800000).any() and (mb == 0xFFC00001).any()
    assert not (xb == 0x7FC00BAD).any()


# ------------------------------------------------------------------------------------ the pixel encodings

@pytest.mark.parametrize("encoding,rf,lag", [("ray", 27, 13), ("intrinsic", 9, 0), ("screen", 9, 4)])
def test_ring_rows_are_what_clips_encode_writes(encoding, rf, lag):
    """Pixels through a distorted H36M camera row: the ring holds, bit for bit, what r3d_debug_clips_encode_host writes for the same
    pixels and row (pads 0), and the windows are gathered from it."""
    from test_clips_encode_host import cameras, pixels, run_hook
    J, S, N = 17, 2, 12
    enc = sc.evaluate.ENCODINGS[encoding]
    F = _capi.ENCODE_FLOATS[enc]
    cams = [cameras()[1], cameras()[2]]
    rows = np.stack([c.cam_row(distortion=True) for c in cams])
    px = pixels("streams.%s" % encoding, (S, N, J, 2))
    rig = Rig("cpu", S, rf, lag, J, F, enc, None, cam_rows=rows)
    wins = [[] for _ in range(S)]
    for t in range(N + lag):
        act = np.full(S, RESTART if t == 0 else (PUSH if t < N else DRAIN), np.int32)
        out = rig.tick(px[:, t] if t < N else sc.garbage_frame(S, J, 2), act)
        assert out["rc"] == 0 and (out["status"] == 0).all()
        for s in range(S):
            if out["emit"][s] >= 0:
                wins[s].append(out["x"][s])
    ring = rig.state()[1]
    for s in range(S):
        table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
        table[0]["n_frames"], table[0]["cam"] = N, rows[s]
        rc, want, _, status = run_hook(J, encoding, table, px[s], N, N, mirror=False)
        assert rc == 0 and status.tolist() == [0]
        for f in range(max(0, N - rf), N):
            assert same_bits(ring[s, f % rf], want[f]), (s, f)
        pad_front = rf - 1 - lag
        padded = np.concatenate([np.repeat(want[:1], pad_front, axis=0), want, np.repeat(want[-1:], lag, axis=0)], axis=0)
        assert len(wins[s]) == N
        for n in range(N):
            assert same_bits(wins[s][n], padded[n:n + rf]), (s, n)


# ------------------------------------------------------------------------------------ the argument rules

def test_argument_rules():
    hooks = hooks_library()
    S, J, F, rf, lag = 3, 17, 3, 9, 4
    state = np.zeros(S * 16 + S * rf * J * F * 4 + 8, np.uint8)
    state = state[(-state.ctypes.data) % 8:][:S * 16 + S * rf * J * F * 4]
    frame = np.zeros((S, J, F), np.float32)
    cam = np.ones((S, 16), np.float64)
    action = np.full(S, RESTART, np.int32)
    x, xm = np.full((S, rf, J, F), FILL, np.float32), np.full((S, rf, J, F), FILL, np.float32)
    emit, status = np.full(S, sc.FILL_EMIT, np.int64), np.full(S, sc.FILL_STATUS, np.int32)
    perm = sc.evaluate.mirror_permutation(J, [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16])
    base = dict(state=state.ctypes.data, S=S, rf=rf, lag=lag, J=J, F=F, enc=NONE, frame=frame.ctypes.data, cam=cam.ctypes.data,
                action=action.ctypes.data, x=x.ctypes.data, xm=xm.ctypes.data, perm=perm, emit=emit.ctypes.data, status=status.ctypes.data)

    def call(**kw):
        a = dict(base, **kw)
        return _capi.debug_streams_step_host(a["state"], a["S"], a["rf"], a["lag"], a["J"], a["F"], a["enc"], a["frame"], a["cam"], a["action"],
                                             a["x"], a["xm"], a["perm"], a["emit"], a["status"])

    big = _capi.ENCODE_MAX_POINTS
    ray, intr, scr = _capi.R3D_ENCODE_RAY, _capi.R3D_ENCODE_INTRINSIC, _capi.R3D_ENCODE_SCREEN
    bad = [dict(state=0), dict(frame=0), dict(action=0), dict(x=0), dict(emit=0), dict(status=0),
           dict(S=0), dict(S=-1), dict(S=_capi.CLIPS_MAX + 1), dict(J=0, xm=0, perm=None), dict(J=18, xm=0, perm=None), dict(rf=0, lag=0), dict(rf=-3),
           dict(lag=-1), dict(lag=rf), dict(lag=rf + 5), dict(enc=4), dict(enc=-1), dict(F=1), dict(F=4), dict(enc=ray, F=2), dict(enc=intr, F=3),
           dict(enc=scr, F=3), dict(enc=ray, cam=0), dict(enc=intr, F=2, cam=0), dict(enc=scr, F=2, cam=0), dict(xm=0), dict(perm=None),
           dict(perm=[0] * J), dict(perm=[J] + perm[1:]), dict(perm=[-1] + perm[1:]), dict(rf=big // J + 1, lag=0), dict(rf=2 ** 20, lag=0, S=200),
           dict(state=state.ctypes.data + 4), dict(emit=emit.ctypes.data + 4), dict(enc=ray, cam=cam.ctypes.data + 4)]
    for kw in bad:
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
        assert hooks.r3d_last_error()
    assert (x == FILL).all() and (xm == FILL).all() and (emit == sc.FILL_EMIT).all() and (status == sc.FILL_STATUS).all()      # nothing was written
    assert not state.any()
    assert call() == 0 and call(xm=0, perm=None) == 0 and call(cam=0) == 0 and call(enc=ray) == 0 and call(enc=intr, F=2) == 0
    assert call(lag=0) == 0 and call(lag=rf - 1) == 0
    with pytest.raises(_capi.Ray3DHipError):
        call(perm=perm[:-1])


def test_device_entry_point_refuses_before_any_device_call():
    """The same rules through r3d_streams_step itself, on pointers that are never followed: R3D_ERR_ARG without a GPU."""
    lib = _capi.load()
    perm = (C.c_int32 * 17)(*range(17))

    def call(state=BOGUS, S=6, rf=27, lag=13, J=17, F=3, enc=NONE, frame=BOGUS, cam=BOGUS, action=BOGUS, x=BOGUS, xm=BOGUS, perm=perm, emit=BOGUS,
             status=BOGUS):
        return lib.r3d_streams_step(state, S, rf, lag, J, F, enc, frame, cam, action, x, xm, perm, emit, status, None)

    for kw in (dict(state=None), dict(frame=None), dict(action=None), dict(x=None), dict(emit=None), dict(status=None), dict(S=0), dict(S=65536),
               dict(J=0), dict(J=18), dict(rf=0), dict(lag=-1), dict(lag=27), dict(enc=4), dict(F=4), dict(enc=0, F=2), dict(enc=1), dict(enc=2),
               dict(enc=0, cam=None), dict(xm=None), dict(perm=None), dict(perm=(C.c_int32 * 17)(*([0] * 17))), dict(rf=2 ** 27, lag=0),
               dict(rf=2 ** 20, lag=0, S=200), dict(state=BOGUS + 4)):
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
    with pytest.raises(_capi.Ray3DHipError, match="mirror_perm"):
        _capi.streams_step(BOGUS, 6, 27, 13, 17, 3, NONE, BOGUS, None, BOGUS, BOGUS, BOGUS, [0] * 17, BOGUS, BOGUS, 0)
