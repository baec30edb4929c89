"""CPU suite: the host side of r3d_streams_repair (live streams that survive dropped keypoints) - the exports, r3d_streams_track_bytes,
the argument rules (all checked before any device call: they run without a GPU), and the host hook r3d_debug_streams_repair_host
followed by r3d_debug_streams_step_host, tick by tick and bit for bit, against a NumPy restatement of the header's rules
(tests/streams_repair_cases.py) and against the REFERENCE: the restatement's window builder reproduces tests/golden/windows.npz
(UnchunkedGenerator + Trainer.eval_data_prepare), a stream without gaps stays what it is, and a repaired stream's windows are the
reference-built windows of the clip repaired offline.  Every buffer lies inside guard bands (tests/buffers_util.py), checked after
both calls of every tick.  tests/test_gpu_streams_repair.py runs the kernel on the same scenarios."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, hooks_library

import streams_cases as sc
import streams_repair_cases as rc
from streams_cases import DRAIN, IDLE, NONE, PUSH, RESTART
from streams_repair_cases import FILL_BITS, QNAN, bits, same_bits
from ray3d_amd import _capi

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed
GOLDEN_PARAMS = [(case, shift) for case in ("rf27", "rf9") for shift in ("centred", "causal")]


def follow(scn, model, results):
    """Every tick of a played scenario equals the restatement in everything the two calls write: frame_out (rows of streams that
    take no push keep their fill), the ring after the repair and after the step, age, last and missing, synthetic, the heads (the
    repair call writes none), the step's x / x_mirror / emit / status.  -> per stream the emitted (n, x, x_mirror, synthetic)."""
    S = model.S
    emitted = [[] for _ in range(S)]
    for t, ((frame, act, conf), out) in enumerate(zip(scn["ticks"], results)):
        ring0, age0, last0, missing0 = model.ring.copy(), model.age.copy(), model.last.copy(), model.missing.copy()
        heads0 = list(zip(model.count, model.drained))
        fo, syn, pushed = model.repair(frame, act, conf)
        assert out["rc"] == 0, t
        for s in range(S):
            if pushed[s]:
                assert np.array_equal(out["frame_out"][s], fo[s]), (t, s)
            else:                            # nothing of the stream's track, ring or frame_out row is written
                assert (out["frame_out"][s] == FILL_BITS).all(), (t, s)
                assert np.array_equal(out["ring_r"][s], ring0[s]) and np.array_equal(out["age"][s], age0[s]), (t, s)
                assert np.array_equal(out["last"][s], last0[s]) and np.array_equal(out["missing"][s], missing0[s]), (t, s)
        assert out["synthetic"].tolist() == syn.tolist(), (t, out["synthetic"], syn)
        assert np.array_equal(out["ring_r"], model.ring), t
        assert np.array_equal(out["age"], model.age) and np.array_equal(out["last"], model.last), t
        assert np.array_equal(out["missing"], model.missing), t
        assert out["heads_r"].tolist() == heads0, t
        x, xm, emit, status = model.step(fo, act)
        assert out["rc_step"] == 0 and out["emit"].tolist() == emit.tolist() and out["status"].tolist() == status.tolist(), t
        for s in range(S):
            if s in x:
                assert np.array_equal(out["x"][s], x[s]), (t, s)
                if model.perm is not None:
                    assert np.array_equal(out["x_mirror"][s], xm[s]), (t, s)
                emitted[s].append((int(emit[s]), out["x"][s], out["x_mirror"][s], int(out["synthetic"][s])))
            else:
                assert (out["x"][s] == FILL_BITS).all() and (out["x_mirror"][s] == FILL_BITS).all(), (t, s)
        assert np.array_equal(out["ring"], model.ring), t
        assert out["heads"].tolist() == list(zip(model.count, model.drained)), t
    return emitted


def mask_of(observed_row):
    return sum(1 << j for j, o in enumerate(observed_row) if not o)


def final_ring_is(results, s, frames, rf):
    """The ring of stream s after the last tick holds `frames` (N, J, F) bits: its last min(N, RF) frames at slot frame % RF."""
    N = frames.shape[0]
    ring = results[-1]["ring"][s]
    return all(np.array_equal(ring[f % rf], frames[f]) for f in range(max(0, N - rf), N))


# ------------------------------------------------------------------------------------ header, binding, exports

def test_exports_header_and_abi():
    assert {"r3d_streams_track_bytes", "r3d_streams_repair"} <= set(_capi.EXPORTS) and "r3d_debug_streams_repair_host" in _capi.HOOK_EXPORTS
    assert re.search(r"\bsize_t r3d_streams_track_bytes\(", HDR) and re.search(r"\bint r3d_streams_repair\(", HDR)
    assert HDR.index("int r3d_debug_streams_repair_host(") > HDR.index("#ifdef R3D_TEST_HOOKS") > HDR.index("int r3d_streams_repair(")
    for word in (r"int32\s+age\[S\]\[J\]", r"float32\s+last\[S\]\[J\]\[width\]", r"uint32\s+missing\[S\]\[RF\]", "THE WHOLE BOUNDS STORY"):
        assert re.search(word, HDR[HDR.index("one call in front of a tick's r3d_streams_step"):]), word        # the layout is documented
    product = C.CDLL(_capi.LIB_PATH)
    assert hasattr(product, "r3d_streams_repair") and hasattr(product, "r3d_streams_track_bytes")
    assert not hasattr(product, "r3d_debug_streams_repair_host")
    hooks = hooks_library()
    assert hasattr(hooks, "r3d_streams_repair") and hasattr(hooks, "r3d_debug_streams_repair_host")
    assert hooks.r3d_abi_version() == 6 == _capi.ABI_VERSION            # no existing struct changed


def test_track_bytes_is_the_formula():
    for S, rf, J, W in ((1, 1, 1, 2), (6, 27, 17, 3), (6, 9, 14, 2), (3, 9, 17, 3), (1024, 243, 17, 3), (_capi.CLIPS_MAX, 243, 17, 2)):
        assert _capi.streams_track_bytes(S, rf, J, W) == (4 * S * (J + J * W + rf) + 7) // 8 * 8
    big = _capi.ENCODE_MAX_POINTS
    for bad in ((0, 27, 17, 3), (_capi.CLIPS_MAX + 1, 27, 17, 3), (6, 0, 17, 3), (6, 27, 0, 3), (6, 27, 18, 3), (6, 27, 17, 1), (6, 27, 17, 4),
                (1, big // 17 + 1, 17, 3), (200, 2 ** 20, 17, 3)):
        assert _capi.streams_track_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------------ 1: the window builder is the reference's

@pytest.mark.parametrize("case,shift", GOLDEN_PARAMS)
def test_window_builder_is_the_reference(case, shift):
    """Edge padding plus slicing of a golden clip is rf*_eval_s*_f0 of windows.npz, and of the flipped clip rf*_eval_s*_f1, bit for
    bit: every later expectation stands on reference_windows()."""
    clips, rf, lag, perm, want, want_mirror = sc.golden_case(case, shift)
    for c, w, wm in zip(clips, want, want_mirror):
        assert same_bits(rc.reference_windows(c, rf, lag), w)
        assert np.array_equal(rc.reference_windows(rc.mirrored(c, perm), rf, lag), bits(wm))


# ------------------------------------------------------------------------------------ 2: no gaps, no change

@pytest.mark.parametrize("kind", ["nogap0", "nogapK", "nogapmax"])
@pytest.mark.parametrize("case,shift", GOLDEN_PARAMS)
def test_no_gaps_no_change(case, shift, kind):
    scn, model, results = rc.host_run("golden", case, shift, kind)
    ring_before = [None] + [r["ring"] for r in results[:-1]]
    for t, ((frame, act, _), out) in enumerate(zip(scn["ticks"], results)):
        pushing = np.isin(act, (PUSH, RESTART))
        assert np.array_equal(out["frame_out"][pushing], bits(frame)[pushing]), t        # frame_out has the bits of frame
        assert not out["synthetic"].any(), t
        if t:
            assert np.array_equal(out["ring_r"], ring_before[t]), t                       # the repair call leaves the ring as it found it
    emitted = follow(scn, model, results)
    for s, c in enumerate(scn["clips"]):                                                  # ... and the step emits the golden windows
        assert [e[0] for e in emitted[s]] == list(range(c.shape[0]))
        for n, x, xm, _ in emitted[s]:
            assert np.array_equal(x, bits(scn["want"][s][n])) and np.array_equal(xm, bits(scn["want_mirror"][s][n])), (s, n)


# ------------------------------------------------------------------------------------ 3: hold

@pytest.mark.parametrize("case,shift", GOLDEN_PARAMS)
def test_hold(case, shift):
    """max_gap = 0 over every gap shape (rc.hold_holes): every tick equals the restatement; the synthetic word of an emitted frame
    is the mask of its joints that were not observed; and for the clips whose leading gaps are shorter than lag (or that have
    none, or whose joint never shows) every emitted window is the reference-built window of the forward- / back-filled clip."""
    scn, model, results = rc.host_run("golden", case, shift, "hold")
    rf, lag = model.rf, model.lag
    emitted = follow(scn, model, results)
    compared = 0
    for s, (c, obs) in enumerate(zip(scn["clips"], scn["observed"])):
        N = c.shape[0]
        assert [e[0] for e in emitted[s]] == list(range(N))
        assert [e[3] for e in emitted[s]] == [mask_of(obs[n]) for n in range(N)], s
        held = rc.offline_repair(bits(c), obs, 0)
        assert final_ring_is(results, s, held, rf), s
        if all(L == 0 or L < lag or L == N for L in rc.leading_gaps(obs)):
            want = rc.reference_windows(held, rf, lag)
            for n, x, xm, _ in emitted[s]:
                assert np.array_equal(x, want[n]) and np.array_equal(xm, rc.mirrored(want[n], model.perm)), (s, n)
            compared += int(not obs.all())
    assert compared >= (3 if lag else 2), compared           # gapped clips among them (causal: those without a leading gap)


# ------------------------------------------------------------------------------------ 4: interpolation

@pytest.mark.parametrize("case,shift", GOLDEN_PARAMS)
def test_interpolation(case, shift):
    """Gaps of 1, max_gap and max_gap + 1 frames, one across ring slot RF - 1 -> 0, one that closes while c < RF: every tick equals
    the restatement; the rewritten entries are the formula's bits and `missing` keeps its bits; at the end every ring is the clip
    repaired offline, and the windows the drain emits for the last `lag` frames of the clips whose gaps all close are the
    reference-built windows of that clip."""
    scn, model, results = rc.host_run("golden", case, shift, "interp")
    rf, lag, K = model.rf, model.lag, rc.MAX_GAP[case]
    emitted = follow(scn, model, results)
    # the gap of K frames of stream 5, joint 2 (frames 14 .. 14 + K - 1) closes at the tick that pushes frame 14 + K
    c5 = bits(scn["clips"][5])
    a, e, t = c5[13, 2], c5[14 + K, 2], 14 + K
    before, after = results[t - 1]["ring"][5], results[t]["ring_r"][5]
    for m in range(1, K + 1):
        f = 13 + m
        assert np.array_equal(before[f % rf, 2], a)                                          # held until then
        assert after[f % rf, 2].tolist() == [rc.interp_bits(a[i], e[i], m, K) for i in range(c5.shape[2])]
        assert not np.array_equal(after[f % rf, 2], a)
        assert results[t]["missing"][5, f % rf] & (1 << 2)                                   # synthetic, however good the repair
    for s, (c, obs) in enumerate(zip(scn["clips"], scn["observed"])):
        N = c.shape[0]
        assert [e[3] for e in emitted[s]] == [mask_of(obs[n]) for n in range(N)], s
        fixed = rc.offline_repair(bits(c), obs, K)
        assert final_ring_is(results, s, fixed, rf), s
        if s == 3:                           # the gap of K + 1 frames stays held
            assert all(np.array_equal(fixed[f, 5], bits(c)[2, 5]) for f in range(3, 4 + K))
        if s in (4, 5):
            assert obs[-1].all()
            want = rc.reference_windows(fixed, rf, lag)
            for n, x, xm, _ in emitted[s][N - lag:] if lag else []:
                assert np.array_equal(x, want[n]) and np.array_equal(xm, rc.mirrored(want[n], model.perm)), (s, n)


# ------------------------------------------------------------------------------------ 5: the pixel encodings

@pytest.mark.parametrize("encoding", [c[0] for c in rc.PIXEL_CASES])
def test_pixel_encodings(encoding):
    """RAY through a distorted camera row, INTRINSIC and SCREEN: hold happens in PIXEL space (frame_out of a missing joint is the
    last observed pixel pair), interpolation in ENCODED space (the final ring is the offline repair of the encoded clip), and the
    endpoint e has the bits the step pushes for the same pixel (r3d_debug_clips_encode_host)."""
    scn, model, results = rc.host_run("pixels", encoding)
    rf, K = model.rf, scn["rig"]["max_gap"]
    follow(scn, model, results)
    for s, (c, obs) in enumerate(zip(scn["clips"], scn["observed"])):
        N, px = c.shape[0], bits(c)
        for t in range(N):
            for j in range(c.shape[1]):
                seen = np.nonzero(obs[:t + 1, j])[0]
                want = px[seen[-1], j] if seen.size else np.full(2, QNAN, np.uint32)
                assert np.array_equal(results[t]["frame_out"][s, j], want), (s, t, j)
        enc = np.stack([[scn["encode"](s, px[t, j]) if obs[t, j] else np.zeros(model.F, np.uint32) for j in range(c.shape[1])] for t in range(N)])
        assert final_ring_is(results, s, rc.offline_repair(enc, obs, K), rf), s
    ring0 = results[-1]["ring"][0]
    assert len({tuple(ring0[f % rf, 9]) for f in range(7, 8 + K)}) == K + 1      # frame 7 and the K frames behind it: a gap was interpolated


# ------------------------------------------------------------------------------------ 6: confidences

def test_confidences():
    """A threshold at, one float below and above min_conf, and a NaN confidence: a finite keypoint below the threshold is treated
    exactly as a missing one - the run with confidences has the bits of the run whose rejected keypoints are NaN."""
    scn, model, results = rc.host_run("conf", 0)
    _, _, twin = rc.host_run("conf", 1)
    follow(scn, model, results)
    rc.agree(results, twin, "confidences against NaN keypoints")
    assert any(r["synthetic"].any() for r in results)
    at = np.float32(scn["rig"]["min_conf"])
    for t, ((_, act, conf), out) in enumerate(zip(scn["ticks"], results)):
        for s in np.nonzero(np.isin(act, (PUSH, RESTART)))[0]:
            slot = (int(out["heads"]["count"][s]) - 1) % model.rf
            assert int(out["missing"][s, slot]) == mask_of(conf[s] >= at), (t, s)        # == at: observed; NaN: not


# ------------------------------------------------------------------------------------ 7: actions

def test_actions_on_a_poisoned_state_and_track():
    scn, model, results = rc.host_run("actions")
    emitted = follow(scn, model, results)
    st = [r["status"].tolist() for r in results]
    assert st[0] == [0, 0, 0, 1, 0, 0] and st[2] == [0, 0, 1, 0, 0, 0] and st[3] == [0, 0, 0, 0, 0, 1] and st[7] == [1, 0, 0, 1, 0, 0]
    # a poisoned track (negative ages) under a valid head, PUSHed without a RESTART: the ages read as 0; joint 1 comes late
    assert results[0]["frame_out"][4, 1].tolist() == [QNAN] * model.W and results[0]["age"][4, 1] == 0 and results[0]["age"][4, 0] == 1
    assert results[0]["missing"][4, 3] == 2 and results[1]["missing"][4, 4] == 2
    # DRAINs that emit report the emitted frame's mask; every other stream without a push reports 0
    assert results[6]["emit"].tolist()[4] == 4 and results[6]["synthetic"][4] == 2
    assert results[6]["emit"].tolist()[0] == 2 and results[6]["synthetic"][0] == 0
    assert results[6]["synthetic"][2] == 0 and results[7]["synthetic"][0] == 0 and results[7]["synthetic"][3] == 0
    # RESTART clears the track, whatever it held
    r8 = results[8]
    assert r8["age"][0].tolist() == [0 if j in (4, 5) else 1 for j in range(model.J)]
    assert r8["missing"][0].tolist() == [(1 << 4) | (1 << 5)] + [0] * (model.rf - 1)
    assert (r8["last"][0, [4, 5]] == 0).all()
    assert sum(len(e) for e in emitted) > 10


# ------------------------------------------------------------------------------------ 8: the argument rules

def _host_buffers(S, J, F, rf):
    def aligned(nbytes):
        raw = np.zeros(nbytes + 8, np.uint8)
        return raw[(-raw.ctypes.data) % 8:][:nbytes]
    state, track = aligned(S * 16 + S * rf * J * F * 4), aligned((4 * S * (J + J * F + rf) + 7) // 8 * 8)
    return dict(state=state, track=track, frame=np.zeros((2 * S, J, F), np.float32), conf=np.ones((S, J), np.float32),
                cam=np.ones((S, 16), np.float64), action=np.full(S, RESTART, np.int32), out=np.full((S, J, F), -7.0, np.float32),
                syn=np.full(S, 77, np.uint32))


def test_argument_rules():
    hooks = hooks_library()
    S, J, F, rf, lag = 3, 17, 3, 9, 4
    b = _host_buffers(S, J, F, rf)
    p = {k: v.ctypes.data for k, v in b.items()}
    base = dict(state=p["state"], track=p["track"], S=S, rf=rf, lag=lag, J=J, F=F, enc=NONE, frame=p["frame"], conf=p["conf"], min_conf=0.5,
                cam=p["cam"], action=p["action"], max_gap=2, out=p["out"], syn=p["syn"])

    def call(**kw):
        a = dict(base, **kw)
        return _capi.debug_streams_repair_host(a["state"], a["track"], a["S"], a["rf"], a["lag"], a["J"], a["F"], a["enc"], a["frame"], a["conf"],
                                               a["min_conf"], a["cam"], a["action"], a["max_gap"], a["out"], a["syn"])

    big = _capi.ENCODE_MAX_POINTS
    ray, intr, scr = _capi.R3D_ENCODE_RAY, _capi.R3D_ENCODE_INTRINSIC, _capi.R3D_ENCODE_SCREEN
    row = S * J * F * 4
    bad = [  # what r3d_streams_step refuses for the arguments the two share
        (dict(state=0), "null"), (dict(frame=0), "null"), (dict(action=0), "null"), (dict(S=0), "num_streams"), (dict(S=-1), "num_streams"),
        (dict(S=_capi.CLIPS_MAX + 1), "num_streams"), (dict(J=0), "num_joints"), (dict(J=18), "num_joints"), (dict(rf=0, lag=0, max_gap=0), "receptive_field"),
        (dict(rf=-3), "receptive_field"), (dict(lag=-1), "lag"), (dict(lag=rf), "lag"), (dict(enc=4), "encoding"), (dict(enc=-1), "encoding"),
        (dict(F=1), "in_features"), (dict(F=4), "in_features"), (dict(enc=ray, F=2), "in_features"), (dict(enc=intr, F=3), "in_features"),
        (dict(enc=scr, F=3), "in_features"), (dict(enc=ray, cam=0), "cam_dev"), (dict(enc=intr, F=2, cam=0), "cam_dev"),
        (dict(rf=big // J + 1, lag=0), "receptive_field"), (dict(rf=2 ** 20, lag=0, S=200), "receptive_field"),
        (dict(state=p["state"] + 4), "state"), (dict(enc=ray, cam=p["cam"] + 4), "cam_dev"),
        # its own
        (dict(track=0), "track_dev"), (dict(out=0), "frame_out_dev"), (dict(syn=0), "synthetic_dev"), (dict(max_gap=-1), "max_gap"),
        (dict(max_gap=rf), "max_gap"), (dict(max_gap=rf + 7), "max_gap"), (dict(min_conf=float("nan")), "min_conf"),
        (dict(min_conf=float("inf")), "min_conf"), (dict(min_conf=float("-inf")), "min_conf"), (dict(track=p["track"] + 4), "track_dev"),
        (dict(out=p["frame"]), "frame_dev"), (dict(out=p["frame"] + row - 4), "frame_dev"), (dict(frame=p["out"] + row - 4), "frame_dev"),
        (dict(out=p["conf"]), "conf_dev"), (dict(out=p["state"] + 8), "state"), (dict(out=p["state"] + b["state"].nbytes - 4), "state"),
        (dict(out=p["track"]), "track"), (dict(out=p["track"] + b["track"].nbytes - 4), "track")]
    for kw, word in bad:
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
        assert word in hooks.r3d_last_error().decode(), (kw, hooks.r3d_last_error())
    assert (b["out"] == -7.0).all() and (b["syn"] == 77).all() and not b["state"].any() and not b["track"].any()       # nothing was written
    assert call() == 0 and call(conf=0) == 0 and call(cam=0) == 0 and call(enc=ray) == 0 and call(enc=intr, F=2) == 0
    assert call(max_gap=0) == 0 and call(max_gap=rf - 1) == 0 and call(min_conf=-3.0) == 0
    assert call(frame=p["frame"] + row, out=p["frame"]) == 0          # adjacent extents do not overlap


def test_device_entry_point_refuses_before_any_device_call():
    """The same rules through r3d_streams_repair itself, on pointers that are never followed: R3D_ERR_ARG without a GPU."""
    lib = _capi.load()

    def call(state=BOGUS, track=2 * BOGUS, S=6, rf=27, lag=13, J=17, F=3, enc=NONE, frame=3 * BOGUS, conf=4 * BOGUS, min_conf=0.0, cam=5 * BOGUS,
             action=6 * BOGUS, max_gap=5, out=7 * BOGUS, syn=8 * BOGUS):
        return lib.r3d_streams_repair(state, track, S, rf, lag, J, F, enc, frame, conf, min_conf, cam, action, max_gap, out, syn, None)

    for kw in (dict(state=None), dict(track=None), dict(frame=None), dict(action=None), dict(out=None), dict(syn=None), dict(S=0), dict(S=65536),
               dict(J=0), dict(J=18), dict(rf=0), dict(lag=-1), dict(lag=27), dict(enc=4), dict(F=4), dict(enc=0, F=2), dict(enc=1), dict(enc=2),
               dict(enc=0, cam=None), dict(rf=2 ** 27, lag=0), dict(rf=2 ** 20, lag=0, S=200), dict(state=BOGUS + 4), dict(track=2 * BOGUS + 4),
               dict(max_gap=-1), dict(max_gap=27), dict(min_conf=float("nan")), dict(out=3 * BOGUS), dict(out=4 * BOGUS), dict(out=BOGUS + 64),
               dict(out=2 * BOGUS + 64)):
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
        assert lib.r3d_last_error()
