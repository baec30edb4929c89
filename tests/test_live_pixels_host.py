"""CPU suite of the end-to-end layer (tests/live_cases.py; tests/test_gpu_live_pixels.py runs the device on the same scenes).  Two
jobs.  It proves, from the restatements alone, that the scenes hold what the GPU suite needs - every action, a slot reused, synthetic
pushes, detections dropped for lack of slots, gaps interpolated, held and back-filled, a preview at every look, a group of two
members that both emit - and that at least 90 % of the (tick, stream) pairs that emit a pose have an all-finite reference window:
the GPU suite's oracle comparison may skip only the pairs marked non-finite here.  And it plays one whole tick chain on the host
hooks - assign -> repair -> step -> poses (fed a seeded stand-in for the forwards' raw outputs) -> fuse -> peek - on CPU buffers, in
the order and with the pointer wiring OnlineLifter is meant to have, against the chain of NumPy restatements, tick by tick and bit
for bit; the freshly encoded ring rows are also held against the float64 host chain under the one-ulp rule."""
import numpy as np
import pytest

import live_cases as lc
import streams_assign_cases as ac
import streams_fuse_cases as fc
import streams_peek_cases as pk
import streams_poses_cases as pc
import streams_repair_cases as rc
from conftest import hooks_library
from live_cases import CENTRED, DRAIN, IDLE, PUSH, RESTART
from ray3d_amd import _capi, evaluate
from test_clips_encode_host import KPS, host_encode, ulps

CAP = 0.9


# ------------------------------------------------------------------ the scenes are what the GPU suite needs

@pytest.mark.parametrize("with_conf,repair", lc.CLIP_CASES, ids=["conf-repair2", "repair0"])
def test_the_clip_scene_holds_every_case(with_conf, repair):
    scn, cams, hist = lc.clip_history(with_conf, repair)
    rf, lag, J, _ = lc.shape_of(CENTRED)
    assert [c.shape[0] for c in scn["clips"]] == [1, 5, 2 * rf + 3, lc.SECOND_CLIP] and 2 * rf + 3 > 2 * rf   # (the ring wraps twice)
    acts = np.stack([a for _, a, _ in scn["ticks"]])
    assert (acts[:, 3] == IDLE).all() and set(acts.flatten().tolist()) == {IDLE, PUSH, RESTART, DRAIN}
    restarts = np.flatnonzero(acts[:, 0] == RESTART)
    assert restarts.tolist() == [0, lag + 2] and (acts[1:1 + lag, 0] == DRAIN).all()      # RESTART after the drain
    assert all((rec["status"] == 0).all() for rec in hist)
    kinds = {"nan": 0, "inf": 0, "one": 0}
    for c in scn["clips"]:
        kinds["nan"] += int(np.isnan(c).all(-1).sum())
        kinds["inf"] += int(np.isinf(c).any(-1).sum())
        kinds["one"] += int((np.isnan(c).sum(-1) == 1).sum())
    assert all(v > 0 for v in kinds.values()) and any((c == -np.inf).any() for c in scn["clips"]) and any((c == np.inf).any() for c in scn["clips"])
    n = lc.gap_census(hist, repair)
    assert n["backfilled"] > 0 and n["held"] > 0 and n["missing"] > 0
    assert (n["interpolated"] > 0) == (repair > 0)
    assert sum(int((rec["synthetic"] != 0).sum()) for rec in hist) > 0
    emitted = [0] * scn["S"]
    for rec in hist:
        for s in rec["x"]:
            emitted[s] += 1
    assert emitted == [1 + lc.SECOND_CLIP, 5, 2 * rf + 3, 0]
    for k, L in enumerate(lc.looks_of(CENTRED)):                     # a preview at every look, also of a frame whose gap just closed
        assert sum(len(rec["previews"][k]["x"]) for rec in hist) == sum(max(c.shape[0] - L, 0) for c in scn["clips"])
    if repair:
        assert any(s in hist[t]["previews"][0]["x"] and hist[t]["previews"][0]["finite"][s] for t, s, _, _ in n["closures"])
    both = sum(1 for rec in hist if 1 in rec["x"] and 2 in rec["x"])
    assert lc.GROUPS[0] == [1, 2] and both == 5 and cams[1] is cams[2]           # a group of two members on one camera; both emit
    if not with_conf:                       # ... and see the same window of frame 0: there the group is fused from both
        assert lag + 1 <= 5 and rc.same_bits(hist[lag]["x"][1], hist[lag]["x"][2]) and not rc.same_bits(hist[lag + 1]["x"][1], hist[lag + 1]["x"][2])
    assert any(not (set(lc.GROUPS[1]) & set(rec["x"])) for rec in hist) and any(set(lc.GROUPS[1]) & set(rec["x"]) for rec in hist)
    assert lc.FUSE["fuse_max_px"] > 0 and lc.FUSE["fuse_max_dist"] > 0           # the gates are configured
    pairs, finite = lc.finite_share(hist)
    print("clip scene conf=%s repair=%d: %d of %d emitting pairs have an all-finite reference window" % (with_conf, repair, finite, pairs))
    assert finite >= CAP * pairs


@pytest.mark.parametrize("name,fill,repair,with_conf", lc.TRACK_CASES, ids=lc.TRACK_IDS)
def test_the_tracking_scene_holds_every_case(name, fill, repair, with_conf):
    scene, cams, wants, hist = lc.track_history(name, fill, repair, with_conf)
    _, lag, J, _ = lc.shape_of(name)
    assert len(scene) == lc.TICKS == 40 and scene[0][0].shape == (2, 4, J, 2)
    actions, reused, ended, synthetic, dropped, births = set(), 0, set(), 0, 0, 0
    for w in wants:
        actions |= set(w["action"].tolist())
        synthetic += int(((w["action"] == PUSH) & (w["match"] < 0)).sum())
        dropped += int(w["stats"][:, 3].sum())
        births += int(w["stats"][:, 2].sum())
        for s in np.flatnonzero(w["action"] == RESTART):
            reused += int(s) in ended
        if lag:
            ended |= set(np.flatnonzero(w["action"] == DRAIN).tolist())
        else:                               # a causal track ends with IDLE: a slot that held a track and is free again
            ended |= set(np.flatnonzero((w["action"] == IDLE) & (w["id"] >= 0)).tolist())
    assert actions == ({IDLE, PUSH, RESTART, DRAIN} if lag else {IDLE, PUSH, RESTART})
    assert reused > 0 and synthetic >= 2 and dropped > 0 and births >= 5
    assert all((rec["status"] == 0).all() for rec in hist)
    shuffled = sum(1 for a, b in zip(wants, wants[1:]) if not np.array_equal(a["match"], b["match"]))
    assert shuffled > 10                                             # the detection row a track takes changes from tick to tick
    if repair is not None:
        n = lc.gap_census(hist, repair)
        assert n["interpolated"] > 0 and n["held"] > 0 and n["backfilled"] > 0
        late = [rec for rec in hist[lc.SPANS["E"][0]:] if any(not ok for ok in rec["finite"].values())]
        assert len(late) >= (2 if lag else 1)                        # E's first poses on camera 0 are legitimately NaN
    if lag:
        for k in range(2):
            assert sum(len(rec["previews"][k]["x"]) for rec in hist) > 0
    pairs, finite = lc.finite_share(hist)
    print("tracking scene %s: %d of %d emitting pairs have an all-finite reference window" % ((name, fill, repair, with_conf), finite, pairs))
    assert finite >= CAP * pairs


def test_the_lift_clips_fixtures_are_all_finite():
    for name, encodings in lc.FIXTURES.items():
        rf = lc.shape_of(name)[0]
        clips = lc.pixel_clips(name, "lift")
        assert [c.shape[0] for c in clips] == [1, 5, 2 * rf + 3] and all(np.isfinite(c).all() for c in clips)
        cams = lc.stream_cameras(lc.LIFT_CAMERAS)
        for encoding in encodings:
            for cam, clip in zip(cams, clips):
                assert np.isfinite(host_encode(cam, clip, encoding)).all()


# ------------------------------------------------------------------ one whole tick chain on the host hooks

def _ptr(a):
    return a.ctypes.data if a is not None else None


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_tick_chain_on_the_host_hooks_equals_the_chain_of_restatements():
    """assign -> repair -> step -> poses -> fuse -> peek per tick on ONE set of CPU buffers, wired as OnlineLifter._final_tick and
    _preview_tick wire the device's: the assign call writes action, frame and conf; the repair reads them and the state and writes
    frame_out and synthetic; the step pushes frame_out; the poses call reads the step's emit, status and windows; the fuse reads
    world, reproj, emit, status and synthetic; the peek reads the state the repair rewrote.  Tracking scene, encoding "ray", flip,
    confidences, every tick against tests/streams_assign_cases.restate, the repair / step restatement (its encoder the host hook
    of r3d_clips_encode: the contract defines the pushed bits as that routine's), tests/streams_poses_cases.restate,
    tests/streams_fuse_cases.restate and tests/streams_peek_cases.expected - bits everywhere.  The freshly encoded ring rows are
    within one float32 ulp of the float64 host chain."""
    name, fill, repair, with_conf = lc.TRACK_CASES[0]
    scene = lc.tracking_scene(name, True, with_conf)
    cams = lc.stream_cameras(lc.TRACK_CAMERAS)
    rows = lc.camera_rows(name, cams)
    rf, lag, J, F = lc.shape_of(name)
    S, C, P, D = lc.S_LIVE, lc.C_LIVE, lc.P_LIVE, lc.D_LIVE
    looks = lc.looks_of(name)
    K = len(looks)
    enc = evaluate.ENCODINGS["ray"]
    perm = evaluate.mirror_permutation(J, *KPS[J])
    out_perm = [int(v) for v in perm]
    min_conf = lc.MIN_CONF
    prm_d = lc.assign_params(name, fill, min_conf)
    prm = _capi.assign_params(C, P, D, J, 2, lag, prm_d["min_joints"], prm_d["min_common"], prm_d["max_missed"], prm_d["fill"], min_conf,
                              prm_d["max_cost"])
    hooks_library()
    b = dict(assign=np.zeros(_capi.streams_assign_bytes(C, P, J, 2) // 8, np.int64), det=np.zeros((C, D, J, 2), np.float32),
             det_conf=np.zeros((C, D, J), np.float32), det_count=np.zeros(C, np.int32), action=np.zeros(S, np.int32),
             frame=np.zeros((S, J, 2), np.float32), conf=np.zeros((S, J), np.float32), match=np.zeros(S, np.int32),
             track_id=np.zeros(S, np.int64), stats=np.zeros((C, 4), np.int32),
             state=np.zeros(_capi.streams_state_bytes(S, rf, J, F) // 8, np.int64),
             track=np.zeros(_capi.streams_track_bytes(S, rf, J, 2) // 8, np.int64), cam=rows["cam_rows"].copy(),
             frame_out=np.zeros((S, J, 2), np.float32), synthetic=np.zeros(S, np.int32), x=np.zeros((S, rf, J, F), np.float32),
             x_mirror=np.zeros((S, rf, J, F), np.float32), emit=np.zeros(S, np.int64), status=np.zeros(S, np.int32),
             raw=np.zeros((S, J, 3), np.float32), raw_m=np.zeros((S, J, 3), np.float32), desc=rows["transforms"].copy(),
             pred=np.zeros((S, J, 3), np.float32), world=np.zeros((S, J, 3)), reproj=np.zeros((S, J)), quality=np.zeros((S, 2)),
             member=lc.member_table(lc.TRACK_GROUPS), fused=np.zeros((3, J, 3)), spread=np.zeros((3, J)),
             count=np.zeros((3, J), np.int32), used=np.zeros((3, 16), np.int32), px=np.zeros((K, S, rf, J, F), np.float32),
             px_mirror=np.zeros((K, S, rf, J, F), np.float32), pemit=np.zeros((K, S), np.int64), pstatus=np.zeros((K, S), np.int32))
    st = ac.unpack_state(np.zeros(ac.state_bytes(C, P, J, 2), np.uint8), C, P, J, 2)
    hook_encode = rc.pixel_encoder(dict(rows=rows["cam_rows"], encoding="ray"))
    model = lc.fresh_model(S, rf, lag, J, F, perm, repair, np.float32(min_conf), hook_encode)
    rng = np.random.RandomState(77)
    seen = dict(emits=0, previews=0, fused=0, fresh=0, equal=0, synthetic=0, worst=0)
    for t, (det, counts, conf) in enumerate(scene):
        # ---- r3d_streams_assign
        b["det"][:], b["det_count"][:], b["det_conf"][:] = det, counts, conf
        for k in ("action", "match", "stats"):
            b[k][:] = -77
        b["frame"][:], b["conf"][:], b["track_id"][:] = -7.0, -7.0, -77
        hooks_library()
        assert _capi.debug_streams_assign_host(_ptr(b["assign"]), prm, _ptr(b["det"]), _ptr(b["det_conf"]), _ptr(b["det_count"]), _ptr(b["action"]),
                                               _ptr(b["frame"]), _ptr(b["conf"]), _ptr(b["match"]), _ptr(b["track_id"]), _ptr(b["stats"])) == 0
        want = ac.restate(st, prm_d, det, conf, counts)
        got = dict(action=b["action"], frame_out=_u32(b["frame"]), conf_out=_u32(b["conf"]), match=b["match"], id=b["track_id"], stats=b["stats"],
                   state=b["assign"].view(np.uint8))
        want["state"] = ac.pack_state(st, C, P, J, 2)
        ac.agree(got, want, ("assign", t))
        # ---- r3d_streams_repair on what the assign call wrote
        b["frame_out"][:], b["synthetic"][:] = -7.0, -77
        frame, action, cf = b["frame"].copy(), b["action"].copy(), b["conf"].copy()
        assert _capi.debug_streams_repair_host(_ptr(b["state"]), _ptr(b["track"]), S, rf, lag, J, F, enc, _ptr(b["frame"]), _ptr(b["conf"]), min_conf,
                                               _ptr(b["cam"]), _ptr(b["action"]), repair, _ptr(b["frame_out"]), _ptr(b["synthetic"])) == 0
        fo, syn, pushed = model.repair(frame, action, cf)
        for s in range(S):
            assert np.array_equal(_u32(b["frame_out"][s]), fo[s]) if pushed[s] else (b["frame_out"][s] == -7.0).all(), ("frame_out", t, s)
        assert _u32(b["synthetic"]).tolist() == syn.tolist(), ("synthetic", t)
        ring = b["state"].view(np.uint8)[S * 16:].view(np.uint32).reshape(S, rf, J, F)
        assert np.array_equal(ring, model.ring), ("ring after the repair", t)
        seen["synthetic"] += int((syn != 0).sum())
        # ---- r3d_streams_step on frame_out
        b["x"][:], b["x_mirror"][:], b["emit"][:], b["status"][:] = -7.0, -7.0, -99, -5
        assert _capi.debug_streams_step_host(_ptr(b["state"]), S, rf, lag, J, F, enc, _ptr(b["frame_out"]), _ptr(b["cam"]), _ptr(b["action"]),
                                             _ptr(b["x"]), _ptr(b["x_mirror"]), perm, _ptr(b["emit"]), _ptr(b["status"])) == 0
        x, xm, emit, status = model.step(fo, action)
        assert b["emit"].tolist() == emit.tolist() and b["status"].tolist() == status.tolist() and not status.any(), ("emit", t)
        for s in range(S):
            if s in x:
                assert np.array_equal(_u32(b["x"][s]), x[s]) and np.array_equal(_u32(b["x_mirror"][s]), xm[s]), ("x", t, s)
            else:
                assert (b["x"][s] == -7.0).all() and (b["x_mirror"][s] == -7.0).all(), ("x", t, s)
        assert np.array_equal(ring, model.ring), ("ring after the step", t)
        heads = b["state"].view(np.uint8)[:S * 16].view(_capi.stream_head_dtype())
        assert heads.tolist() == list(zip(model.count, model.drained)), ("heads", t)
        for s in np.flatnonzero(pushed):                             # the freshly encoded rows against the float64 host chain: one ulp
            row = ring[s, (model.count[s] - 1) % rf].view(np.float32)
            host = host_encode(cams[s], fo[s].view(np.float32), "ray")
            ok = np.isfinite(host).all(-1)
            assert not np.isfinite(row[~ok]).any(), ("a row of a joint never observed", t, s)
            seen["worst"] = max(seen["worst"], ulps(np.ascontiguousarray(row[ok]), np.ascontiguousarray(host[ok])))
            seen["fresh"] += int(ok.sum()) * F
            seen["equal"] += int((row[ok] == host[ok]).sum())
        seen["emits"] += len(x)
        # ---- r3d_streams_poses on a seeded stand-in for the forwards' raw outputs, then r3d_streams_fuse
        Xw = 0.3 * rng.standard_normal((P, J, 3)) + np.array([0.0, 0.0, 1.0])      # slot p of both cameras sees the same skeleton
        pn = np.stack([cams[s].world2normalized(Xw[s % P]) for s in range(S)])
        b["raw"][:] = pn + 0.02 * rng.standard_normal(pn.shape)
        b["raw_m"][:] = (pn * np.array([-1.0, 1.0, 1.0]) + 0.02 * rng.standard_normal(pn.shape))[:, np.argsort(perm)]
        b["pred"][:], b["world"][:], b["reproj"][:], b["quality"][:] = pc.FILL32, pc.FILL64, pc.FILL64, pc.FILL64
        assert _capi.debug_streams_poses_host(_ptr(b["raw"]), _ptr(b["raw_m"]), S, J, out_perm, _ptr(b["emit"]), _ptr(b["status"]), _ptr(b["desc"]),
                                              _ptr(b["cam"]), _ptr(b["x"]), rf, lag, _ptr(b["pred"]), _ptr(b["world"]), _ptr(b["reproj"]),
                                              _ptr(b["quality"])) == 0
        fin = pc.restate(dict(raw=b["raw"], raw_m=b["raw_m"], perm=out_perm, desc=b["desc"], cam=b["cam"], x=b["x"], rf=rf, lag=lag,
                              emit=b["emit"], status=b["status"]), True)
        for k in pc.OUTPUTS:
            assert pc.same_bits(b[k], fin[k]), ("poses", t, k)
        for k, fill_ in (("fused", -7.0), ("spread", -7.0), ("count", -77), ("used", -77)):
            b[k][:] = fill_
        assert _capi.debug_streams_fuse_host(_ptr(b["world"]), _ptr(b["reproj"]), _ptr(b["emit"]), _ptr(b["status"]), _ptr(b["synthetic"]), S, J,
                                             _ptr(b["member"]), 3, _capi.FUSE_MAX_MEMBERS, lc.FUSE["fuse_soft_px"], lc.FUSE["fuse_max_px"],
                                             lc.FUSE["fuse_max_dist"], _ptr(b["fused"]), _ptr(b["spread"]), _ptr(b["count"]), _ptr(b["used"])) == 0
        fw = fc.restate(fin["world"], fin["reproj"], b["emit"], b["status"], _u32(b["synthetic"]), b["member"], lc.FUSE["fuse_soft_px"],
                        lc.FUSE["fuse_max_px"], lc.FUSE["fuse_max_dist"])
        fc.agree(dict(fused=fc.bits64(b["fused"]), spread=fc.bits64(b["spread"]), count=b["count"], used=fc.bits32(b["used"])), fw, ("fuse", t))
        seen["fused"] += int((fw["count"] == 2).sum())
        # ---- r3d_streams_peek behind them: the state the repair rewrote
        b["px"][:], b["px_mirror"][:], b["pemit"][:], b["pstatus"][:] = -7.0, -7.0, -99, -5
        assert _capi.debug_streams_peek_host(_ptr(b["state"]), S, rf, lag, J, F, looks, _ptr(b["action"]), _ptr(b["status"]), _ptr(b["px"]),
                                             _ptr(b["px_mirror"]), perm, _ptr(b["pemit"]), _ptr(b["pstatus"])) == 0
        pe, ps = pk.expected(heads, action, status, looks, lag)
        assert np.array_equal(b["pemit"], pe) and np.array_equal(b["pstatus"], ps), ("peek words", t)
        for k in range(K):
            for s in range(S):
                if pe[k, s] >= 0:
                    w = pk.window_of_ring(model.ring[s], int(pe[k, s]), model.count[s], rf, lag)
                    assert np.array_equal(_u32(b["px"][k, s]), w) and np.array_equal(_u32(b["px_mirror"][k, s]), rc.mirrored(w, perm)), ("peek", t, k, s)
                    seen["previews"] += 1
                else:
                    assert (b["px"][k, s] == -7.0).all() and (b["px_mirror"][k, s] == -7.0).all(), ("peek", t, k, s)
    _capi.use_hooks(False)
    print("host chain: %d emits, %d previews, %d joints fused from two cameras, %d synthetic words; fresh ring rows: %.6f of %d elements "
          "equal to the host chain, max %d ulp" % (seen["emits"], seen["previews"], seen["fused"], seen["synthetic"],
                                                   seen["equal"] / seen["fresh"], seen["fresh"], seen["worst"]))
    assert seen["emits"] > 100 and seen["previews"] > 100 and seen["fused"] > 0 and seen["synthetic"] > 0 and seen["worst"] <= 1
