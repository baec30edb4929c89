"""GPU suite: r3d_streams_assign (detections to live streams) and OnlineLifter(cameras=).track on top of it.  The kernel against the
host hook, bit for bit, outputs and state after every tick of the seeded multi-tick cases of tests/streams_assign_cases.py - every
shape from 1 x 1 x 1 to 1 x 32 x 32, det_count below 0 and above D, non-finite keypoints and confidences, bit-identical detections,
a state of 0xA5 bytes - with every buffer inside guard bands and poisoned outputs; the optional outputs left out; the call captured
into a hipGraph and replayed on new inputs; OnlineLifter.track on the j17_rf9_s1 fixture pair with two cameras of three slots,
eager and captured, against a second OnlineLifter without cameras= that is stepped with the frame rows, actions and confidences the
NumPy restatement produced."""
import numpy as np
import pytest
import torch

import buffers_util as bu
import streams_assign_cases as ac
from streams_assign_cases import DRAIN, IDLE, PUSH, RESTART, AssignRig, agree
from ray3d_amd import _capi
from test_gpu_streams import pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAME = "j17_rf9_s1"


# ------------------------------------------------------------------ the kernel against the host hook

@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: "C%d-P%d-D%d" % s)
def test_device_equals_the_host_hook_bit_for_bit(shape):
    for key in [k for k in ac.case_ids() if k[:3] == shape]:
        case, want = ac.host_run(*key)
        rig = AssignRig(DEV, case, pattern=bu.NANS if key[3] == 17 else bu.ZEROS)
        for t, tick in enumerate(case["ticks"]):
            rc, got = rig.run(tick)                                  # (run() checks the guards around every buffer)
            assert rc == 0
            agree(got, want[t], (key, t))


def test_optional_outputs_left_out_stay_untouched():
    key = [k for k in ac.case_ids() if k[:3] == (2, 3, 5) and k[7]][-1]      # (with confidences)
    case, want = ac.host_run(*key)
    for left_out in (("conf_out",), ("stats",), ("conf_out", "stats")):
        rig = AssignRig(DEV, case)
        for t, tick in enumerate(case["ticks"]):
            rc, got = rig.run(tick, **{k: None for k in left_out})
            for k in ac.OUT_KEYS + ("state",):
                if k in left_out:
                    assert (ac.bits32(got[k]) == ac.FILL32).all(), (left_out, k, t)
                else:
                    assert np.array_equal(got[k], want[t][k]), (left_out, k, t)


def test_the_call_is_captured_and_replayed_on_new_inputs():
    """One launch, no allocation, no copy: captured into a hipGraph once, then every tick of a case is a replay on new inputs."""
    key = [k for k in ac.case_ids() if k[:3] == (3, 5, 3)][-1]
    case, want = ac.host_run(*key)
    rig = AssignRig(DEV, case)
    dev = torch.device(DEV)
    state0 = rig.t["state"].clone()
    rig.load(case["ticks"][0])
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _capi.streams_assign(*rig.ptrs(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    rig.t["state"].copy_(state0)                                     # (a capture does not run the launch; the state starts over anyway)
    for t, tick in enumerate(case["ticks"]):
        rig.load(tick)
        rig.poison()
        g.replay()
        rig.arena.check()
        agree(rig.read(), want[t], t)
    del g


# ------------------------------------------------------------------ OnlineLifter.track

C_LIVE, P_LIVE, D_LIVE, J_LIVE = 2, 3, 4, 17
S_LIVE = C_LIVE * P_LIVE
TICKS = 40
MAX_MISSED = 2


def _detections(holes):
    """Per tick (det (C, D, J, 3) model-input rows, counts (C,)): per camera person A all the way with a miss of two ticks, person B
    from tick 2 to 14 (their track ends, drains and frees its slot), person E from tick 25 (the freed slot is reused), and on camera
    1 a fourth and a fifth person for a few ticks (more births than free slots); the rows shuffled every tick; with `holes` a few
    joints are not delivered."""
    rng = np.random.RandomState(41)
    shape = 0.25 * ac.BONES[:J_LIVE]
    homes = {"A": (-0.6, -0.3), "B": (0.2, 0.3), "E": (0.7, -0.4), "F": (-0.5, 0.6), "G": (0.0, -0.8)}
    spans = {"A": (0, TICKS), "B": (2, 15), "E": (25, TICKS), "F": (27, 33), "G": (28, 33)}
    out = []
    for t in range(TICKS):
        det = np.full((C_LIVE, D_LIVE, J_LIVE, 3), np.nan, np.float32)
        counts = np.zeros(C_LIVE, np.int32)
        for c in range(C_LIVE):
            rows = []
            for who, (a, b) in spans.items():
                if not a <= t < b or (who == "A" and t in (10, 11)) or (who in "FG" and c == 0):
                    continue
                xy = np.array(homes[who]) + 0.004 * t * np.array([1.0, -0.5]) + shape + rng.normal(0, 0.002, (J_LIVE, 2))
                row = np.concatenate([xy, np.ones((J_LIVE, 1))], -1).astype(np.float32)
                if holes:
                    row[rng.uniform(size=J_LIVE) < 0.15] = np.nan
                rows.append(row)
            rng.shuffle(rows)
            for d, row in enumerate(rows[:D_LIVE]):
                det[c, d] = row
            counts[c] = len(rows)                                    # (camera 1 at ticks 28 - 32: five people, D = 4 - read clamped)
        out.append((det, counts))
    return out


def _lifters(fill, repair):
    import ray3d_amd
    lifter, _ = pair(NAME)
    kw = dict(device=DEV, repair=repair)
    track_kw = dict(cameras=C_LIVE, max_detections=D_LIVE, assign_max_cost=0.5, assign_max_missed=MAX_MISSED, assign_fill=fill)
    ols = [ray3d_amd.OnlineLifter(lifter, S_LIVE, **kw), ray3d_amd.OnlineLifter(lifter, S_LIVE, **kw, **track_kw),
           ray3d_amd.OnlineLifter(lifter, S_LIVE, **kw, **track_kw)]
    if lifter.pos.camera_embedding:
        params = np.random.RandomState(5).standard_normal((S_LIVE, lifter.pos.extrinsic_dim)).astype(np.float32)
        for ol in ols:
            ol.set_cameras(params=params)
    return ols


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    view = {8: torch.int64, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.contiguous().view(view), b.contiguous().view(view)), what


@pytest.mark.parametrize("fill,repair", [("nan", 2), ("hold", None)], ids=["repair-nan", "hold"])
def test_online_lifter_track_equals_a_stepped_lifter_eager_and_captured(fill, repair):
    """40 ticks with a birth, a miss, an end, a drain and a slot reuse: poses, frames and extras of track() - eager and captured -
    equal, bit for bit, those of an OnlineLifter without cameras= stepped with the (frame, actions, conf) the restatement produced;
    track_id, match and assign_stats are the restatement's."""
    plain, eager, cap = _lifters(fill, repair)
    prm = dict(C=C_LIVE, P=P_LIVE, D=D_LIVE, J=J_LIVE, width=3, lag=plain.lag, min_joints=4, min_common=3, max_missed=MAX_MISSED,
               fill=ac.FILL_NAN if fill == "nan" else ac.FILL_HOLD, min_conf=0.0, max_cost=0.5)
    st = ac.unpack_state(np.zeros(ac.state_bytes(C_LIVE, P_LIVE, J_LIVE, 3), np.uint8), C_LIVE, P_LIVE, J_LIVE, 3)
    seen_actions, reused, ended, synthetic, dropped, posed = set(), 0, set(), 0, 0, 0
    try:
        cap.capture()
        for t, (det, counts) in enumerate(_detections(holes=repair is not None)):
            want = ac.restate(st, prm, det, None, counts)
            frame = want["frame_out"].view(np.float32)
            if repair is not None:
                pp, fp, xp = plain.step(frame, want["action"], conf=want["conf_out"].view(np.float32))
            else:
                (pp, fp), xp = plain.step(frame, want["action"]), {}
            for name, ol in (("eager", eager), ("captured", cap)):
                p, f, x = ol.track(det, counts)
                assert set(x) == set(xp) | {"track_id", "match", "assign_stats"}, (name, t)
                assert torch.equal(f, fp), (name, t)
                live = (fp >= 0).cpu()
                _same(p.cpu()[live], pp.cpu()[live], (name, t, "poses"))
                for k, v in xp.items():
                    _same(x[k], v, (name, t, k))
                assert x["track_id"].dtype == torch.int64 and x["match"].dtype == torch.int32 and x["assign_stats"].shape == (C_LIVE, 4)
                assert np.array_equal(x["track_id"].cpu().numpy(), want["id"]), (name, t)
                assert np.array_equal(x["match"].cpu().numpy(), want["match"]), (name, t)
                assert np.array_equal(x["assign_stats"].cpu().numpy(), want["stats"]), (name, t)
                _same(ol.action, torch.from_numpy(want["action"]).to(DEV), (name, t, "action"))
            posed += int((fp >= 0).sum())
            seen_actions |= set(want["action"].tolist())
            synthetic += int(((want["action"] == PUSH) & (want["match"] < 0)).sum())
            dropped += int(want["stats"][:, 3].sum())
            for s in np.flatnonzero(want["action"] == RESTART):
                reused += int(s) in ended
            ended |= set(np.flatnonzero(want["action"] == DRAIN).tolist())
        assert seen_actions == {IDLE, PUSH, RESTART, DRAIN} and reused > 0 and synthetic > 0 and dropped > 0 and posed > 0
        pair(NAME)[0].check_status(torch.device(DEV))
        with pytest.raises(ValueError, match="use track"):
            cap.step(np.zeros((S_LIVE, J_LIVE, 3), np.float32))
    finally:
        cap.release()


def test_online_lifter_cameras_argument_errors():
    import ray3d_amd
    lifter, _ = pair(NAME)
    kw = dict(device=DEV, repair=2, max_detections=4)
    for bad, word in ((dict(cameras=4), "cameras \\* P"), (dict(cameras=0), "cameras \\* P"), (dict(cameras=2.0), "cameras \\* P"),
                      (dict(cameras=2, max_detections=0), "max_detections"), (dict(cameras=2, max_detections=33), "max_detections"),
                      (dict(cameras=2, max_detections=None), "max_detections"), (dict(cameras=None), "needs cameras"),
                      (dict(cameras=2, assign_fill="zero"), "assign_fill"), (dict(cameras=2, assign_fill="nan", repair=None), "needs repair"),
                      (dict(cameras=2, assign_max_cost=0.0), "assign_max_cost"), (dict(cameras=2, assign_max_cost=float("nan")), "assign_max_cost"),
                      (dict(cameras=2, assign_max_missed=-1), "assign_max_missed"), (dict(cameras=2, assign_min_joints=0), "assign_min_joints"),
                      (dict(cameras=2, assign_min_common=18), "assign_min_joints")):
        with pytest.raises(ValueError, match=word):
            ray3d_amd.OnlineLifter(lifter, 6, **dict(kw, **bad))
    with pytest.raises(ValueError, match="cameras \\* P"):
        ray3d_amd.OnlineLifter(lifter, 66, cameras=2, **kw)          # 33 slots per camera
    with pytest.raises(ValueError, match="cameras="):
        ray3d_amd.OnlineLifter(lifter, 6, device=DEV).track(np.zeros((2, 4, 17, 3)), [0, 0])
    ol = ray3d_amd.OnlineLifter(lifter, 6, cameras=2, **kw)
    if lifter.pos.camera_embedding:
        ol.set_cameras(params=np.zeros((6, lifter.pos.extrinsic_dim), np.float32))
    with pytest.raises(ValueError, match="detections must be"):
        ol.track(np.zeros((2, 3, 17, 3)), [0, 0])
    with pytest.raises(ValueError, match="counts must be"):
        ol.track(np.zeros((2, 4, 17, 3)), [0, 0, 0])
    with pytest.raises(ValueError, match="conf must be"):
        ol.track(np.zeros((2, 4, 17, 3)), [0, 0], conf=np.zeros((2, 4, 16)))
    p, f, x = ol.track(np.full((2, 4, 17, 3), np.nan), [4, 4])       # nothing valid: every slot stays free
    assert (f == -1).all() and (x["track_id"] == -1).all() and (x["match"] == -1).all() and (x["assign_stats"] == 0).all()
