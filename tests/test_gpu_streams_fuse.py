"""GPU suite: r3d_streams_fuse (one world skeleton per person from several cameras) and OnlineLifter(groups=) on top of it.  The kernel
against the host hook, bit for bit, over the seeded cases of tests/test_streams_fuse_host.py - NaN payloads, empty slots, words that
name no stream, all-empty groups included - with every buffer inside guard bands and poisoned outputs; the optional outputs left
out; OnlineLifter on the j17_rf9_s1 fixture pair with four streams in two groups, eager and captured: the fused outputs equal the
NumPy restatement applied to the tick's own extras, everything else equals a run without groups, and set_groups takes effect on
the next tick."""
import numpy as np
import pytest
import torch

import buffers_util as bu
import streams_fuse_cases as fc
import streams_poses_cases as pc
from streams_cases import DRAIN, IDLE, PUSH, RESTART
from streams_fuse_cases import FILL32, FILL64, QNAN64, FuseRig, agree, restate
from streams_poses_cases import H36M_LEFT, H36M_RIGHT
from ray3d_amd import _capi
from test_gpu_streams import pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAME = "j17_rf9_s1"


# ------------------------------------------------------------------ the kernel against the host hook

@pytest.mark.parametrize("M,J", fc.SHAPES)
def test_device_equals_the_host_hook_bit_for_bit(M, J):
    for variant in fc.VARIANTS:
        case, want = fc.host_run(M, J, *variant)
        rc, got = FuseRig(DEV, case).run()
        assert rc == 0
        agree(got, want, (M, J) + variant)


@pytest.mark.parametrize("pattern", [bu.NANS, bu.ZEROS], ids=["nan", "zeros"])
def test_all_empty_groups_hold_exactly_nan_and_zero_and_nothing_else_is_written(pattern):
    for M in (1, 4, 16):
        for g in range(fc.G_CASE):
            case, want = fc.host_run(M, 17, True, True, True, all_empty_group=g)
            rc, got = FuseRig(DEV, case, pattern=pattern).run()         # (run() checks the guards around every buffer)
            agree(got, want, (M, g))
            assert (got["fused"][g] == QNAN64).all() and (got["spread"][g] == QNAN64).all()
            assert (got["count"][g] == 0).all() and (got["used"][g] == 0).all()


def test_optional_outputs_left_out_stay_untouched():
    case, want = fc.host_run(4, 17, True, True, True)
    for left_out in (("spread",), ("count",), ("used",), ("spread", "count", "used")):
        rc, got = FuseRig(DEV, case).run(**{k: None for k in left_out})
        for k in ("fused", "spread", "count", "used"):
            if k in left_out:
                assert (got[k] == FILL64).all() if got[k].dtype == np.uint64 else (fc.bits32(got[k]) == FILL32).all(), (left_out, k)
            else:
                assert np.array_equal(got[k], want[k]), (left_out, k)


def test_the_call_is_captured_and_replayed_on_new_inputs():
    """One launch, no allocation, no copy: captured into a hipGraph and replayed after the inputs and the member table changed."""
    a, want_a = fc.host_run(4, 17, True, True, True)
    b, want_b = fc.host_run(4, 17, True, True, True, all_empty_group=1)
    rig = FuseRig(DEV, a)
    rig.run()
    dev = torch.device(DEV)
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _capi.streams_fuse(*rig.args(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for case, want in ((b, want_b), (a, want_a)):
        rig.t["member"].copy_(torch.from_numpy(case["member"]))
        for k in ("fused", "spread"):
            rig.t[k].fill_(-1)
        g.replay()
        rig.arena.check()
        agree(rig.read(), want)
    del g


# ------------------------------------------------------------------ OnlineLifter

S_LIVE, GROUPS = 4, [[0, 1], [2, 3]]
FUSE = dict(fuse_soft_px=2.0, fuse_max_px=0.0, fuse_max_dist=0.5)


def _rows(lifter):
    cams = pc.golden_cameras()
    cams = [cams[i % len(cams)] for i in (0, 0, 1, 2)]              # streams 0 and 1 share a camera: fed alike they agree exactly
    rows = dict(cam_rows=np.stack([c.cam_row(distortion=True) for c in cams]), transforms=np.stack([c.stream_pose_row() for c in cams]))
    if lifter.pos.camera_embedding:
        rows["params"] = np.stack([c.param() for c in cams])
    return rows


def _online(groups, **kw):
    import ray3d_amd
    lifter, _ = pair(NAME)
    ol = ray3d_amd.OnlineLifter(lifter, S_LIVE, flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, device=DEV, world=True, quality=True,
                                repair=2, groups=groups, **kw)
    ol.set_cameras(**_rows(lifter))
    return ol


def _frames(ticks):
    """(ticks, S, 17, 3) rays: streams 0 and 1 see the same keypoints, 2 and 3 their own; a few joints are not delivered."""
    rng = np.random.RandomState(31)
    f = (0.3 * rng.standard_normal((ticks, S_LIVE, 17, 3))).astype(np.float32)
    f[:, 1] = f[:, 0]
    f[3:5, 0, 2], f[4, 2, 7], f[6:9, 3, 0] = np.nan, np.nan, np.nan
    return f


def _same(a, b, keys):
    for k in keys:
        assert torch.equal(a[k].view(torch.int64 if a[k].dtype == torch.float64 else torch.int32),
                           b[k].view(torch.int64 if b[k].dtype == torch.float64 else torch.int32)), k


def _table(groups):
    t = np.full((len(groups), 16), -1, np.int32)
    for g, row in enumerate(groups):
        t[g, :len(row)] = row
    return t


def _check_fused(extras, frames, table, what):
    want = restate(extras["world"].cpu().numpy(), extras["reproj"].cpu().numpy(), frames.cpu().numpy(), np.zeros(S_LIVE, np.int32),
                   extras["synthetic"].cpu().numpy().view(np.uint32), table, FUSE["fuse_soft_px"], FUSE["fuse_max_px"], FUSE["fuse_max_dist"])
    got = dict(fused=fc.bits64(extras["fused"].cpu().numpy()), spread=fc.bits64(extras["fused_spread"].cpu().numpy()),
               count=extras["fused_count"].cpu().numpy(), used=fc.bits32(extras["fused_used"].cpu().numpy()))
    agree(got, want, what)
    return got


def test_online_lifter_fuses_groups_eager_and_captured():
    """RF + 3 ticks and the drain: extras["fused*"] equal the restatement applied to that tick's extras; poses, world and the quality
    outputs equal a run without groups; the captured tick equals the eager one; set_groups takes effect on the next tick."""
    plain, eager, cap = _online(None), _online(GROUPS, **FUSE), _online(GROUPS, **FUSE)
    ticks = plain.rf + 3
    frames_in = _frames(ticks)
    table, regrouped, fused_both, synthetic_seen = _table(GROUPS), [[0, 2, 3], [1]], 0, 0
    try:
        cap.capture()
        for t in range(ticks + plain.lag):
            draining = t >= ticks
            act = np.full(S_LIVE, DRAIN if draining else (RESTART if t == 0 else PUSH), np.int32)
            if t == 2:
                act[3] = IDLE                   # stream 3 lags a frame behind from here on
            frame = None if draining else frames_in[t]
            pp, fp, xp = plain.step(frame, act)
            pe, fe, xe = eager.step(frame, act)
            pc_, fc_, xc = cap.step(frame, act)
            assert set(xe) == set(xp) | {"fused", "fused_spread", "fused_count", "fused_used"}
            assert xe["fused"].shape == (2, 17, 3) and xe["fused_spread"].shape == (2, 17) and xe["fused_count"].shape == (2, 17)
            assert xe["fused_used"].shape == (2, 16)
            # everything a run without groups returns, bit for bit (rows of streams without a pose keep what an earlier tick left)
            assert torch.equal(fp, fe) and torch.equal(fp, fc_), t
            live = fp >= 0
            assert torch.equal(pp[live].view(torch.int32), pe[live].view(torch.int32)), t
            assert torch.equal(pe[live].view(torch.int32), pc_[live].view(torch.int32)), t
            _same({k: v[live] if k != "synthetic" else v for k, v in xp.items()},
                  {k: v[live] if k != "synthetic" else v for k, v in xe.items() if k in xp}, xp.keys())
            # the fused outputs: the restatement on this tick's own extras; the captured tick equals the eager one
            got = _check_fused(xe, fe, table, t)
            _same(xe, xc, ("fused", "fused_spread", "fused_count", "fused_used"))
            if live.all():
                assert (got["count"][0] >= 1).all()
            if not live.any():
                assert (got["count"] == 0).all() and (got["fused"] == QNAN64).all()
            fused_both += int((got["count"] == 2).sum())
            synthetic_seen += int((xe["synthetic"] != 0).sum())
            if t == 6:                          # who watches whom changes: the next tick fuses the new groups
                eager.set_groups(regrouped), cap.set_groups(regrouped)
                table = _table(regrouped)
        assert fused_both > 0 and synthetic_seen > 0 and t + 1 == plain.rf + 3 + plain.lag
        pair(NAME)[0].check_status(torch.device(DEV))
    finally:
        cap.release()


def test_lift_clips_returns_the_fused_poses_per_group_and_frame():
    ol = _online(GROUPS, **FUSE)
    rng = np.random.RandomState(33)
    lengths = (5, 5, 7, 3)
    clips = [(0.3 * rng.standard_normal((n, 17, 3))).astype(np.float32) for n in lengths]
    clips[1] = clips[0].copy()
    per_clip, fused = ol.lift_clips(clips, world=True)
    assert len(per_clip) == 4 and [f["fused"].shape[0] for f in fused] == [5, 7]
    table = _table(GROUPS)
    for n in range(7):
        emit = np.array([n if n < N else -1 for N in lengths], np.int64)
        rows = {k: np.stack([per_clip[s][1][k][min(n, lengths[s] - 1)].cpu().numpy() for s in range(4)]) for k in ("world", "reproj", "synthetic")}
        want = restate(rows["world"], rows["reproj"], emit, np.zeros(4, np.int32), rows["synthetic"].view(np.uint32), table,
                       FUSE["fuse_soft_px"], FUSE["fuse_max_px"], FUSE["fuse_max_dist"])
        for g in range(2):
            if n < fused[g]["fused"].shape[0]:
                assert np.array_equal(fc.bits64(fused[g]["fused"][n].cpu().numpy()), want["fused"][g]), (n, g)
                assert np.array_equal(fc.bits64(fused[g]["fused_spread"][n].cpu().numpy()), want["spread"][g]), (n, g)
                assert np.array_equal(fused[g]["fused_count"][n].cpu().numpy(), want["count"][g]), (n, g)
                assert np.array_equal(fc.bits32(fused[g]["fused_used"][n].cpu().numpy()), want["used"][g]), (n, g)
    assert (fused[0]["fused_count"] == 2).all()                    # two cameras fed alike agree exactly


def test_online_lifter_groups_argument_errors():
    import ray3d_amd
    lifter, _ = pair(NAME)
    kw = dict(device=DEV, flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    with pytest.raises(ValueError, match="world=True"):
        ray3d_amd.OnlineLifter(lifter, 4, groups=GROUPS, **kw)
    with pytest.raises(ValueError, match="at most 16"):
        ray3d_amd.OnlineLifter(lifter, 20, world=True, groups=[list(range(17))], **kw)
    with pytest.raises(ValueError, match="outside 0..3"):
        ray3d_amd.OnlineLifter(lifter, 4, world=True, groups=[[0, 4]], **kw)
    with pytest.raises(ValueError, match="groups must be"):
        ray3d_amd.OnlineLifter(lifter, 4, world=True, groups=[], **kw)
    with pytest.raises(ValueError, match="fuse_soft_px"):
        ray3d_amd.OnlineLifter(lifter, 4, world=True, groups=GROUPS, fuse_soft_px=0.0, **kw)
    ol = ray3d_amd.OnlineLifter(lifter, 4, world=True, groups=GROUPS, **kw)
    with pytest.raises(ValueError, match="built for 2 groups"):
        ol.set_groups([[0, 1, 2, 3]])
    with pytest.raises(ValueError, match="groups="):
        ray3d_amd.OnlineLifter(lifter, 4, world=True, **kw).set_groups(GROUPS)
