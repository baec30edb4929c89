"""GPU suite: r3d_streams_link (one person across cameras) and OnlineLifter(cameras=, people=) on top of it.  The kernel against the
host hook, bit for bit, outputs and state after every tick of the seeded multi-tick cases of tests/streams_link_cases.py - every
shape from 1 x 1 x 1 x 1 to 16 cameras, 32 slots and 32 people, non-finite rows, streams that did not finish, identities that change,
bit-identical candidates, a state of 0xA5 bytes and one with a stream linked twice - with every buffer inside guard bands and
poisoned outputs; the optional outputs left out; the call captured into a hipGraph and replayed on new inputs; OnlineLifter.track
with people= on the j17_rf9_s1 fixture pair, 2 scenes x 2 cameras x 3 slots, eager and captured, against a second OnlineLifter built
with groups= that receives the NumPy restatement's member table."""
import numpy as np
import pytest
import torch

import buffers_util as bu
import streams_link_cases as lc
from streams_link_cases import LinkRig, agree
from ray3d_amd import _capi
from test_gpu_streams import pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAME = "j17_rf9_s1"


# ------------------------------------------------------------------ the kernel against the host hook

@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "N%d-C%d-P%d-G%d" % s)
def test_device_equals_the_host_hook_bit_for_bit(shape):
    for key in [k for k in lc.case_ids() if k[:4] == shape]:
        case, want = lc.host_run(*key)
        rig = LinkRig(DEV, case, pattern=bu.NANS if key[4] == 17 else bu.ZEROS)
        for t, tick in enumerate(case["ticks"]):
            rc, got = rig.run(tick)                                  # (run() checks the guards around every buffer)
            assert rc == 0
            agree(got, want[t], (key, t))


def test_optional_outputs_left_out_stay_untouched():
    key = [k for k in lc.case_ids() if k[:4] == (2, 3, 5, 3)][-1]
    case, want = lc.host_run(*key)
    for left_out in (("group",), ("stats",), ("group", "stats")):
        rig = LinkRig(DEV, case)
        for t, tick in enumerate(case["ticks"]):
            rc, got = rig.run(tick, **{k: None for k in left_out})
            for k in lc.OUT_KEYS + ("state",):
                if k in left_out:
                    assert lc.poisoned(got[k]), (left_out, k, t)
                else:
                    assert np.array_equal(got[k], want[t][k]), (left_out, k, t)


def test_the_call_is_captured_and_replayed_on_new_inputs():
    """One launch, no allocation, no copy: captured into a hipGraph once, then every tick of a case is a replay on new inputs."""
    key = [k for k in lc.case_ids() if k[:4] == (1, 2, 3, 4)][-1]
    case, want = lc.host_run(*key)
    rig = LinkRig(DEV, case)
    dev = torch.device(DEV)
    state0 = rig.t["state"].clone()
    rig.load(case["ticks"][0])
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _capi.streams_link(*rig.ptrs(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    rig.t["state"].copy_(state0)                                     # (a capture does not run the launch; the state starts over anyway)
    for t, tick in enumerate(case["ticks"]):
        rig.load(tick)
        rig.poison()
        g.replay()
        rig.arena.check()
        agree(rig.read(), want[t], t)
    del g


# ------------------------------------------------------------------ OnlineLifter(cameras=, people=).track

N_LIVE, C_LIVE, P_LIVE, D_LIVE, G_LIVE, J_LIVE = 2, 2, 3, 4, 2, 17
CAMS = N_LIVE * C_LIVE
S_LIVE = CAMS * P_LIVE
TICKS = 40
ASSIGN_MISSED, LINK_MISSED = 2, 3
# The fixture model is untrained: its world poses carry no geometry.  So the people stand still and both cameras of a scene are the
# SAME camera: a person's window is then the same frame nine times over - at its first pose, in the middle of its track, through a
# repaired gap and in its drain alike - and its world pose the same bits in both cameras and on every tick, while two people's
# poses differ by whatever the model makes of two different inputs.  1 mm separates the two.
LINK = dict(link_max_dist=1e-3, link_break_dist=0.0, link_max_missed=LINK_MISSED)
FUSE = dict(fuse_soft_px=2.0, fuse_max_px=0.0, fuse_max_dist=0.5)


def _detections():
    """Per tick (det (4, D, J, 3) model-input rows, counts (4,)).  Per scene: person A in both cameras all the way; person B in both
    from tick 2, gone from tick 8 (its tracks end and drain, the person is left without a link), back on tick 12 on new tracks
    (they finish their first pose on tick 16: the re-join), gone for good from tick 24 (the person is freed); in scene 0 a third
    person E on camera 0 from tick 18 to 23, while A and B hold the scene's two people (a dropped candidate).  The rows shuffled."""
    rng = np.random.RandomState(43)
    shape = 0.25 * np.random.RandomState(7).uniform(-0.5, 0.5, (17, 2))[:J_LIVE]
    homes = {"A": (-0.6, -0.3), "B": (0.2, 0.3), "E": (0.7, -0.4)}
    out = []
    for t in range(TICKS):
        det = np.full((CAMS, D_LIVE, J_LIVE, 3), np.nan, np.float32)
        counts = np.zeros(CAMS, np.int32)
        for cam in range(CAMS):
            n, c = divmod(cam, C_LIVE)
            who = ["A"] + (["B"] if 2 <= t < 8 or 12 <= t < 24 else []) + (["E"] if n == 0 and c == 0 and 18 <= t < 24 else [])
            rows = [np.concatenate([np.array(homes[w]) + shape, np.ones((J_LIVE, 1))], -1).astype(np.float32) for w in who]
            rng.shuffle(rows)
            for d, row in enumerate(rows):
                det[cam, d] = row
            counts[cam] = len(rows)
        out.append((det, counts))
    return out


def _lifters():
    import ray3d_amd
    import streams_poses_cases as pc
    lifter, _ = pair(NAME)
    cams = pc.golden_cameras()
    cams = [cams[(cam // C_LIVE) % len(cams)] for cam in range(CAMS) for _ in range(P_LIVE)]      # one camera per scene
    rows = dict(cam_rows=np.stack([c.cam_row(distortion=True) for c in cams]), transforms=np.stack([c.stream_pose_row() for c in cams]))
    if lifter.pos.camera_embedding:
        rows["params"] = np.stack([c.param() for c in cams])
    kw = dict(device=DEV, world=True, quality=True, repair=2, cameras=CAMS, max_detections=D_LIVE, assign_max_missed=ASSIGN_MISSED, **FUSE)
    ols = [ray3d_amd.OnlineLifter(lifter, S_LIVE, groups=[[] for _ in range(N_LIVE * G_LIVE)], **kw),
           ray3d_amd.OnlineLifter(lifter, S_LIVE, people=G_LIVE, scenes=N_LIVE, **LINK, **kw),
           ray3d_amd.OnlineLifter(lifter, S_LIVE, people=G_LIVE, scenes=N_LIVE, **LINK, **kw)]
    for ol in ols:
        ol.set_cameras(**rows)
    return ols


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    view = {8: torch.int64, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.contiguous().view(view), b.contiguous().view(view)), what


def test_online_lifter_links_people_eager_and_captured():
    """40 ticks of 2 scenes x 2 cameras x 3 slots: the member table, person_id, stream_person and link_stats of track() with people= -
    eager and captured - are the restatement's on the tick's own world poses and track identities; the fused outputs equal
    r3d_streams_fuse run with that table on the buffers of a lifter built with groups=; everything else equals that lifter's
    tick, bit for bit."""
    ref, eager, cap = _lifters()
    NG = N_LIVE * G_LIVE
    prm = dict(N=N_LIVE, C=C_LIVE, P=P_LIVE, G=G_LIVE, M=16, J=J_LIVE, min_joints=4, min_common=3, max_missed=LINK_MISSED,
               max_dist=LINK["link_max_dist"], break_dist=0.0)
    st = lc.unpack_state(np.zeros(lc.state_bytes(N_LIVE, C_LIVE, G_LIVE, J_LIVE), np.uint8), N_LIVE, C_LIVE, G_LIVE, J_LIVE)
    dev = torch.device(DEV)
    two = unlinked = rejoined = freed = dropped = 0
    before = None
    try:
        cap.capture()
        for t, (det, counts) in enumerate(_detections()):
            pp, fp, xp = ref.track(det, counts)
            want = lc.restate(st, prm, xp["world"].cpu().numpy(), fp.cpu().numpy(), ref.status.cpu().numpy(), xp["track_id"].cpu().numpy())
            # the lifter built with groups= gets this tick's table, and r3d_streams_fuse runs again on its buffers
            ref.member.copy_(torch.from_numpy(want["member"]))
            f, z = ref._finish, ref._fuse
            with torch.cuda.device(dev):
                _capi.streams_fuse(f["world"].data_ptr(), f["reproj"].data_ptr(), ref.emit.data_ptr(), ref.status.data_ptr(),
                                   ref.synthetic.data_ptr(), S_LIVE, J_LIVE, ref.member.data_ptr(), NG, 16, FUSE["fuse_soft_px"],
                                   FUSE["fuse_max_px"], FUSE["fuse_max_dist"], z["fused"].data_ptr(), z["fused_spread"].data_ptr(),
                                   z["fused_count"].data_ptr(), z["fused_used"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize(dev)
            for name, ol in (("eager", eager), ("captured", cap)):
                p, fr, x = ol.track(det, counts)
                assert set(x) == set(xp) | {"person_id", "stream_person", "link_stats"}, (name, t)
                assert torch.equal(fr, fp), (name, t)
                # (OnlineLifter.step leaves poses[s] unspecified where frames[s] is -1 - stream s has no pose this tick, the row "is
                # not meaningful" -, so the rows that ARE poses are compared, as tests/test_gpu_streams_assign.py does)
                live = (fp >= 0).cpu()
                _same(p.cpu()[live], pp.cpu()[live], (name, t, "poses"))
                for k, v in xp.items():
                    _same(x[k], z[k] if k.startswith("fused") else v, (name, t, k))
                assert x["person_id"].dtype == torch.int64 and x["stream_person"].dtype == torch.int32 and x["link_stats"].shape == (N_LIVE, 4)
                assert np.array_equal(x["person_id"].cpu().numpy(), want["person"]), (name, t)
                assert np.array_equal(x["stream_person"].cpu().numpy(), want["group"]), (name, t)
                assert np.array_equal(x["link_stats"].cpu().numpy(), want["stats"]), (name, t)
                assert np.array_equal(ol.member.cpu().numpy(), want["member"]), (name, t)
            # what the script is there for, from the restatement alone
            members = (want["member"] >= 0).sum(1)
            two += int((members >= 2).sum())
            dropped += int(want["stats"][:, 3].sum())
            if before is not None:
                same = (before["person"] >= 0) & (before["person"] == want["person"])
                was = (before["member"] >= 0).sum(1)
                ended = xp["track_id"].cpu().numpy() < 0
                unlinked += int(sum(ended[s] for s in before["member"][before["member"] >= 0]))
                rejoined += int((same & (was == 0) & (members > 0)).sum())
                freed += int(((before["person"] >= 0) & (want["person"] < 0)).sum())
            before = want
        print("two %d unlinked %d rejoined %d freed %d dropped %d" % (two, unlinked, rejoined, freed, dropped))
        assert two > 0 and unlinked > 0 and rejoined > 0 and freed > 0 and dropped > 0
        pair(NAME)[0].check_status(dev)
        with pytest.raises(ValueError, match="track\\(\\) only"):
            cap.step(np.zeros((S_LIVE, J_LIVE, 3), np.float32))
    finally:
        cap.release()


def test_online_lifter_people_argument_errors():
    import ray3d_amd
    lifter, _ = pair(NAME)
    kw = dict(device=DEV, world=True, repair=2, cameras=4, max_detections=4, people=2, scenes=2)
    for bad, word in ((dict(cameras=None, max_detections=None), "needs cameras="), (dict(world=False), "needs cameras="),
                      (dict(groups=[[0, 1]]), "excludes groups="), (dict(people=0), "people must be"), (dict(people=33), "people must be"),
                      (dict(people=2.0), "people must be"), (dict(scenes=3), "scenes \\* C"), (dict(scenes=0), "scenes \\* C"),
                      (dict(link_max_dist=0.0), "link_max_dist"), (dict(link_max_dist=float("nan")), "link_max_dist"),
                      (dict(link_break_dist=0.25), "link_break_dist"), (dict(link_break_dist=float("inf")), "link_break_dist"),
                      (dict(link_max_missed=-1), "link_max_missed"), (dict(link_min_joints=0), "link_min_joints"),
                      (dict(link_min_common=18), "link_min_joints")):
        with pytest.raises(ValueError, match=word):
            ray3d_amd.OnlineLifter(lifter, 12, **dict(kw, **bad))
    with pytest.raises(ValueError, match="scenes \\* C"):
        ray3d_amd.OnlineLifter(lifter, 34, **dict(kw, cameras=17, scenes=1))        # 17 cameras in one scene
    ol = ray3d_amd.OnlineLifter(lifter, 12, **kw)
    assert ol.G == 4 and ol.member.shape == (4, 16) and (ol.member == -1).all()
    with pytest.raises(ValueError, match="people="):
        ol.set_groups([[0], [1], [2], [3]])
    with pytest.raises(ValueError, match="track\\(\\) only"):
        ol.lift_clips([np.zeros((3, 17, 3), np.float32)])
    import streams_poses_cases as pc
    cams = [pc.golden_cameras()[0]] * 12
    rows = dict(transforms=np.stack([c.stream_pose_row() for c in cams]))
    if lifter.pos.camera_embedding:
        rows["params"] = np.stack([c.param() for c in cams])
    ol.set_cameras(**rows)
    with pytest.raises(ValueError, match="track\\(\\) only"):
        ol.step(np.zeros((12, 17, 3), np.float32))
    p, f, x = ol.track(np.full((4, 4, 17, 3), np.nan), [4, 4, 4, 4])       # nothing valid: no tracks, no people
    assert (f == -1).all() and (x["person_id"] == -1).all() and (x["stream_person"] == -1).all() and (x["link_stats"] == 0).all()
    assert x["fused_count"].shape == (4, 17) and (x["fused_count"] == 0).all()
