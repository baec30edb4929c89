"""GPU suite: r3d_streams_peek (early poses for live streams of centred models) and OnlineLifter(previews=) on top of it.  The
kernel against the host hook, bit for bit - preview windows, mirrored windows, emit, peek_status - over the scenarios of
tests/test_streams_peek_host.py, every buffer inside guard bands and the state compared around every call: RF 27 x 17 joints (459
points: two workgroups per row block, the second part-filled) with F = 3, RF 9 x 14 (126 points: one part-filled workgroup) with
F = 2, with and without the mirrored output, clips longer than RF.  OnlineLifter on the RF-27 fixture pair: the final poses with
previews are those without, bit for bit; the preview poses are lifter.forward on the reference-built prefix windows (bits) and
within 1e-4 of the oracle chain; lift_clips(previews=True); a captured tick against the eager one over the 53 ticks of the clips;
world / quality previews against the r3d_streams_poses host hook; the argument errors."""
import functools

import numpy as np
import pytest
import torch

import streams_cases as sc
import streams_peek_cases as pc
import streams_poses_cases as spc
import streams_repair_cases as rc_cases
from conftest import check_parity, hooks_library
from ray3d_amd import _capi
from streams_cases import FILL, IDLE, NONE, PUSH, RESTART, same_bits
from streams_peek_cases import PeekRig
from test_gpu_streams import H36M_LEFT, H36M_RIGHT, clips_of, pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("x", "x_mirror", "emit", "status", "emit_rest", "status_rest", "state")


def _agree(got, want, what):
    _capi.use_hooks(False)
    assert len(got) == len(want)
    for t, (g, h) in enumerate(zip(got, want)):
        assert h["rc"] == 0, (what, t)
        for k in KEYS:
            a, b = g[k], h[k]
            assert (same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b)), (what, t, k)
        for k in ("x", "x_mirror", "emit", "status"):
            a, b = g["tick"][k], h["tick"][k]
            assert (same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b)), (what, t, "step", k)


# ------------------------------------------------------------------ the kernel against the host hook

@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_device_equals_the_host_hook_on_the_clips(case):
    """The six clips side by side (the 40-frame one wraps both rings), K = 3 with the looks 0 and lag - 1, mirrored: every tick's
    peek equals the hook's, and the restatement holds on the device as it does on the host (pc.run's checks)."""
    clips, rf, lag, perm, _, _ = sc.golden_case(case, "centred")
    J, F = clips[0].shape[1:]
    frames, actions = pc.clip_schedule(clips, lag)
    runs = [pc.run(PeekRig(d, len(clips), rf, lag, J, F, pc.looks_of(lag), NONE, perm), frames, actions) for d in (DEV, "cpu")]
    _agree(runs[0], runs[1], case)
    assert max(int(o["emit"].max()) for o in runs[0]) == 39 and any((o["emit"] >= 0).any() and (o["emit"] < 0).any() for o in runs[0])


@pytest.mark.parametrize("use_action", [True, False], ids=["actions", "no-actions"])
@pytest.mark.parametrize("mirror", [True, False], ids=["mirror", "plain"])
@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_device_equals_the_host_hook_on_mixed_actions(case, mirror, use_action):
    """IDLE, RESTART, DRAIN and refused streams on a state of 0xA5 bytes, RF + 8 ticks, with and without the mirrored output and the
    action words."""
    clips, rf, lag, perm, _, _ = sc.golden_case(case, "centred")
    J, F = clips[0].shape[1:]
    frames, actions = pc.mixed_schedule(6, J, F, lag, rf, rf + 8)
    runs = [pc.run(PeekRig(d, 6, rf, lag, J, F, pc.looks_of(lag), NONE, perm), frames, actions, use_action=use_action, mirror=mirror)
            for d in (DEV, "cpu")]
    _agree(runs[0], runs[1], (case, mirror, use_action))
    st = np.stack([o["status"][0] for o in runs[0]])
    assert (st[:, 4] == 1).all() and (st[:, 5] == 1).all() and st[5, 3] == 1 and (st[:, 0] == 0).all()


def test_one_look_and_eight_looks():
    """K = 1 (grid z of one) and K = R3D_STREAMS_PEEK_MAX on RF 27 (lag 13): the device equals the hook."""
    clips, rf, lag, perm, _, _ = sc.golden_case("rf27", "centred")
    J, F = clips[0].shape[1:]
    frames, actions = pc.clip_schedule(clips[4:], lag, extra_idle=0)
    for looks in ((lag - 1,), (0, 1, 2, 3, 5, 8, 11, 12)):
        runs = [pc.run(PeekRig(d, 2, rf, lag, J, F, looks, NONE, perm), frames[:30], actions[:30]) for d in (DEV, "cpu")]
        _agree(runs[0], runs[1], looks)


def test_device_entry_point_argument_errors():
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    for looks, lag, message in (((0, 13), 13, r"looks\[1\] must be in 0..lag - 1 = 12"), ((3, 3), 13, "strictly increasing"), ((), 13, "num_looks"),
                                (tuple(range(9)), 13, "num_looks must be in 1..8"), ((0,), 0, "causal")):
        with pytest.raises(_capi.Ray3DHipError, match=message):
            _capi.streams_peek(p, 1, 27, lag, 17, 3, looks, None, p, p, None, None, p, p, stream)
    torch.cuda.synchronize()
    assert not t.any()


# ------------------------------------------------------------------ OnlineLifter

NAME = "j17_rf27_s3"
S_LIFT = 3                                            # two clips (5 and 40 frames) and a stream that stays idle
LOOKS = (0, 6, 12)


def _online(previews=LOOKS, S=S_LIFT, **options):
    import ray3d_amd
    lifter, _ = pair(NAME)
    ol = ray3d_amd.OnlineLifter(lifter, S, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, device=DEV, previews=previews, **options)
    _, params = clips_of(NAME)
    if params is not None and not options.get("world") and not options.get("quality"):
        ol.set_cameras(params=params[:S])
    return lifter, ol


@functools.lru_cache(maxsize=None)
def plain_run():
    """previews=None, eager, no flip -> per clip its final poses (N, 17, 3) as NumPy."""
    _, ol = _online(previews=None)
    return tuple(p.cpu().numpy() for p in ol.lift_clips(clips_of(NAME)[0]))


@functools.lru_cache(maxsize=None)
def preview_run():
    """previews=LOOKS, eager, no flip -> (per clip (poses, extras) as lift_clips(previews=True) returns them, and per tick what
    the lifter's preview buffers held: (the step's result, px, pemit))."""
    lifter, ol = _online()
    ticks, plain = [], ol.step

    def recording(frame=None, actions=None, check=True):
        res = plain(frame, actions, check)
        ticks.append((res, ol.px.clone(), ol.pemit.clone(), ol.x.clone(), ol.emit.clone()))
        return res
    ol.step = recording
    outs = ol.lift_clips(clips_of(NAME)[0], previews=True)
    lifter.check_status(torch.device(DEV))
    return outs, ticks


def test_final_poses_with_previews_are_those_without_bit_for_bit():
    outs, ticks = preview_run()
    for (poses, extras), want in zip(outs, plain_run()):
        assert same_bits(poses.cpu().numpy(), want)
    assert len(ticks) == 40 + 13
    for res, _, _, _, _ in ticks:
        assert len(res) == 3 and [p["look"] for p in res[2]["previews"]] == list(LOOKS)
        assert all(p["poses"].shape == (S_LIFT, 17, 3) and p["frames"].shape == (S_LIFT,) and p["frames"].dtype == torch.int64
                   for p in res[2]["previews"])


def test_preview_poses_are_forward_on_the_reference_prefix_windows():
    """Every tick: the rows of the K * S preview batch that preview hold, bit for bit, window c - 1 - L of the reference's builder
    (edge padding + slicing, tests/streams_repair_cases.py) on the stream's prefix clip[:c]; the preview poses are the bits of
    lifter.forward on that batch - the reference-built windows in the same rows - and the frames are c - 1 - L."""
    lifter, _ = pair(NAME)
    clips, params = clips_of(NAME)
    _, ticks = preview_run()
    K, rf, lag = len(LOOKS), 27, 13
    tiled = torch.from_numpy(np.tile(params, (K, 1))).to(DEV) if params is not None else None
    previewed = 0
    for t, (res, px, pemit, _, _) in enumerate(ticks):
        batch = px.clone()
        for k, L in enumerate(LOOKS):
            frames = res[2]["previews"][k]["frames"].tolist()
            assert frames == pemit[k].tolist()
            for s in range(S_LIFT):
                c = t + 1
                want = c - 1 - L if s < len(clips) and c <= clips[s].shape[0] and c - 1 - L >= 0 else -1
                assert frames[s] == want, (t, k, s)
                if want >= 0:
                    w = rc_cases.reference_windows(clips[s][:c], rf, lag)[want]
                    assert same_bits(px[k, s].cpu().numpy(), w), (t, k, s)
                    batch[k, s] = torch.from_numpy(w).to(DEV)
                    previewed += 1
        with torch.no_grad():
            want_poses = lifter.forward(batch.view(K * S_LIFT, rf, 17, 3), tiled)[:, 0].view(K, S_LIFT, 17, 3)
        for k in range(K):
            assert torch.equal(res[2]["previews"][k]["poses"].view(torch.int32), want_poses[k].view(torch.int32)), (t, k)
    assert previewed == sum(max(c.shape[0] - L, 0) for c in clips for L in LOOKS)


def test_preview_poses_agree_with_the_oracle_chain():
    """The reference's evaluation of every prefix that previews (oracle/torch_port.py on window c - 1 - L of clip[:c]): the
    collected preview poses of lift_clips(previews=True) are within the literal 1e-4."""
    from oracle import torch_port
    _, ((cp, sp), (ct, st)) = pair(NAME)
    clips, params = clips_of(NAME)
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]
    outs, _ = preview_run()
    rf, lag = 27, 13
    wins, prm, got = [], [], []
    for s, (clip, (_, extras)) in enumerate(zip(clips, outs)):
        assert [p["look"] for p in extras["previews"]] == list(LOOKS)
        for p in extras["previews"]:
            L = p["look"]
            assert p["poses"].shape == (max(clip.shape[0] - L, 0), 17, 3)
            for n in range(clip.shape[0] - L):
                wins.append(rc_cases.reference_windows(clip[:n + L + 1], rf, lag)[n])
                prm.append(params[s])
            got.append(p["poses"].cpu().numpy())
    with torch.no_grad():
        xw, pw = torch.from_numpy(np.stack(wins)), torch.from_numpy(np.stack(prm))
        ref = (torch_port.forward(cp, sds[0], xw, pw) + torch_port.forward(ct, sds[1], xw, pw)).numpy().reshape(-1, 17, 3)
    check_parity(np.concatenate(got), ref, "preview poses vs the oracle chain")


def test_lift_clips_previews_lengths_and_the_one_frame_clip():
    """Per look the frames 0 .. N - 1 - L (none for N <= L); and for a one-frame clip on one stream with the look 0 the preview
    batch is the final batch - the same window, the same batch size - so its pose is the final pose, bit for bit."""
    clips, params = clips_of(NAME)
    outs, _ = preview_run()
    for clip, (poses, extras) in zip(clips, outs):
        assert [p["poses"].shape[0] for p in extras["previews"]] == [max(clip.shape[0] - L, 0) for L in LOOKS]
    assert [p["poses"].shape[0] for p in outs[0][1]["previews"]] == [5, 0, 0]
    _, ol = _online(previews=(0,), S=1)
    (poses, extras), = ol.lift_clips([clips[1][:1]], previews=True)
    assert poses.shape == (1, 17, 3) and extras["previews"][0]["poses"].shape == (1, 17, 3)
    assert torch.equal(poses.view(torch.int32), extras["previews"][0]["poses"].view(torch.int32))
    with pytest.raises(ValueError, match="previews=True needs"):
        _online(previews=None)[1].lift_clips([clips[0]], previews=True)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_a_captured_tick_with_previews_equals_the_eager_one(flip):
    """capture() records the longer tick; over the 53 ticks of the clips the replayed finals and previews have the eager bits."""
    clips, _ = clips_of(NAME)
    lifter, eager = _online(flip=flip)
    _, cap = _online(flip=flip)
    try:
        want = eager.lift_clips(clips, previews=True)
        cap.capture()
        got = cap.lift_clips(clips, previews=True)
        lifter.check_status(torch.device(DEV))
    finally:
        cap.release()
    for (a, ea), (b, eb) in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        for pa, pb in zip(ea["previews"], eb["previews"]):
            assert pa["look"] == pb["look"] and torch.equal(pa["poses"].view(torch.int32), pb["poses"].view(torch.int32))
    if not flip:
        for (a, _), w in zip(got, plain_run()):
            assert same_bits(a.cpu().numpy(), w)


def test_world_and_quality_previews_equal_the_streams_poses_host_hook():
    """OnlineLifter(world=True, quality=True, flip=True, previews=): the K * S pseudo-streams' pred, world, reproj and quality are
    what r3d_debug_streams_poses_host computes from the same raw outputs, peek words, tiled rows and preview windows."""
    import test_gpu_streams_poses as tp
    clips, cams, rows = tp.live_case()
    _, ol = _online(flip=True, world=True, quality=True)
    ol.set_cameras(**rows)
    K, KS, J = len(LOOKS), len(LOOKS) * S_LIFT, 17
    frame = np.zeros((S_LIFT, J, 3), np.float32)
    checked = 0
    for t in range(16):
        frame[0], frame[1] = clips[0][min(t, 4)], clips[1][t]
        act = [RESTART if t == 0 else (PUSH if t < 5 else IDLE), RESTART if t == 0 else PUSH, IDLE]
        poses, frames, extras = ol.step(frame, act)
        if t not in (0, 5, 6, 12, 15):
            continue
        f = ol._pfinish
        h = {k: v.cpu().numpy().copy() for k, v in (("raw", f["raw"]), ("raw_m", f["raw_m"]), ("emit", ol.pemit), ("status", ol.pstatus),
                                                   ("desc", ol._ptiled["transforms"]), ("cam", ol._ptiled["cam_rows"]), ("x", ol.px))}
        assert same_bits(h["desc"], np.tile(rows["transforms"], (K, 1))) and same_bits(h["cam"], np.tile(rows["cam_rows"], (K, 1)))
        out = dict(pred=np.full((KS, J, 3), -7, np.float32), world=np.full((KS, J, 3), -7.0), reproj=np.full((KS, J), -7.0),
                   quality=np.full((KS, 2), -7.0))
        hooks_library()
        rc = _capi.debug_streams_poses_host(h["raw"].ctypes.data, h["raw_m"].ctypes.data, KS, J, ol._out_perm_host, h["emit"].ctypes.data,
                                            h["status"].ctypes.data, h["desc"].ctypes.data, h["cam"].ctypes.data, h["x"].ctypes.data, ol.rf, ol.lag,
                                            out["pred"].ctypes.data, out["world"].ctypes.data, out["reproj"].ctypes.data, out["quality"].ctypes.data)
        _capi.use_hooks(False)
        assert rc == 0 and (h["status"] == 0).all()
        for k, pv in enumerate(extras["previews"]):
            assert set(pv) == {"look", "poses", "frames", "world", "reproj", "quality"} and pv["frames"].tolist() == h["emit"][k].tolist()
            for s in np.nonzero(h["emit"][k] >= 0)[0]:
                for name, key in (("pred", "poses"), ("world", "world"), ("reproj", "reproj"), ("quality", "quality")):
                    assert spc.same_bits(pv[key][s].cpu().numpy(), out[name][k * S_LIFT + s]), (t, k, s, name)
                checked += 1
        assert set(extras) == {"world", "reproj", "quality", "previews"}
    assert checked == 2 * 1 + 1 * 1 + 2 + 3 + 3       # ticks 0 (two streams, look 0), 5 (stream 0 idles), 6, 12, 15


def test_online_lifter_preview_argument_errors():
    import ray3d_amd
    lifter, _ = pair(NAME)
    for bad, message in (((0, 13), r"0\.\.12 = lag - 1"), ((-1,), r"0\.\.12 = lag - 1"), ((3, 3), "strictly increasing"), ((5, 2), "strictly increasing"),
                         ((), "1..8 ints"), (tuple(range(9)), "1..8 ints"), ((1.5,), "1..8 ints"), (3, "1..8 ints"), ((True,), "1..8 ints")):
        with pytest.raises(ValueError, match=message):
            ray3d_amd.OnlineLifter(lifter, 2, device=DEV, previews=bad)
    causal, _ = pair("j17_rf81_causal_s3")
    with pytest.raises(ValueError, match=r"causal \(lag 0\).*0\.\.lag - 1"):
        ray3d_amd.OnlineLifter(causal, 2, device=DEV, previews=(0,))
    ol = ray3d_amd.OnlineLifter(lifter, 2, device=DEV)         # previews=None: the return values are what they were
    ol.set_cameras(params=np.zeros((2, lifter.pos.extrinsic_dim), np.float32))
    assert len(ol.step(np.zeros((2, 17, 3), np.float32))) == 2 and ol.looks is None
