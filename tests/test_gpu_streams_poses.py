"""GPU suite: r3d_streams_poses (a live tick's finished poses on the device) and OnlineLifter(world=, quality=) on top of it.  The
kernel against the host hook, bit for bit - pred, world, reproj, quality, together and each alone, finished / idle / refused streams,
a non-finite element and a point in the camera's plane included - with every buffer inside guard bands and poisoned; the 2-feature
rule of the Python layer; the flip average against the torch sequence OnlineLifter runs without the options; the call captured
into a hipGraph and replayed over six ticks; OnlineLifter(world=True, quality=True, flip=True) over clips of 5 and 40 frames, eager
and captured: the options-off poses bit for bit, world within 1e-12 of Camera.normalized2world, the residuals bit for bit the NumPy
restatement, the poses within 1e-4 of the oracle chain."""
import functools

import numpy as np
import pytest
import torch

import streams_cases as sc
import streams_poses_cases as pc
from conftest import check_parity
from ray3d_amd import _capi, evaluate
from streams_poses_cases import H36M_LEFT, H36M_RIGHT, OUTPUTS, Rig, bits, restate, same_bits
from test_gpu_streams import pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMIT, STATUS = [3, -1, 0, 2 ** 40, -1, 7], [0, 0, 0, 0, 0, 1]       # three finished, two idle, one refused


def _inputs(J, rf, lag, seed):
    inp = pc.make_inputs(6, J, rf, lag, seed=seed, emit=EMIT, status=STATUS)
    inp["raw"].view(np.uint32)[2, 5, 1] = 0x7FC00BAD                # a NaN with a payload in a finished stream
    inp["raw"][3, 0, 0] = np.inf
    h32 = np.float32(inp["desc"][0, 12])
    inp["desc"][0, 12] = np.float64(h32)                            # stream 0, joint 8: yy == 0 and z == 0 - a point in the camera's plane
    inp["raw"][0, 8] = (0.25, -h32, 0.0)
    inp["raw_m"][0, inp["perm"][8]] = (-0.25, -h32, 0.0)
    inp["raw"][0, 2, 2] = -4.0                                      # ... and one behind it
    return inp


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("J,rf,lag", [(17, 27, 13), (14, 9, 0)])
def test_device_equals_the_host_hook_bit_for_bit(J, rf, lag, flip):
    inp = _inputs(J, rf, lag, 60 + J)
    dev, host = Rig(DEV, inp), Rig("cpu", inp)
    for which in (OUTPUTS, ("pred",), ("world",), ("reproj",), ("reproj", "quality")):
        want = host.call(flip, which)
        _capi.use_hooks(False)
        got = dev.call(flip, which)
        assert want["rc"] == 0
        for k in OUTPUTS:
            assert same_bits(got[k], want[k]), (J, flip, which, k, np.argwhere(bits(got[k]) != bits(want[k]))[:4].tolist())
            fill = pc.FILL32 if k == "pred" else pc.FILL64
            assert (got[k][[1, 4, 5]] == fill).all() and (k in which or (got[k] == fill).all()), (which, k)
        ref = restate(inp, flip, which)
        assert all(same_bits(got[k], ref[k]) for k in which)
    assert bits(got["reproj"])[0, 8] == pc.QNAN64 and (bits(got["quality"])[[0, 2]] == pc.QNAN64).all() and np.isinf(got["quality"][3]).all()


def test_two_feature_inputs_have_pred_and_world_only():
    """The residual is defined for ray inputs: with 2-feature windows the Python layer refuses reproj_dev with R3D_ERR_ARG before
    the call; pred and world do not look at the windows at all."""
    inp = _inputs(17, 9, 4, 77)
    rig = Rig(DEV, inp)
    t = rig.t
    x2 = torch.full((6, 9, 17, 2), float("nan"), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(which):
        a = rig.args(True, which, x=x2.data_ptr())
        _capi.streams_poses(*a, stream, in_features=2)
    for k in OUTPUTS:
        t[k].fill_(-7.0)
    call(("pred", "world"))
    got, ref = rig.read(), restate(inp, True, ("pred", "world"))
    rig.arena.check()
    assert same_bits(got["pred"], ref["pred"]) and same_bits(got["world"], ref["world"])
    with pytest.raises(_capi.Ray3DHipError, match=r"\(-1\).*3-feature"):
        call(("pred", "reproj"))
    rig.arena.check()
    assert same_bits(rig.read()["pred"], ref["pred"]) and (rig.read()["reproj"] == pc.FILL64).all()
    import ray3d_amd
    with pytest.raises(ValueError, match="3-feature"):
        ray3d_amd.OnlineLifter(_f2_lifter(), 2, quality=True, device=DEV)


@functools.lru_cache(maxsize=None)
def _f2_lifter():
    return pair("j17_f2_rf27_noemb_s3")[0]


def test_two_feature_lifter_returns_world_poses():
    import ray3d_amd
    lifter, cams = _f2_lifter(), pc.golden_cameras()
    clip = (0.3 * np.random.RandomState(4).standard_normal((5, 17, 2))).astype(np.float32)
    off = ray3d_amd.OnlineLifter(lifter, 2, device=DEV)
    on = ray3d_amd.OnlineLifter(lifter, 2, device=DEV, world=True)
    with pytest.raises(RuntimeError, match="set_cameras"):
        on.step(np.zeros((2, 17, 2), np.float32))
    want = off.lift_clips([clip])[0]
    (poses, extras), = on.lift_clips([clip], transforms=np.stack([c.stream_pose_row() for c in cams[:2]]), world=True)
    assert torch.equal(poses.view(torch.int32), want.view(torch.int32)) and set(extras) == {"world"}
    assert np.abs(extras["world"].cpu().numpy() - cams[0].normalized2world(poses.cpu().numpy())).max() <= 1e-12


def test_flip_average_has_the_bits_of_the_torch_sequence():
    """pred_dev against 0.5 * (pred + mirror_output(pred_m)) on the same device tensors - what OnlineLifter runs without the options."""
    inp = pc.make_inputs(6, 17, 9, 4, seed=81)
    rig = Rig(DEV, inp)
    got = rig.call(True, ("pred",))["pred"]
    raw, raw_m = rig.t["raw"].reshape(6, 1, 17, 3), rig.t["raw_m"].reshape(6, 1, 17, 3)
    want = 0.5 * (raw + evaluate.mirror_output(raw_m, H36M_LEFT, H36M_RIGHT))
    assert same_bits(got, want[:, 0].cpu().numpy())


def test_the_call_is_captured_and_replayed_over_six_ticks():
    """r3d_streams_poses captured with torch.cuda.graph (default queue settings); six replays with new raw, emit, status and
    transform contents written into the captured buffers equal six eager calls bit for bit."""
    J, rf, lag, S = 17, 9, 4, 6
    ticks = []
    for t in range(6):
        rng = np.random.RandomState(90 + t)
        inp = pc.make_inputs(S, J, rf, lag, seed=100 + t, emit=rng.randint(-1, 3, S), status=rng.randint(0, 2, S))
        inp["desc"][:, 9:12] += t
        ticks.append(inp)
    assert any(((i["status"] == 0) & (i["emit"] >= 0)).any() for i in ticks) and not all(((i["status"] == 0) & (i["emit"] >= 0)).all() for i in ticks)

    def run(rig, launch):
        seen = []
        for inp in ticks:
            rig.write(**{k: inp[k] for k in ("raw", "raw_m", "emit", "status", "desc", "x")})
            launch()
            torch.cuda.synchronize()
            seen.append(rig.read())
        return seen

    stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
    eager, cap = Rig(DEV, ticks[0]), Rig(DEV, ticks[0])
    want = run(eager, lambda: _capi.streams_poses(*eager.args(True), stream()))
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _capi.streams_poses(*cap.args(True), stream())
    torch.cuda.synchronize()
    assert pc.untouched(cap.read())                                 # the capture ran nothing
    got = run(cap, g.replay)
    del g
    torch.cuda.synchronize()
    eager.arena.check(), cap.arena.check()
    for t in range(6):                                              # (outputs accumulate over the ticks on both sides alike)
        for k in OUTPUTS:
            assert same_bits(got[t][k], want[t][k]), (t, k)
    assert not same_bits(want[5]["world"], want[0]["world"])


# ------------------------------------------------------------------ OnlineLifter

NAME = "j17_rf27_s3"
S_LIFT = 3                                            # two clips and a stream that stays idle


@functools.lru_cache(maxsize=None)
def live_case():
    """The clips of 5 and 40 frames of tests/golden/windows.npz (J 17, rays), a camera per stream."""
    clips = [c for c in sc.golden_case("rf27", "centred")[0] if c.shape[0] in (5, 40)]
    assert [c.shape for c in clips] == [(5, 17, 3), (40, 17, 3)]
    cams = pc.golden_cameras()
    return clips, cams, dict(cam_rows=np.stack([c.cam_row(distortion=True) for c in cams]), params=np.stack([c.param() for c in cams]),
                             transforms=np.stack([c.stream_pose_row() for c in cams]))


def _online(**options):
    import ray3d_amd
    lifter, _ = pair(NAME)
    return ray3d_amd.OnlineLifter(lifter, S_LIFT, flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, device=DEV, **options)


@functools.lru_cache(maxsize=None)
def options_off():
    """-> per clip the poses (N, 17, 3) of the lifter without the options (eager)."""
    clips, _, rows = live_case()
    return tuple(p.cpu().numpy() for p in _online().lift_clips(clips, params=rows["params"]))


@functools.lru_cache(maxsize=None)
def oracle_chain():
    """The reference's evaluation of the clips through oracle/torch_port.py, flip-averaged (tests/test_gpu_streams.py's chain)."""
    from oracle import torch_port
    _, ((cp, sp), (ct, st)) = pair(NAME)
    clips, _, rows = live_case()
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]
    rf = cp.receptive_field
    pad = (rf - 1) // 2

    def lift(w, p):
        with torch.no_grad():
            xw, pw = torch.from_numpy(w), torch.from_numpy(p)
            return (torch_port.forward(cp, sds[0], xw, pw) + torch_port.forward(ct, sds[1], xw, pw)).numpy()

    out = []
    for s, c in enumerate(clips):
        n = c.shape[0]
        padded = evaluate.pad_clip(c, pad, 0)
        windows = np.stack([padded[i:i + rf] for i in range(n)])
        prm = np.tile(rows["params"][s].astype(np.float32), (n, 1))
        ref = lift(windows, prm)
        wm = windows.copy()
        wm[..., 0] *= -1
        wm[:, :, H36M_LEFT + H36M_RIGHT] = wm[:, :, H36M_RIGHT + H36M_LEFT]
        refm = lift(wm, prm)
        refm[..., 0] *= -1
        refm[:, :, H36M_LEFT + H36M_RIGHT] = refm[:, :, H36M_RIGHT + H36M_LEFT]
        out.append((0.5 * (ref.astype(np.float64) + refm)).astype(np.float32).reshape(n, -1, 3))
    return out


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_online_lifter_world_and_quality_end_to_end(captured):
    clips, cams, rows = live_case()
    ol = _online(world=True, quality=True)
    with pytest.raises(ValueError, match="transforms"):
        ol.set_cameras(rows["cam_rows"], rows["params"])
    try:
        ol.set_cameras(**rows)
        if captured:
            ol.capture()
        poses, frames, extras = ol.step(np.zeros((S_LIFT, 17, 3), np.float32), [sc.IDLE] * S_LIFT)
        assert frames.tolist() == [-1] * S_LIFT and set(extras) == {"world", "reproj", "quality"}
        assert extras["world"].shape == (S_LIFT, 17, 3) and extras["reproj"].shape == (S_LIFT, 17) and extras["quality"].shape == (S_LIFT, 2)
        assert all(v.dtype == torch.float64 for v in extras.values()) and poses.dtype == torch.float32
        outs = ol.lift_clips(clips, world=True)
        pair(NAME)[0].check_status(torch.device(DEV))
    finally:
        ol.release()
    for s, ((poses, extras), want, ref, clip) in enumerate(zip(outs, options_off(), oracle_chain(), clips)):
        n = clip.shape[0]
        p = poses.cpu().numpy()
        assert same_bits(p, want), ("poses", s)
        assert np.abs(extras["world"].cpu().numpy() - cams[s].normalized2world(p)).max() <= 1e-12
        desc, cam = np.tile(rows["transforms"][s], (n, 1)), np.tile(rows["cam_rows"][s], (n, 1))
        res = pc.reproj_of(desc, cam, p, clip)
        assert same_bits(extras["reproj"].cpu().numpy(), res) and same_bits(extras["quality"].cpu().numpy(), pc.quality_of(res))
        check_parity(p, ref, "clip of %d frames vs the oracle chain" % n)
