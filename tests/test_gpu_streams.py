"""GPU suite: r3d_streams_step (live streams lifted a frame at a time) and OnlineLifter on top of it.  The kernel's two launches
against the host hook, bit for bit - windows, mirrored windows, emit, status and the whole state, refusals included - with every
buffer inside guard bands and a state nobody zeroed; the ring rows of the pixel encodings against r3d_clips_encode; the call
captured into a hipGraph and replayed over ten ticks; OnlineLifter.lift_clips against lifter.forward on each tick's windows (bits)
and against the oracle chain over whole clips (1e-4), plain and flip-averaged, eager and captured.  S = 6 streams for the kernel
(the clips of tests/golden/windows.npz: 1, 2, 5, 13, 14 and 40 frames), RF 27 / RF 9; S = 3 for the lifter (clips of 5 and 40)."""
import functools

import numpy as np
import pytest
import torch

import streams_cases as sc
from conftest import case_out_scale, check_parity, load_model_fixture, synth_states
from ray3d_amd import _capi, evaluate
from streams_cases import DRAIN, FILL, IDLE, NONE, PUSH, RESTART, Rig, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H36M_LEFT, H36M_RIGHT = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
KEYS = ("x", "x_mirror", "emit", "status", "state")


def _agree(got, want, what):
    _capi.use_hooks(False)
    assert want["rc"] == 0, what
    for k in KEYS:
        a, b = got[k], want[k]
        assert (same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b)), (what, k)


# ------------------------------------------------------------------ the kernel against the host hook

@pytest.mark.parametrize("shift", ["centred", "causal"])
@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_device_equals_the_host_hook_bit_for_bit(case, shift):
    """The six clips side by side (RESTART, PUSH ..., DRAIN x lag, IDLE) on a poisoned state, then one tick of refusals - an
    unknown action, a PUSH after the drain, a corrupted head - beside a RESTART, an IDLE and a DRAIN: every tick's windows,
    mirrored windows, emit, status and state equal the hook's, and the emitted windows are the reference's."""
    clips, rf, lag, perm, want, want_mirror = sc.golden_case(case, shift)
    J, F = clips[0].shape[1:]
    dev, host = Rig(DEV, len(clips), rf, lag, J, F, NONE, perm), Rig("cpu", len(clips), rf, lag, J, F, NONE, perm)
    got, ref = sc.run_clips(dev, clips), sc.run_clips(host, clips)
    emitted = [0] * len(clips)
    for t, (g, h) in enumerate(zip(got, ref)):
        _agree(g, h, (case, shift, t))
        for s in np.nonzero(g["emit"] >= 0)[0]:
            n = int(g["emit"][s])
            assert same_bits(g["x"][s], want[s][n]) and same_bits(g["x_mirror"][s], want_mirror[s][n])
            emitted[s] += 1
        assert (g["x"][g["emit"] < 0] == FILL).all() and (g["x_mirror"][g["emit"] < 0] == FILL).all()
    assert emitted == [c.shape[0] for c in clips]
    frame = np.random.RandomState(6).standard_normal((len(clips), J, F)).astype(np.float32)
    act = np.array([9, PUSH, DRAIN, RESTART, IDLE, DRAIN], np.int32)
    for rig in (dev, host):
        rig.set_head(2, 2 ** 62 + 1, 0)
    g, h = dev.tick(frame, act), host.tick(frame, act)
    g["state"], h["state"] = dev.state()[2], host.state()[2]
    _agree(g, h, (case, shift, "refusals"))
    assert g["status"].tolist() == [1, 1 if lag else 0, 1, 0, 0, 0]
    assert g["emit"][0] == -1 and g["emit"][2] == -1 and (g["x"][[0, 2]] == FILL).all()
    for k, (count, drained) in enumerate(((-1, 0), (5, lag + 1))):
        for rig in (dev, host):
            rig.set_head(4, count, drained)
        act = np.array([IDLE, IDLE, RESTART, PUSH, PUSH if k else DRAIN, IDLE], np.int32)
        g, h = dev.tick(frame, act), host.tick(frame, act)
        g["state"], h["state"] = dev.state()[2], host.state()[2]
        _agree(g, h, (case, shift, "corrupted head", k))
        assert g["status"].tolist() == [0, 0, 0, 0, 1, 0] and dev.state()[0][4].tolist() == (count, drained)


@pytest.mark.parametrize("encoding,rf,lag", [("ray", 27, 13), ("intrinsic", 9, 0), ("screen", 9, 4)])
def test_pixel_rings_hold_what_clips_encode_writes(encoding, rf, lag):
    """Pixels through distorted H36M camera rows: every tick equals the hook's, and the ring rows are, bit for bit, what
    r3d_clips_encode writes on the device for the same pixels and camera row."""
    from test_clips_encode_host import cameras, pixels
    J, S, N = 17, 6, 12
    enc = evaluate.ENCODINGS[encoding]
    F = _capi.ENCODE_FLOATS[enc]
    rows = np.stack([cameras()[s % 4].cam_row(distortion=True) for s in range(S)])
    assert np.abs(rows[:, 8:13]).max() > 0
    px = pixels("streams.gpu.%s" % encoding, (S, N, J, 2))
    perm = evaluate.mirror_permutation(J, H36M_LEFT, H36M_RIGHT)
    dev, host = Rig(DEV, S, rf, lag, J, F, enc, perm, cam_rows=rows), Rig("cpu", S, rf, lag, J, F, enc, perm, cam_rows=rows)
    for t in range(N + lag):
        act = np.full(S, RESTART if t == 0 else (PUSH if t < N else DRAIN), np.int32)
        frame = px[:, t] if t < N else sc.garbage_frame(S, J, 2)
        g, h = dev.tick(frame, act), host.tick(frame, act)
        g["state"], h["state"] = dev.state()[2], host.state()[2]
        _agree(g, h, (encoding, t))
        assert (g["status"] == 0).all()
    ring = dev.state()[1]
    tdev = torch.device(DEV)
    for s in range(S):
        table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
        table[0]["n_frames"], table[0]["cam"] = N, rows[s]
        x = torch.full((N, J, F), float(FILL), device=tdev)
        status = torch.full((1,), -1, dtype=torch.int32, device=tdev)
        p_dev, t_dev = torch.from_numpy(px[s].copy()).to(tdev), torch.from_numpy(table.view(np.uint8)).to(tdev)
        _capi.clips_encode(p_dev.data_ptr(), N, J, enc, t_dev.data_ptr(), 1, N, x.data_ptr(), N, None, None, status.data_ptr(),
                           torch.cuda.current_stream(tdev).cuda_stream)
        want = x.cpu().numpy()
        assert status.tolist() == [0]
        for f in range(max(0, N - rf), N):
            assert same_bits(ring[s, f % rf], want[f]), (s, f)


def test_the_call_is_captured_and_replayed_over_ten_ticks():
    """r3d_streams_step captured with torch.cuda.graph (default queue settings); ten replays with new contents written into the
    captured frame and action buffers equal ten eager calls bit for bit: windows, mirrored windows, emit, status, state."""
    S, rf, lag, J, F = 6, 9, 4, 14, 2
    perm = evaluate.mirror_permutation(J, [4, 5, 6, 10, 11], [1, 2, 3, 12, 13])
    tdev = torch.device(DEV)
    rng = np.random.RandomState(12)
    frames = rng.standard_normal((10, S, J, F)).astype(np.float32)
    acts = np.full((10, S), PUSH, np.int32)
    acts[0] = RESTART
    acts[3:7, 0], acts[7, 0] = DRAIN, RESTART          # stream 0: a clip of 3 frames, its drain, the next clip
    acts[2, 1] = acts[5, 1] = IDLE                     # stream 1 skips ticks
    acts[6:, 2] = DRAIN                                # stream 2 drains to the end (and past it)
    acts[4, 3] = 11                                    # stream 3: an unknown action is refused, the stream goes on

    def buffers():
        nbytes = _capi.streams_state_bytes(S, rf, J, F)
        b = dict(state=torch.full((nbytes,), sc.STATE_POISON, dtype=torch.uint8, device=tdev), frame=torch.zeros((S, J, F), device=tdev),
                 action=torch.zeros((S,), dtype=torch.int32, device=tdev), x=torch.full((S, rf, J, F), float(FILL), device=tdev),
                 x_mirror=torch.full((S, rf, J, F), float(FILL), device=tdev), emit=torch.full((S,), -99, dtype=torch.int64, device=tdev),
                 status=torch.full((S,), -5, dtype=torch.int32, device=tdev))
        return b

    def call(b):
        _capi.streams_step(b["state"].data_ptr(), S, rf, lag, J, F, NONE, b["frame"].data_ptr(), None, b["action"].data_ptr(), b["x"].data_ptr(),
                           b["x_mirror"].data_ptr(), perm, b["emit"].data_ptr(), b["status"].data_ptr(), torch.cuda.current_stream(tdev).cuda_stream)

    def run(b, launch):
        seen = []
        for t in range(10):
            b["frame"].copy_(torch.from_numpy(frames[t]))
            b["action"].copy_(torch.from_numpy(acts[t]))
            launch()
            torch.cuda.synchronize()
            seen.append({k: b[k].cpu().numpy().copy() for k in KEYS})
        return seen

    eager = buffers()
    want = run(eager, lambda: call(eager))
    cap = buffers()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call(cap)
    torch.cuda.synchronize()
    assert (cap["state"].cpu().numpy() == sc.STATE_POISON).all()      # the capture ran nothing
    got = run(cap, g.replay)
    del g
    torch.cuda.synchronize()
    assert [int(w["status"][3]) for w in want] == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0] and any((w["emit"] >= 0).any() for w in want)
    for t in range(10):
        for k in KEYS:
            assert np.array_equal(got[t][k].view(np.uint8), want[t][k].view(np.uint8)), (t, k)


# ------------------------------------------------------------------ OnlineLifter

FIXTURES = ["j17_rf27_s3", "j17_rf81_causal_s3"]
CLIP_FRAMES = (5, 40)
S_LIFT = 3                                            # two clips and a stream that stays idle


@functools.lru_cache(maxsize=None)
def pair(name):
    import ray3d_amd
    _, mc = load_model_fixture(name)
    states = synth_states(mc, case_out_scale(name))
    (cp, sp), (ct, st) = states
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos.eval(), trj.eval()
    return ray3d_amd.Ray3DLifter(pos, trj).eval(), states


@functools.lru_cache(maxsize=None)
def clips_of(name):
    """-> (clips of 5 and 40 frames of model inputs, params (S_LIFT, E) or None)."""
    _, ((cp, _), _) = pair(name)
    rng = np.random.RandomState(21)
    clips = tuple((0.3 * rng.standard_normal((n, cp.num_joints, cp.in_features))).astype(np.float32) for n in CLIP_FRAMES)
    params = rng.standard_normal((S_LIFT, cp.extrinsic_dim)).astype(np.float32) if cp.camera_embedding else None
    return clips, params


@functools.lru_cache(maxsize=None)
def oracle_chain(name):
    """The reference's evaluation of the clips through oracle/torch_port.py: edge padding (generators.py:213-216), the sliding
    windows (trainer.py:47-58), pos + trj -> per clip (plain (N, J, 3), flip-averaged (N, J, 3)) (trainer.py:299-302, 340-345)."""
    from oracle import torch_port
    _, ((cp, sp), (ct, st)) = pair(name)
    clips, params = clips_of(name)
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]
    rf = cp.receptive_field
    pad = (rf - 1) // 2

    def lift(w, p):
        with torch.no_grad():
            xw, pw = torch.from_numpy(w), (torch.from_numpy(p) if p is not None else None)
            return (torch_port.forward(cp, sds[0], xw, pw) + torch_port.forward(ct, sds[1], xw, pw)).numpy()

    out = []
    for s, c in enumerate(clips):
        n = c.shape[0]
        padded = evaluate.pad_clip(c, pad, pad if cp.causal else 0)
        windows = np.stack([padded[i:i + rf] for i in range(n)])
        prm = np.tile(params[s], (n, 1)) if params is not None else None
        ref = lift(windows, prm)
        wm = windows.copy()
        wm[..., 0] *= -1
        wm[:, :, H36M_LEFT + H36M_RIGHT] = wm[:, :, H36M_RIGHT + H36M_LEFT]
        refm = lift(wm, prm)
        refm[..., 0] *= -1
        refm[:, :, H36M_LEFT + H36M_RIGHT] = refm[:, :, H36M_RIGHT + H36M_LEFT]
        both = (0.5 * (ref.astype(np.float64) + refm)).astype(np.float32)
        out.append((ref.reshape(n, -1, 3), both.reshape(n, -1, 3)))
    return out


def _online(name, flip):
    import ray3d_amd
    lifter, _ = pair(name)
    ol = ray3d_amd.OnlineLifter(lifter, S_LIFT, flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, device=DEV)
    _, params = clips_of(name)
    if params is not None:
        ol.set_cameras(params=params)
    return lifter, ol


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("name", FIXTURES)
def test_lift_clips_has_the_bits_of_forward_and_agrees_with_the_oracle_chain(name, flip):
    """lift_clips on clips of 5 and 40 frames: each tick's poses are lifter.forward on that tick's windows (the same call on the
    same bits; with flip the average through evaluate.mirror_output), and the collected per-frame poses are within the literal 1e-4
    of the oracle chain over the whole clip."""
    lifter, ol = _online(name, flip)
    clips, _ = clips_of(name)
    assert ol.lag == (0 if "causal" in name else (ol.rf - 1) // 2)
    ticks, plain = [0], ol.step

    def checked(frame=None, actions=None, check=True):
        poses, frames = plain(frame, actions, check)
        with torch.no_grad():
            want = lifter.forward(ol.x, ol.param)
            if flip:
                want = 0.5 * (want + evaluate.mirror_output(lifter.forward(ol.x_mirror, ol.param), H36M_LEFT, H36M_RIGHT))
        assert poses.shape == (S_LIFT, 17, 3) and frames.shape == (S_LIFT,) and frames.dtype == torch.int64
        assert torch.equal(poses.view(torch.int32), want[:, 0].view(torch.int32)) and frames[2] == -1
        ticks[0] += 1
        return poses, frames

    ol.step = checked
    outs = ol.lift_clips(clips)
    lifter.check_status(torch.device(DEV))
    assert ticks[0] == max(CLIP_FRAMES) + ol.lag
    for c, got, refs in zip(clips, outs, oracle_chain(name)):
        assert got.shape == (c.shape[0], 17, 3)
        check_parity(got.cpu().numpy(), refs[1 if flip else 0], "clip of %d frames vs the oracle chain" % c.shape[0])


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_captured_steps_equal_eager_steps_bit_for_bit(flip):
    """capture(), then step: the replayed tick has the bits of the eager one over whole clips - also when the capture comes in the
    middle of a clip; a refused stream still raises."""
    name = "j17_rf27_s3"
    lifter, eager = _online(name, flip)
    _, cap = _online(name, flip)
    clips, _ = clips_of(name)
    try:
        want = eager.lift_clips(clips)
        frame = np.zeros((S_LIFT, 17, 3), np.float32)
        frame[0] = clips[1][0]
        first = cap.step(frame, [RESTART, IDLE, IDLE])          # one eager tick, then the capture, then the clips from the start
        assert first[1].tolist() == [-1, -1, -1]
        cap.capture()
        got = cap.lift_clips(clips)
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        with pytest.raises(RuntimeError, match=r"refused streams \[1\]"):
            cap.step(frame, [IDLE, PUSH, IDLE])                 # (stream 1 was drained: PUSH needs a RESTART first)
        lifter.check_status(torch.device(DEV))
    finally:
        cap.release()


def test_online_lifter_argument_errors():
    import ray3d_amd
    lifter, _ = pair("j17_rf27_s3")
    with pytest.raises(ValueError, match="encoding"):
        ray3d_amd.OnlineLifter(lifter, 2, encoding="intrinsic", device=DEV)      # a 2-float encoding on a ray model
    ol = ray3d_amd.OnlineLifter(lifter, 2, device=DEV)
    with pytest.raises(RuntimeError, match="set_cameras"):
        ol.step(np.zeros((2, 17, 3), np.float32))
    ol.set_cameras(params=np.zeros((2, lifter.pos.extrinsic_dim), np.float32))
    with pytest.raises(ValueError, match="frame must be"):
        ol.step(np.zeros((3, 17, 3), np.float32))
    with pytest.raises(RuntimeError, match=r"refused streams \[0\]"):
        ol.step(np.zeros((2, 17, 3), np.float32), [17, IDLE])
    with pytest.raises(ValueError, match="clips on"):
        ol.lift_clips([np.zeros((1, 17, 3), np.float32)] * 3)
