"""GPU suite: r3d_streams_repair (live streams that survive dropped keypoints) and OnlineLifter(repair=) on top of it.  The kernel
against the host hook, bit for bit, over the scenarios of tests/test_streams_repair_host.py - frame_out, the ring after the repair
and after the step, the track, synthetic, then the step's windows - with every buffer inside guard bands and a state and a track
nobody zeroed; a captured tick with repair against the eager one; OnlineLifter end to end on the RF-27 fixture pair: gapped clips
give finite poses with the bits of lifter.forward on the reference-built windows of the held / offline-repaired clip, the same
input without repair gives NaN, and gap-free input gives the bits of the lifter without repair."""
import numpy as np
import pytest
import torch

import streams_repair_cases as rc
from streams_cases import DRAIN, IDLE, PUSH, RESTART
from streams_repair_cases import bits
from ray3d_amd import _capi, evaluate
from test_gpu_streams import DEV, H36M_LEFT, H36M_RIGHT, S_LIFT, clips_of, pair

pytestmark = pytest.mark.gpu

NAME = "j17_rf27_s3"
SCENARIOS = ([("golden", case, shift, kind) for case in ("rf27", "rf9") for shift in ("centred", "causal") for kind in ("nogapK", "hold", "interp")]
             + [("pixels", c[0]) for c in rc.PIXEL_CASES] + [("conf", 0), ("actions",)])


# ------------------------------------------------------------------ the kernel against the host hook

@pytest.mark.parametrize("key", SCENARIOS, ids=lambda k: "-".join(str(v) for v in k))
def test_device_equals_the_host_hook_bit_for_bit(key):
    scn, _, want = rc.host_run(*key)
    _capi.use_hooks(False)
    _, _, got = rc.play(DEV, scn)
    rc.agree(got, want, key)


# ------------------------------------------------------------------ OnlineLifter

def _online(flip, repair, **kw):
    import ray3d_amd
    lifter, _ = pair(NAME)
    ol = ray3d_amd.OnlineLifter(lifter, S_LIFT, flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, device=DEV, repair=repair, **kw)
    _, params = clips_of(NAME)
    if params is not None:
        ol.set_cameras(params=params)
    return lifter, ol


def _gapped(K):
    """The clips of 5 and 40 frames with joints missing: every gap closes and is at most K frames long, every joint is observed
    in the last frame and at least once within the first lag + 1 = 14 frames (leading gaps of 2 and 6 frames)."""
    clips, _ = clips_of(NAME)
    holes = [(1, 3, 9, 9), (1, 5, 20, 20 + K - 1), (1, 0, 0, 1), (1, 16, 0, 5), (1, None, 30, 31), (1, 8, 25, 27), (0, 2, 1, 2), (0, 11, 0, 0)]
    gapped, observed = rc.punch(list(clips), holes)
    for c, obs in zip(gapped, observed):
        assert obs[-1].all() and max(rc.leading_gaps(obs)) < 13
    return gapped, observed


def _expect(lifter, ol, flip, windows):
    """lifter.forward of this tick's batch with the rows of the emitting streams replaced by `windows` {s: (RF, J, F) bits} - the
    flip average through evaluate.mirror_output, as the eager tick computes it."""
    x, xm = ol.x.clone(), ol.x_mirror.clone() if flip else None
    for s, w in windows.items():
        x[s] = torch.from_numpy(w.view(np.float32)).to(x.device)
        if flip:
            xm[s] = torch.from_numpy(rc.mirrored(w, ol.perm).view(np.float32)).to(x.device)
    with torch.no_grad():
        want = lifter.forward(x, ol.param)
        if flip:
            want = 0.5 * (want + evaluate.mirror_output(lifter.forward(xm, ol.param), H36M_LEFT, H36M_RIGHT))
    return want[:, 0]


def _run_clips(lifter, ol, flip, clips, want_windows, only_drain):
    """The clips through ol tick by tick; every emitted pose must have the bits of the forward of want_windows[s][n] (only_drain:
    only the frames a DRAIN emits are compared).  -> (per clip the poses, the synthetic words)."""
    lengths = [c.shape[0] for c in clips]
    poses_of, syn_of = [np.zeros((n, 17, 3), np.float32) for n in lengths], [np.zeros(n, np.int64) for n in lengths]
    frame, compared = np.zeros((S_LIFT, 17, 3), np.float32), 0
    for t in range(max(lengths) + ol.lag):
        act = np.full(S_LIFT, IDLE, np.int32)
        for s, (c, n) in enumerate(zip(clips, lengths)):
            if t < n:
                act[s], frame[s] = (RESTART if t == 0 else PUSH), c[t]
            elif t < n + ol.lag:
                act[s] = DRAIN
        poses, frames, extras = ol.step(frame, act)
        emitting = {s: int(n) for s, n in enumerate(frames.tolist()) if n >= 0}
        assert frames[2] == -1
        want = _expect(lifter, ol, flip, {s: want_windows[s][n] for s, n in emitting.items()})
        for s, n in emitting.items():
            if act[s] == DRAIN or not only_drain:
                assert torch.equal(poses[s].view(torch.int32), want[s].view(torch.int32)), (t, s, n)
                compared += 1
            poses_of[s][n], syn_of[s][n] = poses[s].cpu().numpy(), int(extras["synthetic"][s])
    assert compared >= (sum(lengths) if not only_drain else 5 + ol.lag)
    return poses_of, syn_of


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_held_clips_have_the_bits_of_forward_on_the_reference_windows(flip):
    """repair=0 on gapped clips whose leading gaps are shorter than lag: finite poses, each with the bits of lifter.forward on the
    reference-built window of the held (forward- / back-filled) clip; the synthetic words are the masks of the missing joints."""
    lifter, ol = _online(flip, 0)
    gapped, observed = _gapped(5)
    held = [rc.offline_repair(bits(c), obs, 0) for c, obs in zip(gapped, observed)]
    assert all(np.isfinite(h.view(np.float32)).all() for h in held)                   # checked on the CPU before relying on it
    windows = [rc.reference_windows(h, ol.rf, ol.lag) for h in held]
    poses, syn = _run_clips(lifter, ol, flip, gapped, windows, only_drain=False)
    for p, sy, obs in zip(poses, syn, observed):
        assert np.isfinite(p).all()
        assert sy.tolist() == [sum(1 << j for j in range(17) if not o[j]) for o in obs]
    lifter.check_status(torch.device(DEV))
    # lift_clips takes the same clips, NaNs included
    for got, p in zip(ol.lift_clips(gapped), poses):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), p.view(np.uint32))


def test_interpolated_clips_end_as_the_offline_repair():
    """repair=5: the poses of the frames the drain emits have the bits of the forward of the offline-repaired clip's windows."""
    lifter, ol = _online(False, 5)
    gapped, observed = _gapped(5)
    fixed = [rc.offline_repair(bits(c), obs, 5) for c, obs in zip(gapped, observed)]
    assert all(np.isfinite(h.view(np.float32)).all() for h in fixed)
    assert not np.array_equal(fixed[1], rc.offline_repair(bits(gapped[1]), observed[1], 0))      # something is interpolated
    poses, _ = _run_clips(lifter, ol, False, gapped, [rc.reference_windows(h, ol.rf, ol.lag) for h in fixed], only_drain=True)
    assert all(np.isfinite(p).all() for p in poses)


def test_without_repair_the_same_input_gives_nan():
    """Today's behaviour, asserted so the need stays visible: one dropped joint makes the stream's poses NaN."""
    _, ol = _online(False, None)
    gapped, _ = _gapped(5)
    for got in ol.lift_clips(gapped):
        assert torch.isnan(got).any()
    assert torch.isnan(ol.lift_clips(gapped)[1][-1]).any()          # ... up to the clip's last frame


def test_gap_free_input_is_unchanged_by_repair():
    """On gap-free input repair=5 and repair=None return the same pose bits and the same frames, tick by tick."""
    _, a = _online(True, None)
    _, b = _online(True, 5)
    clips, _ = clips_of(NAME)
    lengths = [c.shape[0] for c in clips]
    frame = np.zeros((S_LIFT, 17, 3), np.float32)
    for t in range(max(lengths) + a.lag):
        act = np.full(S_LIFT, IDLE, np.int32)
        for s, (c, n) in enumerate(zip(clips, lengths)):
            if t < n:
                act[s], frame[s] = (RESTART if t == 0 else PUSH), c[t]
            elif t < n + a.lag:
                act[s] = DRAIN
        pa, fa = a.step(frame, act)
        pb, fb, extras = b.step(frame, act)
        assert torch.equal(fa, fb) and not extras["synthetic"].any(), t
        live = fa >= 0
        assert torch.equal(pa[live].view(torch.int32), pb[live].view(torch.int32)), t


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_captured_tick_with_repair_equals_the_eager_tick(flip):
    """capture(), then the gapped clips (53 ticks >= RF + 2) with confidences on every tick: the replayed tick has the bits of the
    eager one in poses, frames and synthetic."""
    _, eager = _online(flip, 5, min_conf=0.25)
    _, cap = _online(flip, 5, min_conf=0.25)
    gapped, _ = _gapped(5)
    lengths = [c.shape[0] for c in gapped]
    rng = np.random.RandomState(5)
    try:
        frame = np.zeros((S_LIFT, 17, 3), np.float32)
        conf = np.ones((S_LIFT, 17), np.float32)
        first = cap.step(frame, [RESTART, IDLE, IDLE], conf=conf)      # one eager tick, then the capture, then the clips from the start
        assert first[1].tolist() == [-1, -1, -1]
        cap.capture()
        for t in range(max(lengths) + eager.lag):
            act = np.full(S_LIFT, IDLE, np.int32)
            for s, (c, n) in enumerate(zip(gapped, lengths)):
                if t < n:
                    act[s], frame[s] = (RESTART if t == 0 else PUSH), c[t]
                elif t < n + eager.lag:
                    act[s] = DRAIN
            conf = rng.uniform(0.2, 1.0, (S_LIFT, 17)).astype(np.float32)
            pe, fe, xe = eager.step(frame, act, conf=conf)
            pc, fc, xc = cap.step(frame, act, conf=conf)
            assert torch.equal(fe, fc) and torch.equal(xe["synthetic"], xc["synthetic"]), t
            live = fe >= 0
            assert torch.equal(pe[live].view(torch.int32), pc[live].view(torch.int32)), t
        assert t + 1 >= eager.rf + 2
        with pytest.raises(ValueError, match="recorded with confidences"):
            cap.step(frame, [IDLE] * S_LIFT)
    finally:
        cap.release()


def test_online_lifter_repair_argument_errors():
    import ray3d_amd
    lifter, _ = pair(NAME)
    for bad in (-1, 27, 2.5, True):
        with pytest.raises(ValueError, match="repair must be"):
            ray3d_amd.OnlineLifter(lifter, 2, device=DEV, repair=bad)
    with pytest.raises(ValueError, match="min_conf"):
        ray3d_amd.OnlineLifter(lifter, 2, device=DEV, repair=0, min_conf=float("nan"))
    ol = ray3d_amd.OnlineLifter(lifter, 2, device=DEV)
    ol.set_cameras(params=np.zeros((2, lifter.pos.extrinsic_dim), np.float32))
    with pytest.raises(ValueError, match="conf needs"):
        ol.step(np.zeros((2, 17, 3), np.float32), conf=np.ones((2, 17), np.float32))
