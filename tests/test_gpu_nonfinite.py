"""-m gpu: non-finite keypoints (a detector's NaN / Inf for a missed joint) through every form of the forward, held to the
reference's behaviour as tests/test_nonfinite_host.py pins it on the CPU: every output of a window that reads a non-finite
element is non-finite, every other window has the bits of the same call on finite input and is within the literal 1e-4 of the
torch port, and r3d_status stays clean - a bad keypoint is no error at the boundary and costs no wait.  The values include
ACT_SENTINEL, the quiet NaN that marks "not there yet" in the activation banks of calls of up to 16 windows."""
import functools
import os
import time

import numpy as np
import pytest
import torch

from buffers_util import NANS, Arena
from conftest import dev_switch, synth_states
import nonfinite_util as nf

pytestmark = pytest.mark.gpu

ALL = list(nf.VALUES)
POLL_MAX = 16                      # calls of up to this many windows take data as their own ready flag (r3d_forward.cpp)
DEFAULT = (("ARCHITECTURE", "3,3,3"),)


def _key(over):
    return tuple(sorted(over.items()))


@functools.lru_cache(maxsize=None)
def _states(key):
    import ray3d_amd
    mc = ray3d_amd.default_model_config(**dict(key))
    return mc, synth_states(mc)


def _build(key, **extra):
    """Fresh modules (a development switch is read when a schedule is built; options stay with their handles) on cached weights."""
    import ray3d_amd
    mc, ((cp, sp), (ct, st)) = _states(key)
    fac = ray3d_amd.Model(dict(mc, **extra), {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos.eval(), trj.eval()
    return getattr(pos, "module", pos), getattr(trj, "module", trj), cp


def _lifter(key, B=None, **extra):
    import ray3d_amd
    pos, trj, cp = _build(key, **extra)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    if B is not None and B <= POLL_MAX:
        lifter.set_spin_timeout_ms(200)      # a missed canonicalisation then costs 0.2 s and ends in NaN, never in a hang
    return lifter, cp


@functools.lru_cache(maxsize=None)
def _inputs(key, B):
    from ray3d_amd import synth
    cp = _states(key)[1][0][0]
    x, p = synth.synth_rays(B, cp, seed=700 + B), synth.synth_param(B, seed=800 + B)
    x.setflags(write=False), p.setflags(write=False)
    return x, p


def _port(key, x, p):
    """(pos, trj) of the torch port (the reference graph on the CPU, pinned to the reference fixtures)."""
    from oracle import torch_port
    _, ((cp, sp), (ct, st)) = _states(key)
    outs = []
    with torch.no_grad():
        for c, s in ((cp, sp), (ct, st)):
            sd = {k: torch.from_numpy(np.asarray(v)) for k, v in s.items()}
            outs.append(torch.cat([torch_port.forward(c, sd, torch.from_numpy(np.array(x[i:i + 512])), torch.from_numpy(np.array(p[i:i + 512])))
                                   for i in range(0, x.shape[0], 512)]).numpy())
    return outs


@functools.lru_cache(maxsize=None)
def _ref(key, B):
    """The torch port on _inputs(key, B): computed once, shared, read-only: (pos + trj, trj, pos)."""
    rp, rt = _port(key, *_inputs(key, B))
    out = (rp + rt, rt, rp)
    for o in out:
        o.setflags(write=False)
    return out


def _pair_call(lifter, cp):
    def call(x, p):
        with torch.no_grad():
            out, trj = lifter(torch.from_numpy(x).cuda(), torch.from_numpy(np.array(p)).cuda() if cp.camera_embedding else None, return_trj=True)
        lifter.check_status()                   # (synchronises; a non-finite input is not an error at the boundary)
        return [out.cpu().numpy(), trj.cpu().numpy()]
    return call


def _module_call(m, cp):
    def call(x, p):
        with torch.no_grad():
            out = m(torch.from_numpy(x).cuda(), torch.from_numpy(np.array(p)).cuda() if cp.camera_embedding else None)
        m.check_status()
        return [out.cpu().numpy()]
    return call


def _sweep(call, x, p, refs, cp, label, values=ALL, repeats=1, timed=False):
    """The clean call once, then every value at the three rotations of (window, position): windows first / middle / last, at most
    three per call, every remaining window compared."""
    B, rf, J, F = x.shape[0], cp.receptive_field, cp.num_joints, cp.in_features
    x = np.array(x)
    call(x, p)                                   # (builds the schedule)
    t0 = time.perf_counter()
    clean = call(x, p)
    t_clean = time.perf_counter() - t0
    for o in clean:
        assert np.isfinite(o).all(), label
    for value in values:
        for r, (rows, elements) in enumerate(nf.rotations(B, rf, J, F)):
            bad = nf.poisoned_copy(x, elements, nf.VALUES[value])
            t0 = time.perf_counter()
            outs = call(bad, p)
            dt = time.perf_counter() - t0
            if timed and value == "sentinel" and r == 0:
                print("NONFINITE-TIMING %s: B %d clean call %.3f ms, sentinel call %.3f ms" % (label, B, 1e3 * t_clean, 1e3 * dt))
            for _ in range(repeats - 1):        # (both sentinel-armed activation banks)
                again = call(bad, p)
                assert all(nf.same_bits(a, b) for a, b in zip(again, outs)), (label, value, r)
            for got, gc, ref in zip(outs, clean, refs):
                nf.check_poisoned(got, gc, ref, rows, "%s %s rotation %d" % (label, value, r))
    after = call(x, p)                           # the next clean call is correct again
    assert all(nf.same_bits(a, b) for a, b in zip(after, clean)), label


# ------------------------------------------------------------------ plan kinds and poll paths

BATCHES = [1, 4, 5, 16, 17, 48, 49, 96, 97, 200, 1024]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("arch", ["3,3", "3,3,3"], ids=["rf9", "rf27"])
def test_pair_every_plan_kind(arch, B):
    key = _key(dict(ARCHITECTURE=arch))
    lifter, cp = _lifter(key, B)
    _sweep(_pair_call(lifter, cp), *_inputs(key, B), _ref(key, B)[:2], cp, "pair %s B %d" % (arch, B),
           repeats=3 if B <= POLL_MAX else 1, timed=B <= POLL_MAX)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", ["pos", "trj"])
def test_modules_alone_every_plan_kind(kind, B):
    key = _key(dict(DEFAULT))
    pos, trj, cp = _build(key)
    m = pos if kind == "pos" else trj
    if B <= POLL_MAX:
        m.set_spin_timeout_ms(200)
    ref = _ref(key, B)[2 if kind == "pos" else 1]
    _sweep(_module_call(m, cp), *_inputs(key, B), [ref], cp, "%s alone B %d" % (kind, B), repeats=3 if B <= POLL_MAX else 1)


@pytest.mark.parametrize("switch,B", [("R3D_NO_GEMV", 1), ("R3D_NO_GEMV", 4), ("R3D_NO_LAT", 5), ("R3D_NO_LAT", 16), ("R3D_NO_SMALL_PLAN", 3)])
def test_pair_with_the_other_tiles_of_small_calls(switch, B, monkeypatch):
    """R3D_NO_GEMV: the latency tiles take the layers of up to four rows; R3D_NO_LAT: the split-K tiles take those of 5 .. 32;
    R3D_NO_SMALL_PLAN: the fused plan's partial tiles with one valid row poisoned."""
    dev_switch(monkeypatch, switch, "1")
    key = _key(dict(DEFAULT))
    lifter, cp = _lifter(key, B)
    _sweep(_pair_call(lifter, cp), *_inputs(key, B), _ref(key, B)[:2], cp, "pair %s B %d" % (switch, B), repeats=3)


# ------------------------------------------------------------------ forms

@pytest.mark.parametrize("B", [3, 37, 200])
def test_pair_level_by_level(B):
    key = _key(dict(DEFAULT))
    lifter, cp = _lifter(key, B)
    lifter.set_staged(True)
    _sweep(_pair_call(lifter, cp), *_inputs(key, B), _ref(key, B)[:2], cp, "staged B %d" % B)


def test_pair_bf16x3():
    """The three-term bf16 split of an Inf is Inf - Inf: the window must still come out non-finite, its neighbours untouched."""
    if os.environ.get("R3D_BF16X3") is not None and os.environ["R3D_BF16X3"] != "1":
        pytest.skip("R3D_BF16X3 in the environment overrides the configuration key")
    key, B = _key(dict(DEFAULT)), 128
    lifter, cp = _lifter(key, B, BF16X3=True)
    _sweep(_pair_call(lifter, cp), *_inputs(key, B), _ref(key, B)[:2], cp, "bf16x3 B %d" % B)
    assert lifter.precision("cuda:0") == "bf16x3"


def test_pair_bf16x3_pixel_input():
    """... and through r3d_forward_uv_b3 (first_level_taps_b3 with the UV gather): a bad pixel becomes a non-finite ray inside the
    bf16x3 first level; 97 windows with a 3DHP camera row each, the oracle's camera chain + torch port."""
    if os.environ.get("R3D_BF16X3") is not None and os.environ["R3D_BF16X3"] != "1":
        pytest.skip("R3D_BF16X3 in the environment overrides the configuration key")
    key, B, rf = _key(dict(DEFAULT)), 97, 27
    lifter, _ = _lifter(key, B, BF16X3=True)
    cams, ocams, _, _ = _dhp()
    uv = _px("nonfinite.uvrow.b3.%d" % B, (B, rf, 17, 2), 2048.0)
    pick = [(5 * i + i // 14) % 14 for i in range(B)]
    rays = np.stack([ocams[c].rays_from_uv(uv[i].astype(np.float64)) for i, c in enumerate(pick)]).astype(np.float32)
    rows_d = torch.from_numpy(np.stack([cams[c].cam_row() for c in pick])).cuda()
    par = np.stack([cams[c].param() for c in pick]).astype(np.float32)
    par_d = torch.from_numpy(par).cuda()

    def call(u):
        with torch.no_grad():
            out = lifter.forward_uv(torch.from_numpy(u).cuda(), rows_d, par_d)
        lifter.check_status()
        return out.cpu().numpy()
    rp, rt = _port(key, rays, par)
    clean = call(uv)
    assert lifter.precision("cuda:0") == "bf16x3"
    spots = [(0, 0, 0), (nf.current_frame(rf, 3), 0, 0), (rf - 1, 16, 1)]
    for value in BAD_PIXELS:
        for r in range(3):
            wins = nf.windows_to_poison(B)
            bad = nf.poisoned_copy(uv, [(w,) + spots[(k + r) % 3] for k, w in enumerate(wins)], nf.VALUES[value])
            nf.check_poisoned(call(bad), clean, rp + rt, wins, "uv rows bf16x3 B %d %s rotation %d" % (B, value, r))


@pytest.mark.parametrize("B", [3, 200])
def test_pair_captured_in_a_hip_graph(B):
    """After prepare([B]): one capture, replayed on clean input and on poisoned input behind the same pointers."""
    import ray3d_amd
    key = _key(dict(DEFAULT))
    lifter, cp = _lifter(key, B)
    x, p = _inputs(key, B)
    dev = torch.device("cuda:0")
    xd, pd = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(p)).cuda()
    lifter.prepare([B])
    out = torch.empty((B, 1, 17, 3), device=dev)
    lifter._ws.get(ray3d_amd._capi.workspace_bytes(lifter.pos.handle(dev), lifter.trj.handle(dev), B), dev)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            lifter._run(ray3d_amd._capi.R3D_INPUT_RAYS, xd, cp.receptive_field, B, pd, 2, out=out)

    def call(xx, pp):
        xd.copy_(torch.from_numpy(xx))
        out.zero_()
        g.replay()
        lifter.check_status()
        return [out.cpu().numpy()]
    _sweep(call, x, p, _ref(key, B)[:1], cp, "captured B %d" % B)
    del g
    torch.cuda.synchronize()
    lifter.release_prepared()


# ------------------------------------------------------------------ variants

VARIANTS = [pytest.param(dict(ARCHITECTURE="3,3,3", NUM_KPTS=14, STAGE=2), id="j14-s2"),
            pytest.param(dict(ARCHITECTURE="3,3,3", NUM_KPTS=15), id="j15"),
            pytest.param(dict(ARCHITECTURE="3,3,3", INPUT_DIM=2, CAMERA_EMBDDING=False), id="f2-noemb"),
            pytest.param(dict(ARCHITECTURE="3,3,3", CHANNELS=128, LATENT_FEATURES_DIM=160), id="c128"),
            pytest.param(dict(ARCHITECTURE="3,3,3,3", DISABLE_OPTIMIZATIONS=True, CAUSAL=True), id="rf81-causal-dilated")]


@pytest.mark.parametrize("B", [37, 130])
@pytest.mark.parametrize("over", VARIANTS)
def test_pair_variants(over, B):
    key = _key(over)
    lifter, cp = _lifter(key, B)
    _sweep(_pair_call(lifter, cp), *_inputs(key, B), _ref(key, B)[:2], cp, "variant B %d" % B)


# ------------------------------------------------------------------ inputs_param

@pytest.mark.parametrize("B", [4, 16, 37, 130])
@pytest.mark.parametrize("value", ["nan", "sentinel"])
def test_one_bad_inputs_param_row(value, B):
    """The camera embedding reads the caller's [height, pitch] rows: one bad float makes that window NaN and no other."""
    key = _key(dict(DEFAULT))
    lifter, cp = _lifter(key, B)
    call = _pair_call(lifter, cp)
    x, p = _inputs(key, B)
    x = np.array(x)
    clean = call(x, p)
    for w in nf.windows_to_poison(B):
        for col in (0, 1):
            outs = call(x, nf.poisoned_copy(p, [(w, col)], nf.VALUES[value]))
            for got, gc, ref in zip(outs, clean, _ref(key, B)[:2]):
                nf.check_poisoned(got, gc, ref, [w], "param %s window %d column %d" % (value, w, col))


# ------------------------------------------------------------------ clip calls

def _clip(n, rf, J=17, F=3, seed=0):
    rng = np.random.default_rng(900 + n + seed)
    return (rng.normal(0, 0.4, (1, J, F)) + np.cumsum(rng.normal(0, 0.03, (n + rf - 1, J, F)), axis=0)).astype(np.float32)


PROW = np.array([1.4, 0.15], np.float32)


def _windows_reading(clip, rf):
    """The windows of a sliding clip that touch a non-finite frame - from the array itself."""
    bad = ~np.isfinite(clip.reshape(clip.shape[0], -1)).all(axis=1)
    n = clip.shape[0] - rf + 1
    return [i for i in range(n) if bad[i:i + rf].any()]


@functools.lru_cache(maxsize=None)
def _clip_ref(n, rf):
    clip = _clip(n, rf)
    windows = np.stack([clip[i:i + rf] for i in range(n)])
    rp, rt = _port(_key(dict(DEFAULT)), windows, np.tile(PROW, (n, 1)))
    return rp + rt, rt


def _clip_sweep(lifter, n, label, values=ALL):
    rf = 27
    clip = _clip(n, rf)
    prow = torch.from_numpy(PROW).cuda()

    def call(c):
        with torch.no_grad():
            out, trj = lifter.forward_clip(torch.from_numpy(c).cuda(), prow, return_trj=True)
        lifter.check_status()
        return [out.cpu().numpy(), trj.cpu().numpy()]
    clean = call(clip)
    assert clean[0].shape == (n, 1, 17, 3) and np.isfinite(clean[0]).all()
    spots = nf.positions(rf, 17, 3)
    for k, f in enumerate((0, rf - 1, (n + rf - 1) // 2, n + rf - 2)):
        for v, value in enumerate(values):
            _, joint, feat = spots[(k + v) % 3]
            bad = nf.poisoned_copy(clip, [(f, joint, feat)], nf.VALUES[value])
            rows = list(range(max(0, f - rf + 1), min(n - 1, f) + 1))
            assert rows == _windows_reading(bad, rf)
            for got, gc, ref in zip(call(bad), clean, _clip_ref(n, rf)):
                nf.check_poisoned(got, gc, ref, rows, "%s n %d frame %d %s" % (label, n, f, value))


@pytest.mark.parametrize("n", [40, 130, 300])
@pytest.mark.parametrize("per_frame", [True, False], ids=["per-frame-first-layers", "gathered"])
def test_clip_calls(per_frame, n, monkeypatch):
    """forward_clip, one forward of exactly n windows: the per-frame [E | V] first layers where the plan has them, and the
    gathered first level (R3D_NO_SHARED_L0).  One bad frame poisons exactly the windows that slide over it."""
    if not per_frame:
        dev_switch(monkeypatch, "R3D_NO_SHARED_L0", "1")
    lifter, _ = _lifter(_key(dict(DEFAULT)))
    lifter.CLIP_ROUND = 0
    _clip_sweep(lifter, n, "clip call")


@pytest.mark.parametrize("n", [40, 130])
def test_clip_call_in_chunks(n):
    """CLIP_CHUNK 64, CLIP_ROUND 32: 40 windows are lifted as one call of 64 (24 surplus windows over repeated last frames - a
    bad LAST frame is repeated into them, and their poses are cut off), 130 as 64 + 64 + a two-window call that polls."""
    lifter, _ = _lifter(_key(dict(DEFAULT)), 2)
    lifter.CLIP_CHUNK, lifter.CLIP_ROUND = 64, 32
    assert lifter.clip_batch_sizes(n) == {40: [64], 130: [64, 64, 2]}[n]
    _clip_sweep(lifter, n, "chunked clip call", values=["nan", "sentinel", "-inf"])


def test_clip_through_pad_clip():
    """evaluate.pad_clip replicates a bad FIRST frame into the front pad: the poisoned set is every window that touches any copy,
    computed from the padded array."""
    from ray3d_amd import evaluate
    rf, n = 27, 60
    lifter, _ = _lifter(_key(dict(DEFAULT)))
    raw = _clip(n - rf + 1, rf, seed=5)                          # n frames
    prow = torch.from_numpy(PROW).cuda()

    def call(frames):
        with torch.no_grad():
            out = lifter.forward_clip(torch.from_numpy(evaluate.pad_clip(frames, 13)).cuda(), prow)
        lifter.check_status()
        return out.cpu().numpy()
    padded = evaluate.pad_clip(raw, 13)
    windows = np.stack([padded[i:i + rf] for i in range(n)])
    rp, rt = _port(_key(dict(DEFAULT)), windows, np.tile(PROW, (n, 1)))
    clean = call(raw)
    for frame, value in ((0, "nan"), (0, "sentinel"), (n - 1, "+inf"), (20, "snan")):
        bad = nf.poisoned_copy(raw, [(frame, 3, 1)], nf.VALUES[value])
        rows = _windows_reading(evaluate.pad_clip(bad, 13), rf)
        assert len(rows) == {0: 14, n - 1: 14, 20: 27}[frame]
        nf.check_poisoned(call(bad), clean, rp + rt, rows, "pad_clip frame %d %s" % (frame, value))


# ------------------------------------------------------------------ pixel inputs

BAD_PIXELS = ["nan", "+inf"]


def _dhp():
    from test_gpu_parity import _dhp_cameras
    return _dhp_cameras()


def _px(tag, shape, scale):
    from ray3d_amd import synth
    return (scale * synth.hash_uniform(tag, shape, 13)).astype(np.float32)


@pytest.mark.parametrize("n", [12, 40, 130])
def test_forward_uv_one_camera_for_the_clip(n):
    """r3d_forward_clip_uv_f32 (12 windows: the gathered UV first layers of a call that polls): a 3DHP camera, the oracle camera +
    torch port on the materialised windows."""
    rf = 27
    cams, ocams, _, _ = _dhp()
    cam, ocam = cams[4], ocams[4]
    lifter, _ = _lifter(_key(dict(DEFAULT)), n)
    lifter.CLIP_ROUND = 0
    uv = _px("nonfinite.uvclip.%d" % n, (n + rf - 1, 17, 2), 2048.0)
    row, prow = torch.from_numpy(cam.cam_row()).cuda(), torch.from_numpy(cam.param()).cuda()

    def call(u):
        with torch.no_grad():
            out = lifter.forward_uv(torch.from_numpy(u).cuda(), row, prow)
        lifter.check_status()
        return out.cpu().numpy()
    rays = ocam.rays_from_uv(uv.astype(np.float64)).astype(np.float32)
    rp, rt = _port(_key(dict(DEFAULT)), np.stack([rays[i:i + rf] for i in range(n)]), np.tile(cam.param(), (n, 1)).astype(np.float32))
    clean = call(uv)
    for k, f in enumerate((0, rf - 1, (n + rf - 1) // 2, n + rf - 2)):
        for value in BAD_PIXELS:
            bad = nf.poisoned_copy(uv, [(f, (5 * k) % 17, k % 2)], nf.VALUES[value])
            nf.check_poisoned(call(bad), clean, rp + rt, _windows_reading(bad, rf), "uv clip n %d frame %d %s" % (n, f, value))


@pytest.mark.parametrize("B", [5, 37, 130])
@pytest.mark.parametrize("distorted", [False, True], ids=["uv", "uv-dist"])
def test_forward_uv_a_camera_row_per_window(distorted, B):
    """r3d_forward_uv_f32 with 8-wide rows of the 14 3DHP cameras, and the distorted-camera mode (16-wide H36M rows, the float64
    pre-pass in front): the oracle's camera chain + torch port."""
    from test_gpu_undistort import _h36m_distorted_cameras, _oracle_rays
    rf = 27
    key = _key(dict(DEFAULT))
    lifter, _ = _lifter(key, B)
    if distorted:
        cams, ocams = _h36m_distorted_cameras()
        uv = _px("nonfinite.uvdist.%d" % B, (B, rf, 17, 2), 1000.0)
        pick = [(3 * i + 1) % 4 for i in range(B)]
        rays = np.stack([_oracle_rays(ocams[c], uv[i]) for i, c in enumerate(pick)])
        rows = np.stack([cams[c].cam_row(distortion=True) for c in pick])
    else:
        cams, ocams, _, _ = _dhp()
        uv = _px("nonfinite.uvrow.%d" % B, (B, rf, 17, 2), 2048.0)
        pick = [(5 * i + i // 14) % 14 for i in range(B)]
        rays = np.stack([ocams[c].rays_from_uv(uv[i].astype(np.float64)) for i, c in enumerate(pick)]).astype(np.float32)
        rows = np.stack([cams[c].cam_row() for c in pick])
    par = np.stack([cams[c].param() for c in pick]).astype(np.float32)
    rows_d, par_d = torch.from_numpy(rows).cuda(), torch.from_numpy(par).cuda()

    def call(u):
        with torch.no_grad():
            out = lifter.forward_uv(torch.from_numpy(u).cuda(), rows_d, par_d)
        lifter.check_status()
        return out.cpu().numpy()
    rp, rt = _port(key, rays, par)
    clean = call(uv)
    spots = [(0, 0, 0), (nf.current_frame(rf, 3), 0, 0), (rf - 1, 16, 1)]       # (the rays have three features: current frame 9)
    for value in BAD_PIXELS:
        for r in range(3):
            wins = nf.windows_to_poison(B)
            bad = nf.poisoned_copy(uv, [(w,) + spots[(k + r) % 3] for k, w in enumerate(wins)], nf.VALUES[value])
            nf.check_poisoned(call(bad), clean, rp + rt, wins, "uv rows B %d %s rotation %d" % (B, value, r))


@pytest.mark.parametrize("keyword,dist", [("screen", True), ("intrinsic", False), ("intrinsic", True)], ids=["screen", "intrinsic-zero", "intrinsic-h36m"])
def test_two_feature_pixel_modes(keyword, dist):
    """R3D_INPUT_PX_SCREEN / R3D_INPUT_PX_INTRINSIC of tests/test_gpu_px2d.py (INPUT_DIM 2, no embedding), batches with a camera
    row per window and a sliding sequence with one camera: the host encoding + torch port."""
    from test_gpu_parity import _oracle_lift
    from test_gpu_px2d import _cameras, _host, _pair, _rows
    lifter, states = _pair("3,3,3")
    rf, J = 27, 17
    cams = _cameras(dist)
    for B in (5, 37):
        uv = _px("nonfinite.px2d.%s.%d" % (keyword, B), (B, rf, J, 2), 1000.0)
        pick = [(3 * i + 1) % 4 for i in range(B)]
        rows = _rows(cams, pick)
        windows = np.stack([_host(cams[c], uv[i], keyword) for i, c in enumerate(pick)])
        ref = _oracle_lift(states, windows, np.zeros((B, 2), np.float32))

        def call(u):
            with torch.no_grad():
                out = lifter.forward_uv(torch.from_numpy(u).cuda(), rows, encoding=keyword)
            lifter.check_status()
            return out.cpu().numpy()
        clean = call(uv)
        spots = nf.positions(rf, J, 2)
        for value in BAD_PIXELS:
            wins = nf.windows_to_poison(B)
            bad = nf.poisoned_copy(uv, [(w,) + spots[k % 3] for k, w in enumerate(wins)], nf.VALUES[value])
            nf.check_poisoned(call(bad), clean, ref, wins, "px2d %s B %d %s" % (keyword, B, value))
    n = 40                                                         # a sliding sequence, one camera
    seq = _px("nonfinite.px2d.seq.%s" % keyword, (n + rf - 1, J, 2), 1000.0)
    row = _rows(cams, [2])[0]
    enc = _host(cams[2], seq, keyword)
    ref = _oracle_lift(states, np.stack([enc[i:i + rf] for i in range(n)]), np.zeros((n, 2), np.float32))
    keep = (lifter.CLIP_CHUNK, lifter.CLIP_ROUND)
    lifter.CLIP_ROUND = 0
    try:
        def call_seq(u):
            with torch.no_grad():
                out = lifter.forward_uv(torch.from_numpy(u).cuda(), row, window_stride=1, encoding=keyword)
            lifter.check_status()
            return out.cpu().numpy()
        clean = call_seq(seq)
        for f, value in ((0, "nan"), (33, "+inf"), (n + rf - 2, "nan")):
            bad = nf.poisoned_copy(seq, [(f, 7, f % 2)], nf.VALUES[value])
            nf.check_poisoned(call_seq(bad), clean, ref, _windows_reading(bad, rf), "px2d %s sequence frame %d %s" % (keyword, f, value))
    finally:
        lifter.CLIP_CHUNK, lifter.CLIP_ROUND = keep


# ------------------------------------------------------------------ r3d_clips_encode

@pytest.mark.parametrize("encoding", ["ray", "intrinsic", "screen"])
def test_clips_encode_one_bad_pixel_in_the_middle_clip(encoding):
    """Three clips on three camera rows (two distorted, one zero-coefficient), flip buffers on, every buffer an exact-size region
    between guard bands: the bits of r3d_debug_clips_encode_host, only that keypoint - and its mirrored slot - non-finite in
    every output row that repeats the frame (pad and surplus rows too), status words 0, guards intact."""
    from ray3d_amd import _capi, evaluate
    from test_clips_encode_host import FILL, mirror_perm, run_hook
    from test_nonfinite_host import CLIP_SPOTS, bad_clip_pixels, check_clips_encode_outputs, three_clips
    J = 17
    table, px, out_rows, max_rows = three_clips()
    enc = evaluate.ENCODINGS[encoding]
    F = _capi.ENCODE_FLOATS[enc]
    nx = out_rows * J * F * 4
    arena = Arena("cuda", NANS, Arena.capacity_for([px.nbytes, table.nbytes, nx, nx, 4 * len(table)]))
    put_px = arena.put(px, name="px")
    tab = arena.put(np.array(table).view(np.uint8), name="table")()
    x, xm = arena.carve(nx, name="x"), arena.carve(nx, name="x_mirror")
    status = arena.carve(4 * len(table), name="status")

    def run(pixels_):
        pxd = put_px()
        pxd.copy_(torch.from_numpy(pixels_))
        x.view(torch.float32).fill_(float(FILL)), xm.view(torch.float32).fill_(float(FILL))
        status.view(torch.int32).fill_(-1)
        _capi.clips_encode(pxd.data_ptr(), px.shape[0], J, enc, tab.data_ptr(), len(table), max_rows, x.data_ptr(), out_rows,
                           xm.data_ptr(), mirror_perm(J), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        arena.check()
        return (x.view(torch.float32).view(out_rows, J, F).cpu().numpy(), xm.view(torch.float32).view(out_rows, J, F).cpu().numpy(),
                status.view(torch.int32).cpu().numpy())
    cx, cxm, cstatus = run(np.array(px))
    assert not cstatus.any()
    for frame, joint, comp in CLIP_SPOTS:
        bad_px, rows = bad_clip_pixels(frame, joint, comp, float("nan"))
        gx, gxm, gstatus = run(bad_px)
        assert not gstatus.any(), gstatus
        check_clips_encode_outputs(gx, gxm, cx, cxm, rows, joint)
        rc, hx, hxm, hstatus = run_hook(J, encoding, table, bad_px, out_rows, max_rows)
        assert rc == 0 and not hstatus.any()
        for name, g, h in (("x", gx, hx), ("x_mirror", gxm, hxm)):
            fin = np.isfinite(h)
            assert np.array_equal(np.isfinite(g), fin), (name, frame)
            diff = g.view(np.uint32) != h.view(np.uint32)
            steps = np.abs(g[fin].view(np.int32).astype(np.int64) - h[fin].view(np.int32).astype(np.int64)).max(initial=0)
            print("clips_encode %s %s frame %d: %d of %d elements differ from the host hook, max %d ulp" % (encoding, name, frame, int(diff.sum()), g.size, int(steps)))
            assert nf.same_bits(g, h), (name, frame, int(diff.sum()), int(steps))


# ------------------------------------------------------------------ metrics

def test_clips_metrics_one_nan_prediction_in_the_middle_clip():
    """r3d_clips_metrics over three clips, one NaN in the ROOT joint of one frame of the middle clip (every one of the five
    formulas reads the root): that clip's five sums are NaN - as the float64 NumPy oracle's are -, the other clips' rows have the
    bits of the clean call."""
    from oracle import metrics_oracle as mo
    from test_gpu_clips_metrics import layout, run_batched
    J, lengths = 17, (63, 65, 64)
    cases, table, pred, gt, total = layout(J, lengths)
    g = torch.from_numpy(np.array(gt)).cuda()
    clean, cdet, _ = run_batched(torch.from_numpy(np.array(pred)).cuda(), g, table, J, max(lengths))
    assert bool(torch.isfinite(clean).all())
    at = int(table[1]["first_frame"])
    for frame in (0, 31, 64):
        bad = np.array(pred)
        bad[at + frame, 0, 1] = np.nan
        rows, det, fr = run_batched(torch.from_numpy(bad).cuda(), g, table, J, max(lengths))
        assert bool(torch.isnan(rows[1]).all()), (frame, rows[1])
        for c in (0, 2):
            assert torch.equal(rows[c].view(torch.int64), clean[c].view(torch.int64)) and torch.equal(det[c].view(torch.int64), cdet[c].view(torch.int64))
        # (the NumPy oracle: MPJPE and the root's MPJPE are NaN; its Procrustes fit raises on the NaN frame - np.linalg.svd - so
        #  the reference is loud there too, never finite)
        p, gg, R, T, _ = cases[1]
        pw = bad[at:at + lengths[1]].astype(np.float64) @ R.T + T.reshape(1, 1, 3)
        gw = gg.astype(np.float64) @ R.T + T.reshape(1, 1, 3)
        assert np.isnan(mo.mpjpe(pw, gw)) and np.isnan(mo.mpjpe(pw[:, :1], gw[:, :1]))
        assert bool(torch.isnan(fr[at + frame, [0, 1, 2, 4]]).all())   # the frame's own terms: not skipped


@pytest.mark.parametrize("variant", ["trj", "sum"])
def test_clip_valid_losses_one_nan_prediction(variant):
    """r3d_clip_valid_losses on one clip with one NaN in the predicted poses: exactly the sums the NumPy oracle of the reference's
    formulas finds NaN are NaN (the position losses and the bone terms - not a finite value that skipped the frame), the others
    are its values."""
    import valid_oracle as vo
    from test_gpu_valid import _run
    n, J = 65, 17
    pos, trj, gt, flags = vo.variant_inputs(n, J, variant)
    for frame, joint in ((0, 0), (40, 9), (64, 16)):
        bad = np.array(pos)
        bad[frame, joint, 2] = np.nan
        out, fr, _ = _run(bad, trj, gt, vo.tree_for(J), flags)
        with np.errstate(invalid="ignore"):
            want = vo.oracle(bad, trj, gt, vo.tree_for(J), flags)
        assert np.isnan(want["out"][:2]).all() and np.isnan(out[:2]).all(), (frame, joint, out[:7])
        assert np.array_equal(np.isnan(out), np.isnan(want["out"])), (frame, joint, out[:7], want["out"][:7])
        fin = np.isfinite(want["out"])
        assert vo.sums_close(out[fin], want["out"][fin])
        assert np.array_equal(np.isnan(fr), np.isnan(want["frames"]))
