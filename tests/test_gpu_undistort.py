"""-m gpu: R3D_INPUT_UV_DIST - raw pixels of a distorted camera (CameraInfoPacket(..., undistort=True), the H36M loaders'
default) undistorted by the r3d_undistort_rays_f64 pre-pass in front of the R3D_INPUT_RAYS forward.  Comparand: the
oracle chain - oracle.undistort_points -> the oracle camera's rays (float64) -> float32 (lib/train_val/trainer.py:298) ->
oracle.forward (pos + trj) - at the literal 1e-4 bound; and with zero coefficients, R3D_INPUT_UV bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, check_parity, dev_switch
from test_gpu_parity import PLANS, _oracle_lift, _reference_cameras, build_modules

pytestmark = pytest.mark.gpu


def _h36m_distorted_cameras():
    """The four H36M cameras of cameras.npz (S9) with the four coefficient sets of undistort.npz (their own intrinsics):
    [(product camera, undistort=True), (oracle camera, K, dist)]."""
    import ray3d_amd
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    u = np.load(os.path.join(GOLDEN, "undistort.npz"))
    cams, ocams = [], []
    for i in range(int(u["n"])):
        t = "h36m_S9_%d" % i
        K, dist = u["cam%d/K" % i], u["cam%d/dist" % i]
        assert np.array_equal(z[t + "/K"], K)
        cams.append(ray3d_amd.Camera(K, z[t + "/R"], z[t + "/t"], dist_coeff=dist, undistort=True))
        ocams.append((oracle.Camera(K, z[t + "/R"], z[t + "/t"]), K, dist))
    return cams, ocams


def _oracle_rays(ocam, uv):
    """The oracle chain's rays of raw pixels (..., 2): undistort, re-project, encode in float64; cast once."""
    from oracle import oracle
    oc, K, dist = ocam
    uv = np.asarray(uv, dtype=np.float64)
    return oc.rays_from_uv(oracle.undistort_points(K, dist, uv.reshape(-1, 2)).reshape(uv.shape)).astype(np.float32)


def _pixels(tag, shape):
    """Keypoints over the whole 1000 x 1002 H36M image, corners included."""
    from ray3d_amd import synth
    return (1000.0 * synth.hash_uniform(tag, shape, 7)).astype(np.float32)


def _oracle_check(states, rays, par, out, what, few=None):
    """pos + trj on the oracle chain's rays: oracle.forward on every window (or `few` of them, with the torch port of the
    oracle on all)."""
    from oracle import oracle
    (cp, sp), (ct, st) = states
    out = out.detach().cpu().numpy() if hasattr(out, "detach") else out
    if few is None:
        check_parity(out, oracle.forward(cp, sp, rays, par) + oracle.forward(ct, st, rays, par), what)
        return
    check_parity(out, _oracle_lift(states, rays, par), what + " (torch port of the oracle, all windows)")
    check_parity(out[few], oracle.forward(cp, sp, rays[few], par[few]) + oracle.forward(ct, st, rays[few], par[few]),
                 what + " (C oracle, %d windows)" % len(few))


@pytest.mark.parametrize("fused", PLANS)
@pytest.mark.parametrize("arch,B", [("3,3", 1), ("3,3", 17), ("3,3", 256), ("3,3,3,3,3", 1), ("3,3,3,3,3", 17),
                                    ("3,3,3,3,3", 256)])
def test_uv_dist_batches_match_the_oracle_chain(arch, B, fused, monkeypatch):
    """(B, RF, J, 2) raw pixels, RF 9 and RF 243, with a camera row PER WINDOW (the four H36M coefficient sets in turn) and
    with ONE broadcast row."""
    import ray3d_amd
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")
    cams, ocams = _h36m_distorted_cameras()
    pos, trj, (cp, sp), (ct, st) = build_modules(ray3d_amd.default_model_config(ARCHITECTURE=arch))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    rf = cp.receptive_field
    uv = _pixels("uvdist.%d.%d" % (rf, B), (B, rf, 17, 2))
    pick = [(i * 3 + 1) % 4 for i in range(B)]
    few = None if B * rf <= 17 * 243 else [0, 1, 2, 3, B // 2, B - 1]
    uvd = torch.from_numpy(uv).cuda()
    # per-window rows
    rays = np.stack([_oracle_rays(ocams[c], uv[i]) for i, c in enumerate(pick)])
    rows = np.stack([cams[c].cam_row(distortion=True) for c in pick])
    par = np.stack([cams[c].param() for c in pick])
    with torch.no_grad():
        a = lifter.forward_uv(uvd, torch.from_numpy(rows).cuda(), torch.from_numpy(par).cuda())
        b = lifter(torch.from_numpy(rays).cuda(), torch.from_numpy(par).cuda())
    _oracle_check(((cp, sp), (ct, st)), rays, par, a, "per-window rows", few)
    check_parity(a, b.cpu().numpy(), "per-window rows vs the rays mode on the oracle's rays")
    # one broadcast row
    c = 2
    rays1 = _oracle_rays(ocams[c], uv)
    par1 = np.tile(cams[c].param(), (B, 1))
    with torch.no_grad():
        a1 = lifter.forward_uv(uvd, torch.from_numpy(cams[c].cam_row(distortion=True)).cuda(), torch.from_numpy(par1).cuda())
    _oracle_check(((cp, sp), (ct, st)), rays1, par1, a1, "one broadcast row", few)


@pytest.mark.parametrize("fused", PLANS)
@pytest.mark.parametrize("arch", ["3,3", "3,3,3,3,3"])
def test_uv_dist_sequences_match_the_oracle_chain(arch, fused, monkeypatch):
    """Frame sequences with window_stride 1 (one camera: the per-frame shared first level; a camera per window: the
    materialised windows), 5 (overlapping windows with their own cameras) and RF + 3 (gaps between windows, a camera per
    window: one ray per input frame), lifted in the batch sizes of clip_batch_sizes (surplus windows cut off)."""
    import ray3d_amd
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")
    cams, ocams = _h36m_distorted_cameras()
    pos, trj, (cp, sp), (ct, st) = build_modules(ray3d_amd.default_model_config(ARCHITECTURE=arch))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    rf = cp.receptive_field
    B = 17
    for stride, per_window in ((1, False), (1, True), (5, True), (5, False), (rf + 3, True)):
        T = (B - 1) * stride + rf
        seq = _pixels("uvdistseq.%d.%d" % (rf, stride), (T, 17, 2))
        pick = [(i + stride) % 4 for i in range(B)] if per_window else [3] * B
        windows = np.stack([_oracle_rays(ocams[c], seq[i * stride:i * stride + rf]) for i, c in enumerate(pick)])
        par = np.stack([cams[c].param() for c in pick])
        rows = np.stack([cams[c].cam_row(distortion=True) for c in pick]) if per_window else cams[3].cam_row(distortion=True)
        with torch.no_grad():
            a = lifter.forward_uv(torch.from_numpy(seq).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(par).cuda(),
                                  window_stride=stride)
        assert a.shape == (B, 1, 17, 3)
        _oracle_check(((cp, sp), (ct, st)), windows, par, a, "stride %d, %s" % (stride, "per-window rows" if per_window else "one row"),
                      None if rf < 243 else [0, 7, B - 1])


def _ws_rays(lifter, hp, ht, inp, B, nrays, J, dev):
    """One UV_DIST forward through the C ABI on a workspace of exactly r3d_input_workspace_bytes; the pre-pass's rays, which
    start at r3d_workspace_bytes(B) rounded up to 256 bytes."""
    from ray3d_amd import _capi
    ws = torch.zeros(_capi.input_workspace_bytes(hp, ht, inp, B), dtype=torch.uint8, device=dev)
    out = torch.empty((B, 1, J, 3), device=dev)
    _capi.forward_pair(hp, ht, inp, B, out.data_ptr(), None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    off = (_capi.workspace_bytes(hp, ht, B) + 255) // 256 * 256
    return ws[off:off + nrays * J * 12].view(torch.float32).view(nrays, J, 3).cpu().numpy(), out


def _ulp_check(got, want, what):
    """>= 99.99 % of the elements equal, the rest within one float32 ulp."""
    assert got.shape == want.shape, what
    eq = got == want
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    frac = float(eq.mean())
    print("%s: %.6f of %d elements equal, max %d ulp" % (what, frac, got.size, int(ulps.max())))
    assert frac >= 0.9999, (what, frac)
    assert int(ulps[~eq].max(initial=0)) <= 1, (what, int(ulps.max()))


def test_pre_pass_rays_equal_the_host_chain_in_every_layout():
    """The pre-pass's float32 rays against the host chain's (oracle.undistort_points -> oracle rays -> float32): B 256 x RF
    243 x J 17 with per-window rows (1.06 M keypoints, whole image); a sliding clip with one camera (one ray per frame); and
    overlapping windows with their own cameras (materialised (B, RF, J, 3))."""
    import ray3d_amd
    from ray3d_amd import _capi
    cams, ocams = _h36m_distorted_cameras()
    pos, trj, (cp, _), _ = build_modules(ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3"))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    dev = torch.device("cuda:0")
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    rf, J = cp.receptive_field, 17
    # (B, RF, J, 2) with a camera per window
    B = 256
    uv = _pixels("prepass.batch", (B, rf, J, 2))
    pick = [i % 4 for i in range(B)]
    rows = torch.from_numpy(np.stack([cams[c].cam_row(distortion=True) for c in pick])).cuda()
    par = torch.from_numpy(np.stack([cams[c].param() for c in pick])).cuda()
    uvd = torch.from_numpy(uv).cuda()
    inp = _capi.make_input(_capi.R3D_INPUT_UV_DIST, uvd.data_ptr(), rf, par.data_ptr(), 2, rows.data_ptr(), 16)
    got, _ = _ws_rays(lifter, hp, ht, inp, B, B * rf, J, dev)
    want = np.stack([_oracle_rays(ocams[c], uv[i]) for i, c in enumerate(pick)]).reshape(B * rf, J, 3)
    _ulp_check(got, want, "B 256 x RF 243, per-window rows")
    # a sliding clip, one camera: one ray per input frame
    n = 300
    clip = _pixels("prepass.clip", (n + rf - 1, J, 2))
    clipd = torch.from_numpy(clip).cuda()
    row1 = torch.from_numpy(cams[1].cam_row(distortion=True)).cuda()
    p1 = torch.from_numpy(cams[1].param()).cuda()
    inp = _capi.make_input(_capi.R3D_INPUT_UV_DIST, clipd.data_ptr(), 1, p1.data_ptr(), 0, row1.data_ptr(), 0)
    got, _ = _ws_rays(lifter, hp, ht, inp, n, n + rf - 1, J, dev)
    _ulp_check(got, _oracle_rays(ocams[1], clip), "sliding clip, one camera")
    # overlapping windows (stride 5) with their own cameras (rows 20 doubles apart): materialised windows
    B, stride = 40, 5
    seq = _pixels("prepass.seq", ((B - 1) * stride + rf, J, 2))
    seqd = torch.from_numpy(seq).cuda()
    pick = [(2 * i + 1) % 4 for i in range(B)]
    rows20 = np.zeros((B, 20))
    rows20[:, :16] = np.stack([cams[c].cam_row(distortion=True) for c in pick])
    rows20 = torch.from_numpy(rows20).cuda()
    parB = torch.from_numpy(np.stack([cams[c].param() for c in pick])).cuda()
    inp = _capi.make_input(_capi.R3D_INPUT_UV_DIST, seqd.data_ptr(), stride, parB.data_ptr(), 2, rows20.data_ptr(), 20)
    got, _ = _ws_rays(lifter, hp, ht, inp, B, B * rf, J, dev)
    want = np.stack([_oracle_rays(ocams[c], seq[i * stride:i * stride + rf]) for i, c in enumerate(pick)]).reshape(B * rf, J, 3)
    _ulp_check(got, want, "overlapping windows, own cameras")


def _plain_cameras():
    """The reference cameras without distortion: the 16-double rows carry zero coefficients."""
    cams, _, _, _ = _reference_cameras()
    return cams


def test_zero_coefficients_are_bit_identical_to_uv_mode(monkeypatch):
    """Rows with zero coefficients (undistort=False): UV_DIST equals R3D_INPUT_UV bit for bit, for batches with per-window
    rows and one row, clips (stride 1, one camera), overlapping windows with their own cameras (stride 5) and windows
    with gaps (stride RF + 3); level by level (R3D_OPT_STAGED) too; and r3d_forward of a single model."""
    import ray3d_amd
    from ray3d_amd import _capi
    cams = _plain_cameras()
    pos, trj, (cp, _), _ = build_modules(ray3d_amd.default_model_config(ARCHITECTURE="3,3,3"))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    rf, B = cp.receptive_field, 40
    pick = [cams[(5 * i) % len(cams)] for i in range(B)]
    rows8 = torch.from_numpy(np.stack([c.cam_row() for c in pick])).cuda()
    rows16 = torch.from_numpy(np.stack([c.cam_row(distortion=True) for c in pick])).cuda()
    assert not rows16[:, 8:].any()
    par = torch.from_numpy(np.stack([c.param() for c in pick])).cuda()
    uv = torch.from_numpy(_pixels("zero.batch", (B, rf, 17, 2))).cuda()
    calls = [("batch, per-window rows", lambda r8, r16: (uv, r16 if r16 is not None else r8, par, None), True),
             ("batch, one row", lambda r8, r16: (uv, (r16 if r16 is not None else r8)[3], par, None), False)]
    for stride in (1, 5, rf + 3):
        seq = torch.from_numpy(_pixels("zero.seq%d" % stride, ((B - 1) * stride + rf, 17, 2))).cuda()
        calls.append(("stride %d, one row" % stride,
                      lambda r8, r16, seq=seq, stride=stride: (seq, (r16 if r16 is not None else r8)[1], par[1], stride), False))
        calls.append(("stride %d, per-window rows" % stride,
                      lambda r8, r16, seq=seq, stride=stride: (seq, r16 if r16 is not None else r8, par, stride), True))
    for staged in (False, True):
        lifter.set_staged(staged)
        with torch.no_grad():
            for what, args, _ in calls:
                x, r, p, s = args(rows8, None)
                want = lifter.forward_uv(x, r, p, window_stride=s)
                x, r, p, s = args(rows8, rows16)
                got = lifter.forward_uv(x, r, p, window_stride=s)
                assert torch.equal(got, want), (what, staged, float((got - want).abs().max()))
    lifter.set_staged(False)
    # r3d_forward of each model alone, through the C ABI
    dev = torch.device("cuda:0")
    for h in (lifter.pos.handle(dev), lifter.trj.handle(dev)):
        outs = []
        for mode, rows, cs in ((_capi.R3D_INPUT_UV, rows8, 8), (_capi.R3D_INPUT_UV_DIST, rows16, 16)):
            inp = _capi.make_input(mode, uv.data_ptr(), rf, par.data_ptr(), 2, rows.data_ptr(), cs)
            pos_h = h is lifter.pos.handle(dev)
            ws = torch.empty(_capi.input_workspace_bytes(h if pos_h else None, None if pos_h else h, inp, B), dtype=torch.uint8, device=dev)
            out = torch.full((B, 1, 17 if pos_h else 1, 3), float("nan"), device=dev)
            _capi.forward(h, inp, B, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_uv_dist_on_lanes_equals_the_lane_less_result():
    """set_lanes(2): two UV_DIST forwards relayed from a caller's stream (by the module, and by the library through the C
    ABI), joined, equal the forward without lanes."""
    import ray3d_amd
    from ray3d_amd import _capi
    cams, _ = _h36m_distorted_cameras()
    pos, trj, (cp, _), _ = build_modules(ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3"))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    dev = torch.device("cuda:0")
    rf, B = cp.receptive_field, 128
    pick = [i % 4 for i in range(B)]
    rows = torch.from_numpy(np.stack([cams[c].cam_row(distortion=True) for c in pick])).cuda()
    par = torch.from_numpy(np.stack([cams[c].param() for c in pick])).cuda()
    uva = torch.from_numpy(_pixels("lanes.a", (B, rf, 17, 2))).cuda()
    uvb = torch.from_numpy(_pixels("lanes.b", (B, rf, 17, 2))).cuda()
    with torch.no_grad():
        want_a, want_b = lifter.forward_uv(uva, rows, par).clone(), lifter.forward_uv(uvb, rows, par).clone()
        torch.cuda.synchronize()
        lifter.set_lanes(2)
        s = torch.cuda.Stream()
        try:
            with torch.cuda.stream(s):                              # the module relays to lanes 0 and 1
                oa = lifter.forward_uv(uva, rows, par)
                ob = lifter.forward_uv(uvb, rows, par)
                lifter.join_lanes()
                ca, cb = oa.clone(), ob.clone()
            torch.cuda.synchronize()
            # (a lane has half the CUs: other tile schedules, other split-K sums - HIP against HIP at a bound that scales with |ref|)
            tol = 2e-5 * max(1.0, float(want_a.abs().max()), float(want_b.abs().max()))
            check_parity(ca, want_a.cpu().numpy(), "module relay, lane 0 (HIP against HIP)", tol=tol)
            check_parity(cb, want_b.cpu().numpy(), "module relay, lane 1 (HIP against HIP)", tol=tol)
            hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)   # the library relays (C ABI, caller's stream)
            outs = []
            for uv in (uva, uvb):
                inp = _capi.make_input(_capi.R3D_INPUT_UV_DIST, uv.data_ptr(), rf, par.data_ptr(), 2, rows.data_ptr(), 16)
                ws = torch.empty(_capi.input_workspace_bytes(hp, ht, inp, B), dtype=torch.uint8, device=dev)
                out = torch.zeros_like(want_a)
                torch.cuda.synchronize()
                _capi.forward_pair(hp, ht, inp, B, out.data_ptr(), None, ws.data_ptr(), ws.numel(), s.cuda_stream)
                outs.append((out, ws, inp))
            hp.lanes_join(s.cuda_stream)
            with torch.cuda.stream(s):
                snaps = [o.clone() for o, _, _ in outs]
            torch.cuda.synchronize()
            check_parity(snaps[0], want_a.cpu().numpy(), "library relay, lane 0 (HIP against HIP)", tol=tol)
            check_parity(snaps[1], want_b.cpu().numpy(), "library relay, lane 1 (HIP against HIP)", tol=tol)
            lifter.check_status()
        finally:
            lifter.set_lanes(0)


def test_uv_dist_forward_captured_in_a_hip_graph():
    """A UV_DIST forward captured with torch.cuda.graph after prepare (the pre-pass is captured with it): replayed after new
    pixels were written into the captured input, it equals the eager call on those pixels."""
    import ray3d_amd
    from ray3d_amd import _capi
    cams, _ = _h36m_distorted_cameras()
    pos, trj, (cp, _), _ = build_modules(ray3d_amd.default_model_config(ARCHITECTURE="3,3,3"))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    dev = torch.device("cuda:0")
    rf, B = cp.receptive_field, 211                              # (a batch size nothing else here uses)
    pick = [i % 4 for i in range(B)]
    rows = torch.from_numpy(np.stack([cams[c].cam_row(distortion=True) for c in pick])).cuda()
    par = torch.from_numpy(np.stack([cams[c].param() for c in pick])).cuda()
    uv = torch.from_numpy(_pixels("graph.a", (B, rf, 17, 2))).cuda()
    uv2 = torch.from_numpy(_pixels("graph.b", (B, rf, 17, 2))).cuda()
    lifter.prepare([B])
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    inp = _capi.make_input(_capi.R3D_INPUT_UV_DIST, uv.data_ptr(), rf, par.data_ptr(), 2, rows.data_ptr(), 16)
    lifter._ws.get(_capi.input_workspace_bytes(hp, ht, inp, B), dev)
    out = torch.empty((B, 1, 17, 3), device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            lifter._run(_capi.R3D_INPUT_UV_DIST, uv, rf, B, par, 2, rows, 16, out=out)
    uv.copy_(uv2)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = lifter.forward_uv(uv2, rows, par)
    assert torch.isfinite(eager).all() and torch.equal(out, eager)
    del g
    torch.cuda.synchronize()
    _capi.release(hp, ht, B)


def test_profile_records_are_the_rays_calls_plus_one_pre_pass():
    import ray3d_amd
    cams, ocams = _h36m_distorted_cameras()
    pos, trj, (cp, _), _ = build_modules(ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3"))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    rf, B = cp.receptive_field, 40
    uv = _pixels("profile", (B, rf, 17, 2))
    rays = torch.from_numpy(np.stack([_oracle_rays(ocams[i % 4], uv[i]) for i in range(B)])).cuda()
    rows = torch.from_numpy(np.stack([cams[i % 4].cam_row(distortion=True) for i in range(B)])).cuda()
    par = torch.from_numpy(np.stack([cams[i % 4].param() for i in range(B)])).cuda()
    uvd = torch.from_numpy(uv).cuda()
    with torch.no_grad():
        lifter.forward_uv(uvd, rows, par)                        # (each profiled call follows one on other buffers: both bind)
        r_rays = lifter.profile_call(lambda: lifter(rays, par), "cuda:0")
        r_dist = lifter.profile_call(lambda: lifter.forward_uv(uvd, rows, par), "cuda:0")
    names = lambda recs: sorted(r["kernel"] for r in recs)
    pre = [r for r in r_dist if r["kernel"] == "r3d_undistort_rays_f64"]
    assert len(pre) == 1 and pre[0]["stage"] == 0 and pre[0]["blocks"] == (B * rf * 17 + 255) // 256, r_dist
    assert names(r_dist) == sorted(names(r_rays) + ["r3d_undistort_rays_f64"]), (names(r_dist), names(r_rays))


def test_uv_dist_argument_errors():
    """R3D_ERR_ARG: a model of INPUT_DIM 2, no cam_dev, cam_stride 8; R3D_ERR_WORKSPACE: a workspace of r3d_workspace_bytes."""
    import ray3d_amd
    from ray3d_amd import _capi
    cams, _ = _h36m_distorted_cameras()
    dev = torch.device("cuda:0")
    lib = _capi.load()
    pos, trj, (cp, _), _ = build_modules(ray3d_amd.default_model_config(ARCHITECTURE="3,3"))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    rf, B = cp.receptive_field, 17
    uv = torch.from_numpy(_pixels("errors", (B, rf, 17, 2))).cuda()
    rows = torch.from_numpy(np.stack([cams[i % 4].cam_row(distortion=True) for i in range(B)])).cuda()
    par = torch.from_numpy(np.stack([cams[i % 4].param() for i in range(B)])).cuda()
    out = torch.empty((B, 1, 17, 3), device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(h_pos, h_trj, inp, ws_bytes):
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        return lib.r3d_forward_pair(h_pos.ptr, h_trj.ptr, C.byref(inp), B, out.data_ptr(), None, ws.data_ptr(), ws_bytes, st)

    good = _capi.make_input(_capi.R3D_INPUT_UV_DIST, uv.data_ptr(), rf, par.data_ptr(), 2, rows.data_ptr(), 16)
    big = _capi.input_workspace_bytes(hp, ht, good, B)
    assert call(hp, ht, good, big) == 0
    no_cam = _capi.make_input(_capi.R3D_INPUT_UV_DIST, uv.data_ptr(), rf, par.data_ptr(), 2, None, 16)
    assert call(hp, ht, no_cam, big) == _capi.R3D_ERR_ARG and b"cam_dev" in lib.r3d_last_error()
    stride8 = _capi.make_input(_capi.R3D_INPUT_UV_DIST, uv.data_ptr(), rf, par.data_ptr(), 2, rows.data_ptr(), 8)
    assert call(hp, ht, stride8, big) == _capi.R3D_ERR_ARG and b"cam_stride" in lib.r3d_last_error()
    small = _capi.workspace_bytes(hp, ht, B)
    assert small < big
    assert call(hp, ht, good, small) == _capi.R3D_ERR_WORKSPACE
    with pytest.raises(_capi.Ray3DHipError, match=r"\(-6\)"):
        _capi.forward_pair(hp, ht, good, B, out.data_ptr(), None, lifter._ws.get(big, dev).data_ptr(), small, st)
    torch.cuda.synchronize()
    # a pair of INPUT_DIM 2: no rays to undistort into
    pos2, trj2, _, _ = build_modules(ray3d_amd.default_model_config(ARCHITECTURE="3,3", INPUT_DIM=2))
    lifter2 = ray3d_amd.Ray3DLifter(pos2, trj2).eval()
    h2p, h2t = lifter2.pos.handle(dev), lifter2.trj.handle(dev)
    assert call(h2p, h2t, good, big) == _capi.R3D_ERR_ARG and b"in_features" in lib.r3d_last_error()
    with pytest.raises(RuntimeError, match="INPUT_DIM == 3"):
        lifter2.forward_uv(uv, rows, par)
    # the module refuses rows of any other width
    with pytest.raises(RuntimeError, match="cam_rows"):
        lifter.forward_uv(uv, rows[:, :12], par)
