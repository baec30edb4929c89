"""-m gpu: R3D_INPUT_PX_INTRINSIC / R3D_INPUT_PX_SCREEN - raw pixels in for the 2-feature (cfg_rie_*) models: the
r3d_undistort_rays_f64 pre-pass writes 2 floats per keypoint into the workspace tail, the R3D_INPUT_RAYS forward reads
them.  Comparands: the host's float64 -> float32 encodings (Camera.screen_from_uv / intrinsic_from_uv) bit for bit, the
R3D_INPUT_RAYS forward on them, the torch port of the oracle at the literal 1e-4 bound, and Trainer.evaluate_core's
metrics for the RAY_ENCODING False branches (tests/golden/px2d.npz)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, check_parity, record_parity
from test_gpu_parity import _oracle_lift, build_modules
from test_gpu_undistort import _pixels, _ulp_check

pytestmark = pytest.mark.gpu

J = 17
MPJPE_MM, OTHERS_MM = 2e-2, 5e-2     # the evalcore bounds of test_host.py / test_gpu_parity.py, millimetres
# (name, encoding keyword, distorted cameras?, exact?): the screen encoding ignores the coefficients; the intrinsic one is
# bit-exact against the host with zero coefficients and within the pre-pass's ulp rule with H36M's
ENCODINGS = [("screen", "screen", True, True), ("intrinsic-zero", "intrinsic", False, True), ("intrinsic-h36m", "intrinsic", True, False)]


@functools.lru_cache(maxsize=None)
def _cameras(distorted):
    """The four H36M cameras (S9; 1000 x 1002 pixels) with their coefficient sets (undistort=True) or without."""
    import ray3d_amd
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    u = np.load(os.path.join(GOLDEN, "undistort.npz"))
    return tuple(ray3d_amd.Camera(u["cam%d/K" % i], z["h36m_S9_%d/R" % i], z["h36m_S9_%d/t" % i], res_w=1000, res_h=1002,
                                  dist_coeff=u["cam%d/dist" % i] if distorted else None, undistort=distorted) for i in range(4))


@functools.lru_cache(maxsize=None)
def _pair(arch):
    """A pos + trj pair of INPUT_DIM 2 without the camera embedding: (lifter, ((cfg, state) pos, (cfg, state) trj))."""
    import ray3d_amd
    pos, trj, sp, st = build_modules(ray3d_amd.default_model_config(ARCHITECTURE=arch, INPUT_DIM=2, CAMERA_EMBDDING=False))
    return ray3d_amd.Ray3DLifter(pos, trj).eval(), (sp, st)


def _mode(keyword):
    from ray3d_amd import _capi
    return _capi.R3D_INPUT_PX_SCREEN if keyword == "screen" else _capi.R3D_INPUT_PX_INTRINSIC


def _host(cam, uv, keyword):
    """The host chain: float32 pixels promoted to float64, the encoding in float64, one cast."""
    uv = np.asarray(uv, dtype=np.float32).astype(np.float64)
    return (cam.screen_from_uv(uv) if keyword == "screen" else cam.intrinsic_from_uv(uv)).astype(np.float32)


def _rows(cams, pick):
    return torch.from_numpy(np.stack([cams[c].cam_row(distortion=True) for c in pick])).cuda()


def _layouts(rf):
    """(name, B, window_stride, per-window cameras?, frames of pixels, frames the pre-pass writes): per-window rows on a
    (B, RF, J, 2) batch - 765 points at RF 9, three workgroups, the last one partial -, a 30-frame sliding sequence with one
    camera, overlapping windows with their own cameras (materialised), and one window."""
    return [("batch of 5, per-window rows", 5, rf, True, 5 * rf, 5 * rf),
            ("30-frame sequence, one camera", 30 - rf + 1, 1, False, 30, 30),
            ("4 overlapping windows, own cameras", 4, 1, True, 3 + rf, 4 * rf),
            ("one window", 1, rf, False, rf, rf)]


def _layout_case(name, B, stride, per_window, n_in, keyword, cams, rf):
    """(pixels (n_in, J, 2), camera picks, camera rows on the device, cam_stride, the host encoding as (B, RF, J, 2) windows)."""
    uv = _pixels("px2d.%s.%s.%d" % (name, keyword, rf), (n_in, J, 2))
    pick = [(3 * i + 1) % 4 for i in range(B)] if per_window else [2] * B
    rows = _rows(cams, pick) if per_window else _rows(cams, pick[:1])[0]
    windows = np.stack([_host(cams[c], uv[i * stride:i * stride + rf], keyword) for i, c in enumerate(pick)])
    return uv, pick, rows, (16 if per_window else 0), windows


def test_pre_pass_output_equals_the_host_encoding_in_every_layout():
    """The pre-pass's float32 output, read from the workspace tail at r3d_workspace_bytes rounded up to 256."""
    from ray3d_amd import _capi
    lifter, _ = _pair("3,3")
    dev = torch.device("cuda:0")
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    rf = lifter.receptive_field()
    assert rf == 9
    for ename, keyword, distorted, exact in ENCODINGS:
        cams = _cameras(distorted)
        for name, B, stride, per_window, n_in, n_out in _layouts(rf):
            uv, pick, rows, cstride, windows = _layout_case(name, B, stride, per_window, n_in, keyword, cams, rf)
            uvd = torch.from_numpy(uv).cuda()
            inp = _capi.make_input(_mode(keyword), uvd.data_ptr(), stride, None, 0, rows.data_ptr(), cstride)
            nbytes = _capi.input_workspace_bytes(hp, ht, inp, B)
            off = (_capi.workspace_bytes(hp, ht, B) + 255) // 256 * 256
            assert off + n_out * J * 8 <= nbytes <= off + n_out * J * 8 + 256
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty((B, 1, J, 3), device=dev)
            _capi.forward_pair(hp, ht, inp, B, out.data_ptr(), None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = ws[off:off + n_out * J * 8].view(torch.float32).view(n_out, J, 2).cpu().numpy()
            if n_out == B * rf:                  # (B, RF, J, 2): the batch itself, or the materialised windows
                want = windows.reshape(B * rf, J, 2)
            else:                                # one point per input frame, one camera
                want = _host(cams[pick[0]], uv, keyword)
            what = "%s, %s" % (ename, name)
            if exact:
                assert np.array_equal(got, want), (what, float(np.abs(got - want).max()))
            else:
                _ulp_check(got, want, what)
            assert torch.isfinite(out).all(), what


@pytest.mark.parametrize("staged", [False, True], ids=["single-launch", "staged"])
@pytest.mark.parametrize("arch", ["3,3", "3,3,3"])
def test_forward_from_pixels_equals_the_rays_forward_on_the_host_encoding(arch, staged):
    """forward_uv(..., encoding=) (r3d_forward_pair) in the four layouts: bit-equal to the R3D_INPUT_RAYS forward on the
    host-encoded input for the exact encodings, and within 1e-4 of the oracle chain (the torch port on that input) for all."""
    lifter, states = _pair(arch)
    rf = lifter.receptive_field()
    lifter.set_staged(staged)
    try:
        for ename, keyword, distorted, exact in ENCODINGS:
            cams = _cameras(distorted)
            for name, B, stride, per_window, n_in, n_out in _layouts(rf):
                if n_in < rf:
                    continue
                uv, pick, rows, cstride, windows = _layout_case(name, B, stride, per_window, n_in, keyword, cams, rf)
                uvd = torch.from_numpy(uv).cuda()
                with torch.no_grad():
                    if stride == rf:
                        got = lifter.forward_uv(uvd.view(B, rf, J, 2), rows, encoding=keyword)
                        want = lifter(torch.from_numpy(windows).cuda(), None)
                    else:
                        got = lifter.forward_uv(uvd, rows, window_stride=stride, encoding=keyword)
                        if per_window:           # materialised windows: the batch forward on the same windows
                            want = lifter(torch.from_numpy(windows).cuda(), None)
                        else:                    # a sliding sequence: forward_clip on the host-encoded sequence
                            want = lifter.forward_clip(torch.from_numpy(_host(cams[pick[0]], uv, keyword)).cuda(), None)
                what = "%s, %s" % (ename, name)
                assert got.shape == (B, 1, J, 3), what
                if exact:
                    assert torch.equal(got, want), (what, float((got - want).abs().max()))
                else:
                    check_parity(got, want.cpu().numpy(), what + " vs the rays mode on the host encoding")
                check_parity(got, _oracle_lift(states, windows, np.zeros((B, 2), dtype=np.float32)), what + " vs the oracle chain")
    finally:
        lifter.set_staged(False)


@pytest.mark.parametrize("staged", [False, True], ids=["single-launch", "staged"])
def test_r3d_forward_of_one_model_from_pixels(staged):
    """r3d_forward on a pos-only and on a trj-only handle through the C ABI: both pixel modes equal R3D_INPUT_RAYS on the
    host-encoded batch bit for bit."""
    from ray3d_amd import _capi
    lifter, _ = _pair("3,3,3")
    dev = torch.device("cuda:0")
    rf, B = lifter.receptive_field(), 5
    st = torch.cuda.current_stream().cuda_stream
    lifter.set_staged(staged)
    try:
        for ename, keyword, distorted, exact in ENCODINGS[:2]:
            cams = _cameras(distorted)
            uv, pick, rows, cstride, windows = _layout_case("single", B, rf, True, B * rf, keyword, cams, rf)
            uvd, xd = torch.from_numpy(uv).cuda(), torch.from_numpy(windows).cuda()
            for h, pos_h in ((lifter.pos.handle(dev), True), (lifter.trj.handle(dev), False)):
                outs = []
                for inp in (_capi.make_input(_capi.R3D_INPUT_RAYS, xd.data_ptr(), rf, None, 0),
                            _capi.make_input(_mode(keyword), uvd.data_ptr(), rf, None, 0, rows.data_ptr(), 16)):
                    ws = torch.empty(_capi.input_workspace_bytes(h if pos_h else None, None if pos_h else h, inp, B), dtype=torch.uint8, device=dev)
                    out = torch.full((B, 1, J if pos_h else 1, 3), float("nan"), device=dev)
                    _capi.forward(h, inp, B, out.data_ptr(), ws.data_ptr(), ws.numel(), st)
                    torch.cuda.synchronize()
                    outs.append(out)
                assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]), (ename, pos_h)
    finally:
        lifter.set_staged(False)


RIE_CASES = [("screen_trj", "screen", True), ("screen_notrj", "screen", False), ("intrinsic_trj", "intrinsic", True)]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case,keyword,with_trj", RIE_CASES)
def test_clip_evaluation_from_raw_pixels_reproduces_evaluate_core(case, keyword, with_trj, flip):
    """Trainer.evaluate_core's five metrics with RAY_ENCODING False (tests/golden/px2d.npz) on the GPU from the clip's raw
    pixels: the pair through forward_uv(..., window_stride=1) and camera2world (r3d_clip_metrics with Rc2w / Tc2w); the
    pos-only model through r3d_forward and the root-relative ground truth.  The flip pass mirrors the pixels
    (evaluate.mirror_pixels)."""
    import ray3d_amd
    from ray3d_amd import _capi, evaluate
    z = np.load(os.path.join(GOLDEN, "px2d.npz"))
    w, h = z["eval/res"]
    cam = ray3d_amd.Camera(z["eval/K"], z["eval/R"], z["eval/t"], res_w=w, res_h=h)
    lifter, _ = _pair("3,3,3")
    dev = torch.device("cuda:0")
    row = torch.from_numpy(cam.cam_row(distortion=True)).cuda()
    if with_trj:
        lift = lambda padded, prow: lifter.forward_uv(padded, row, window_stride=1, encoding=keyword)
    else:
        hp = lifter.pos.handle(dev)

        def lift(padded, prow):
            n = padded.shape[0] - 27 + 1
            padded = padded.contiguous()
            inp = _capi.make_input(_mode(keyword), padded.data_ptr(), 1, None, 0, row.data_ptr(), 0)
            ws = torch.empty(_capi.input_workspace_bytes(hp, None, inp, n), dtype=torch.uint8, device=dev)
            out = torch.empty((n, 1, J, 3), device=dev)
            _capi.forward(hp, inp, n, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()             # (ws and padded are this call's own)
            return out
    kl, kr = list(z["eval/kps_left"]), list(z["eval/kps_right"])
    clip = evaluate.Clip(cam, z["eval/uv"], z["eval/gt_cam"], "A", 0, frame="camera")
    with torch.no_grad():
        named, _, rows = evaluate.evaluate_clips(lift, [clip], 27, dev, flip=flip, kps_left=kl, kps_right=kr,
                                                 root_relative=not with_trj, mirror=evaluate.mirror_pixels(cam, keyword, kl, kr))
    got, ref = np.array(named["A"]), z["eval/%s/metrics_flip%d" % (case, int(flip))]
    print(case, "flip", flip, "got", got, "ref", ref, "diff", got - ref)
    for name, g, r, tol in zip(_capi.METRIC_NAMES, got, ref, (MPJPE_MM,) + (OTHERS_MM,) * 4):
        record_parity("px2d clip evaluation %s flip%d %s (mm)" % (case, int(flip), name), abs(g - r), tol, abs(r))
    assert abs(got[0] - ref[0]) < MPJPE_MM, (got, ref)
    assert np.abs(got - ref).max() < OTHERS_MM, (got, ref)


def test_px_forward_on_lanes_equals_the_lane_less_result():
    """set_lanes(2): two pixel-mode forwards relayed from a caller's stream (by the module, and by the library through the C
    ABI), joined, equal the forward without lanes."""
    from ray3d_amd import _capi
    lifter, _ = _pair.__wrapped__("3,3,3")                          # (a pair of its own: the lanes change the handles)
    dev = torch.device("cuda:0")
    rf, B = lifter.receptive_field(), 64
    cams = _cameras(True)
    rows = _rows(cams, [i % 4 for i in range(B)])
    uva = torch.from_numpy(_pixels("px2d.lanes.a", (B, rf, J, 2))).cuda()
    uvb = torch.from_numpy(_pixels("px2d.lanes.b", (B, rf, J, 2))).cuda()
    with torch.no_grad():
        want_a = lifter.forward_uv(uva, rows, encoding="screen").clone()
        want_b = lifter.forward_uv(uvb, rows, encoding="intrinsic").clone()
        torch.cuda.synchronize()
        lifter.set_lanes(2)
        s = torch.cuda.Stream()
        try:
            with torch.cuda.stream(s):                              # the module relays to lanes 0 and 1
                oa = lifter.forward_uv(uva, rows, encoding="screen")
                ob = lifter.forward_uv(uvb, rows, encoding="intrinsic")
                lifter.join_lanes()
                ca, cb = oa.clone(), ob.clone()
            torch.cuda.synchronize()
            # (a lane has half the CUs: other tile schedules, other split-K sums - HIP against HIP at a bound that scales with |ref|)
            tol = 2e-5 * max(1.0, float(want_a.abs().max()), float(want_b.abs().max()))
            check_parity(ca, want_a.cpu().numpy(), "module relay, lane 0 (HIP against HIP)", tol=tol)
            check_parity(cb, want_b.cpu().numpy(), "module relay, lane 1 (HIP against HIP)", tol=tol)
            hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)   # the library relays (C ABI, caller's stream)
            outs = []
            for uv, mode in ((uva, _capi.R3D_INPUT_PX_SCREEN), (uvb, _capi.R3D_INPUT_PX_INTRINSIC)):
                inp = _capi.make_input(mode, uv.data_ptr(), rf, None, 0, rows.data_ptr(), 16)
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


def test_px_forward_captured_in_a_hip_graph():
    """A pixel-mode forward captured with torch.cuda.graph after prepare (the pre-pass is captured with it): replayed after
    new pixels were written into the captured input, it equals the eager call on those pixels."""
    from ray3d_amd import _capi
    lifter, _ = _pair.__wrapped__("3,3,3")                          # (a pair of its own: it pins a schedule)
    dev = torch.device("cuda:0")
    rf, B = lifter.receptive_field(), 53                             # (a batch size nothing else here uses)
    rows = _rows(_cameras(True), [i % 4 for i in range(B)])
    uv = torch.from_numpy(_pixels("px2d.graph.a", (B, rf, J, 2))).cuda()
    uv2 = torch.from_numpy(_pixels("px2d.graph.b", (B, rf, J, 2))).cuda()
    lifter.prepare([B])
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    inp = _capi.make_input(_capi.R3D_INPUT_PX_SCREEN, uv.data_ptr(), rf, None, 0, rows.data_ptr(), 16)
    lifter._ws.get(_capi.input_workspace_bytes(hp, ht, inp, B), dev)
    out = torch.empty((B, 1, J, 3), device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            lifter._run(_capi.R3D_INPUT_PX_SCREEN, uv, rf, B, None, 0, rows, 16, out=out)
    uv.copy_(uv2)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = lifter.forward_uv(uv2, rows, encoding="screen")
    assert torch.isfinite(eager).all() and torch.equal(out, eager)
    del g
    torch.cuda.synchronize()
    _capi.release(hp, ht, B)


def test_profile_records_are_the_rays_calls_plus_one_pre_pass():
    lifter, _ = _pair("3,3,3")
    rf, B = lifter.receptive_field(), 40
    cams = _cameras(True)
    uv = _pixels("px2d.profile", (B, rf, J, 2))
    x = torch.from_numpy(np.stack([_host(cams[i % 4], uv[i], "screen") for i in range(B)])).cuda()
    rows = _rows(cams, [i % 4 for i in range(B)])
    uvd = torch.from_numpy(uv).cuda()
    with torch.no_grad():
        lifter.forward_uv(uvd, rows, encoding="screen")             # (each profiled call follows one on other buffers: both bind)
        r_rays = lifter.profile_call(lambda: lifter(x, None), "cuda:0")
        r_px = lifter.profile_call(lambda: lifter.forward_uv(uvd, rows, encoding="screen"), "cuda:0")
    names = lambda recs: sorted(r["kernel"] for r in recs)
    pre = [r for r in r_px if r["kernel"] == "r3d_undistort_rays_f64"]
    assert len(pre) == 1 and pre[0]["stage"] == 0 and pre[0]["blocks"] == (B * rf * J + 255) // 256, r_px
    assert pre[0]["bytes"] == B * rf * J * (2 + 2) * 4                # 2 floats read and 2 written per keypoint
    assert names(r_px) == sorted(names(r_rays) + ["r3d_undistort_rays_f64"]), (names(r_px), names(r_rays))


def test_px_mode_argument_errors_on_the_device_path():
    """R3D_ERR_WORKSPACE: a workspace of r3d_workspace_bytes; R3D_ERR_ARG on finalised handles; the module's own checks."""
    import ray3d_amd
    from ray3d_amd import _capi
    lifter, _ = _pair("3,3")
    dev = torch.device("cuda:0")
    lib = _capi.load()
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    rf, B = lifter.receptive_field(), 17
    uv = torch.from_numpy(_pixels("px2d.errors", (B, rf, J, 2))).cuda()
    rows = _rows(_cameras(True), [i % 4 for i in range(B)])
    out = torch.empty((B, 1, J, 3), device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(h_pos, h_trj, inp, ws_bytes):
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        return lib.r3d_forward_pair(h_pos.ptr, h_trj.ptr, C.byref(inp), B, out.data_ptr(), None, ws.data_ptr(), ws_bytes, st)

    for mode, name in ((_capi.R3D_INPUT_PX_INTRINSIC, b"R3D_INPUT_PX_INTRINSIC"), (_capi.R3D_INPUT_PX_SCREEN, b"R3D_INPUT_PX_SCREEN")):
        good = _capi.make_input(mode, uv.data_ptr(), rf, None, 0, rows.data_ptr(), 16)
        big, small = _capi.input_workspace_bytes(hp, ht, good, B), _capi.workspace_bytes(hp, ht, B)
        assert small < big
        assert call(hp, ht, good, big) == 0
        assert call(hp, ht, good, small) == _capi.R3D_ERR_WORKSPACE and name in lib.r3d_last_error()
        assert call(hp, ht, _capi.make_input(mode, uv.data_ptr(), rf, None, 0, None, 16), big) == _capi.R3D_ERR_ARG
        assert name in lib.r3d_last_error() and b"cam_dev" in lib.r3d_last_error()
        assert call(hp, ht, _capi.make_input(mode, uv.data_ptr(), rf, None, 0, rows.data_ptr(), 8), big) == _capi.R3D_ERR_ARG
        assert name in lib.r3d_last_error() and b"cam_stride" in lib.r3d_last_error()
        with pytest.raises(_capi.Ray3DHipError, match=r"\(-6\)"):
            _capi.forward_pair(hp, ht, good, B, out.data_ptr(), None, lifter._ws.get(big, dev).data_ptr(), small, st)
    torch.cuda.synchronize()
    # a pair of INPUT_DIM 3 takes rays: the 2-float encodings are refused by the library and by the module
    pos3, trj3, _, _ = build_modules(ray3d_amd.default_model_config(ARCHITECTURE="3,3"))
    lifter3 = ray3d_amd.Ray3DLifter(pos3, trj3).eval()
    h3p, h3t = lifter3.pos.handle(dev), lifter3.trj.handle(dev)
    assert call(h3p, h3t, good, big) == _capi.R3D_ERR_ARG and b"in_features" in lib.r3d_last_error()
    with pytest.raises(RuntimeError, match="INPUT_DIM == 2"):
        lifter3.forward_uv(uv, rows, torch.zeros((B, 2)).cuda(), encoding="screen")
    with pytest.raises(RuntimeError, match="INPUT_DIM == 3"):
        lifter.forward_uv(uv, rows)
    no_res = rows.clone()
    no_res[3, 6] = 0.0
    with pytest.raises(RuntimeError, match="res_w"):
        lifter.forward_uv(uv, no_res, encoding="screen")
    torch.cuda.synchronize()
