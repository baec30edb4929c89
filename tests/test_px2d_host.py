"""CPU suite: the 2-feature (cfg_rie_*) models' inputs from raw pixels and their camera-frame evaluation, without a GPU -
the pre-pass's two 2-float encodings run on the host through the hooks build (r3d_debug_encode_px_host) against the
reference's own values (tests/golden/px2d.npz, written by tests/golden/make_golden_px2d.py), the Camera additions,
evaluate_clips with frame="camera" / root_relative against Trainer.evaluate_core's five metrics, the argument errors
of R3D_INPUT_PX_INTRINSIC / R3D_INPUT_PX_SCREEN that need no device, and the defaults."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, hooks_library, synth_states

import ray3d_amd
from ray3d_amd import _capi, evaluate
from ray3d_amd.spec import config_from_dicts, default_model_config

ENC_INTRINSIC, ENC_SCREEN = 1, 2
# the evalcore bounds of this suite, in millimetres (test_host.py test_evaluate_reproduces_reference_evaluate_core,
# test_gpu_parity.py test_evaluate_clips_reproduces_reference_metrics): MPJPE to 2e-2, the other four to 5e-2
MPJPE_MM, OTHERS_MM = 2e-2, 5e-2


def _px2d():
    return np.load(os.path.join(GOLDEN, "px2d.npz"))


def _encode2d_host(row16, uv, encoding):
    """r3d_debug_encode_px_host: (n, 2) float64, the values before the cast."""
    lib = hooks_library()
    row16 = np.ascontiguousarray(row16, dtype=np.float64)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    out = np.full_like(uv, np.nan)
    rc = lib.r3d_debug_encode_px_host(row16.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p), uv.shape[0], encoding,
                                     out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.r3d_last_error()
    return out


def _fixture_camera(z, prefix):
    w, h = z[prefix + "/res"]
    return ray3d_amd.Camera(z[prefix + "/K"], z[prefix + "/R"], z[prefix + "/t"], res_w=w, res_h=h)


def _ulp_check(got, want, what):
    """>= 99.99 % of the elements equal, the rest within one float32 ulp (the rule of test_gpu_undistort.py)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    eq = got == want
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    frac = float(eq.mean())
    print("%s: %.6f of %d elements equal, max %d ulp" % (what, frac, got.size, int(ulps.max())))
    assert frac >= 0.9999, (what, frac)
    assert int(ulps[~eq].max(initial=0)) <= 1, (what, int(ulps.max()))


# ------------------------------------------------------------------ the encodings

def test_hook_encodings_equal_the_reference_bit_for_bit():
    """normalize_screen_coordinates and encode_uv_with_intrinsic (undistort=False) of ~200 pixel pairs per camera - principal
    point, corners, points outside the image - are the same IEEE operations in the same order: float64 equality."""
    z = _px2d()
    assert len(z["enc/tags"]) == 2
    for tag in z["enc/tags"]:
        p = "enc/%s" % tag
        cam = _fixture_camera(z, p)
        X = z[p + "/X"]
        assert X.shape == (200, 2) and X.dtype == np.float64
        row = cam.cam_row(distortion=True)
        assert not row[8:].any()
        got_s, got_i = _encode2d_host(row, X, ENC_SCREEN), _encode2d_host(row, X, ENC_INTRINSIC)
        assert np.array_equal(got_s, z[p + "/screen"]), (tag, np.abs(got_s - z[p + "/screen"]).max())
        assert np.array_equal(got_i, z[p + "/intrinsic"]), (tag, np.abs(got_i - z[p + "/intrinsic"]).max())
        # the screen encoding reads the resolution slots and nothing else; the intrinsic one does not read them
        other = row.copy()
        other[:6] = 7.0
        other[8:13] = 0.1
        assert np.array_equal(_encode2d_host(other, X, ENC_SCREEN), got_s)
        other = row.copy()
        other[4:8] = -3.0
        assert np.array_equal(_encode2d_host(other, X, ENC_INTRINSIC), got_i)
    # a 1000 x 1002 image: the second component is shifted by h / w, not by 1
    w, h = z["enc/h36m_S9_0/res"]
    assert (w, h) == (1000.0, 1002.0)
    corner = _encode2d_host(_fixture_camera(z, "enc/h36m_S9_0").cam_row(distortion=True), [[w, h]], ENC_SCREEN)
    assert corner[0, 0] == 1.0 and corner[0, 1] == h / w * 2 - h / w


def _h36m_distorted_cameras():
    """The four H36M cameras of cameras.npz (S9) with the four coefficient sets of undistort.npz, built undistort=True."""
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    u = np.load(os.path.join(GOLDEN, "undistort.npz"))
    return u, [ray3d_amd.Camera(u["cam%d/K" % i], z["h36m_S9_%d/R" % i], z["h36m_S9_%d/t" % i], dist_coeff=u["cam%d/dist" % i],
                                undistort=True, res_w=1000, res_h=1002) for i in range(int(u["n"]))]


def test_hook_intrinsic_encoding_undistorts_first():
    """The four H36M coefficient sets on the dense 65 x 65 grid of undistort.npz (whole image, corners included) and on the
    9 x 9 grid of the host suite's consistency test: the hook's intrinsic encoding against Camera.intrinsic_from_uv, after
    the float32 cast."""
    u, cams = _h36m_distorted_cameras()
    coarse = np.stack(np.meshgrid(np.linspace(100, 900, 9), np.linspace(100, 900, 9)), -1).reshape(-1, 2)
    for i, cam in enumerate(cams):
        pts = np.concatenate([u["cam%d/dense_distorted" % i], coarse])
        row = cam.cam_row(distortion=True)
        assert np.array_equal(row[8:13], u["cam%d/dist" % i])
        got = _encode2d_host(row, pts, ENC_INTRINSIC)
        want = cam.intrinsic_from_uv(pts)
        _ulp_check(got.astype(np.float32), want.astype(np.float32), "intrinsic encoding, H36M coefficient set %d" % i)
        plain = ray3d_amd.Camera(cam.K, cam.Rw2c, cam.Tw2c)
        assert np.abs(want - plain.intrinsic_from_uv(pts)).max() > 1e-3          # ... and the undistortion is not a no-op
        assert np.array_equal(want, plain.intrinsic_from_uv(cam.undistort_points(pts)))
        # the screen encoding does NOT undistort: the coefficients change nothing
        assert np.array_equal(_encode2d_host(row, pts, ENC_SCREEN), cam.screen_from_uv(pts))


def test_hook_rejects_bad_arguments():
    lib = hooks_library()
    row, uv, out = np.ones(16), np.ones((1, 2)), np.empty((1, 2))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.r3d_debug_encode_px_host(None, ptr(uv), 1, ENC_SCREEN, ptr(out)) == _capi.R3D_ERR_ARG
    assert lib.r3d_debug_encode_px_host(ptr(row), ptr(uv), 1, ENC_SCREEN, None) == _capi.R3D_ERR_ARG
    for bad in (0, 3, -1):
        assert lib.r3d_debug_encode_px_host(ptr(row), ptr(uv), 1, bad, ptr(out)) == _capi.R3D_ERR_ARG
        assert b"encoding" in lib.r3d_last_error()
    assert lib.r3d_debug_encode_px_host(ptr(row), None, 0, ENC_SCREEN, ptr(out)) == 0


# ------------------------------------------------------------------ Camera

def test_camera_encodings_frames_and_row():
    z = _px2d()
    for tag in z["enc/tags"]:
        p = "enc/%s" % tag
        cam = _fixture_camera(z, p)
        X = z[p + "/X"]
        assert np.array_equal(cam.screen_from_uv(X), z[p + "/screen"])
        assert np.array_equal(cam.intrinsic_from_uv(X), z[p + "/intrinsic"])
        assert cam.screen_from_uv(X.astype(np.float32)).dtype == np.float64       # float64 whatever the archive's dtype
        assert cam.screen_from_uv(X.reshape(20, 10, 2)).shape == (20, 10, 2)
        # world <-> camera: the two are inverse rigid motions, and the camera centre is the camera frame's origin.  The
        # tables' R is rounded to float32 (entries off by <= 2^-25), so R^T R - I has entries of up to ~2e-7 and Rc2w = Rw2c^T
        # - the reference's definition - inverts it to that much times the distance from the camera (<= ~15 m here): 1e-5;
        # an exactly orthonormal camera round-trips to float64 rounding.
        pts = np.random.default_rng(3).normal(0.0, 2.0, (50, 17, 3))
        assert np.abs(cam.camera2world(cam.world2camera(pts)) - pts).max() < 1e-5
        assert np.abs(cam.world2camera(cam.camera2world(pts)) - pts).max() < 1e-5
        exact = ray3d_amd.synthetic_camera(35.0, 4.5, -12.0)
        assert np.abs(exact.camera2world(exact.world2camera(pts)) - pts).max() < 1e-12
        assert np.abs(exact.world2camera(exact.camera2world(pts)) - pts).max() < 1e-12
        assert np.array_equal(cam.Rc2w, cam.Rw2c.T) and np.array_equal(cam.Tc2w, -(cam.Rw2c.T @ cam.Tw2c))
        assert np.abs(cam.world2camera(cam.position_world.T)).max() < 1e-5
        assert np.abs(exact.world2camera(exact.position_world.T)).max() < 1e-12
        # ... and the normalised frame is the camera frame rotated by the pitch and shifted by the height
        assert np.abs(cam.world2camera(pts) @ cam.Rc2n.T + cam.Tc2n.T - cam.world2normalized(pts)).max() < 1e-12
        # the 16-double row: slots 6 / 7 carry the resolution, everything else is as without one; the 8-double row is unchanged
        w, h = z[p + "/res"]
        row = cam.cam_row(distortion=True)
        bare = ray3d_amd.Camera(z[p + "/K"], z[p + "/R"], z[p + "/t"])
        assert (row[6], row[7]) == (w, h)
        assert tuple(bare.cam_row(distortion=True)[6:8]) == (0.0, 0.0)
        keep = [0, 1, 2, 3, 4, 5] + list(range(8, 16))
        assert np.array_equal(row[keep], bare.cam_row(distortion=True)[keep])
        assert np.array_equal(cam.cam_row(), bare.cam_row()) and cam.cam_row().shape == (8,)
        with pytest.raises(ValueError, match="resolution"):
            bare.screen_from_uv(X)


def test_camera_tables_pass_the_resolution_through():
    from ray3d_amd import dataset
    ext = {"S0": [{"R": np.eye(3), "translation": [1841.1, 4955.3, 1563.4]}]}
    intr = [{"focal_length": [1145.0, 1143.8], "center": [512.5, 515.5], "res_w": 1000, "res_h": 1002,
             "radial_distortion": [-0.2, 0.24, -0.002], "tangential_distortion": [-0.0009, -0.0016]}]
    cam = dataset.cameras_from_tables(ext, intr, translation_divisor=1000, undistort=True)["S0"][0]
    assert (cam.res_w, cam.res_h) == (1000.0, 1002.0) and tuple(cam.cam_row(distortion=True)[6:8]) == (1000.0, 1002.0)
    no_res = [{k: v for k, v in intr[0].items() if not k.startswith("res_")}]
    cam = dataset.cameras_from_tables(ext, no_res, translation_divisor=1000)["S0"][0]
    assert cam.res_w is None and not cam.cam_row(distortion=True)[6:8].any()
    meta = [{"id": "c0", "center": [512.5, 515.5], "focal_length": [1145.0, 1143.8], "radial_distortion": [0.0, 0.0, 0.0],
             "tangential_distortion": [0.0, 0.0], "res_w": 1000, "res_h": 1002, "azimuth": 70, "R": np.eye(3).tolist(),
             "translation": [1.8, 4.9, 1.5]}]
    cams, ids = dataset.cameras_from_json(meta, subjects=("S1",))
    assert ids == ["c0"] and (cams["S1"][0].res_w, cams["S1"][0].res_h) == (1000.0, 1002.0)
    hev = dataset.cameras_humaneva({"S1": ext["S0"]}, [dict(intr[0], res_w=640, res_h=480)])
    assert (hev["Train/S1"][0].res_w, hev["Validate/S1"][0].res_h) == (640.0, 480.0)


# ------------------------------------------------------------------ evaluation

def _torch_lift_clip(mc, rf, with_trj=True):
    """CPU stand-in for the clip forward, built on the torch port of the oracle (checker role only): pos (+ trj)."""
    from oracle import torch_port
    (cp, sp), (ct, st) = synth_states(mc)
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]

    seen = {}                                  # (the same padded clip is lifted again by the detail / wrong-frame calls)

    def lift(padded, prow):
        key = hash(padded.numpy().tobytes())
        if key not in seen:
            seen[key] = _lift(padded, prow)
        return seen[key].clone()

    def _lift(padded, prow):
        n = padded.shape[0] - rf + 1
        win = torch.stack([padded[i:i + rf] for i in range(n)])
        par = prow.reshape(1, -1).repeat(n, 1) if cp.camera_embedding else None
        with torch.no_grad():
            out = torch_port.forward(cp, sds[0], win, par)
            if with_trj:
                out = out + torch_port.forward(ct, sds[1], win, par)
        return out
    return lift


RIE_CASES = [("screen_trj", "screen", True), ("screen_notrj", "screen", False), ("intrinsic_trj", "intrinsic", True)]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case,encoding,with_trj", RIE_CASES)
def test_evaluate_clips_reproduces_the_rie_branches_of_evaluate_core(case, encoding, with_trj, flip):
    """Trainer.evaluate_core with RAY_ENCODING False on the 100-frame clip: the camera2world branch (trajectory model), the
    root-relative branch (none), and the INTRINSIC_ENCODING input - the five metrics, in millimetres."""
    z = _px2d()
    cam = _fixture_camera(z, "eval")
    uv = z["eval/uv"]
    assert uv.dtype == np.float32 and uv.shape == (100, 17, 2)
    x = (cam.screen_from_uv(uv) if encoding == "screen" else cam.intrinsic_from_uv(uv)).astype(np.float32)
    clip = evaluate.Clip(cam, x, z["eval/gt_cam"], "A", 0, frame="camera")
    mc = default_model_config(ARCHITECTURE="3,3,3", INPUT_DIM=2, CAMERA_EMBDDING=False, TRAJECTORY_MODEL=with_trj)
    kl, kr = list(z["eval/kps_left"]), list(z["eval/kps_right"])
    lift = _torch_lift_clip(mc, 27, with_trj)
    named, _, rows = evaluate.evaluate_clips(lift, [clip], 27, "cpu", flip=flip, kps_left=kl, kps_right=kr, root_relative=not with_trj)
    got, ref = np.array(named["A"]), z["eval/%s/metrics_flip%d" % (case, int(flip))]
    print(case, flip, "got", got, "ref", ref, "diff", got - ref)
    assert abs(got[0] - ref[0]) < MPJPE_MM, (got, ref)
    assert np.abs(got - ref).max() < OTHERS_MM, (got, ref)
    # the detail entry point takes the same frame / root_relative and returns the same five sums
    named_d, _, rows_d, _ = evaluate.evaluate_clips_detail(lift, [clip], 27, "cpu", flip=flip, kps_left=kl, kps_right=kr,
                                                           root_relative=not with_trj)
    assert torch.equal(rows_d, rows)
    # the frame matters: the same clip read as a normalised-frame clip gives other numbers (the root-relative branch
    # transforms nothing, so there it does not)
    if with_trj:
        wrong = evaluate.Clip(cam, x, z["eval/gt_cam"], "A", 0)
        named_w, _, _ = evaluate.evaluate_clips(lift, [wrong], 27, "cpu", flip=flip, kps_left=kl, kps_right=kr)
        assert abs(named_w["A"][3] - ref[3]) < OTHERS_MM            # (velocity: invariant under any rigid motion)
        assert named_w["A"] != named["A"]
    assert np.array_equal(clip.gt_norm, z["eval/gt_cam"])           # the caller's ground truth is not modified


def test_root_relative_ground_truth():
    gt = np.arange(2 * 4 * 3, dtype=np.float32).reshape(2, 4, 3) ** 1.5
    rel = evaluate.root_relative_gt(gt)
    assert not rel[:, 0].any() and np.array_equal(rel[:, 1:], gt[:, 1:] - gt[:, :1]) and gt[0, 0, 1] == 1.0
    cam = ray3d_amd.synthetic_camera(30, 4.5, -12.0)
    R, T = evaluate.clip_world_transform(evaluate.Clip(cam, None, None, frame="camera"))
    assert R is cam.Rc2w and T is cam.Tc2w
    R, T = evaluate.clip_world_transform(evaluate.Clip(cam, None, None))
    assert R is cam.Rn2w and T is cam.Tn2w
    R, T = evaluate.clip_world_transform(evaluate.Clip(cam, None, None, frame="camera"), root_relative=True)
    assert np.array_equal(R, np.eye(3)) and not T.any()
    with pytest.raises(ValueError, match="frame"):
        evaluate.clip_world_transform(evaluate.Clip(cam, None, None, frame="world"))


# ------------------------------------------------------------------ argument errors that need no device

def _inp(mode, x=None, window_stride=9, cam=None, cam_stride=0):
    return _capi.make_input(mode, x, window_stride, None, 0, cam, cam_stride)


def test_px_mode_argument_errors_without_a_device():
    """R3D_ERR_ARG naming the mode - a 3-feature handle, a null cam_dev, cam_stride 8 - from r3d_forward / r3d_forward_pair
    before anything touches a device (the handles are not even finalised), and r3d_input_workspace_bytes == 0 with a
    message.  The host buffers below stand in for device pointers: no call gets far enough to read them."""
    lib = _capi.load()
    mc3 = default_model_config(ARCHITECTURE="3,3")
    mc2 = default_model_config(ARCHITECTURE="3,3", INPUT_DIM=2, CAMERA_EMBDDING=False)
    h3 = _capi.Handle(config_from_dicts(mc3, "pos"))
    h2p, h2t = _capi.Handle(config_from_dicts(mc2, "pos")), _capi.Handle(config_from_dicts(mc2, "trj"))
    buf = np.zeros(4096, dtype=np.float64)
    x = out = ws = cam = buf.ctypes.data
    B = 4
    fwd = lambda h, inp: lib.r3d_forward(h.ptr, C.byref(inp), B, out, ws, buf.nbytes, None)
    pair = lambda inp: lib.r3d_forward_pair(h2p.ptr, h2t.ptr, C.byref(inp), B, out, None, ws, buf.nbytes, None)
    for mode, name in ((_capi.R3D_INPUT_PX_INTRINSIC, b"R3D_INPUT_PX_INTRINSIC"), (_capi.R3D_INPUT_PX_SCREEN, b"R3D_INPUT_PX_SCREEN")):
        good = _inp(mode, x, 9, cam, 16)
        assert fwd(h3, good) == _capi.R3D_ERR_ARG
        assert name in lib.r3d_last_error() and b"in_features" in lib.r3d_last_error()
        for call in (lambda i: fwd(h2p, i), lambda i: fwd(h2t, i), pair):
            assert call(_inp(mode, x, 9, None, 16)) == _capi.R3D_ERR_ARG
            assert name in lib.r3d_last_error() and b"cam_dev" in lib.r3d_last_error()
            assert call(_inp(mode, x, 9, cam, 8)) == _capi.R3D_ERR_ARG
            assert name in lib.r3d_last_error() and b"cam_stride" in lib.r3d_last_error()
            assert call(good) == -4 and b"r3d_finalize" in lib.r3d_last_error()      # R3D_ERR_STATE: the arguments were fine
        # r3d_input_workspace_bytes: 0 and a message
        for h_pos, h_trj, bad in ((h3, None, _inp(mode, None, 9, None, 16)), (h2p, h2t, _inp(mode, None, 9, None, 8)),
                                  (h2p, None, _inp(mode, None, 0, None, 0))):
            assert lib.r3d_input_workspace_bytes(h_pos.ptr, h_trj.ptr if h_trj else None, C.byref(bad), 64) == 0
            assert lib.r3d_last_error()
            with pytest.raises(_capi.Ray3DHipError):
                _capi.input_workspace_bytes(h_pos, h_trj, bad, 64)
        assert name in lib.r3d_last_error() or b"window_stride" in lib.r3d_last_error()
    # the existing modes judge a 2-feature handle as before
    assert lib.r3d_input_workspace_bytes(h2p.ptr, None, C.byref(_inp(_capi.R3D_INPUT_UV_DIST, None, 9, None, 16)), 8) == 0
    assert b"R3D_INPUT_UV_DIST needs in_features == 3" in lib.r3d_last_error()
    assert lib.r3d_input_workspace_bytes(h2p.ptr, None, C.byref(_inp(5, None, 9, None, 16)), 8) == 0
    assert b"bad input mode 5" in lib.r3d_last_error()
    for h in (h3, h2p, h2t):
        h.close()


def test_px_mode_workspace_bytes():
    """r3d_workspace_bytes plus the pre-pass's buffer of 2 floats per point: one point per input frame (one camera, or windows
    that do not overlap), the materialised (B, RF, J, 2) windows otherwise; monotonic in B."""
    mc2 = default_model_config(ARCHITECTURE="3,3,3", INPUT_DIM=2, CAMERA_EMBDDING=False)
    hp, ht = _capi.Handle(config_from_dicts(mc2, "pos")), _capi.Handle(config_from_dicts(mc2, "trj"))
    rf, J = 27, 17
    for pair in ((hp, ht), (hp, None), (None, ht)):
        for mode in (_capi.R3D_INPUT_PX_INTRINSIC, _capi.R3D_INPUT_PX_SCREEN):
            prev = {}
            for B in (1, 2, 5, 22, 48, 49, 64, 255, 1024, 4096):
                base = _capi.workspace_bytes(pair[0], pair[1], B)
                for ws, cs, frames in ((rf, 0, B * rf), (1, 0, B + rf - 1), (rf + 3, 16, (B - 1) * (rf + 3) + rf),
                                       (rf, 16, B * rf), (1, 16, B * rf), (5, 16, B * rf), (rf, 20, B * rf)):
                    n = _capi.input_workspace_bytes(pair[0], pair[1], _inp(mode, None, ws, None, cs), B)
                    assert base + frames * J * 2 * 4 <= n <= base + frames * J * 2 * 4 + 512, (B, ws, cs, n, base)
                    assert n >= prev.get((ws, cs), 0)
                    prev[(ws, cs)] = n
    hp.close()
    ht.close()


def test_forward_uv_encoding_keyword_is_checked_before_the_device():
    mc2 = default_model_config(ARCHITECTURE="3,3", INPUT_DIM=2, CAMERA_EMBDDING=False)
    fac = ray3d_amd.Model(mc2, {}, is_train=False)
    lifter2 = ray3d_amd.Ray3DLifter(fac.get_pos_model(), fac.get_trj_model()).eval()
    fac3 = ray3d_amd.Model(default_model_config(ARCHITECTURE="3,3"), {}, is_train=False)
    lifter3 = ray3d_amd.Ray3DLifter(fac3.get_pos_model(), fac3.get_trj_model()).eval()
    uv = torch.zeros((2, 9, 17, 2))
    rows = torch.zeros((2, 16), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="INPUT_DIM == 3"):
        lifter2.forward_uv(uv, rows)                                  # a 2-feature pair needs the keyword
    with pytest.raises(RuntimeError, match="'intrinsic' or 'screen'"):
        lifter2.forward_uv(uv, rows, encoding="ray")
    with pytest.raises(RuntimeError, match="INPUT_DIM == 2"):
        lifter3.forward_uv(uv, rows, encoding="screen")
    with pytest.raises(RuntimeError, match="cam_rows"):
        lifter2.forward_uv(uv, rows[:, :8], encoding="screen")
    with pytest.raises(RuntimeError, match="res_w"):
        lifter2.forward_uv(uv, rows, encoding="screen")               # rows without a resolution: nothing is launched
    rows[:, 6:8] = 1000.0
    rows[1, 6] = 0.0
    with pytest.raises(RuntimeError, match="res_w"):
        lifter2.forward_uv(uv, rows, encoding="screen")


# ------------------------------------------------------------------ defaults

def test_defaults_reproduce_the_ray_path_exactly(tmp_path):
    """load_pose_data and evaluate_clips without the new keywords equal the calls with "ray" / "normalized" / False spelled
    out, bit for bit - and the other encodings / the camera frame are what Camera computes."""
    from ray3d_amd import dataset
    from test_host import _dataset_fixture_archives, _evalcore_clips
    zf, acts, p3, p2, table = _dataset_fixture_archives(tmp_path)
    cams = dataset.cameras_from_tables(table)
    a = dataset.load_pose_data(p3, p2, cams, ["TS1"])
    b = dataset.load_pose_data(p3, p2, cams, ["TS1"], encoding="ray", frame="normalized")
    assert len(a.clips) == len(b.clips) == len(acts)
    for i, (ca, cb) in enumerate(zip(a.clips, b.clips)):
        assert np.array_equal(ca.rays, cb.rays) and np.array_equal(ca.gt_norm, cb.gt_norm)
        assert np.array_equal(ca.rays, zf["rays/%d" % i].astype(np.float32)) and ca.frame == cb.frame == "normalized"
    table["TS1"][0].update(res_w=2048, res_h=2048)
    cams_res = dataset.cameras_from_tables(table)
    kps = [np.asarray(zf["in2d/%d" % i])[..., :2] for i in range(len(acts))]
    world = [np.asarray(zf["in3d/%d" % i]) for i in range(len(acts))]
    for enc in ("intrinsic", "screen"):
        c = dataset.load_pose_data(p3, p2, cams_res, ["TS1"], encoding=enc, frame="camera")
        cam = cams_res["TS1"][0]
        for i, clip in enumerate(c.clips):
            n = world[i].shape[0]
            want = (cam.intrinsic_from_uv if enc == "intrinsic" else cam.screen_from_uv)(kps[i][:n]).astype(np.float32)
            assert clip.rays.shape == (n, 17, 2) and np.array_equal(clip.rays, want)
            assert clip.frame == "camera" and np.array_equal(clip.gt_norm, cam.world2camera(world[i]).astype(np.float32))
    with pytest.raises(ValueError, match="resolution"):
        dataset.load_pose_data(p3, p2, cams, ["TS1"], encoding="screen")
    with pytest.raises(ValueError, match="encoding"):
        dataset.load_pose_data(p3, p2, cams, ["TS1"], encoding="uv")
    with pytest.raises(ValueError, match="frame"):
        dataset.load_pose_data(p3, p2, cams, ["TS1"], frame="world")
    # evaluate_clips / evaluate_clips_detail on a ray clip
    z, clips = _evalcore_clips()
    clips = clips[2:]                                                   # the 31-frame clip
    lift = _torch_lift_clip(default_model_config(ARCHITECTURE="3,3,3"), 27)
    kw = dict(flip=True, kps_left=list(z["kps_left"]), kps_right=list(z["kps_right"]))
    spelled = [evaluate.Clip(c.camera, c.rays, c.gt_norm, c.action, c.clip_id, frame="normalized") for c in clips]
    n0, a0, r0 = evaluate.evaluate_clips(lift, clips, 27, "cpu", **kw)
    n1, a1, r1 = evaluate.evaluate_clips(lift, spelled, 27, "cpu", root_relative=False, **kw)
    assert n0 == n1 and a0 == a1 and torch.equal(r0, r1)
    ref = z["clip2/metrics_flip1"]
    assert abs(n0["A"][0] - ref[0]) < MPJPE_MM and np.abs(np.array(n0["A"]) - ref).max() < OTHERS_MM
    d0 = evaluate.evaluate_clips_detail(lift, clips, 27, "cpu", **kw)
    d1 = evaluate.evaluate_clips_detail(lift, spelled, 27, "cpu", root_relative=False, **kw)
    assert d0[0] == d1[0] and torch.equal(d0[2], d1[2]) and torch.equal(d0[3]["rows"], d1[3]["rows"]) and torch.equal(d0[2], r0)
