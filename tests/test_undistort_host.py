"""CPU suite: R3D_INPUT_UV_DIST without a GPU - the pre-pass's own per-keypoint routine run on the host through the hooks
build (r3d_debug_undistort_host), the 16-double camera row, and r3d_input_workspace_bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, hooks_library

import ray3d_amd
from ray3d_amd import _capi
from ray3d_amd.spec import config_from_dicts, default_model_config


def _undistort_host(row16, uv):
    """r3d_debug_undistort_host: (undistorted pixels (n, 2), float64 rays (n, 3))."""
    lib = hooks_library()
    row16 = np.ascontiguousarray(row16, dtype=np.float64)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    out_uv = np.empty_like(uv)
    out_rays = np.empty((uv.shape[0], 3), dtype=np.float64)
    rc = lib.r3d_debug_undistort_host(row16.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p), uv.shape[0],
                                      out_uv.ctypes.data_as(C.c_void_p), out_rays.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.r3d_last_error()
    return out_uv, out_rays


def _h36m_cameras():
    """The four H36M cameras of cameras.npz (S9, the intrinsics of undistort.npz's four coefficient sets) with their
    distortion: (product camera built undistort=True, oracle camera, K, dist)."""
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    u = np.load(os.path.join(GOLDEN, "undistort.npz"))
    out = []
    for i in range(int(u["n"])):
        t = "h36m_S9_%d" % i
        K, dist = u["cam%d/K" % i], u["cam%d/dist" % i]
        assert np.array_equal(z[t + "/K"], K)
        out.append((ray3d_amd.Camera(K, z[t + "/R"], z[t + "/t"], dist_coeff=dist, undistort=True),
                    oracle.Camera(K, z[t + "/R"], z[t + "/t"]), K, dist))
    return out


def test_cam_row_with_distortion_is_the_uv_row_and_the_coefficients():
    cam, _, K, dist = _h36m_cameras()[0]
    row = cam.cam_row(distortion=True)
    assert row.shape == (16,) and row.dtype == np.float64
    assert np.array_equal(row[:8], cam.cam_row()) and cam.cam_row().shape == (8,)
    assert np.array_equal(row[8:13], dist) and not row[13:].any()
    # no dist_coeff, or undistort=False: the coefficients are zero ("no undistortion")
    for plain in (ray3d_amd.Camera(K, cam.Rw2c, cam.Tw2c), ray3d_amd.Camera(K, cam.Rw2c, cam.Tw2c, dist_coeff=dist)):
        r = plain.cam_row(distortion=True)
        assert np.array_equal(r[:8], plain.cam_row()) and not r[8:].any()


def test_host_routine_reproduces_the_five_iteration_grid_and_the_oracle_rays():
    """The kernel's per-point routine, on the host: undistort.npz's dense 65 x 65 grid (corners included) for the four H36M
    coefficient sets, point by point the fixture generator's five iterations; its rays those of the oracle chain
    (oracle.undistort_points -> oracle rays) and of the product's host chain (Camera.rays_from_uv, undistort=True)."""
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "undistort.npz"))
    for i, (cam, ocam, K, dist) in enumerate(_h36m_cameras()):
        distorted, und5 = z["cam%d/dense_distorted" % i], z["cam%d/dense_und5" % i]
        got_uv, got_rays = _undistort_host(cam.cam_row(distortion=True), distorted)
        assert np.abs(got_uv - und5).max() <= 1e-9, (i, np.abs(got_uv - und5).max())
        want = ocam.rays_from_uv(oracle.undistort_points(K, dist, distorted))
        assert np.abs(got_rays - want).max() <= 1e-12, (i, np.abs(got_rays - want).max())
        assert np.abs(got_rays - cam.rays_from_uv(distorted)).max() <= 1e-12
        assert np.abs(got_uv - distorted).max() > 20.0          # (a distortion of tens of pixels at the corners)


def test_host_routine_with_zero_coefficients_is_the_plain_encoding():
    z = np.load(os.path.join(GOLDEN, "undistort.npz"))
    cam, ocam, K, _ = _h36m_cameras()[2]
    plain = ray3d_amd.Camera(K, cam.Rw2c, cam.Tw2c)
    uv = z["cam2/dense_distorted"]
    got_uv, got_rays = _undistort_host(plain.cam_row(distortion=True), uv)
    assert np.array_equal(got_uv, uv)                           # the pixels unchanged, bit for bit
    assert np.abs(got_rays - plain.rays_from_uv(uv)).max() <= 1e-12
    assert np.abs(got_rays - ocam.rays_from_uv(uv)).max() <= 1e-12


def test_host_routine_rejects_bad_arguments():
    lib = hooks_library()
    assert lib.r3d_debug_undistort_host(None, None, 0, None, None) == _capi.R3D_ERR_ARG


def _inp(mode, window_stride, cam_stride):
    return _capi.make_input(mode, None, window_stride, None, 2, None, cam_stride)


def test_input_workspace_bytes():
    """RAYS / UV: exactly r3d_workspace_bytes.  UV_DIST: at least the ray buffer more - one ray per input frame (one camera,
    or windows that do not overlap), the materialised (B, RF, J, 3) windows otherwise - and monotonic in B.  Bad mode and a
    cam_stride of 8 (an R3D_INPUT_UV row) give 0."""
    for arch, J in (("3,3,3", 17), ("3,3,3,3,3", 17), ("3,3", 14)):
        mc = default_model_config(ARCHITECTURE=arch, NUM_KPTS=J)
        hp, ht = _capi.Handle(config_from_dicts(mc, "pos")), _capi.Handle(config_from_dicts(mc, "trj"))
        rf = 3 ** len(arch.split(","))
        lib = _capi.load()
        for pair in ((hp, ht), (hp, None), (None, ht)):
            prev = {}
            for B in list(range(1, 70)) + [255, 256, 1000, 1024, 1025, 4096]:
                base = _capi.workspace_bytes(pair[0], pair[1], B)
                for mode in (_capi.R3D_INPUT_RAYS, _capi.R3D_INPUT_UV):
                    for ws, cs in ((rf, 0), (1, 8), (rf, 8)):
                        assert _capi.input_workspace_bytes(pair[0], pair[1], _inp(mode, ws, cs), B) == base
                for ws, cs, frames in ((rf, 0, B * rf), (1, 0, B + rf - 1), (rf + 3, 16, (B - 1) * (rf + 3) + rf),
                                       (rf, 16, B * rf), (1, 16, B * rf), (5, 16, B * rf), (rf, 20, B * rf)):
                    n = _capi.input_workspace_bytes(pair[0], pair[1], _inp(_capi.R3D_INPUT_UV_DIST, ws, cs), B)
                    assert n >= base + frames * J * 3 * 4, (arch, B, ws, cs, n, base)
                    assert n <= base + frames * J * 3 * 4 + 512
                    assert n >= prev.get((ws, cs), 0), (arch, B, ws, cs)
                    prev[(ws, cs)] = n
            for bad in (_inp(3, rf, 0), _inp(-1, rf, 0), _inp(_capi.R3D_INPUT_UV_DIST, rf, 8),
                        _inp(_capi.R3D_INPUT_UV_DIST, 1, 8), _inp(_capi.R3D_INPUT_UV_DIST, 0, 0)):
                assert lib.r3d_input_workspace_bytes(pair[0].ptr if pair[0] else None, pair[1].ptr if pair[1] else None,
                                                     C.byref(bad), 64) == 0
                assert lib.r3d_last_error()
                with pytest.raises(_capi.Ray3DHipError):
                    _capi.input_workspace_bytes(pair[0], pair[1], bad, 64)
        assert lib.r3d_input_workspace_bytes(hp.ptr, ht.ptr, None, 64) == 0
        assert lib.r3d_input_workspace_bytes(hp.ptr, ht.ptr, C.byref(_inp(0, rf, 0)), 0) == 0
        hp.close()
        ht.close()
    # a model of INPUT_DIM 2 has no ray encoding to undistort into
    mc2 = default_model_config(ARCHITECTURE="3,3", INPUT_DIM=2)
    h2 = _capi.Handle(config_from_dicts(mc2, "pos"))
    assert _capi.input_workspace_bytes(h2, None, _inp(_capi.R3D_INPUT_RAYS, 9, 0), 8) == _capi.workspace_bytes(h2, None, 8)
    assert _capi.load().r3d_input_workspace_bytes(h2.ptr, None, C.byref(_inp(_capi.R3D_INPUT_UV_DIST, 9, 0)), 8) == 0
    h2.close()
