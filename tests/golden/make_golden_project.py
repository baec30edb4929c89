#!/usr/bin/env python3
"""Generate tests/golden/project.npz by IMPORTING the reference on CPU: what one synthetic camera sweep hands to the model
and to the evaluation, per (clip, virtual camera) - the pinned side of r3d_clips_project.

Needs a checkout of the reference (RAY3D_REFERENCE, as make_golden.py); the tests only read the .npz it writes:

    python tests/golden/make_golden_project.py

What is pinned:
  world/<clip>:  two synthetic world clips, 1 and 19 frames, J = 17, float32, standing near (0, 0, 0.9) metres;
  cam/<c>/...:   three cameras of ray3d_amd.camera.camera_grid around H36M S1 camera 1 (K, R, t as the loader builds them,
                 1000 x 1000 frame as check_in_frame assumes): two that keep every keypoint in frame, a third pitched so
                 that some leave it - K, R, t, res and, for diagnosis, the reference's own P, Rw2n, Tw2n;
  ref/<clip>/<c>/...: per (clip, camera) the reference's float64 pixels (CameraInfoPacket.project on catesian2homogenous of
                 the float32 pose), get_cam_ray_given_uv, encode_uv_with_intrinsic and normalize_screen_coordinates of
                 them, world2normalized and world2camera of the pose, check_in_frame's verdict and the number of
                 keypoints outside the frame.
The script asserts that no pixel lies within 1e-6 px of a frame border, so that a last-bit difference cannot flip a verdict.
Only numbers leave this script; no reference source text is stored.
"""
import os
import sys
import types

import numpy as np

import make_golden as mg                      # puts the reference on sys.path (cv2 stubbed)
from make_golden import CameraInfoPacket, synth
from lib.camera.camera import catesian2homogenous, normalize_screen_coordinates   # noqa: E402
from lib.dataset.h36m_dataset import h36m_cameras_extrinsic_params, h36m_cameras_intrinsic_params   # noqa: E402
from ray3d_amd.camera import camera_grid      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 5
RES = 1000.0
GRID = ((0,), (1.0,), (0, -4))                # yaw, distance ratio, pitch (degrees): everything in frame
GRID_OUT = ((0,), (0.35,), (-30,))           # closer and pitched down: some keypoints leave the frame
CLIPS = (("one", 1), ("walk", 19))
J = 17


def check_in_frame():
    """data/camera_augmentation.py's check_in_frame, imported with the script's other third-party imports stubbed."""
    for name in ("ipdb", "h5py", "mat73", "cdflib", "scipy", "scipy.linalg", "matplotlib", "matplotlib.pyplot", "tqdm"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, os.path.join(mg.REF, "data"))
    from camera_augmentation import check_in_frame as fn
    return fn


def base_camera():
    f32 = lambda v: np.array(v, dtype="float32")
    ext, intr = h36m_cameras_extrinsic_params["S1"][1], h36m_cameras_intrinsic_params[1]
    K = np.eye(3, dtype=np.float64)
    fl, ce = f32(intr["focal_length"]), f32(intr["center"])
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fl[0], fl[1], ce[0], ce[1]
    return K, f32(ext["R"]).astype(np.float64), np.array(f32(ext["translation"]) / 1000, dtype=np.float64).reshape(3, 1)


def world_clip(tag, n):
    """A standing figure's 17 points in a 0.7 x 0.7 x 1.7 m box around (0, 0, 0.9), drifting a few centimetres per frame."""
    body = (synth.hash_uniform("project.body." + tag, (1, J, 3), SEED) - 0.5) * np.array([0.7, 0.7, 1.7])
    drift = np.cumsum((synth.hash_uniform("project.drift." + tag, (n, 1, 3), SEED) - 0.5) * 0.04, axis=0)
    sway = (synth.hash_uniform("project.sway." + tag, (n, J, 3), SEED) - 0.5) * 0.02
    return (body + drift + sway + np.array([0.0, 0.0, 0.9])).astype(np.float32)


if __name__ == "__main__":
    in_frame = check_in_frame()
    K, R, t = base_camera()
    cams = camera_grid(K, R, t, GRID) + camera_grid(K, R, t, GRID_OUT)
    assert len(cams) == 3
    blob = {"clips": np.array([c for c, _ in CLIPS]), "res": np.array([RES, RES])}
    worlds = {tag: world_clip(tag, n) for tag, n in CLIPS}
    for tag, w in worlds.items():
        assert w.dtype == np.float32 and w.shape[1:] == (J, 3)
        blob["world/" + tag] = w
    blob["cam/names"] = np.array([c.name for c in cams])
    for ci, c in enumerate(cams):
        pkt = CameraInfoPacket(P=None, K=c.K, R=c.Rw2c, t=c.Tw2c, res_w=RES, res_h=RES, azimuth=0, dist_coeff=None, undistort=False)
        blob.update({"cam/%d/K" % ci: c.K, "cam/%d/R" % ci: c.Rw2c, "cam/%d/t" % ci: c.Tw2c, "cam/%d/P" % ci: pkt.P,
                     "cam/%d/Rw2n" % ci: pkt.Rw2n, "cam/%d/Tw2n" % ci: pkt.Tw2n})
        for tag, w in worlds.items():
            px = pkt.project(catesian2homogenous(w))
            assert px.dtype == np.float64 and px.shape == w.shape[:2] + (2,)
            border = np.minimum(np.abs(px), np.abs(px - RES)).min()
            assert border > 1e-6, "a pixel within 1e-6 px of the border: change SEED"
            outside = int((~((px[..., 0] >= 0) & (px[..., 0] <= RES) & (px[..., 1] >= 0) & (px[..., 1] <= RES))).sum())
            verdict = bool(in_frame(px, RES, RES))
            assert verdict == (outside == 0)
            key = "ref/%s/%d/" % (tag, ci)
            blob.update({key + "px": px, key + "ray": pkt.get_cam_ray_given_uv(px.copy()),
                         key + "intrinsic": pkt.encode_uv_with_intrinsic(px.copy()),
                         key + "screen": normalize_screen_coordinates(px.copy(), w=RES, h=RES),
                         key + "gt_norm": pkt.world2normalized(w.astype(np.float64)),
                         key + "gt_cam": pkt.world2camera(w.astype(np.float64)),
                         key + "in_frame": np.array(verdict), key + "outside": np.array(outside)})
            print("%-5s cam %d (%s): in frame %s, %d of %d points outside, nearest border %.3g px"
                  % (tag, ci, c.name, verdict, outside, px.shape[0] * J, border))
    counts = [int(blob["ref/walk/%d/outside" % ci]) for ci in range(3)]
    assert counts[0] == 0 and counts[1] == 0 and 0 < counts[2] < 19 * J, counts
    path = os.path.join(HERE, "project.npz")
    np.savez_compressed(path, **blob)
    print("project.npz: %d arrays, %d bytes" % (len(blob), os.path.getsize(path)))
