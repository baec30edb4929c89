#!/usr/bin/env python3
"""Generate tests/golden/streams_poses.npz by IMPORTING the reference on CPU: what the reference's own camera functions make of a
live tick's finished poses - the pinned side of r3d_streams_poses.

Needs a checkout of the reference (RAY3D_REFERENCE, as make_golden.py); the tests only read the .npz it writes:

    python tests/golden/make_golden_streams_poses.py

What is pinned, for the first three H36M cameras of cameras.npz (S9; K, R, t are read from that file, CameraInfoPacket built as
make_golden.py builds them, undistort=False):
  <tag>/pose    (12, 17, 3) float32: poses in the NORMALISED frame - world2normalized of world points N(0, 0.3^2) + [0, 0, 1] m
                (numpy RandomState, seed fixed), cast to float32, plus a float32 perturbation of up to 3 cm per component so that
                the residual is not zero;
  <tag>/ray     (12, 17, 3) float32: the keypoints that "were fed in" - get_cam_ray_given_uv of the UNPERTURBED points' projection
                (CameraInfoPacket.project), cast to float32;
  <tag>/world   (12, 17, 3) float64: normalized2world of the float32 pose promoted to float64;
  <tag>/reproj  (12, 17) float64: the undistorted pixel distance between the pixel of normalized2camera(pose) (x / z, y / z through
                decouple_uv_with_intrinsic) and get_uv_given_cam_ray(ray) - the overlay lib/train_val/trainer.py:535-537 draws;
  <tag>/zc_min  the smallest camera-frame depth of the perturbed poses (the script asserts >= 1 m).
Only numbers and camera tags leave this script; no reference source text is stored.
"""
import os

import numpy as np

import make_golden as mg                      # puts the reference on sys.path (cv2 stubbed)  # noqa: F401
from make_golden import CameraInfoPacket

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 18
TAGS = ("h36m_S9_0", "h36m_S9_1", "h36m_S9_2")
FRAMES, J = 12, 17
RES_W, RES_H = 1000, 1002


def homogeneous(X):
    return np.concatenate([X, np.ones_like(X[..., :1])], -1)


if __name__ == "__main__":
    cams = np.load(os.path.join(HERE, "cameras.npz"))
    rng = np.random.RandomState(SEED)
    blob = {"tags": np.array(TAGS)}
    for tag in TAGS:
        K, R, t = cams[tag + "/K"], cams[tag + "/R"], cams[tag + "/t"]
        pkt = CameraInfoPacket(P=None, K=K, R=R, t=t, res_w=RES_W, res_h=RES_H, azimuth=0, dist_coeff=None, undistort=False)
        Xw = 0.3 * rng.standard_normal((FRAMES, J, 3)) + np.array([0.0, 0.0, 1.0])
        bump = (0.06 * (rng.random_sample((FRAMES, J, 3)) - 0.5)).astype(np.float32)
        pose = (pkt.world2normalized(Xw).astype(np.float32) + bump).astype(np.float32)
        uv = pkt.project(homogeneous(Xw))
        ray = pkt.get_cam_ray_given_uv(uv.copy()).astype(np.float32)
        p64 = pose.astype(np.float64)
        world = pkt.normalized2world(p64)
        pc = pkt.normalized2camera(p64)
        assert pc[..., 2].min() >= 1.0, "a pose closer than 1 m to the camera: change SEED"
        predicted = pkt.decouple_uv_with_intrinsic(pc[..., :2] / pc[..., 2:])
        observed = pkt.get_uv_given_cam_ray(ray.astype(np.float64))
        reproj = np.sqrt(((predicted - observed) ** 2).sum(-1))
        assert world.dtype == np.float64 and reproj.dtype == np.float64 and reproj.shape == (FRAMES, J) and reproj.min() > 0.1
        blob.update({tag + "/pose": pose, tag + "/ray": ray, tag + "/world": world, tag + "/reproj": reproj,
                     tag + "/zc_min": np.float64(pc[..., 2].min())})
        print("%s: depth %.2f - %.2f m, residual %.2f - %.2f px (mean %.2f)" % (tag, pc[..., 2].min(), pc[..., 2].max(), reproj.min(),
                                                                                 reproj.max(), reproj.mean()))
        # how far the library's stated arithmetic (include/ray3d_hip.h, restated here) is from the reference's: DESIGN 4.18
        c, sn, h = np.cos(pkt.cam_pitch_rad), np.sin(pkt.cam_pitch_rad), float(np.ravel(pkt.cam_orig_world)[2])
        yy, z = p64[..., 1] + h, p64[..., 2]
        zc = sn * yy + c * z
        du = K[0, 0] * (p64[..., 0] / zc - ray[..., 0].astype(np.float64))
        dv = K[1, 1] * ((c * yy - sn * z) / zc - (c * ray[..., 1].astype(np.float64) - sn * ray[..., 2].astype(np.float64)))
        print("    stated arithmetic against the reference's: worst |difference| %.3g px" % np.abs(np.sqrt(du * du + dv * dv) - reproj).max())
    path = os.path.join(HERE, "streams_poses.npz")
    np.savez_compressed(path, **blob)
    print("streams_poses.npz: %d arrays, %d bytes" % (len(blob), os.path.getsize(path)))
