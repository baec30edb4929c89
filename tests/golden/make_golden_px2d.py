#!/usr/bin/env python3
"""Generate tests/golden/px2d.npz by IMPORTING the reference on CPU: the inputs and the evaluation of the 2-feature
(cfg_rie_*) configurations - INPUT_DIM 2, RAY_ENCODING False, CAMERA_EMBDDING False.

Needs a checkout of the reference (RAY3D_REFERENCE, as make_golden.py); the tests only read the .npz it writes:

    python tests/golden/make_golden_px2d.py

What is pinned:
  (a) enc/<cam>/...: for H36M S9 camera 0 (1000 x 1002) and the first MPI-INF-3DHP camera (2048 x 2048), both
      undistort=False, ~200 float64 pixel pairs - the principal point, the image corners, points outside the image, the
      rest spread over the image - with normalize_screen_coordinates(X, w, h) and encode_uv_with_intrinsic(X) of them.
  (b) eval/<case>/metrics_flip{0,1}: Trainer.evaluate_core's five metrics on the cfg-1-shaped synthetic clip (100 frames,
      RF 27, J 17; pixels rounded to float32 first, so that a float32 pixel tensor holds exactly what the reference saw)
      for  "screen_trj"    TRAJECTORY_MODEL True  (camera2world branch, trainer.py:361-362),
           "screen_notrj"  TRAJECTORY_MODEL False (root-relative branch, :315-320, :382-384),
           "intrinsic_trj" the INTRINSIC_ENCODING variant of the first,
      with the clip's pixels, camera and camera-frame ground truth.
Only numbers leave this script; no reference source text is stored.  Weights come from ray3d_amd.synth's seeded generator.
"""
import os

import numpy as np

import make_golden as mg                      # puts the reference on sys.path (cv2 stubbed), imports Trainer & co.
from make_golden import CameraInfoPacket, RefModel, Trainer, UnchunkedGenerator, config_from_dicts, default_model_config, synth
from lib.camera.camera import normalize_screen_coordinates   # noqa: E402
from lib.dataset.h36m_dataset import h36m_cameras_extrinsic_params, h36m_cameras_intrinsic_params   # noqa: E402
from lib.dataset.mpii_3dhp_dataset import camera_params as dhp_camera_params   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = lambda v: np.array(v, dtype="float32")


def _table_camera(cam):
    """K, R, t, res_w, res_h of one table entry (intrinsic keys merged in), numbers through float32 as the loaders do."""
    fl, ce = f32(cam["focal_length"]), f32(cam["center"])
    K = np.eye(3, dtype=np.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fl[0], fl[1], ce[0], ce[1]
    return K, f32(cam["R"]), cam["res_w"], cam["res_h"]


def cameras():
    h = dict(h36m_cameras_extrinsic_params["S9"][0])
    h.update(h36m_cameras_intrinsic_params[0])
    K, R, w, hh = _table_camera(h)
    out = [("h36m_S9_0", K, R, np.array(f32(h["translation"]) / 1000, dtype=np.float64).reshape(3, 1), w, hh)]
    d = dhp_camera_params["S1_Seq1_0"][0]
    K, R, w, hh = _table_camera(d)
    out.append(("3dhp_S1_Seq1_0", K, R, np.array(f32(d["translation"]), dtype=np.float64).reshape(3, 1), w, hh))
    return out


def packet(K, R, t, w, h):
    return CameraInfoPacket(P=None, K=K, R=R, t=t, res_w=w, res_h=h, azimuth=0, dist_coeff=None, undistort=False)


def gen_encodings(blob):
    tags = []
    for tag, K, R, t, w, h in cameras():
        cam = packet(K, R, t, w, h)
        fixed = np.array([[K[0, 2], K[1, 2]], [0.0, 0.0], [w, 0.0], [0.0, h], [w, h], [w - 1.0, h - 1.0],
                          [-37.25, 0.1 * h], [1.3 * w, -12.5], [0.5 * w, 1.2 * h], [-0.1 * w, -0.1 * h], [2.0 * w, 2.0 * h],
                          [1.0 / 3.0, 2.0 / 3.0]], dtype=np.float64)
        spread = synth.hash_uniform("px2d." + tag, (200 - len(fixed), 2), 13) * np.array([w, h], dtype=np.float64)
        X = np.concatenate([fixed, spread], axis=0)
        assert X.dtype == np.float64 and X.shape == (200, 2)
        screen = normalize_screen_coordinates(X.copy(), w=w, h=h)
        intrinsic = cam.encode_uv_with_intrinsic(X.copy().reshape(-1, 1, 2)).reshape(-1, 2)
        assert screen.dtype == np.float64 and intrinsic.dtype == np.float64
        tags.append(tag)
        blob.update({"enc/%s/K" % tag: K, "enc/%s/R" % tag: R.astype(np.float64), "enc/%s/t" % tag: t,
                     "enc/%s/res" % tag: np.array([w, h], dtype=np.float64), "enc/%s/X" % tag: X,
                     "enc/%s/screen" % tag: screen, "enc/%s/intrinsic" % tag: intrinsic})
    blob["enc/tags"] = np.array(tags)


def gen_eval(blob):
    tag, K, R, t, w, h = cameras()[0]
    cam = packet(K, R, t, w, h)
    n = 100
    Xw, uv, _, _ = mg.synth_clip(tag, n, cam, 11)
    uv = uv.astype(np.float32).astype(np.float64)            # what a float32 pixel tensor holds, exactly
    gt_cam = cam.world2camera(Xw).astype(np.float32)         # lib/dataset/__init__.py:79-94
    inputs = {"screen": normalize_screen_coordinates(uv.copy(), w=w, h=h).astype(np.float32),
              "intrinsic": cam.encode_uv_with_intrinsic(uv.copy()).astype(np.float32)}
    kps_left, kps_right = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
    blob.update({"eval/K": K, "eval/R": R.astype(np.float64), "eval/t": t, "eval/res": np.array([w, h], dtype=np.float64),
                 "eval/uv": uv.astype(np.float32), "eval/gt_cam": gt_cam, "eval/Xw": Xw,
                 "eval/kps_left": np.array(kps_left), "eval/kps_right": np.array(kps_right)})
    for case, enc, with_trj in (("screen_trj", "screen", True), ("screen_notrj", "screen", False), ("intrinsic_trj", "intrinsic", True)):
        mc = default_model_config(ARCHITECTURE="3,3,3", INPUT_DIM=2, CAMERA_EMBDDING=False, TRAJECTORY_MODEL=with_trj)
        ref = RefModel(mc, {}, is_train=False)
        pos, trj = ref.get_pos_model(), ref.get_trj_model()
        cpos = config_from_dicts(mc, "pos")
        mg.load_synth(pos, cpos, 1, 1.0)
        if with_trj:
            mg.load_synth(trj, config_from_dicts(mc, "trj"), 2, 1.0)
        else:
            assert trj is None
        data_config = {"RAY_ENCODING": False, "INTRINSIC_ENCODING": enc == "intrinsic"}
        tr = Trainer(data_config, mc, {"LEARNING_RATE": 1e-3}, {}, None, None,
                     {"train_pos": pos, "test_pos": pos, "train_trj": trj, "test_trj": trj},
                     None, kps_left, kps_right, kps_left, kps_right, None)
        pad = (cpos.receptive_field - 1) // 2
        for flip in (False, True):
            gen = UnchunkedGenerator([cam], [gt_cam.copy()], [inputs[enc].copy()], pad=pad, causal_shift=0, kps_left=kps_left,
                                     kps_right=kps_right, joints_left=kps_left, joints_right=kps_right)
            e = np.array(tr.evaluate_core(gen, flip_test=flip), dtype=np.float64)
            blob["eval/%s/metrics_flip%d" % (case, int(flip))] = e
            print("evaluate_core %s flip=%s ->" % (case, flip), e)


if __name__ == "__main__":
    blob = {}
    gen_encodings(blob)
    gen_eval(blob)
    path = os.path.join(HERE, "px2d.npz")
    np.savez_compressed(path, **blob)
    print("px2d.npz: %d arrays, %d bytes" % (len(blob), os.path.getsize(path)))
