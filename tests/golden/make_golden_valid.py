#!/usr/bin/env python3
"""Generate tests/golden/valid.npz by IMPORTING the reference on CPU: the validation losses of Trainer.test
(lib/train_val/trainer.py:187-223) on synthetic float32 poses, computed by the reference's own lib.loss.loss (mpjpe,
weighted_mpjpe) and lib.skeleton.bone (bone lengths and unit vectors) in the order and shapes Trainer.test uses them.

Needs a checkout of the reference (RAY3D_REFERENCE, as make_golden.py); the tests only read the .npz it writes:

    python tests/golden/make_golden_valid.py

Cases (J = 17 throughout - bone.py's matrix is the 17-joint skeleton's):
  "trj_n37"     TRAJECTORY_MODEL True, 37 frames       "trj_n1"      the same, one frame
  "notrj_abs"   no trajectory model, RAY_ENCODING True (absolute ground truth, :190-194 do nothing)
  "notrj_rel"   no trajectory model, RAY_ENCODING False (root-relative ground truth, :195-197)
Data: the ground truth is a plausible skeleton (the H36M tree, bones of 0.15 - 0.5 m, slowly turning and swaying, its root 2 - 6 m
in front of the camera), the prediction the ground truth plus N(0, 0.03 m) per coordinate, split into the pos network's
root-relative part and the trj network's root.  The script ASSERTS |root depth| in [2, 6] m and every true and predicted bone
>= 0.05 m, so that 1/z and the unit vectors are finite without help from a test.
Per case it stores: the float32 inputs; `ref/<name>`: the reference's per-clip float32 value times n (what one batch adds to
an epoch accumulator) for loss, pos, trj_logged (the (B,1) x (B,1,1) broadcast of :217-218), trj_train (the weights shaped as
in :119-120), bone_len, bone_dir; `f64/<name>`: the same expressions in float64 NumPy on the promoted inputs; and, over
all cases and figures, `ref_fp32_vs_f64_rel`: the largest relative difference between the two - the reference's own float32
error, which the tests scale their bound by.  Only numbers leave this script; no reference source text is stored.
"""
import os

import numpy as np
import torch

import make_golden as mg                      # noqa: F401  puts the reference on sys.path (cv2 stubbed)
from lib.loss.loss import mpjpe, weighted_mpjpe   # noqa: E402
from lib.skeleton.bone import get_bone_length_from_3d_pose, get_bone_unit_vector_from_3d_pose   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
NAMES = ("loss", "pos", "trj_logged", "trj_train", "bone_len", "bone_dir")


def skeleton_clip(n, seed):
    """(n, 17, 3) float64 absolute poses in the camera's normalised frame."""
    rng = np.random.default_rng(seed)
    length = rng.uniform(0.15, 0.5, 16)
    direction = rng.normal(size=(16, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    t = np.arange(n)[:, None, None]
    sway = direction + 0.2 * np.sin(0.3 * t + rng.uniform(0, 6.28, (16, 1)))
    sway /= np.linalg.norm(sway, axis=2, keepdims=True)
    root = np.array([0.3, -0.2, 4.0]) + np.stack([0.5 * np.sin(0.11 * np.arange(n)), 0.1 * np.cos(0.07 * np.arange(n)),
                                                   1.5 * np.sin(0.05 * np.arange(n) + seed)], axis=1)
    pose = np.zeros((n, 17, 3))
    pose[:, 0] = root
    for j in range(1, 17):
        pose[:, j] = pose[:, PARENTS[j]] - length[j - 1] * sway[:, j - 1]      # bone = parent - child
    return pose


def bones_of(p):
    return np.stack([p[:, PARENTS[j]] - p[:, j] for j in range(1, 17)], axis=1)


def reference_values(pos, trj, gt, gt_root_relative):
    """trainer.py:187-223 for one batch (B = n, one frame each), float32 torch: the reference's functions on copies."""
    n = pos.shape[0]
    predicted_3d_pos = torch.from_numpy(pos.copy()).reshape(n, 1, 17, 3)
    inputs_3d = torch.from_numpy(gt.copy()).reshape(n, 1, 17, 3)
    has_trj = trj is not None
    if has_trj:
        inputs_traj = inputs_3d.clone()                                            # :188
    if has_trj or gt_root_relative:
        inputs_3d[:, :, 1:] -= inputs_3d[:, :, 0:1]                                # :193 / :196
        inputs_3d[:, :, 0] = 0
    out = {"pos": n * mpjpe(predicted_3d_pos, inputs_3d).item()}                   # :200
    out["bone_len"] = n * mpjpe(get_bone_length_from_3d_pose(predicted_3d_pos), get_bone_length_from_3d_pose(inputs_3d)).item()
    out["bone_dir"] = n * mpjpe(get_bone_unit_vector_from_3d_pose(predicted_3d_pos),
                                get_bone_unit_vector_from_3d_pose(inputs_3d)).item()   # :203-209
    if has_trj:
        predicted_3d_trj = torch.from_numpy(trj.copy()).reshape(n, 1, 1, 3)
        predicted_3d_pos += predicted_3d_trj                                       # :215
        out["loss"] = n * mpjpe(predicted_3d_pos, inputs_traj).item()              # :216
        w = torch.abs(1 / inputs_traj[:, :, 0, 2])                                 # :217, shape (B, 1)
        out["trj_logged"] = n * weighted_mpjpe(predicted_3d_trj, inputs_traj[:, :, 0:1], w).item()   # :218
        w3 = torch.abs(1 / inputs_traj[:, :, 0:1][:, :, :, 2])                     # :119, shape (B, 1, 1)
        out["trj_train"] = n * weighted_mpjpe(predicted_3d_trj, inputs_traj[:, :, 0:1], w3).item()   # :120
    else:
        out["loss"] = n * mpjpe(predicted_3d_pos, inputs_3d).item()                # :220
        out["trj_logged"] = out["trj_train"] = 0.0
    return out


def float64_values(pos, trj, gt, gt_root_relative):
    """The same expressions in float64 NumPy, the float32 inputs promoted first."""
    pos, gt = pos.astype(np.float64), gt.astype(np.float64)
    n = pos.shape[0]
    norm = lambda v: np.sqrt((v ** 2).sum(axis=-1))
    g_rel = gt.copy()
    if trj is not None or gt_root_relative:
        g_rel[:, 1:] -= g_rel[:, :1]
        g_rel[:, 0] = 0
    out = {"pos": n * norm(pos - g_rel).mean()}
    bp, bg = bones_of(pos), bones_of(g_rel)
    lp, lg = norm(bp), norm(bg)
    out["bone_len"] = n * np.abs(lp - lg).mean()
    out["bone_dir"] = n * norm(bp / lp[..., None] - bg / lg[..., None]).mean()
    if trj is not None:
        t = trj.astype(np.float64)
        out["loss"] = n * norm(pos + t[:, None] - gt).mean()
        w, d = np.abs(1.0 / gt[:, 0, 2]), norm(t - gt[:, 0])
        out["trj_logged"] = n * w.mean() * d.mean()
        out["trj_train"] = n * (w * d).mean()
    else:
        out["loss"] = out["pos"]
        out["trj_logged"] = out["trj_train"] = 0.0
    return out


def main():
    torch.set_num_threads(1)
    blob, worst = {"cases": np.array(["trj_n37", "trj_n1", "notrj_abs", "notrj_rel"]), "parents": np.array(PARENTS, dtype=np.int32)}, 0.0
    for ci, (case, n, has_trj, rel) in enumerate((("trj_n37", 37, True, False), ("trj_n1", 1, True, False),
                                                  ("notrj_abs", 29, False, False), ("notrj_rel", 29, False, True))):
        rng = np.random.default_rng(100 + ci)
        gt = skeleton_clip(n, 7 + ci)
        gt_rel = gt - gt[:, :1]
        if has_trj:
            pos = (gt_rel + rng.normal(0, 0.03, gt.shape)).astype(np.float32)
            trj = (gt[:, 0] + rng.normal(0, 0.03, (n, 3))).astype(np.float32)
        else:
            pos = ((gt_rel if rel else gt) + rng.normal(0, 0.03, gt.shape)).astype(np.float32)
            trj = None
        gt = gt.astype(np.float32)
        assert np.all((np.abs(gt[:, 0, 2]) >= 2.0) & (np.abs(gt[:, 0, 2]) <= 6.0)), "root depth outside [2, 6] m"
        for name, p in (("gt", gt), ("pred", pos)):
            shortest = np.linalg.norm(bones_of(p.astype(np.float64)), axis=-1).min()
            assert shortest >= 0.05, "%s: a %s bone of %.3f m" % (case, name, shortest)
        ref, f64 = reference_values(pos, trj, gt, rel), float64_values(pos, trj, gt, rel)
        blob.update({case + "/pos": pos, case + "/gt": gt, case + "/gt_root_relative": np.array(rel)})
        if has_trj:
            blob[case + "/trj"] = trj
        for name in NAMES:
            blob["%s/ref/%s" % (case, name)] = np.float64(ref[name])
            blob["%s/f64/%s" % (case, name)] = np.float64(f64[name])
            assert np.isfinite(ref[name]) and np.isfinite(f64[name])
            if f64[name] != 0.0:
                worst = max(worst, abs(ref[name] - f64[name]) / abs(f64[name]))
        print(case, {k: (ref[k], f64[k]) for k in NAMES})
    blob["ref_fp32_vs_f64_rel"] = np.float64(worst)
    print("ref_fp32_vs_f64_rel = %.3e" % worst)
    path = os.path.join(HERE, "valid.npz")
    np.savez_compressed(path, **blob)
    print("valid.npz: %d arrays, %d bytes" % (len(blob), os.path.getsize(path)))


if __name__ == "__main__":
    main()
