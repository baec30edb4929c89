"""Pose-error metrics of the evaluation loop, in torch (float64, any device).

Counterparts of lib/loss/loss.py: mpjpe (:12-18), n_mpjpe (:72-82), p_mpjpe (:30-69, NumPy SVD in
the reference, batched torch.linalg.svd here so it can stay on the GPU), mean_velocity_error
(:95-104).  All take (..., J, 3) tensors and return a 0-d tensor.  clip_detail restates what r3d_clip_metrics_detail
keeps of them: per-frame terms, per-joint sums and PCK counts.
clip_valid restates r3d_clip_valid_losses: the validation losses of Trainer.test (mpjpe, weighted_mpjpe :21-27, and the
bone terms of lib/skeleton/bone.py) in the reference's float32 / float64 rounding.

HOST-SIDE ONLY: the product path computes these on the device in float64 (r3d_clip_metrics, csrc/r3d_metrics.hip), which
is what `evaluate.clip_partials` / `evaluate.clip_detail` call for every CUDA tensor.  This module serves CPU tensors - the host-logic tests that
drive the evaluation loop with a stand-in lifter (tests/test_host.py) and callers without a GPU tensor in hand; it is
never a fallback for the HIP kernels.
"""
from __future__ import annotations

import torch


def mpjpe(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    assert pred.shape == target.shape
    return torch.linalg.vector_norm(pred - target, dim=-1).mean()


def n_mpjpe(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Scale-aligned MPJPE; per-frame scale = <target,pred> / <pred,pred> over joints."""
    assert pred.shape == target.shape
    num = (target * pred).sum(dim=-1, keepdim=True).mean(dim=-2, keepdim=True)
    den = (pred * pred).sum(dim=-1, keepdim=True).mean(dim=-2, keepdim=True)
    return mpjpe(num / den * pred, target)


def procrustes_distances(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(N, J) per-joint distances after the per-frame similarity (Procrustes) fit of pred onto target."""
    assert pred.shape == target.shape
    pred = pred.reshape(-1, pred.shape[-2], 3)
    target = target.reshape(-1, target.shape[-2], 3)
    mu_t, mu_p = target.mean(dim=1, keepdim=True), pred.mean(dim=1, keepdim=True)
    t0, p0 = target - mu_t, pred - mu_p
    nt = torch.sqrt((t0 ** 2).sum(dim=(1, 2), keepdim=True))
    np_ = torch.sqrt((p0 ** 2).sum(dim=(1, 2), keepdim=True))
    t0, p0 = t0 / nt, p0 / np_
    H = t0.transpose(1, 2) @ p0
    U, s, Vt = torch.linalg.svd(H)
    V = Vt.transpose(1, 2)
    R = V @ U.transpose(1, 2)
    sign = torch.sign(torch.linalg.det(R)).unsqueeze(1)      # undo reflections
    V = torch.cat([V[:, :, :-1], V[:, :, -1:] * sign.unsqueeze(2)], dim=2)
    s = torch.cat([s[:, :-1], s[:, -1:] * sign], dim=1)
    R = V @ U.transpose(1, 2)
    a = s.sum(dim=1, keepdim=True).unsqueeze(2) * nt / np_
    t = mu_t - a * (mu_p @ R)
    return torch.linalg.vector_norm(a * (pred @ R) + t - target, dim=-1)


def p_mpjpe(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Procrustes-aligned MPJPE (similarity transform per frame)."""
    return procrustes_distances(pred, target).mean()


def mean_velocity_error(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Mean norm of the first temporal difference of the error; frames along dim 0."""
    assert pred.shape == target.shape
    if pred.shape[0] < 2:
        return torch.full((), float("nan"), dtype=pred.dtype, device=pred.device)
    return torch.linalg.vector_norm(torch.diff(pred, dim=0) - torch.diff(target, dim=0), dim=-1).mean()


# ---- per-joint, per-frame and PCK detail (the host restatement of r3d_clip_metrics_detail; the project's own definition -
# the reference computes the five clip means only)

DETAIL_THRESHOLDS = 31          # t_k = 0.005 * k metres, k = 0..30: 0, 5, ..., 150 mm
DETAIL_JOINT_ROWS = 3           # raw, after the Procrustes fit, root-relative
DETAIL_MAX_JOINTS = 17
DETAIL_DOUBLES = DETAIL_JOINT_ROWS * DETAIL_MAX_JOINTS + DETAIL_THRESHOLDS


def clip_detail(pred: torch.Tensor, target: torch.Tensor):
    """(N, J, 3) float64 world-frame poses of one clip -> (detail (DETAIL_DOUBLES,), frames (N, 5)), float64:

    * detail[r * 17 + j], r = 0, 1, 2: the sum over frames of joint j's distance |pred_j - gt_j|, of its distance after the
      frame's Procrustes fit and of its root-relative distance |(pred_j - pred_0) - (gt_j - gt_0)|; columns j >= J are 0;
    * detail[51 + k]: the number of (frame, joint >= 1) pairs whose root-relative distance is strictly below 0.005 * k m
      (so detail[51] is 0; the root joint, whose distance is 0 by construction, is left to the caller);
    * frames[f]: the frame's MPJPE, P-MPJPE, N-MPJPE, first-difference error against frame f + 1 (0.0 in the last row) and
      root-joint error - the terms the five clip sums add up."""
    assert pred.shape == target.shape and pred.dim() == 3 and pred.shape[-1] == 3
    n, J = pred.shape[0], pred.shape[1]
    assert 1 <= J <= DETAIL_MAX_JOINTS
    pred, target = pred.to(torch.float64), target.to(torch.float64)
    raw = torch.linalg.vector_norm(pred - target, dim=-1)
    fit = procrustes_distances(pred, target)
    rel = torch.linalg.vector_norm((pred - pred[:, :1]) - (target - target[:, :1]), dim=-1)
    num = (target * pred).sum(dim=-1, keepdim=True).mean(dim=-2, keepdim=True)
    den = (pred * pred).sum(dim=-1, keepdim=True).mean(dim=-2, keepdim=True)
    frames = torch.zeros((n, 5), dtype=torch.float64, device=pred.device)
    frames[:, 0] = raw.mean(dim=1)
    frames[:, 1] = fit.mean(dim=1)
    frames[:, 2] = torch.linalg.vector_norm(num / den * pred - target, dim=-1).mean(dim=1)
    if n > 1:
        frames[:-1, 3] = torch.linalg.vector_norm(torch.diff(pred, dim=0) - torch.diff(target, dim=0), dim=-1).mean(dim=1)
    frames[:, 4] = raw[:, 0]
    detail = torch.zeros(DETAIL_DOUBLES, dtype=torch.float64, device=pred.device)
    for r, d in enumerate((raw, fit, rel)):
        detail[r * DETAIL_MAX_JOINTS: r * DETAIL_MAX_JOINTS + J] = d.sum(dim=0)
    thr = torch.tensor([0.005 * k for k in range(DETAIL_THRESHOLDS)], dtype=torch.float64, device=pred.device)
    detail[DETAIL_JOINT_ROWS * DETAIL_MAX_JOINTS:] = (rel[:, 1:, None] < thr).sum(dim=(0, 1)).to(torch.float64)
    return detail, frames


# ---- validation losses (the host restatement of r3d_clip_valid_losses: Trainer.test, lib/train_val/trainer.py:187-223)

VALID_COUNT, VALID_MAX_BONES, VALID_BONE_ROWS = 7, 16, 4
VALID_DOUBLES = VALID_COUNT + VALID_BONE_ROWS * VALID_MAX_BONES


def clip_valid(pos: torch.Tensor, trj, gt: torch.Tensor, parents=None, pos_is_sum: bool = False,
               gt_root_relative: bool = False):
    """pos (N, J, 3), trj (N, 3) or None, gt (N, J, 3), float32 -> (row (VALID_DOUBLES,), frames (N, VALID_COUNT)), float64,
    by the rounding contract of include/ray3d_hip.h: the reference's sums and differences in float32 (one rounding each),
    everything from the norms on in float64.  Row layout: loss, pos, trj_w, trj_wsum, trj_dsum, bone_len, bone_dir, then
    four rows of 16 per-bone sums (|len_p - len_g|, len_p, len_p^2, len_g).  The inputs are not modified."""
    assert pos.shape == gt.shape and pos.dim() == 3 and pos.shape[-1] == 3
    assert not (pos_is_sum and trj is None) and not (gt_root_relative and trj is not None)
    n, J = pos.shape[0], pos.shape[1]
    pos, gt = pos.to(torch.float32), gt.to(torch.float32)
    f64 = torch.float64

    def norm(v):                                  # float32 difference in, float64 norm out
        return torch.sqrt((v.to(f64) ** 2).sum(dim=-1))

    def rel(g):                                   # trainer.py:193-194
        out = g - g[:, :1]
        out[:, 0] = 0
        return out

    frames = torch.zeros((n, VALID_COUNT), dtype=f64, device=pos.device)
    if trj is not None:
        t = trj.to(torch.float32).reshape(n, 1, 3)
        p_abs = pos if pos_is_sum else pos + t
        p_rel = pos - t if pos_is_sum else pos
        g_rel = rel(gt)
        frames[:, 0] = norm(p_abs - gt).mean(dim=1)
        frames[:, 1] = norm(p_rel - g_rel).mean(dim=1)
        w = torch.abs(1.0 / gt[:, 0, 2].to(f64))
        d = norm(t[:, 0] - gt[:, 0])
        frames[:, 2], frames[:, 3], frames[:, 4] = w * d, w, d
    else:
        p_rel = pos
        g_rel = rel(gt) if gt_root_relative else gt
        frames[:, 0] = norm(pos - g_rel).mean(dim=1)
        frames[:, 1] = frames[:, 0]
    row = torch.zeros(VALID_DOUBLES, dtype=f64, device=pos.device)
    if parents is not None:
        par = [int(v) for v in parents[1:J]]
        child = list(range(1, J))
        bp, bg = p_rel[:, par] - p_rel[:, child], g_rel[:, par] - g_rel[:, child]       # float32, parent minus child
        lp, lg = norm(bp), norm(bg)
        frames[:, 5] = torch.abs(lp - lg).mean(dim=1)
        frames[:, 6] = torch.sqrt(((bp.to(f64) / lp[..., None] - bg.to(f64) / lg[..., None]) ** 2).sum(dim=-1)).mean(dim=1)
        for r, v in enumerate((torch.abs(lp - lg), lp, lp * lp, lg)):
            row[VALID_COUNT + r * VALID_MAX_BONES: VALID_COUNT + r * VALID_MAX_BONES + J - 1] = v.sum(dim=0)
    row[:VALID_COUNT] = frames.sum(dim=0)
    return row, frames
