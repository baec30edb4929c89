"""Helpers of tests/test_valid_host.py and tests/test_gpu_valid.py: a NumPy oracle of r3d_clip_valid_losses' contract
(include/ray3d_hip.h: the reference's sums and differences in float32 with one rounding each, float64 from the norms on),
seeded inputs, and the ctypes calls of the host hook and the kernel."""
import ctypes as C
import functools
import os
import types

import numpy as np

from conftest import GOLDEN

COUNT, MAX_BONES, BONE_ROWS, DOUBLES = 7, 16, 4, 71
POS_IS_SUM, GT_ROOT_RELATIVE = 1, 2
H36M = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
ULP32 = 2.0 ** -23


def chain(J):
    """A valid tree for any J: every joint hangs on the one before it."""
    return tuple(range(-1, J - 1))


def tree_for(J):
    return H36M if J == 17 else chain(J)


def _norm(v32):
    v = v32.astype(np.float64)
    return np.sqrt((v * v).sum(axis=-1))


def oracle(pos, trj, gt, parents, flags):
    """float32 (n, J, 3), (n, 3) or None, (n, J, 3) -> dict(out (71,), frames (n, 7), bones (4, J-1) per-bone sums)."""
    pos, gt = np.asarray(pos, np.float32), np.asarray(gt, np.float32)
    n, J = pos.shape[:2]
    frames = np.zeros((n, COUNT))

    def rel(g):
        out = g - g[:, :1]                       # float32
        out[:, 0] = 0
        return out

    if trj is not None:
        t = np.asarray(trj, np.float32).reshape(n, 1, 3)
        p_abs = pos if flags & POS_IS_SUM else pos + t
        p_rel = pos - t if flags & POS_IS_SUM else pos
        g_rel = rel(gt)
        assert p_abs.dtype == p_rel.dtype == g_rel.dtype == np.float32
        frames[:, 0] = _norm(p_abs - gt).sum(axis=1) / J
        frames[:, 1] = _norm(p_rel - g_rel).sum(axis=1) / J
        w = np.abs(1.0 / gt[:, 0, 2].astype(np.float64))
        d = _norm(t[:, 0] - gt[:, 0])
        frames[:, 2], frames[:, 3], frames[:, 4] = w * d, w, d
    else:
        p_rel = pos
        g_rel = rel(gt) if flags & GT_ROOT_RELATIVE else gt
        frames[:, 0] = _norm(pos - g_rel).sum(axis=1) / J
        frames[:, 1] = frames[:, 0]
    out = np.zeros(DOUBLES)
    bones = np.zeros((BONE_ROWS, max(J - 1, 0)))
    if parents is not None:
        par, child = list(parents[1:J]), list(range(1, J))
        bp, bg = p_rel[:, par] - p_rel[:, child], g_rel[:, par] - g_rel[:, child]
        assert bp.dtype == bg.dtype == np.float32
        lp, lg = _norm(bp), _norm(bg)
        with np.errstate(invalid="ignore", divide="ignore"):
            frames[:, 5] = np.abs(lp - lg).sum(axis=1) / np.float64(J - 1)
            u = bp.astype(np.float64) / lp[..., None] - bg.astype(np.float64) / lg[..., None]
            frames[:, 6] = np.sqrt((u * u).sum(axis=-1)).sum(axis=1) / np.float64(J - 1)
        bones = np.stack([np.abs(lp - lg).sum(axis=0), lp.sum(axis=0), (lp * lp).sum(axis=0), lg.sum(axis=0)])
        for r in range(BONE_ROWS):
            out[COUNT + r * MAX_BONES: COUNT + r * MAX_BONES + J - 1] = bones[r]
    out[:COUNT] = frames.sum(axis=0)
    return dict(out=out, frames=frames, bones=bones)


@functools.lru_cache(maxsize=None)
def make_inputs(n, J, seed=0):
    """(pos, trj, gt) float32, read-only: a chain-like skeleton with bones of 0.15 - 0.5 m whose root is 2 - 6 m deep, the
    prediction 3 cm (per coordinate) off; pos is root-relative, trj the predicted root."""
    rng = np.random.default_rng(5000 + 31 * n + J + 7919 * seed)
    tree = tree_for(J)
    gt = np.zeros((n, J, 3))
    gt[:, 0] = np.array([0.2, -0.1, 4.0]) + rng.uniform(-1, 1, (n, 3)) * np.array([1.0, 0.5, 1.9])
    for j in range(1, J):
        d = rng.normal(size=(n, 3))
        gt[:, j] = gt[:, tree[j]] - rng.uniform(0.15, 0.5) * d / np.linalg.norm(d, axis=1, keepdims=True)
    pos = (gt - gt[:, :1] + rng.normal(0, 0.03, gt.shape)).astype(np.float32)
    trj = (gt[:, 0] + rng.normal(0, 0.03, (n, 3))).astype(np.float32)
    gt = gt.astype(np.float32)
    for v in (pos, trj, gt):
        v.setflags(write=False)
    return pos, trj, gt


def variant_inputs(n, J, variant):
    """-> (pos, trj, gt, flags) for "trj" | "sum" (POS_IS_SUM) | "abs" (no trj, absolute gt) | "rel" (no trj, GT_ROOT_RELATIVE)."""
    pos, trj, gt = make_inputs(n, J)
    if variant == "trj":
        return pos, trj, gt, 0
    if variant == "sum":
        return pos + trj[:, None], trj, gt, POS_IS_SUM          # float32 sum, one rounding: what the forward writes
    if variant == "abs":
        return pos + trj[:, None], None, gt, 0
    assert variant == "rel"
    return pos, None, gt, GT_ROOT_RELATIVE


def _fptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def host_call(lib, pos, trj, gt, parents, flags, frames=True, n=None, J=None):
    """r3d_debug_valid_losses_host on the hooks library `lib` -> (rc, out (71,), frame (n, 7) or None)."""
    pos = np.ascontiguousarray(pos, np.float32) if pos is not None else None
    gt = np.ascontiguousarray(gt, np.float32) if gt is not None else None
    trj = np.ascontiguousarray(trj, np.float32) if trj is not None else None
    n = (pos if pos is not None else gt).shape[0] if n is None else n
    J = (pos if pos is not None else gt).shape[1] if J is None else J
    out = np.full(DOUBLES, -7.0)
    fr = np.full((max(n, 1), COUNT), -7.0) if frames else None
    par = (C.c_int32 * len(parents))(*parents) if parents is not None else None
    rc = lib.r3d_debug_valid_losses_host(_fptr(pos), _fptr(trj), _fptr(gt), n, J, par, flags, _fptr(out), _fptr(fr))
    return rc, out, fr


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / np.abs(want)
    return np.where(want == 0.0, np.where(got == 0.0, 0.0, np.inf), r)


def sums_close(got, want, tol=1e-12):
    """Sums and per-bone sums: |got - want| <= tol * |want| element by element (a zero must be a zero)."""
    return bool(np.all(rel_err(got, want) <= tol))


def frames_close(got, want, tol=1e-9):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))))


# ------------------------------------------------------------------ the reference's values (tests/golden/valid.npz)

REF_NAMES = ("loss", "pos", "trj_logged", "trj_train", "bone_len", "bone_dir")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "valid.npz"))


def golden_case(case):
    """-> (pos, trj or None, gt, flags, {name: the reference's float32 value times n})."""
    z = golden()
    trj = z[case + "/trj"] if case + "/trj" in z.files else None
    flags = GT_ROOT_RELATIVE if bool(z[case + "/gt_root_relative"]) else 0
    return z[case + "/pos"], trj, z[case + "/gt"], flags, {k: float(z["%s/ref/%s" % (case, k)]) for k in REF_NAMES}


def figures_of(out, n):
    """The six figures of the fixture from a result row."""
    return {"loss": out[0], "pos": out[1], "trj_logged": out[3] * out[4] / n, "trj_train": out[2], "bone_len": out[5], "bone_dir": out[6]}


def check_against_reference(out, n, ref):
    """Bound: 4 x the fixture's measured float32-against-float64 relative difference of the reference's own values (4:
    torch's float32 reduction order varies with the thread count), never below 4 float32 ulps of the value."""
    rel = float(golden()["ref_fp32_vs_f64_rel"])
    got = figures_of(out, n)
    for k in REF_NAMES:
        bound = max(4.0 * rel * abs(ref[k]), 4.0 * float(np.spacing(np.float32(abs(ref[k])))))
        print("%-10s got %.9g  reference %.9g  |diff| %.3e  bound %.3e" % (k, got[k], ref[k], abs(got[k] - ref[k]), bound))
        assert abs(got[k] - ref[k]) <= bound, (k, got[k], ref[k], bound)


# ------------------------------------------------------------------ clips and a stand-in lifter for validate_clips

def stub_camera():
    return types.SimpleNamespace(param=lambda: np.array([1.5, 0.1], np.float32))


def valid_clips():
    """Three clips (two actions) whose `rays` hold the stand-in lifter's answer: joint 0 the predicted root, the others the
    predicted root-relative joints."""
    from ray3d_amd import evaluate
    clips = []
    for ci, (n, action) in enumerate(((23, "A"), (9, "B"), (14, "A"))):
        pos, trj, gt = make_inputs(n, 17, seed=1 + ci)
        rays = np.array(pos)
        rays[:, 0] = trj
        clips.append(evaluate.Clip(stub_camera(), rays, np.array(gt), action, ci))
    return clips


RF = 9


def standin_lift(padded, prow):
    """(sum (N,1,17,3), trj (N,1,1,3)) from an edge-padded clip of valid_clips(): what Ray3DLifter.forward_clip(...,
    return_trj=True) returns - pos + trj and trj."""
    import torch
    pad = (RF - 1) // 2
    x = padded[pad:padded.shape[0] - pad].to(torch.float32)
    trj = x[:, :1].clone()
    pos = x.clone()
    pos[:, 0] = 0.01 * x[:, 1]
    return (pos + trj).reshape(-1, 1, 17, 3), trj.reshape(-1, 1, 1, 3)


def standin_parts(clip):
    """The stand-in lifter's (sum, trj) of one clip as float32 arrays."""
    rays = np.asarray(clip.rays, np.float32)
    trj = rays[:, 0].copy()
    pos = rays.copy()
    pos[:, 0] = np.float32(0.01) * rays[:, 1]
    return pos + trj[:, None], trj
