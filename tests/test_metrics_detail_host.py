"""CPU suite: the per-joint / per-frame / PCK detail of the clip metrics - its torch restatement (ray3d_amd.metrics.clip_detail,
the path CPU tensors take), the clip evaluation built on it and the two-rank gather - against a NumPy oracle kept here
(built on oracle/metrics_oracle.py; tests/test_gpu_metrics_detail.py checks the HIP kernel against the same oracle)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, synth_states

import ray3d_amd
from ray3d_amd import evaluate, metrics
from ray3d_amd.spec import default_model_config

THRESHOLDS = np.array([0.005 * k for k in range(31)])        # metres: 0, 5, ..., 150 mm
ROW = 17                                                      # width of a per-joint row of the detail vector


# ------------------------------------------------------------------ the oracle

def procrustes_distances(pred, target):
    """(N, J) per-joint distances after the per-frame similarity fit: oracle/metrics_oracle.py's p_mpjpe (loss.py:30-69)
    with the final mean left out; oracle_detail() pins it to that function."""
    muX, muY = target.mean(axis=1, keepdims=True), pred.mean(axis=1, keepdims=True)
    X0, Y0 = target - muX, pred - muY
    nX = np.sqrt((X0 ** 2).sum(axis=(1, 2), keepdims=True))
    nY = np.sqrt((Y0 ** 2).sum(axis=(1, 2), keepdims=True))
    X0, Y0 = X0 / nX, Y0 / nY
    U, s, Vt = np.linalg.svd(X0.transpose(0, 2, 1) @ Y0)
    V = Vt.transpose(0, 2, 1)
    sign = np.sign(np.linalg.det(V @ U.transpose(0, 2, 1)))[:, None]
    V[:, :, -1] *= sign
    s[:, -1] *= sign.flatten()
    R = V @ U.transpose(0, 2, 1)
    a = s.sum(axis=1, keepdims=True)[:, :, None] * nX / nY
    t = muX - a * (muY @ R)
    return np.linalg.norm(a * (pred @ R) + t - target, axis=-1)


def oracle_detail(pw, gw):
    """World-frame float64 (N, J, 3) poses -> dict(frames (N, 5), joints (3, J) sums over frames, counts (31,) int64,
    rel (N, J) root-relative distances)."""
    from oracle import metrics_oracle as mo
    n, J = pw.shape[:2]
    raw = np.linalg.norm(pw - gw, axis=-1)
    fit = procrustes_distances(pw, gw)
    assert abs(fit.mean() - mo.p_mpjpe(pw, gw)) <= 1e-12 * max(1.0, fit.mean())
    for f in sorted(set([0, n - 1] + [f for f in (7, 11, 13) if f < n])):
        assert abs(fit[f].mean() - mo.p_mpjpe(pw[f:f + 1], gw[f:f + 1])) <= 1e-12
    rel = np.linalg.norm((pw - pw[:, :1]) - (gw - gw[:, :1]), axis=-1)
    frames = np.zeros((n, 5))
    frames[:, 0] = raw.mean(axis=1)
    frames[:, 1] = fit.mean(axis=1)
    sc = np.mean(np.sum(gw * pw, axis=2, keepdims=True), axis=1, keepdims=True) / \
        np.mean(np.sum(pw ** 2, axis=2, keepdims=True), axis=1, keepdims=True)              # loss.py:78-80 per frame
    frames[:, 2] = np.linalg.norm(sc * pw - gw, axis=-1).mean(axis=1)
    assert abs(frames[:, 2].mean() - mo.n_mpjpe(pw[:, None], gw[:, None])) <= 1e-12
    if n > 1:
        frames[:-1, 3] = np.linalg.norm(np.diff(pw, axis=0) - np.diff(gw, axis=0), axis=-1).mean(axis=1)
        assert abs(frames[:-1, 3].mean() - mo.mean_velocity_error(pw, gw)) <= 1e-12
    frames[:, 4] = raw[:, 0]
    counts = (rel[:, 1:, None] < THRESHOLDS).sum(axis=(0, 1)).astype(np.int64)
    return dict(frames=frames, joints=np.stack([raw.sum(axis=0), fit.sum(axis=0), rel.sum(axis=0)]), counts=counts, rel=rel)


def threshold_margin(rel):
    """Smallest distance of a root-relative distance (joints >= 1) from a threshold k >= 1."""
    return float(np.abs(rel[:, 1:, None] - THRESHOLDS[1:]).min()) if rel.shape[1] > 1 else float("inf")


@functools.lru_cache(maxsize=None)
def make_case(n, J):
    """The inputs of tests/test_gpu_parity.py::test_clip_metrics_kernel_matches_oracle (seed 1000 + n + J; from 257 frames
    on with a mirrored, an exact and a planar frame), a random proper rotation and translation, and their oracle."""
    rng = np.random.default_rng(1000 + n + J)
    gt = rng.normal(0, 0.4, (n, J, 3)).astype(np.float32) + np.array([0, 0, 1.0], np.float32)
    pred = gt + rng.normal(0, 0.05, (n, J, 3)).astype(np.float32)
    if n >= 257:
        pred[7] = gt[7] * np.array([-1, 1, 1], np.float32)          # a mirrored pose: the fit must not reflect
        pred[11] = gt[11]                                            # exact prediction: zero error, no NaN
        gt[13, :, 2] = 1.0                                           # planar ground truth: rank-2 correlation
        pred[13, :, 2] = 1.0
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R, T = q * np.sign(np.linalg.det(q)), rng.normal(size=3)
    pw = pred.astype(np.float64) @ R.T + T.reshape(1, 1, 3)
    gw = gt.astype(np.float64) @ R.T + T.reshape(1, 1, 3)
    want = oracle_detail(pw, gw)
    for v in (pred, gt, R, T) + tuple(want.values()):
        v.setflags(write=False)
    return pred, gt, R, T, want


def close(got, want, tol=1e-9):
    """|got - want| <= tol * max(1, |want|), element by element."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))))


def stub_clip(pred, gt, R, T):
    cam = types.SimpleNamespace(Rn2w=np.array(R), Tn2w=np.array(T).reshape(3, 1))
    return evaluate.Clip(cam, np.zeros((gt.shape[0], gt.shape[1], 3), np.float32), np.array(gt), "A", 0)


# ------------------------------------------------------------------ clip_detail on CPU tensors

CPU_CASES = [(1, 17), (2, 17), (257, 17), (300, 14), (777, 15)]


@pytest.mark.parametrize("n,J", CPU_CASES)
def test_clip_detail_on_cpu_tensors_matches_oracle(n, J):
    pred, gt, R, T, want = make_case(n, J)
    assert threshold_margin(want["rel"]) > 1e-12
    clip = stub_clip(pred, gt, R, T)
    detail, frames = evaluate.clip_detail(torch.from_numpy(np.array(pred)).reshape(n, 1, J, 3), clip, frames=True)
    only = evaluate.clip_detail(torch.from_numpy(np.array(pred)), clip)
    assert detail.dtype == torch.float64 and detail.shape == (evaluate.DETAIL_COLS,) == (82,) and frames.shape == (n, 5)
    assert torch.equal(only, detail)
    detail, frames = detail.numpy(), frames.numpy()
    assert close(frames, want["frames"])
    joints = detail[:3 * ROW].reshape(3, ROW)
    assert close(joints[:, :J], want["joints"]) and np.all(joints[:, J:] == 0.0)
    assert np.array_equal(detail[3 * ROW:], want["counts"].astype(np.float64)) and detail[3 * ROW] == 0.0
    assert frames[-1, 3] == 0.0
    assert np.all(joints[2, 0] == 0.0)                                # the root's root-relative distance


@pytest.mark.parametrize("n,J", CPU_CASES)
def test_frame_columns_add_up_to_clip_partials(n, J):
    """The per-frame table is what the five clip sums are made of: its column sums reproduce clip_partials (the velocity
    column scaled by n / (n - 1); with one frame the velocity sum is NaN and the column 0).  Bound: both sides add the
    same n <= 777 float64 terms in another order, n * 2^-53 < 1e-13 relative."""
    pred, gt, R, T, _ = make_case(n, J)
    clip = stub_clip(pred, gt, R, T)
    p = torch.from_numpy(np.array(pred)).reshape(n, 1, J, 3)
    row = evaluate.clip_partials(p, clip).numpy()
    _, frames = evaluate.clip_detail(p, clip, frames=True)
    sums = frames.numpy().sum(axis=0)
    if n > 1:
        sums[3] *= n / (n - 1)
    else:
        assert np.isnan(row[6]) and sums[3] == 0.0
        sums[3] = row[6] = 0.0
    assert np.all(np.abs(sums - row[3:8]) <= 1e-12 * np.maximum(1.0, np.abs(row[3:8]))), (sums, row[3:8])


def test_metrics_clip_detail_on_the_reference_losses_fixture():
    """The per-frame columns average to the values the reference's lib/loss/loss.py computed (tests/golden/losses.npz)."""
    z = np.load(os.path.join(GOLDEN, "losses.npz"))
    a, b = torch.from_numpy(z["pred"]).reshape(-1, 17, 3), torch.from_numpy(z["target"]).reshape(-1, 17, 3)
    detail, frames = metrics.clip_detail(a, b)
    n = a.shape[0]
    assert abs(float(frames[:, 0].mean()) - float(z["mpjpe"])) < 1e-12
    assert abs(float(frames[:, 1].mean()) - float(z["p_mpjpe"])) < 1e-10
    assert abs(float(frames[:, 2].mean()) - float(z["n_mpjpe"])) < 1e-12
    assert abs(float(frames[:-1, 3].mean()) - float(z["mpjve"])) < 1e-12
    assert abs(float(detail[:17].sum()) / (17 * n) - float(z["mpjpe"])) < 1e-12
    assert abs(float(detail[17:34].sum()) / (17 * n) - float(z["p_mpjpe"])) < 1e-10


# ------------------------------------------------------------------ evaluate_clips_detail (oracle as the lifter)

def evalcore_clips():
    z = np.load(os.path.join(GOLDEN, "evalcore.npz"))
    clips = []
    for ci in range(3):
        cam = ray3d_amd.Camera(z["clip%d/K" % ci], z["clip%d/R" % ci], z["clip%d/t" % ci])
        clips.append(evaluate.Clip(cam, z["clip%d/rays" % ci], z["clip%d/gt_norm" % ci], action="B" if ci == 1 else "A", clip_id=ci))
    return clips


@functools.lru_cache(maxsize=None)
def oracle_lift_clip():
    """CPU stand-in for Ray3DLifter.forward_clip built on the C oracle (checker role only); it remembers the clips it
    has lifted, the tests here lift the same three several times."""
    from oracle import oracle
    (cp, sp), (ct, st) = synth_states(default_model_config(ARCHITECTURE="3,3,3"))
    done = {}

    def lift(padded, prow):
        pad = padded.numpy()
        key = (pad.tobytes(), prow.numpy().tobytes())
        if key not in done:
            n = pad.shape[0] - 27 + 1
            win = np.stack([pad[i:i + 27] for i in range(n)])
            par = np.tile(prow.numpy(), (n, 1))
            done[key] = oracle.forward(cp, sp, win, par) + oracle.forward(ct, st, win, par)
        return torch.from_numpy(done[key].copy())
    return lift


def near_clips(lift, clips, device="cpu"):
    """The clips with their ground truth replaced by the lifter's own poses plus 50 mm of seeded noise per coordinate: the
    synthetic weights of the fixtures lift metres away from the recorded ground truth, where every PCK is 0."""
    rng = np.random.default_rng(150)
    out = []
    for c in clips:
        with torch.no_grad():
            pred = evaluate.predict_clip(lift, c, 27, device).cpu().numpy().reshape(-1, 17, 3)
        gt = (pred + rng.normal(0, 0.05, pred.shape)).astype(np.float32)
        out.append(evaluate.Clip(c.camera, c.rays, gt, c.action, c.clip_id))
    return out


def expected_tables(lift, clips, include_root):
    """{action / "overall": table} from the oracle, clip by clip."""
    per_clip = []
    for c in clips:
        pred = evaluate.predict_clip(lift, c, 27, "cpu").numpy().reshape(-1, 17, 3)
        want = oracle_detail(c.camera.normalized2world(pred), c.camera.normalized2world(c.gt_norm))
        assert threshold_margin(want["rel"]) > 1e-12
        per_clip.append((c.action, pred.shape[0], want))
    out = {}
    for key in sorted(set(a for a, _, _ in per_clip)) + ["overall"]:
        sel = [(n, w) for a, n, w in per_clip if key in (a, "overall")]
        N = sum(n for n, _ in sel)
        joints = sum(w["joints"] for _, w in sel) / N * 1000.0
        counts = sum(w["counts"] for _, w in sel).astype(np.float64)
        if include_root:
            counts[1:] += N
        pck = counts / (N * (17 if include_root else 16)) * 100.0
        out[key] = dict(mpjpe=joints[0], p_mpjpe=joints[1], root_rel=joints[2], pck=pck, pck150=pck[-1], auc=pck.mean())
    return out


@pytest.mark.parametrize("include_root", [False, True])
def test_evaluate_clips_detail_tables_pck_and_auc(include_root):
    lift = oracle_lift_clip()
    clips = near_clips(lift, evalcore_clips())
    named, avg, rows, detail = evaluate.evaluate_clips_detail(lift, clips, 27, "cpu", include_root=include_root)
    named0, avg0, rows0 = evaluate.evaluate_clips(lift, clips, 27, "cpu")
    assert avg == avg0 and set(named) == set(named0) == {"A", "B"}
    for a in named0:
        assert np.allclose(named[a], named0[a], rtol=0, atol=1e-9)
    assert rows[:, 0].tolist() == [0.0, 1.0, 2.0] and detail["rows"].shape == (3, 82)
    assert torch.equal(rows, rows0[torch.argsort(rows0[:, 0])])
    want = expected_tables(lift, clips, include_root)
    assert set(detail) == set(want) | {"rows"}
    for key, w in want.items():
        t = detail[key]
        for name in ("mpjpe", "p_mpjpe", "root_rel"):
            assert len(t[name]) == 17 and close(t[name], w[name], 1e-9 * 1000.0), (key, name)     # millimetres
        assert t["root_rel"][0] == 0.0
        assert len(t["pck"]) == 31 and t["pck"][0] == 0.0
        assert np.allclose(t["pck"], w["pck"], rtol=0, atol=1e-12) and abs(t["pck150"] - w["pck150"]) <= 1e-12
        assert abs(t["auc"] - w["auc"]) <= 1e-12
        assert 0.0 < t["auc"] < t["pck150"] <= 100.0
        # the frame-weighted mean over joints of the per-joint table is the action's MPJPE / P-MPJPE
        if key != "overall":
            assert abs(np.mean(t["mpjpe"]) - named[key][0]) < 1e-9 and abs(np.mean(t["p_mpjpe"]) - named[key][1]) < 1e-9
    lines = evaluate.format_detail_report(detail["overall"])
    assert len(lines) == 18 and all(isinstance(s, str) for s in lines)
    assert "PCK@150mm: %.1f" % detail["overall"]["pck150"] in lines[-1] and "AUC: %.1f" % detail["overall"]["auc"] in lines[-1]
    assert evaluate.format_detail_report(detail["A"], ["j%d" % j for j in range(17)])[16].startswith("j16: MPJPE ")


def _tables_as_arrays(detail):
    return {k: {n: np.asarray(v, np.float64) for n, v in t.items()} for k, t in detail.items() if k != "rows"}


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lift = oracle_lift_clip()
        named, avg, rows, detail = evaluate.evaluate_clips_detail(lift, near_clips(lift, evalcore_clips()), 27, "cpu",
                                                                  rank=rank, world_size=world)
        q.put((rank, named, avg, rows.numpy(), detail["rows"].numpy(), _tables_as_arrays(detail)))
    finally:
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def test_two_rank_detail_gather_equals_single_process_exactly():
    """Two gloo ranks, clips sharded over them, the detail rows in their own all_gather: every rank ends with exactly the
    single-process result (clips are added up in clip-id order, whatever the sharding)."""
    import torch.multiprocessing as mp
    lift = oracle_lift_clip()
    named1, avg1, rows1, detail1 = evaluate.evaluate_clips_detail(lift, near_clips(lift, evalcore_clips()), 27, "cpu")
    assert 0.0 < detail1["overall"]["auc"] < detail1["overall"]["pck150"] < 100.0
    tables1 = _tables_as_arrays(detail1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == [0, 1]
    for rank, named, avg, rows, drows, tables in res:
        assert named == named1 and avg == avg1
        assert np.array_equal(rows, rows1.numpy()) and np.array_equal(drows, detail1["rows"].numpy())
        assert set(tables) == set(tables1)
        for key in tables1:
            for name, v in tables1[key].items():
                assert np.array_equal(tables[key][name], v), (rank, key, name)


def test_gather_partials_column_count_defaults_to_the_partial_rows():
    import inspect
    sig = inspect.signature(evaluate.gather_partials)
    assert sig.parameters["cols"].default == evaluate.PARTIAL_COLS == 8
