"""-m gpu: r3d_clip_metrics_detail - per-frame errors, per-joint sums and PCK counts from the clip-metrics kernels - against
the NumPy oracle of tests/test_metrics_detail_host.py, against the plain r3d_clip_metrics call, and end to end through
evaluate_clips_detail."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, synth_states
from test_metrics_detail_host import ROW, close, evalcore_clips, make_case, near_clips, threshold_margin

pytestmark = pytest.mark.gpu

# one frame (velocity NaN), one difference, one frame past a workgroup, 14 and 15 joints (padded joint rows), and more
# frames than the 128 x 256 of one sweep of the grid
CASES = [(1, 17), (2, 17), (257, 17), (300, 14), (777, 15), (33100, 17)]
SENTINEL = -7.0


def _run(pred, gt, R, T, frames=True, detail=True):
    """One call; every output buffer pre-filled with a sentinel.  -> (five sums, per-frame table or None, detail row)."""
    from ray3d_amd import _capi
    p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).cuda()
    n, J = p.shape[0], p.shape[1]
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((_capi.METRIC_OUT_DOUBLES,), SENTINEL, dtype=torch.float64, device="cuda")
    if not detail:
        _capi.clip_metrics(p.data_ptr(), g.data_ptr(), n, J, R, T, out.data_ptr(), stream)
        torch.cuda.synchronize()
        return out[:5].cpu().numpy(), None, None
    fr = torch.full((n, 5), SENTINEL, dtype=torch.float64, device="cuda") if frames else None
    det = torch.full((_capi.DETAIL_OUT_DOUBLES,), SENTINEL, dtype=torch.float64, device="cuda")
    _capi.clip_metrics_detail(p.data_ptr(), g.data_ptr(), n, J, R, T, out.data_ptr(), fr.data_ptr() if frames else None,
                              det.data_ptr(), stream)
    torch.cuda.synchronize()
    return out[:5].cpu().numpy(), fr.cpu().numpy() if frames else None, det[:_capi.DETAIL_DOUBLES].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gpu_case(n, J):
    pred, gt, R, T, _ = make_case(n, J)
    return _run(pred, gt, R, T)


@pytest.mark.parametrize("n,J", CASES)
def test_detail_kernel_matches_oracle(n, J):
    """Per-frame values and per-joint sums within 1e-9 * max(1, |want|) of the oracle, element by element."""
    want = make_case(n, J)[4]
    _, frames, detail = _gpu_case(n, J)
    assert np.all(np.isfinite(frames)) and np.all(np.isfinite(detail))
    worst = float(np.abs(frames - want["frames"]).max())
    joints = detail[:3 * ROW].reshape(3, ROW)
    print("n %d J %d: per-frame max abs err %.3e, per-joint sums max abs err %.3e (sums up to %.1f)"
          % (n, J, worst, np.abs(joints[:, :J] - want["joints"]).max(), want["joints"].max()))
    assert close(frames, want["frames"])
    assert frames[-1, 3] == 0.0                                       # no next frame
    assert close(joints[:, :J], want["joints"])
    assert np.all(joints[:, J:] == 0.0)                               # padding of the joint rows
    assert joints[2, 0] == 0.0                                        # the root's root-relative distance


@pytest.mark.parametrize("n,J", CASES)
def test_pck_counts_equal_the_oracle_exactly(n, J):
    want = make_case(n, J)[4]
    margin = threshold_margin(want["rel"])
    print("n %d J %d: smallest |distance - threshold| %.3e m" % (n, J, margin))
    assert margin > 1e-12                                             # no distance sits on a threshold: the counts are well defined
    counts = _gpu_case(n, J)[2][3 * ROW:]
    assert counts.shape == (31,) and counts[0] == 0.0
    assert np.array_equal(counts, want["counts"].astype(np.float64)), (counts, want["counts"])
    assert np.all(np.diff(counts) >= 0) and counts[-1] <= n * (J - 1)


@pytest.mark.parametrize("n,J", CASES)
def test_detail_call_keeps_the_five_sums_and_frames_add_up_to_them(n, J):
    pred, gt, R, T, _ = make_case(n, J)
    sums, frames, _ = _gpu_case(n, J)
    plain, _, _ = _run(pred, gt, R, T, detail=False)
    assert sums.tobytes() == plain.tobytes(), (sums, plain)          # bit for bit, the NaN of a one-frame clip included
    cols = frames.sum(axis=0)
    if n > 1:
        cols[3] *= n / (n - 1)
    else:
        assert np.isnan(sums[3]) and cols[3] == 0.0
        cols, sums = np.delete(cols, 3), np.delete(sums, 3)
    rel = np.abs(cols - sums) / np.abs(sums)
    print("n %d J %d: column sums vs the five sums, relative %s" % (n, J, rel))
    assert np.all(rel <= 1e-12), (cols, sums)


@pytest.mark.parametrize("n,J", CASES)
def test_detail_is_deterministic_and_frame_buffer_is_optional(n, J):
    pred, gt, R, T, _ = make_case(n, J)
    sums, frames, detail = _gpu_case(n, J)
    sums2, frames2, detail2 = _run(pred, gt, R, T)
    assert sums2.tobytes() == sums.tobytes() and frames2.tobytes() == frames.tobytes() and detail2.tobytes() == detail.tobytes()
    sums3, none, detail3 = _run(pred, gt, R, T, frames=False)         # frame_dev = NULL
    assert none is None and sums3.tobytes() == sums.tobytes() and detail3.tobytes() == detail.tobytes()


def test_detail_known_answers_and_errors():
    from ray3d_amd import _capi
    z = np.load(os.path.join(GOLDEN, "losses.npz"))            # values computed by the reference's lib/loss/loss.py
    a, b = z["pred"].reshape(-1, 17, 3), z["target"].reshape(-1, 17, 3)
    _, frames, detail = _run(a, b, np.eye(3), np.zeros(3))
    n = a.shape[0]
    # the fixture's inputs are float64; the kernel takes the model's float32 outputs
    assert abs(frames[:, 0].mean() - float(z["mpjpe"])) < 1e-6
    assert abs(frames[:, 1].mean() - float(z["p_mpjpe"])) < 1e-6
    assert abs(frames[:, 2].mean() - float(z["n_mpjpe"])) < 1e-6
    assert abs(detail[:17].sum() / (17 * n) - float(z["mpjpe"])) < 1e-6
    assert abs(detail[17:34].sum() / (17 * n) - float(z["p_mpjpe"])) < 1e-6
    t = torch.zeros(_capi.DETAIL_OUT_DOUBLES, dtype=torch.float64, device="cuda")
    with pytest.raises(_capi.Ray3DHipError, match="num_joints"):
        _capi.clip_metrics_detail(t.data_ptr(), t.data_ptr(), 4, 18, np.eye(3), np.zeros(3), t.data_ptr(), None, t.data_ptr(), 0)
    with pytest.raises(_capi.Ray3DHipError, match="n_frames"):
        _capi.clip_metrics_detail(t.data_ptr(), t.data_ptr(), 0, 17, np.eye(3), np.zeros(3), t.data_ptr(), None, t.data_ptr(), 0)
    with pytest.raises(_capi.Ray3DHipError, match="null pointer"):
        _capi.clip_metrics_detail(t.data_ptr(), t.data_ptr(), 4, 17, np.eye(3), np.zeros(3), t.data_ptr(), None, None, 0)


def test_evaluate_clips_detail_gpu_against_the_cpu_path():
    """Two short clips (two actions) through the RF-27 model on the GPU: forward_clip + r3d_clip_metrics_detail, against
    the same call on CPU tensors - the same lifted poses copied to the host, the torch restatement of the detail."""
    import ray3d_amd
    from ray3d_amd import evaluate
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    (_, sp), (_, st) = synth_states(mc)
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos.eval(), trj.eval()
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    # 57 frames of action B, 31 of action A; ground truth near the lifted poses, so that the PCK curve is not flat
    clips = near_clips(lifter.forward_clip, evalcore_clips()[1:], torch.device("cuda:0"))

    def lift_to_host(padded, prow):
        return lifter.forward_clip(padded.cuda(), prow.cuda()).cpu()

    with torch.no_grad():
        named, avg, rows, detail = evaluate.evaluate_clips_detail(lifter.forward_clip, clips, 27, torch.device("cuda:0"))
        named_c, avg_c, rows_c, detail_c = evaluate.evaluate_clips_detail(lift_to_host, clips, 27, "cpu")
    assert rows.is_cuda and detail["rows"].is_cuda and detail["rows"].shape == (2, 82)
    assert set(detail) == {"A", "B", "overall", "rows"}
    assert close(rows.cpu().numpy(), rows_c.numpy())
    for a in named_c:
        assert np.allclose(named[a], named_c[a], rtol=0, atol=1e-6)          # millimetres
    for key in ("A", "B", "overall"):
        t, w = detail[key], detail_c[key]
        for name in ("mpjpe", "p_mpjpe", "root_rel"):
            assert len(t[name]) == 17 and close(t[name], w[name], 1e-6), (key, name)
        assert t["pck"] == w["pck"] and t["pck150"] == w["pck150"] and t["auc"] == w["auc"]
        assert t["pck"][0] == 0.0 and 0.0 < t["auc"] < t["pck150"] <= 100.0
    assert np.array_equal(detail["rows"].cpu().numpy()[:, 3 * ROW:], detail_c["rows"].numpy()[:, 3 * ROW:])
