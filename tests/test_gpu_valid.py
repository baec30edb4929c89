"""-m gpu: r3d_clip_valid_losses - the validation losses of Trainer.test on the device - against the same per-frame routines
run on the host (r3d_debug_valid_losses_host, itself pinned to a NumPy oracle and to the reference's values by
tests/test_valid_host.py), the reference's float32 values through evaluate.clip_valid, and end to end through
validate_clips on the smallest model fixture."""
import functools

import numpy as np
import pytest
import torch

from conftest import hooks_library, load_model_fixture, synth_states
import valid_oracle as vo

pytestmark = pytest.mark.gpu

# one frame, one wavefront and its neighbours, one workgroup and its neighbours, and one frame more than the 128 x 256 a
# sweep of the capped grid takes (a thread then owns two frames)
NS = [1, 2, 63, 64, 65, 255, 256, 257, 128 * 256 + 1]
JS = [14, 15, 17]
VARIANTS = ("trj", "sum", "abs", "rel")
SENTINEL = -7.0


def _run(pos, trj, gt, parents, flags, frames=True):
    """One call on the product library, every output buffer pre-filled with a sentinel -> (out (71,), frame table or None,
    the three inputs as they are afterwards)."""
    from ray3d_amd import _capi
    _capi.use_hooks(False)
    p = torch.from_numpy(np.array(pos, dtype=np.float32)).cuda()
    g = torch.from_numpy(np.array(gt, dtype=np.float32)).cuda()
    t = torch.from_numpy(np.array(trj, dtype=np.float32)).cuda() if trj is not None else None
    n, J = p.shape[0], p.shape[1]
    out = torch.full((_capi.VALID_OUT_DOUBLES,), SENTINEL, dtype=torch.float64, device="cuda")
    fr = torch.full((n, _capi.VALID_COUNT), SENTINEL, dtype=torch.float64, device="cuda") if frames else None
    _capi.clip_valid_losses(p.data_ptr(), t.data_ptr() if t is not None else None, g.data_ptr(), n, J, parents, flags,
                            out.data_ptr(), fr.data_ptr() if frames else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    after = (p.cpu().numpy(), t.cpu().numpy() if t is not None else None, g.cpu().numpy())
    return out[:_capi.VALID_DOUBLES].cpu().numpy(), fr.cpu().numpy() if frames else None, after


@functools.lru_cache(maxsize=None)
def _host_case(n, J, variant, bones=True):
    pos, trj, gt, flags = vo.variant_inputs(n, J, variant)
    rc, out, fr = vo.host_call(hooks_library(), pos, trj, gt, vo.tree_for(J) if bones else None, flags)
    assert rc == 0
    return out, fr


@functools.lru_cache(maxsize=None)
def _gpu_case(n, J, variant, bones=True):
    pos, trj, gt, flags = vo.variant_inputs(n, J, variant)
    return _run(pos, trj, gt, vo.tree_for(J) if bones else None, flags)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("n", NS)
def test_kernel_matches_the_host_hook(n, J, variant):
    """Sums and per-bone sums within 1e-12 relative, per-frame terms within 1e-9 * max(1, |want|) - the host suite's bounds:
    the same float64 terms from the same routines, added in the kernel's tree order instead of index order."""
    want, want_fr = _host_case(n, J, variant)
    out, fr, (p, t, g) = _gpu_case(n, J, variant)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(fr))
    print("n %d J %d %s: sums max rel err %.3e, frames max abs err %.3e"
          % (n, J, variant, vo.rel_err(out, want).max(), np.abs(fr - want_fr).max()))
    assert vo.sums_close(out, want)
    assert vo.frames_close(fr, want_fr)
    bones = out[vo.COUNT:].reshape(vo.BONE_ROWS, vo.MAX_BONES)
    assert np.all(bones[:, J - 1:] == 0.0) and np.all(bones[:, :J - 1] > 0.0)
    if variant in ("abs", "rel"):
        assert out[1] == out[0] and np.all(out[2:5] == 0.0)
    # the call only reads its inputs (the reference overwrites its own in place, trainer.py:193-194, :215)
    pos, trj, gt, _ = vo.variant_inputs(n, J, variant)
    assert np.array_equal(p, pos) and np.array_equal(g, gt) and (t is None or np.array_equal(t, trj))


@pytest.mark.parametrize("variant", ("trj", "rel"))
@pytest.mark.parametrize("n", NS)
def test_frame_columns_add_up_to_the_seven_sums(n, variant):
    out, fr, _ = _gpu_case(n, 17, variant)
    cols = np.add.reduce(fr, axis=0)                                   # index order
    print("n %d %s: column sums vs the seven sums, relative %s" % (n, variant, vo.rel_err(cols, out[:vo.COUNT])))
    assert vo.sums_close(cols, out[:vo.COUNT])


@pytest.mark.parametrize("variant", ("sum", "abs"))
@pytest.mark.parametrize("n", NS)
def test_two_runs_are_bit_identical_and_the_frame_buffer_is_optional(n, variant):
    pos, trj, gt, flags = vo.variant_inputs(n, 15, variant)
    out, fr, _ = _gpu_case(n, 15, variant)
    out2, fr2, _ = _run(pos, trj, gt, vo.tree_for(15), flags)
    assert out2.tobytes() == out.tobytes() and fr2.tobytes() == fr.tobytes()
    out3, none, _ = _run(pos, trj, gt, vo.tree_for(15), flags, frames=False)      # frame_dev = NULL
    assert none is None and out3.tobytes() == out.tobytes()


@pytest.mark.parametrize("n,J", [(65, 17), (257, 14)])
def test_no_parent_table_means_no_bone_terms(n, J):
    want, want_fr = _host_case(n, J, "trj", bones=False)
    out, fr, _ = _gpu_case(n, J, "trj", bones=False)
    assert vo.sums_close(out, want) and vo.frames_close(fr, want_fr)
    assert np.all(out[5:] == 0.0) and np.all(fr[:, 5:] == 0.0)
    assert out[:5].tobytes() == _gpu_case(n, J, "trj")[0][:5].tobytes()          # the other sums do not depend on it


@pytest.mark.parametrize("case", ["trj_n37", "trj_n1", "notrj_abs", "notrj_rel"])
def test_clip_valid_on_device_tensors_against_the_reference_fp32_values(case):
    from ray3d_amd import evaluate
    pos, trj, gt, flags, ref = vo.golden_case(case)
    n = pos.shape[0]
    clip = evaluate.Clip(vo.stub_camera(), np.zeros((n, 17, 3), np.float32), gt, "A", 3)
    row = evaluate.clip_valid(torch.from_numpy(pos).cuda().reshape(n, 1, 17, 3),
                              torch.from_numpy(trj).cuda().reshape(n, 1, 1, 3) if trj is not None else None, clip,
                              gt_root_relative=bool(flags & vo.GT_ROOT_RELATIVE))
    assert row.is_cuda and row.shape == (evaluate.VALID_COLS,) and row[:3].tolist() == [3.0, 0.0, float(n)]
    vo.check_against_reference(row[3:].cpu().numpy(), n, ref)
    # ... and with the ground truth already on the device, into a prepared row
    rows = torch.zeros((1, evaluate.VALID_COLS), dtype=torch.float64, device="cuda")
    evaluate.clip_valid(torch.from_numpy(pos).cuda(), torch.from_numpy(trj).cuda() if trj is not None else None, clip,
                        gt_dev=torch.from_numpy(gt).cuda(), out=rows[0], gt_root_relative=bool(flags & vo.GT_ROOT_RELATIVE))
    assert torch.equal(rows[0, 3:], row[3:])


def test_validate_clips_end_to_end_on_the_smallest_model():
    """model_j17_rf9_s1, a 12-frame clip: validate_clips over Ray3DLifter.forward_clip(return_trj=True) against clip_valid fed
    by the oracle chain's pos and trj.  The forward's outputs (pos + trj, and trj) are within e = 1e-4 m of the oracle's per
    coordinate (the suite's output bound), so, per frame and in the mean over frames:
      valid (LOSS)  a joint's error vector moves by <= e per coordinate: sqrt(3) e;
      pos           the recovered pos = sum - trj by <= 2 e per coordinate: 2 sqrt(3) e;
      trj           d moves by sqrt(3) e, weighted by w <= wmax = max |1 / gt_root_z|: wmax sqrt(3) e - for the figure as
                    logged, mean(w) mean(d), the same;
      bone length   a bone vector (a difference of two recovered joints) by <= 4 e per coordinate, its length by
                    dl = 4 sqrt(3) e;  bone direction: a unit vector by <= 2 dl / Lmin, Lmin the shortest predicted bone
                    (oracle side, less dl).
    The lifter's row recovers pos from the sum (R3D_VALID_POS_IS_SUM), the oracle chain's row is given pos itself: at most
    2^-23 max|sum| per coordinate more (the header's contract), added to e."""
    import ray3d_amd
    from oracle import oracle
    from ray3d_amd import evaluate
    z, mc = load_model_fixture("j17_rf9_s1")
    (cp, sp), (ct, st) = synth_states(mc)
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos_m, trj_m = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos_m, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj_m, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos_m.eval(), trj_m.eval()
    lifter = ray3d_amd.Ray3DLifter(pos_m, trj_m).eval()
    n, rf, pad = 12, cp.receptive_field, (cp.receptive_field - 1) // 2
    e = 1e-4
    assert rf == 9
    from ray3d_amd import synth
    rays = synth.synth_rays(n, cp, seed=3)[:, 0]                                     # (12, 17, 3): one frame per window
    cam = vo.stub_camera()
    padded = evaluate.pad_clip(rays, pad)
    win = np.stack([padded[i:i + rf] for i in range(n)])
    par = np.tile(cam.param(), (n, 1))
    o_pos = oracle.forward(cp, sp, win, par).reshape(n, 17, 3)
    o_trj = oracle.forward(ct, st, win, par).reshape(n, 3)
    rng = np.random.default_rng(12)
    # ground truth near the oracle's poses, every frame moved along the optical axis so that its root is 4 m deep: 1 / z is tame
    gt = o_pos + o_trj[:, None] + rng.normal(0, 0.03, (n, 17, 3))
    gt[:, :, 2] += (4.0 - gt[:, 0, 2])[:, None]
    gt = gt.astype(np.float32)
    clip = evaluate.Clip(cam, rays, gt, "A", 0)
    dev = torch.device("cuda:0")
    with torch.no_grad():
        table, rows = evaluate.validate_clips(lambda p, q: lifter.forward_clip(p, q, return_trj=True), [clip], rf, dev)
        total, trj = lifter.forward_clip(torch.from_numpy(padded).to(dev), torch.from_numpy(cam.param()).to(dev), return_trj=True)
        plain = lifter.forward_clip(torch.from_numpy(padded).to(dev), torch.from_numpy(cam.param()).to(dev))
    assert total.shape == (n, 1, 17, 3) and trj.shape == (n, 1, 1, 3) and torch.equal(total, plain)    # the default is unchanged
    assert np.abs(total.cpu().numpy().reshape(n, 17, 3) - (o_pos + o_trj[:, None])).max() <= e
    assert np.abs(trj.cpu().numpy().reshape(n, 3) - o_trj).max() <= e
    e += 2.0 ** -23 * float(np.abs(total.cpu().numpy()).max())          # pos recovered from the sum (R3D_VALID_POS_IS_SUM) against pos given
    want_row = evaluate.clip_valid(torch.from_numpy(o_pos).to(dev), torch.from_numpy(o_trj).to(dev), clip)
    want = evaluate.reduce_valid(want_row[None], 17)
    assert rows.is_cuda and rows.shape == (1, evaluate.VALID_COLS) and table["frames"] == n
    wmax = float(np.abs(1.0 / gt[:, 0, 2].astype(np.float64)).max())
    tree = vo.H36M
    lmin = float(np.linalg.norm((o_pos[:, list(tree[1:])] - o_pos[:, 1:]).astype(np.float64), axis=-1).min())
    s3, dl = np.sqrt(3.0), 4 * np.sqrt(3.0) * e
    assert lmin > 2 * dl
    bounds = {"valid_mm": s3 * e, "pos_mm": 2 * s3 * e, "trj_mm": wmax * s3 * e, "trj_mm_as_logged": wmax * s3 * e,
              "bone_len_mm": dl, "bone_mm": dl + 2 * dl / (lmin - dl)}
    for k, b in bounds.items():
        print("%-17s lifter %.6f  oracle chain %.6f  |diff| %.3e  bound %.3e" % (k, table[k], want[k], abs(table[k] - want[k]), b * 1e3))
        assert np.isfinite(table[k]) and abs(table[k] - want[k]) <= b * 1e3 * (1 + 1e-9), k
    for got, w in zip(table["bones"], want["bones"]):
        assert abs(got["len_err_mm"] - w["len_err_mm"]) <= dl * 1e3 and abs(got["len_pred_mm"] - w["len_pred_mm"]) <= dl * 1e3
        assert got["len_gt_mm"] == w["len_gt_mm"]
