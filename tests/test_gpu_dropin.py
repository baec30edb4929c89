"""-m gpu: the drop-in seam on the device.  r3d_forward_pair_split against r3d_forward_pair bit for bit and against the
reference's fixtures; Trainer.evaluate_core's two branches (lib/train_val/trainer.py:296-353) replayed through the objects
Model(...) returns - the order of its calls and its tensor operations, in this file's own words - with the pair seam off and on;
guard bands around the split call's buffers; non-finite input."""
import functools
import os

import numpy as np
import pytest
import torch

from buffers_util import PATTERN_IDS, PATTERNS, Arena, ExactWorkspace
from conftest import GOLDEN, MODEL_CASES, case_out_scale, check_parity, load_model_fixture
from nonfinite_util import VALUES, poisoned_copy, positions
from test_gpu_parity import build_modules

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous().numpy(), b.detach().cpu().contiguous().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _pair(name, b3=False, staged=False):
    """(lifter, pos cfg) of a reference fixture's configuration, on the product library, built once per session."""
    import ray3d_amd
    _, mc = load_model_fixture(name)
    pos, trj, (cp, _), _ = build_modules(dict(mc, BF16X3=True) if b3 else mc, case_out_scale(name))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.set_staged(staged)
    return lifter, cp


def _assert_contract(pair, split, what):
    """The two equalities include/ray3d_hip.h states for r3d_forward_pair_split."""
    (out, trj), (spos, strj) = pair, split
    assert spos.shape == out.shape and strj.shape == trj.shape, what
    assert torch.isfinite(spos).all() and torch.isfinite(strj).all(), what
    assert _bits_equal(strj, trj), "%s: out_trj differs from r3d_forward_pair's" % what
    assert _bits_equal(spos + strj, out), "%s: out_pos + out_trj differs from r3d_forward_pair's out" % what
    assert not _bits_equal(spos, out), "%s: out_pos still holds the trajectory" % what


# ---------------------------------------------------------------- 1. split against pair, bit for bit

@pytest.mark.parametrize("name,B", [("j17_rf27_s3", 1), ("j17_rf27_s3", 3), ("j17_rf27_s3", 33), ("j17_rf27_s3", 127),
                                    ("j17_rf27_s3", 130), ("j15_rf9_s3", 130)])
def test_split_equals_pair_bit_for_bit(name, B):
    from ray3d_amd import synth
    lifter, cp = _pair(name)
    x = torch.from_numpy(synth.synth_rays(B, cp, seed=11)).to(DEV)
    p = torch.from_numpy(synth.synth_param(B, seed=12)).to(DEV)
    with torch.no_grad():
        pair = lifter(x, p, return_trj=True)
        split = lifter.forward_split(x, p)
    lifter.check_status()
    _assert_contract(pair, split, "%s B=%d" % (name, B))


@pytest.mark.parametrize("form", ["clip-stride-1", "uv", "staged", "bf16x3"])
def test_split_equals_pair_in_the_other_input_modes_and_forms(form):
    from ray3d_amd import _capi, synth
    lifter, cp = _pair("j17_rf27_s3", b3=form == "bf16x3", staged=form == "staged")
    rf, J = cp.receptive_field, cp.num_joints
    if form == "clip-stride-1":
        B = 130
        clip = synth.synth_rays(6, cp, seed=21).reshape(-1, J, cp.in_features)[:B + rf - 1].copy()     # (B + RF - 1 frames)
        args = (_capi.R3D_INPUT_RAYS, torch.from_numpy(clip).to(DEV), 1, B, torch.from_numpy(synth.synth_param(1, seed=22)[0]).to(DEV), 0)
        kw = {}
    elif form == "uv":
        B = 33
        uv = (1000.0 * synth.hash_uniform("dropin.uv", (B, rf, J, 2), 23)).astype(np.float32)
        rows = np.tile(np.asarray(_evalcore()[1][0].camera.cam_row(), dtype=np.float64), (B, 1))
        args = (_capi.R3D_INPUT_UV, torch.from_numpy(uv).to(DEV), rf, B, torch.from_numpy(synth.synth_param(B, seed=24)).to(DEV), 2)
        kw = dict(cam=torch.from_numpy(rows).to(DEV), cam_stride=8)
    else:
        B = 130
        args = (_capi.R3D_INPUT_RAYS, torch.from_numpy(synth.synth_rays(B, cp, seed=25)).to(DEV), rf, B,
                torch.from_numpy(synth.synth_param(B, seed=26)).to(DEV), 2)
        kw = {}
    with torch.no_grad():
        pair = lifter._run(*args, return_trj=True, **kw)
        split = lifter._run(*args, return_trj=True, split=True, **kw)
    lifter.check_status()
    if form == "bf16x3":
        assert lifter.precision(torch.device(DEV)) == "bf16x3"
    _assert_contract(pair, split, form)


# ---------------------------------------------------------------- 2. split against the reference

SPLIT_CASES = [n for n in MODEL_CASES if load_model_fixture(n)[1]["TRAJECTORY_MODEL"]]    # every fixture that has a trj model


@pytest.mark.parametrize("name", SPLIT_CASES)
def test_split_matches_the_reference_fixture(name):
    z, mc = load_model_fixture(name)
    lifter, _ = _pair(name)
    x, p = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["param"]).to(DEV)      # (the fixture's own few windows)
    with torch.no_grad():
        spos, strj = lifter.forward_split(x, p)
    lifter.check_status()
    check_parity(spos, z["out_pos"], "split out_pos vs reference fixture")
    check_parity(strj, z["out_trj"], "split out_trj vs reference fixture")


# ---------------------------------------------------------------- 3. / 4. evaluate_core through Model(...) objects

@functools.lru_cache(maxsize=None)
def _evalcore():
    import ray3d_amd
    from ray3d_amd import evaluate
    z = np.load(os.path.join(GOLDEN, "evalcore.npz"))
    clips = [evaluate.Clip(ray3d_amd.Camera(z["clip%d/K" % i], z["clip%d/R" % i], z["clip%d/t" % i]),
                           z["clip%d/rays" % i], z["clip%d/gt_norm" % i], "A", i) for i in range(3)]
    return z, clips


def _models(fuse):
    """pos, trj as the reference's unchanged Model(model_config, data_config, is_train) call returns them; the one-import
    user's switch is the module-level default."""
    import ray3d_amd
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    if not fuse:
        return build_modules(mc)[:2]
    ray3d_amd.fuse_pair_default(True)
    try:
        pos, trj = build_modules(mc)[:2]
    finally:
        ray3d_amd.fuse_pair_default(False)
    assert pos._seam is trj._seam and pos._seam.on
    return pos, trj


def _windows(seq, rf):
    """What the evaluation feeds a model for an unchunked sequence (N, J, F): edge-padded by (RF - 1) / 2 on both sides and
    cut into every window of RF frames - materialised, (N, RF, J, F)."""
    pad = (rf - 1) // 2
    padded = torch.cat([seq[:1].expand(pad, -1, -1), seq, seq[-1:].expand(pad, -1, -1)], dim=0)
    return torch.stack([padded[i:i + rf] for i in range(seq.shape[0])]).contiguous()


@pytest.mark.parametrize("fuse", [False, True], ids=["separate", "fuse_pair"])
def test_return_predictions_branch_with_cpu_inputs(fuse):
    """trainer.py:304-311: CPU windows and CPU parameter rows straight into the two models, the sum brought back by the
    caller.  (Before the wrappers moved CPU arguments to their device this raised on the CPU tensor.)"""
    z, clips = _evalcore()
    pos, trj = _models(fuse)
    x = _windows(torch.from_numpy(z["clip0/rays"].astype("float32")), 27)
    p = torch.from_numpy(np.tile(clips[0].camera.param(), (x.shape[0], 1)))
    assert tuple(x.shape) == (100, 27, 17, 3) and not x.is_cuda and not p.is_cuda
    with torch.no_grad():
        pos.eval(), trj.eval()
        out = pos(x, p) + trj(x, p)
    assert out.is_cuda                                     # (the caller's .cpu() brings it back, as with DataParallel)
    check_parity(out.cpu().numpy(), z["clip0/predictions"], "evaluate_core(return_predictions=True), clip 0")


def _forward_launches(handles):
    return sum(1 for h in handles for r in h.profile_read() if r["kernel"].startswith("r3d_forward"))


@pytest.mark.parametrize("flip", [False, True], ids=["flip0", "flip1"])
@pytest.mark.parametrize("fuse", [False, True], ids=["separate", "fuse_pair"])
def test_metric_branch_in_the_references_call_order(fuse, flip):
    """trainer.py:322-353 per clip - device inputs; pos, pos_flip, trj, trj_flip with the in-place un-flips and the per-network
    means, then += - and the five figures through the project's metrics, at the bounds of
    test_evaluate_clips_reproduces_reference_metrics.  The forward launches of each clip's module calls are counted."""
    from ray3d_amd import evaluate
    z, clips = _evalcore()
    pos, trj = _models(fuse)
    left, right = list(z["kps_left"]), list(z["kps_right"])
    dev = torch.device(DEV)
    rows = []
    with torch.no_grad():
        pos.eval(), trj.eval()
        handles = [pos.module.handle(dev), trj.module.handle(dev)]
        for clip in clips:
            seq = torch.from_numpy(clip.rays.astype("float32"))
            if flip:
                seq_flip = seq.clone()
                seq_flip[:, :, 0] *= -1
                seq_flip[:, left + right, :] = seq_flip[:, right + left, :]
            x = _windows(seq, 27).cuda()
            p = torch.from_numpy(np.tile(clip.camera.param(), (x.shape[0], 1))).cuda()
            if flip:
                x_flip = _windows(seq_flip, 27).cuda()
            launches = 0

            def call(model, *args):
                nonlocal launches
                for h in handles:
                    h.profile_enable(True)                # (clears the handle's records: a parked result leaves none)
                out = model(*args)
                launches += _forward_launches(handles)
                return out
            try:
                pred = call(pos, x, p)
                if flip:
                    pred_flip = call(pos, x_flip, p)
                    pred_flip[:, :, :, 0] *= -1
                    pred_flip[:, :, left + right] = pred_flip[:, :, right + left]
                    pred = torch.mean(torch.cat((pred, pred_flip), dim=1), dim=1, keepdim=True)
                t = call(trj, x, p)
                if flip:
                    t_flip = call(trj, x_flip, p)
                    t_flip[:, :, :, 0] *= -1
                    t = torch.mean(torch.cat((t, t_flip), dim=1), dim=1, keepdim=True)
                pred += t
            finally:
                for h in handles:
                    h.profile_enable(False)
            calls = 4 if flip else 2
            assert launches == (calls // 2 if fuse else calls), (launches, calls, fuse)
            rows.append(evaluate.clip_partials_hip(pred, clip, 0))
    got = np.array(evaluate.reduce_partials(torch.stack(rows))[0])
    ref = z["metrics_flip%d" % int(flip)]
    print("metric branch fuse=%s flip=%s: got %s ref %s" % (fuse, flip, got, ref))
    assert abs(got[0] - ref[0]) < 2e-2, (got, ref)         # mm
    assert np.abs(got - ref).max() < 5e-2, (got, ref)


# ---------------------------------------------------------------- 5. guard bands

OUT_SENTINEL = 12345.0


@pytest.mark.parametrize("B", [5, 130])
def test_split_call_writes_nothing_outside_its_buffers(B):
    """Every buffer of one r3d_forward_pair_split call carved exact-sized from one pattern-filled allocation, once per
    pattern (the workspace starts poisoned): the guards stay clean, both outputs are finite and fully written, and they
    have the bits of the ordinary call."""
    from ray3d_amd import _capi, synth
    lifter, cp = _pair("j17_rf27_s3")
    dev = torch.device(DEV)
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    J, rf = cp.num_joints, cp.receptive_field
    x_np, p_np = synth.synth_rays(B, cp, seed=31), synth.synth_param(B, seed=32)
    with torch.no_grad():
        plain_pos, plain_trj = lifter.forward_split(torch.from_numpy(x_np).to(dev), torch.from_numpy(p_np).to(dev))
    nbytes = _capi.workspace_bytes(hp, ht, B)
    sizes = [x_np.nbytes, p_np.nbytes, B * J * 3 * 4, B * 3 * 4, nbytes]
    arena = Arena(dev, PATTERNS[0], Arena.capacity_for(sizes))
    put_x, put_p = arena.put(x_np, name="x_dev"), arena.put(p_np, name="param_dev")
    out_pos = arena.carve(B * J * 3 * 4, name="out_pos_dev").view(torch.float32).view(B, 1, J, 3)
    out_trj = arena.carve(B * 3 * 4, name="out_trj_dev").view(torch.float32).view(B, 1, 1, 3)
    wsv = ExactWorkspace(arena, "workspace_dev").get(nbytes, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for pid, pattern in zip(PATTERN_IDS, PATTERNS):
        arena.refill(pattern)
        x, p = put_x(), put_p()
        out_pos.fill_(OUT_SENTINEL), out_trj.fill_(OUT_SENTINEL)
        inp = _capi.make_input(_capi.R3D_INPUT_RAYS, x.data_ptr(), rf, p.data_ptr(), 2)
        with torch.cuda.device(dev):
            _capi.forward_pair_split(hp, ht, inp, B, out_pos.data_ptr(), out_trj.data_ptr(), wsv.data_ptr(), nbytes, stream)
        arena.check()                                      # (synchronises)
        lifter.check_status(dev)
        for o, plain in ((out_pos, plain_pos), (out_trj, plain_trj)):
            assert torch.isfinite(o).all(), pid
            assert not (o == OUT_SENTINEL).any(), pid
            assert _bits_equal(o, plain), pid


# ---------------------------------------------------------------- 6. non-finite input

def test_a_nan_keypoint_poisons_its_window_in_both_outputs_and_no_other():
    from ray3d_amd import synth
    lifter, cp = _pair("j17_rf27_s3")
    B, k = 33, 16
    x_np, p_np = synth.synth_rays(B, cp, seed=41), synth.synth_param(B, seed=42)
    p = torch.from_numpy(p_np).to(DEV)
    with torch.no_grad():
        clean = lifter.forward_split(torch.from_numpy(x_np).to(DEV), p)
        for where in positions(cp.receptive_field, cp.num_joints, cp.in_features):
            bad = poisoned_copy(x_np, [(k,) + where], VALUES["nan"])
            got = lifter.forward_split(torch.from_numpy(bad).to(DEV), p)
            lifter.check_status()
            others = [i for i in range(B) if i != k]
            for g, c, what in zip(got, clean, ("pos", "trj")):
                assert not torch.isfinite(g[k]).any(), (what, where)
                assert _bits_equal(g[others], c[others]), (what, where)
