"""-m gpu: r3d_clips_repair - a shard's encoded inputs repaired in place behind r3d_clips_encode - against its host hook over the
cases of tests/clips_repair_cases.py, bit for bit in all five outputs, inside guard bands with the outputs pre-poisoned; captured
in a hipGraph and replayed over three inputs; and end to end through predict_clips_batched / evaluate_clips_batched(repair=) on
pixel archives with dropped keypoints, for the ray pair and for a 2-feature pair."""
import functools

import numpy as np
import pytest
import torch

import clips_repair_cases as cc
from clips_repair_cases import FILL_STATE, FILL_STATS, QNAN, bits
from conftest import check_parity
from test_clips_encode_host import KPS, cameras, pixels

pytestmark = pytest.mark.gpu

H36M_LEFT, H36M_RIGHT = KPS[17]


# ------------------------------------------------------------------ the device against the host hook

@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_device_equals_the_host_hook(name):
    """x, x_mirror, state, stats and status of the kernel - every buffer an exact-size region between guard bands, x / x_mirror / conf
    4 bytes off their alignment, the outputs pre-poisoned - are the host hook's, bit for bit; no byte outside the regions is written."""
    got = cc.run_case("cuda", name)
    cc.agree(got, cc.host_case(name), name)


def test_optional_outputs_left_out_stay_poisoned():
    name = "j17_f3_gap5"
    got, want = cc.run_case("cuda", name, want_state=False, want_stats=False), cc.host_case(name)
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["xm"], want["xm"]) and np.array_equal(got["status"], want["status"])
    assert (got["state"] == FILL_STATE).all() and (got["stats"].view(np.uint32) == FILL_STATS).all()


def test_one_observation_then_missing_to_the_longest_clip_s_end():
    """R3D_REPAIR_MAX_ROWS rows, J 3: joint 0 observed once and then missing for 65 535 rows (a hold that reaches back over every
    step), joint 1 observed only in the last row (a back-fill over every step), joint 2 gap-free - the hook's bits, the exact counts."""
    from ray3d_amd import _capi
    R, J, F = _capi.REPAIR_MAX_ROWS, 3, 3
    rng = np.random.default_rng(3)
    x = bits(rng.normal(0, 1, (R, J, F)).astype(np.float32)).copy()
    x[1:, 0] = QNAN
    x[:-1, 1] = cc.PINF
    table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
    table[0]["n_frames"], table[0]["pad_front"], table[0]["pad_back"] = R - 20, 13, 7
    args = (x, None, None, table, R, R, None, 0.0, 10)
    got, want = cc.run("cuda", *args), cc.run("cpu", *args)
    cc.agree(got, want, "longest clip")
    assert got["stats"].tolist() == [[[0, R - 20, 0, 0], [0, 0, R - 20, 0], [0, 0, 0, 0]]]       # (the two observations are padding rows)
    assert (bits(got["x"])[:, 0] == x[0, 0]).all() and (bits(got["x"])[:, 1] == x[-1, 1]).all() and np.array_equal(got["x"][:, 2], x[:, 2])


# ------------------------------------------------------------------ hipGraph

def test_captured_once_and_replayed_over_three_inputs():
    """shard_repair_hip captured into a hipGraph with its output tensors handed in (torch.cuda.graph, default queue settings); three
    different inputs are copied into the captured addresses - the copies staged outside the graph - and each replay gives the bits
    of an eager call on that input."""
    from ray3d_amd import evaluate
    c = cc.make_case("j17_f2_gap1_conf")
    dev = torch.device("cuda:0")
    n, J, F = len(c["table"]), c["J"], c["F"]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)
    x = i32(c["x"]).view(torch.float32)
    xm = i32(c["xm"]).view(torch.float32)
    tab = torch.from_numpy(c["table"].view(np.uint8).copy()).to(dev)
    conf = torch.from_numpy(c["conf"]).to(dev)
    state = torch.empty((c["out_rows"], J), dtype=torch.uint8, device=dev)
    stats = torch.empty((n, J, 4), dtype=torch.int32, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            evaluate.shard_repair_hip(x, tab, n, c["out_rows"], c["max_rows"], c["max_gap"], xm, c["perm"], conf, c["min_conf"],
                                      state=state, stats=stats, status=status)
    rng = np.random.default_rng(8)
    for k in range(3):
        xin = c["x"].copy()
        if k:                                                            # other inputs: more points knocked out
            xin[rng.random(xin.shape[:2]) < 0.1 * k] = QNAN
        xmin = xin[:, c["perm"]].copy()
        xmin[..., 0] ^= cc.SIGN
        eager = cc.run("cuda", xin, xmin, c["perm"], c["table"], c["out_rows"], c["max_rows"], c["conf"], c["min_conf"], c["max_gap"])
        sx, sxm = i32(xin).view(torch.float32), i32(xmin).view(torch.float32)       # staged outside the graph
        x.copy_(sx), xm.copy_(sxm)
        state.fill_(FILL_STATE), stats.fill_(-1), status.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = dict(x=x.view(torch.int32).cpu().numpy().view(np.uint32), xm=xm.view(torch.int32).cpu().numpy().view(np.uint32),
                   state=state.cpu().numpy(), stats=stats.cpu().numpy(), status=status.cpu().numpy())
        cc.agree(got, eager, "replay %d" % k)
        assert k == 0 or not np.array_equal(got["x"], first)
        first = got["x"] if k == 0 else first
    del g
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end

@functools.lru_cache(maxsize=None)
def _lifter(encode):
    if encode == "ray":                                                  # the RF-27, J-17 ray pair of tests/test_gpu_clips_metrics.py
        from test_gpu_clips_metrics import _lifter as make
        return make()
    from test_gpu_px2d import _pair                                      # the RF-27, J-17 2-feature pair of tests/test_gpu_px2d.py
    return _pair("3,3,3")[0]


LENGTHS, GAP_FREE, K = (30, 50, 90, 120), 2, 5


def _dropped_clips(encode):
    """Four clips of 30 - 120 frames of raw pixels on four cameras; in all but clip GAP_FREE some joints are NaN for runs of 1 - 8
    frames (runs longer than K = 5 are held, a run at frame 0 is back-filled, the others are interpolated)."""
    from ray3d_amd import evaluate
    rng = np.random.default_rng(21)
    out = []
    for k, n in enumerate(LENGTHS):
        px = pixels("clips_repair.%s.%d" % (encode, k), (n, 17, 2)).copy()
        if k != GAP_FREE:
            for j, start, run in ((0, 0, 3), (3, n - 2, 2), (5, 7, 8), (16, 11, 1), (16, 14, 5)):
                px[start:start + run, j] = np.nan
            for _ in range(4):
                j, run = int(rng.integers(6, 16)), int(rng.integers(1, 9))
                start = int(rng.integers(0, n - run))
                px[start:start + run, j, int(rng.integers(0, 2))] = np.nan
        gt = rng.normal(0, 0.5, (n, 17, 3)).astype(np.float32)
        out.append(evaluate.Clip(cameras()[k], px, gt, "AB"[k % 2], k))
    return out


def _reads_a_nan(px, pad=13):
    """Per frame: the window of RF 27 around it (edge-padded) reads a NaN keypoint."""
    bad = np.isnan(px).any(axis=(1, 2))
    idx = np.clip(np.arange(len(px))[:, None] + np.arange(-pad, pad + 1)[None], 0, len(px) - 1)
    return bad[idx].any(axis=1)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("encode", ["ray", "intrinsic"])
def test_shard_pipeline_survives_dropped_keypoints(encode):
    """(a) without repair= the windows that read a NaN keypoint are NaN and the others finite: the existing contract, the baseline;
    (b) with repair=5 every pose is finite and repair_out["stats"] holds the restatement's counts; (c) the gap-free clip's poses and
    metric row keep the bits they have without repair=; (d) the repaired x_all / xm_all are the NumPy restatement applied to the
    downloaded un-repaired encode output, and the poses are forward_clip on slices of that host-repaired buffer uploaded again, bit
    for bit; (e) the same with pool_below=64 (two clips pooled): finite, the same counts, the un-pooled clips keep their bits, the
    pooled ones agree within the bound pooled poses are held to against the per-clip path (HIP against HIP: 2e-5 * max(1, |ref|))."""
    from ray3d_amd import evaluate
    lifter, dev = _lifter(encode), torch.device("cuda:0")
    clips = _dropped_clips(encode)
    kw = dict(flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, encode=encode)
    out, out_pool = {}, {}
    with torch.no_grad():
        base = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, world=False, **kw)
        rep = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, world=False, repair=K, repair_out=out, **kw)
        _, _, rows0 = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, **kw)
        _, _, rows1 = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, repair=K, **kw)
        base_pool = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, world=False, pool_below=64, **kw)
        rep_pool = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, world=False, pool_below=64, repair=K,
                                                  repair_out=out_pool, **kw)
    torch.cuda.synchronize()
    # (a)
    for c, (p, _) in zip(clips, base):
        nan = torch.from_numpy(_reads_a_nan(c.rays)).to(dev)
        assert bool(nan.any()) == (c.clip_id != GAP_FREE)
        assert not torch.isfinite(p[nan]).any() and torch.isfinite(p[~nan]).all()
    # (d) by hand: the encode call of the pass, its output downloaded, the restatement; then the device call on the same buffers
    sizes_of = lifter.clip_batch_sizes
    itable, first, out_rows, max_rows = evaluate.clip_input_table(clips, 27, False, lambda n: sum(sizes_of(n)) - n)
    px_all = torch.from_numpy(np.concatenate([c.rays for c in clips])).to(dev)
    perm = evaluate.mirror_permutation(17, H36M_LEFT, H36M_RIGHT)
    tab = torch.from_numpy(itable.view(np.uint8)).to(dev)
    x_all, xm_all, st = evaluate.shard_encode_hip(px_all, tab, 4, out_rows, max_rows, encode, perm)
    x0, xm0 = bits(x_all.cpu().numpy()), bits(xm_all.cpu().numpy())
    J, F = x0.shape[1:]
    hx, hxm, hstate, hstats, hstatus = cc.restate(x0, xm0, perm, itable, out_rows, max_rows, None, 0.0, K, np.zeros((out_rows, J), np.uint8),
                                                  np.zeros((4, J, 4), np.int32))
    state, stats, status = evaluate.shard_repair_hip(x_all, tab, 4, out_rows, max_rows, K, xm_all, perm)
    torch.cuda.synchronize()
    assert not st.any() and not status.any() and not hstatus.any()
    assert np.array_equal(bits(x_all.cpu().numpy()), hx) and np.array_equal(bits(xm_all.cpu().numpy()), hxm)
    assert np.array_equal(state.cpu().numpy(), hstate) and np.array_equal(stats.cpu().numpy(), hstats)
    assert {1, 2, 3} <= set(np.unique(hstate).tolist()) and not (hstate == 4).any() and not hstats[GAP_FREE].any()
    # (b)
    assert all(torch.isfinite(p).all() for p, _ in rep)
    assert np.array_equal(out["stats"].cpu().numpy(), hstats) and np.array_equal(out["state"].cpu().numpy(), hstate) and not out["status"].any()
    # (d) the poses: forward_clip on slices of the host-repaired buffer, the flip average as predict_clip rounds it
    ux, uxm = (torch.from_numpy(a.view(np.float32).copy()).to(dev) for a in (hx, hxm))
    with torch.no_grad():
        for k, c in enumerate(clips):
            n = c.rays.shape[0]
            rows = slice(first[k], first[k] + n + 26 + sum(sizes_of(n)) - n)
            prow = torch.from_numpy(c.camera.param()).to(dev)
            p = lifter.forward_clip(ux[rows], prow, n_windows=n)
            pm = lifter.forward_clip(uxm[rows], prow, n_windows=n)
            want = 0.5 * (p + evaluate.mirror_output(pm, H36M_LEFT, H36M_RIGHT))
            assert _same(rep[k][0], want.reshape(n, 17, 3)), k
    # (c)
    assert _same(rep[GAP_FREE][0], base[GAP_FREE][0])
    g = rows0[:, 0].tolist().index(float(GAP_FREE))
    assert torch.equal(rows1[g].view(torch.int64), rows0[g].view(torch.int64)) and torch.equal(rows1[:, :3], rows0[:, :3])
    assert torch.isfinite(rows1[:, 3:]).all() and not torch.isfinite(rows0[[r for r in range(4) if r != g], 3]).any()
    # (e)
    assert np.array_equal(out_pool["stats"].cpu().numpy(), hstats) and not out_pool["status"].any()
    assert _same(rep_pool[GAP_FREE][0], base_pool[GAP_FREE][0])
    for k, n in enumerate(LENGTHS):
        assert torch.isfinite(rep_pool[k][0]).all()
        if n >= 64:
            assert _same(rep_pool[k][0], rep[k][0]), k
        else:
            ref = rep[k][0].cpu().numpy()
            check_parity(rep_pool[k][0].cpu().numpy(), ref, "%s: repaired poses of the pooled %d-frame clip vs the per-clip path" % (encode, n),
                         tol=2e-5 * max(1.0, float(np.abs(ref).max())))
    # (e) the buffers: the re-laid-out table (pads 0 for the pooled clips) through the same two calls
    at = 0
    for d in itable:
        if int(d["n_frames"]) < 64:
            d["pad_front"] = d["pad_back"] = 0
        d["out_first"] = at
        at += int(d["pad_front"] + d["n_frames"] + d["pad_back"])
    tab = torch.from_numpy(itable.view(np.uint8)).to(dev)
    x_all, xm_all, st = evaluate.shard_encode_hip(px_all, tab, 4, at, max_rows, encode, perm)
    x0, xm0 = bits(x_all.cpu().numpy()), bits(xm_all.cpu().numpy())
    hx, hxm, hstate, hstats2, _ = cc.restate(x0, xm0, perm, itable, at, max_rows, None, 0.0, K, np.zeros((at, J), np.uint8), np.zeros((4, J, 4), np.int32))
    state, stats, status = evaluate.shard_repair_hip(x_all, tab, 4, at, max_rows, K, xm_all, perm)
    torch.cuda.synchronize()
    assert not status.any() and np.array_equal(hstats2, hstats) and np.array_equal(stats.cpu().numpy(), hstats)
    assert np.array_equal(bits(x_all.cpu().numpy()), hx) and np.array_equal(bits(xm_all.cpu().numpy()), hxm)
    assert np.array_equal(state.cpu().numpy(), hstate) and np.array_equal(out_pool["state"].cpu().numpy(), hstate)


def test_refusals_of_the_python_layer():
    from ray3d_amd import _capi, evaluate
    lifter, dev = _lifter("ray"), torch.device("cuda:0")
    clips = _dropped_clips("ray")
    with pytest.raises(ValueError, match="encode call's buffer"):
        evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, repair=5)
    with pytest.raises(ValueError, match="encode call's buffer"):
        evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, repair=5)
    with pytest.raises(ValueError, match="repair="):
        evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, encode="ray", repair=-1)
    long = evaluate.Clip(clips[0].camera, np.zeros((_capi.REPAIR_MAX_ROWS, 17, 2), np.float32), np.zeros((0, 17, 3), np.float32), "A", 41)
    with pytest.raises(ValueError, match="clip_id 41"):
        evaluate.predict_clips_batched(lifter.forward_clip, [clips[0], long], 27, dev, encode="ray", repair=5)
    x = torch.zeros((10, 17, 3), device=dev)
    tab = torch.zeros(160, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="go together"):
        evaluate.shard_repair_hip(x, tab, 1, 10, 10, 5, x_mirror_all=torch.zeros_like(x))
    with pytest.raises(ValueError, match="max_rows"):
        evaluate.shard_repair_hip(x, tab, 1, 10, _capi.REPAIR_MAX_ROWS + 1, 5)
    with pytest.raises(ValueError, match="conf_all"):
        evaluate.shard_repair_hip(x, tab, 1, 10, 10, 5, conf_all=torch.zeros((4, 16), device=dev))
    with pytest.raises(ValueError, match="state"):
        evaluate.shard_repair_hip(x, tab, 1, 10, 10, 5, state=torch.zeros((10, 17), dtype=torch.int32, device=dev))


def test_confidences_of_some_clips_only():
    """Clip.conf on two of four clips, min_conf 0.5: the clips without one count as +inf - their repair is that of the pass without
    confidences -, and a finite keypoint of low confidence is repaired like a NaN one."""
    from ray3d_amd import evaluate
    lifter, dev = _lifter("ray"), torch.device("cuda:0")
    clips = _dropped_clips("ray")
    rng = np.random.default_rng(2)
    for k in (1, GAP_FREE):
        conf = rng.uniform(0.6, 1.0, (LENGTHS[k], 17)).astype(np.float32)
        conf[10:13, 2], conf[20, 9] = 0.25, np.nan
        clips[k].conf = conf
    kw = dict(flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, encode="ray", world=False, repair=K)
    a, b = {}, {}
    with torch.no_grad():
        plain = evaluate.predict_clips_batched(lifter.forward_clip, _dropped_clips("ray"), 27, dev, repair_out=a, **kw)
        got = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, min_conf=0.5, repair_out=b, **kw)
    torch.cuda.synchronize()
    sa, sb = a["stats"].cpu().numpy(), b["stats"].cpu().numpy()
    assert np.array_equal(sa[[0, 3]], sb[[0, 3]]) and _same(got[0][0], plain[0][0]) and _same(got[3][0], plain[3][0])
    assert sb[GAP_FREE].sum() == 4 and sb[GAP_FREE, 2, 0] == 3 and sb[GAP_FREE, 9, 0] == 1 and not sa[GAP_FREE].any()
    assert all(torch.isfinite(p).all() for p, _ in got) and not _same(got[GAP_FREE][0], plain[GAP_FREE][0])
