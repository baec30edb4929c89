"""GPU suite: r3d_clips_windows (a batch of materialised windows gathered from a pool of windows drawn from many clips) and the
pooled path built on it.  The kernel against the host hook, bit for bit, under guard bands and poisoned destinations;
Ray3DLifter.forward_windows against lifter.forward on host-built windows (bits), the oracle chain (1e-4) and forward_clip (the
clip-vs-materialised bound); evaluate_clips_batched / predict_clips_batched with pool_below=; refusals; one hipGraph capture.
Clips of 1, 2, 5, 13, 14, 40 and 100 frames in batches of 64 windows: batches cut clips and the last one carries surplus."""
import functools
import os

import numpy as np
import pytest
import torch

import windows_cases as wc
from buffers_util import NANS, Arena
from conftest import GOLDEN, case_out_scale, check_parity, load_model_fixture, synth_states
from ray3d_amd import _capi, evaluate
from test_clips_windows_host import host_call, same_bits

pytestmark = pytest.mark.gpu

BATCH = 64
# the J != 17 pair of tests/golden is j14_rf9_s3
FIXTURES = ["j17_rf27_s3", "j14_rf9_s3", "j17_f2_rf27_noemb_s3", "j17_rf81_causal_s3"]
H36M_LEFT, H36M_RIGHT = wc.KPS[17]


@functools.lru_cache(maxsize=None)
def pair(name):
    """(lifter with 64-window call sizes, ((cp, sp), (ct, st))) of a model fixture's configuration and synthetic weights."""
    import ray3d_amd
    _, mc = load_model_fixture(name)
    states = synth_states(mc, case_out_scale(name))
    (cp, sp), (ct, st) = states
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos.eval(), trj.eval()
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.CLIP_CHUNK = lifter.CLIP_ROUND = BATCH
    return lifter, states


@functools.lru_cache(maxsize=None)
def pool(name, flip=False):
    """The evaluation pool of a fixture: (src, table, run_param or None, total_windows, sizes, perm, host-built x, param)."""
    lifter, ((cp, _), _) = pair(name)
    J, F, rf = cp.num_joints, cp.in_features, cp.receptive_field
    sizes = lifter.clip_batch_sizes(sum(wc.CLIP_FRAMES))
    assert sizes == [BATCH] * 3
    E = cp.extrinsic_dim if cp.camera_embedding else 0
    src, table, run_param, total = wc.eval_layout(J, F, rf, cp.causal, flip, sum(sizes) - sum(wc.CLIP_FRAMES), E=E)
    src = (0.3 * src).astype(np.float32)
    perm = wc.mirror_perm(J)
    x, param, status = wc.ref_windows(src, table, run_param, 0, sum(sizes), rf, perm)
    assert (status == 0).all() and not (x == wc.FILL).any()
    return src, table, run_param, total, sizes, perm, x, param


def device_call(src, table, run_param, window0, batch, rf, perm, pattern=NANS):
    """r3d_clips_windows with every buffer carved exact-sized out of one pattern-filled device allocation, x / param poisoned with
    FILL, status with FILL_STATUS -> (x, param or None, status); the guards are checked."""
    total, J, F = src.shape
    E = 0 if run_param is None else run_param.shape[1]
    arrays = [("src", src), ("table", np.array(table).view(np.uint8)), ("run_param", run_param if E else np.zeros(1, np.float32)),
              ("x", np.full((batch, rf, J, F), wc.FILL, np.float32)), ("param", np.full((batch, max(E, 1)), wc.FILL, np.float32)),
              ("status", np.full(len(table), wc.FILL_STATUS, np.int32))]
    arena = Arena("cuda:0", pattern, Arena.capacity_for([a.nbytes for _, a in arrays]))
    t = {n: arena.put(a, 256, 4 if n in ("src", "x") else 0, n)() for n, a in arrays}
    _capi.clips_windows(t["src"].data_ptr(), total, J, F, rf, t["table"].data_ptr(), len(table), t["run_param"].data_ptr() if E else None, E,
                        window0, batch, t["x"].data_ptr(), t["param"].data_ptr() if E else None, perm, t["status"].data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    arena.check()
    assert same_bits(t["src"].cpu().numpy(), src)
    return t["x"].cpu().numpy(), (t["param"].cpu().numpy() if E else None), t["status"].cpu().numpy()


def agree(dev, host):
    (x, p, s), (rc, hx, hp, hs) = dev, host
    _capi.use_hooks(False)
    return rc == 0 and same_bits(x, hx) and (p is None) == (hp is None) and (p is None or same_bits(p, hp)) and np.array_equal(s, hs)


# ------------------------------------------------------------------ the kernel against the host hook

@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_host_hook_bit_for_bit(name, flip):
    """Every batch of the pool - batches that start and end inside clips, the last one in surplus windows - and one launch past
    every run, which must leave everything untouched."""
    src, table, run_param, total, sizes, perm, x_ref, p_ref = pool(name, flip)
    rf = x_ref.shape[1]
    w0 = 0
    for b in sizes + [BATCH]:
        args = (src, table, run_param, w0, b, rf, perm if flip else None)
        got = device_call(*args)
        assert agree(got, host_call(*args)), (name, w0)
        if w0 < sum(sizes):
            assert same_bits(got[0], x_ref[w0:w0 + b]) and (p_ref is None or same_bits(got[1], p_ref[w0:w0 + b]))
        else:
            assert (got[0] == wc.FILL).all() and (got[2] == wc.FILL_STATUS).all()
        w0 += b


@pytest.mark.parametrize("J,F,rf", [(17, 3, 27), (14, 2, 9)])
def test_steps_order_gaps_and_payloads_equal_the_host_hook(J, F, rf):
    src, table, run_param, total = wc.scattered_layout(J, F, rf)
    perm = wc.mirror_perm(J)
    for w0, b in ((0, total), (3, 7), (total - 4, 9)):
        args = (src, table, run_param, w0, b, rf, perm)
        got = device_call(*args)
        assert agree(got, host_call(*args))
        assert same_bits(got[0], wc.ref_windows(*args)[0])


def test_invalid_runs_equal_the_host_hook():
    """Every kind of invalid descriptor in run 2: status 1, the run's windows keep their fill, everything else is the hook's."""
    J, F, rf = 17, 3, 9
    src, table, run_param, total = wc.eval_layout(J, F, rf, lengths=(4, 1, 6, 3, 9))
    perm, r = wc.mirror_perm(J), 2
    w0, w1 = int(table[r]["win_first"]), int(table[r]["win_first"] + table[r]["n_windows"])
    cases = [(name, bad, perm) for name, bad in wc.invalid_cases(table[r], src.shape[0]).items()]
    flipped = table[r].copy()
    flipped["flip"] = 1
    cases.append(("flip without mirror_perm", flipped, None))
    for name, bad, pm in cases:
        t = table.copy()
        t[r] = bad
        args = (src, t, run_param, 0, total, rf, pm)
        got = device_call(*args)
        assert agree(got, host_call(*args)), name
        assert got[2][r] == 1 and (np.delete(got[2], r) == 0).all() and (got[0][w0:w1] == wc.FILL).all() and (got[1][w0:w1] == wc.FILL).all(), name
    shuffled = table[[3, 0, 4, 2, 1]]                             # garbage order: whatever the bisection ends on, the hook ends on too
    args = (src, shuffled, run_param, 0, total, rf, perm)
    assert agree(device_call(*args), host_call(*args))


# ------------------------------------------------------------------ forward_windows

def _oracle(states, windows, prm):
    """pos + trj through oracle/torch_port.py (the PyTorch-CPU restatement, pinned to the reference fixtures)."""
    from oracle import torch_port
    (cp, sp), (ct, st) = states
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]
    xw = torch.from_numpy(windows)
    pw = torch.from_numpy(prm) if prm is not None else None
    with torch.no_grad():
        return (torch_port.forward(cp, sds[0], xw, pw) + torch_port.forward(ct, sds[1], xw, pw)).numpy()


@functools.lru_cache(maxsize=None)
def lifted(name, flip=False):
    """forward_windows over the fixture's pool -> (out (192, 1, J, 3), trj (192, 1, 1, 3)) as NumPy arrays."""
    lifter, _ = pair(name)
    src, table, run_param, total, sizes, perm, _, _ = pool(name, flip)
    dev = torch.device("cuda:0")
    J = src.shape[1]
    out = torch.full((sum(sizes), 1, J, 3), float("nan"), device=dev)
    trj = torch.full((sum(sizes), 1, 1, 3), float("nan"), device=dev)
    with torch.no_grad():
        res = lifter.forward_windows(torch.from_numpy(src).to(dev), torch.from_numpy(np.array(table).view(np.uint8)).to(dev), len(table),
                                     torch.from_numpy(run_param).to(dev) if run_param is not None else None, total, out, trj,
                                     perm=perm if flip else None)
    torch.cuda.synchronize()
    lifter.check_status(dev)
    assert res[0] is out and res[1] is trj
    return out.cpu().numpy(), trj.cpu().numpy()


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("name", FIXTURES)
def test_pooled_batches_have_the_bits_of_forward_and_agree_with_the_oracle(name, flip):
    """Each 64-window batch: the bits of lifter.forward on the same windows built on the host, at the same batch size (the same
    kernel on the same inputs).  Every window: the oracle chain at the literal 1e-4."""
    lifter, states = pair(name)
    _, _, _, total, sizes, _, x_ref, p_ref = pool(name, flip)
    out, trj = lifted(name, flip)
    dev = torch.device("cuda:0")
    w0 = 0
    for b in sizes:
        with torch.no_grad():
            want, want_trj = lifter.forward(torch.from_numpy(x_ref[w0:w0 + b]).to(dev),
                                            torch.from_numpy(p_ref[w0:w0 + b]).to(dev) if p_ref is not None else None, return_trj=True)
        assert same_bits(out[w0:w0 + b], want.cpu().numpy()) and same_bits(trj[w0:w0 + b], want_trj.cpu().numpy()), (name, w0)
        w0 += b
    ref = _oracle(states, x_ref[:total], p_ref[:total] if p_ref is not None else None)
    check_parity(out[:total], ref, "pooled windows vs oracle chain")


@pytest.mark.parametrize("name", FIXTURES)
def test_pooled_windows_agree_with_forward_clip(name):
    """Clip by clip against forward_clip on the edge-padded clip: 2e-5 * max(1, |out|), the clip-vs-materialised bound."""
    lifter, ((cp, _), _) = pair(name)
    src, table, run_param, total, _, _, _, _ = pool(name)
    out, _ = lifted(name)
    dev = torch.device("cuda:0")
    pad = (cp.receptive_field - 1) // 2
    for k, d in enumerate(table):
        first, n, w = int(d["first_frame"]), int(d["n_frames"]), int(d["win_first"])
        padded = torch.from_numpy(evaluate.pad_clip(src[first:first + n], pad, pad if cp.causal else 0)).to(dev)
        with torch.no_grad():
            want = lifter.forward_clip(padded, torch.from_numpy(run_param[k]).to(dev) if run_param is not None else None).cpu().numpy()
        check_parity(out[w:w + n], want, "clip of %d frames vs forward_clip (HIP against HIP)" % n, tol=2e-5 * max(1.0, float(np.abs(want).max())))


def test_a_refused_run_raises_and_lanes_raise():
    lifter, _ = pair("j17_rf27_s3")
    src, table, run_param, total, sizes, perm, _, _ = pool("j17_rf27_s3")
    dev = torch.device("cuda:0")
    bad = np.array(table)
    bad[3]["first_frame"] = src.shape[0]
    out = torch.empty((sum(sizes), 1, 17, 3), device=dev)
    args = (torch.from_numpy(src).to(dev), None, len(table), torch.from_numpy(run_param).to(dev), total, out)
    tab = lambda t: torch.from_numpy(t.view(np.uint8)).to(dev)      # noqa: E731
    with pytest.raises(RuntimeError, match=r"r3d_clips_windows refused the descriptors of runs \[3\]"):
        lifter.forward_windows(args[0], tab(bad), *args[2:])
    flipped = np.array(table)
    flipped["flip"] = 1
    with pytest.raises(RuntimeError, match="refused"):              # flip runs without perm=
        lifter.forward_windows(args[0], tab(flipped), *args[2:])
    with pytest.raises(ValueError, match="sum\\(clip_batch_sizes"):
        lifter.forward_windows(args[0], tab(np.array(table)), *args[2:5], out[:-1])
    lifter.check_status(dev)
    own, _ = pair.__wrapped__("j17_rf27_s3")                        # (a pair of its own: the lanes are an option of its handles)
    try:
        own.set_lanes(2, dev)
        with pytest.raises(ValueError, match="lanes"):
            own.forward_windows(args[0], tab(np.array(table)), *args[2:])
        clips = _mixed_clips()
        with pytest.raises(ValueError, match="lanes"):
            evaluate.evaluate_clips_batched(own.forward_clip, clips, 27, dev, pool_below=50)
    finally:
        own.set_lanes(0)


def test_captured_gather_and_forward_replay_with_the_eager_bits():
    """One batch - the gather into fixed buffers and the forward that reads them - captured into a hipGraph and replayed once."""
    import ray3d_amd
    name = "j17_rf27_s3"
    lifter, ((cp, _), _) = pair(name)
    src, table, run_param, total, sizes, perm, _, _ = pool(name, True)
    want, _ = lifted(name, True)
    dev = torch.device("cuda:0")
    J, F, rf, E = cp.num_joints, cp.in_features, cp.receptive_field, cp.extrinsic_dim
    s_dev, t_dev = torch.from_numpy(src).to(dev), torch.from_numpy(np.array(table).view(np.uint8)).to(dev)
    rp = torch.from_numpy(run_param).to(dev)
    x = torch.full((BATCH, rf, J, F), float("nan"), device=dev)
    p = torch.full((BATCH, E), float("nan"), device=dev)
    status = torch.full((len(table),), -1, dtype=torch.int32, device=dev)
    out = torch.full((BATCH, 1, J, 3), float("nan"), device=dev)
    lifter.prepare([BATCH])
    w0 = BATCH                                                       # the middle batch: it starts and ends inside clips
    g, s_ = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(s_):
            with torch.cuda.graph(g, stream=s_):
                evaluate.shard_windows_hip(s_dev, t_dev, len(table), rp, w0, BATCH, rf, x=x, param=p, perm=perm, status=status)
                lifter._run(ray3d_amd._capi.R3D_INPUT_RAYS, x, rf, BATCH, p, E, out=out)
        g.replay()
        torch.cuda.synchronize()
        lifter.check_status(dev)
        st = status.cpu().numpy()
        assert set(st.tolist()) == {-1, 0} and same_bits(out.cpu().numpy(), want[w0:w0 + BATCH])
    finally:
        del g
        torch.cuda.synchronize()
        lifter.release_prepared()


# ------------------------------------------------------------------ evaluate_clips_batched / predict_clips_batched (pool_below=)

@functools.lru_cache(maxsize=None)
def _lifter27():
    from test_gpu_clips_metrics import _lifter as make
    return make()


def _rows_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_pooled_evaluation_reproduces_the_reference_metrics(flip):
    """The recorded clips of tests/golden/evalcore.npz, all of them pooled: metrics_flip0 / metrics_flip1 within the bounds of
    test_evaluate_clips_reproduces_reference_metrics (0.05 mm, MPJPE 0.02 mm)."""
    from test_metrics_detail_host import evalcore_clips
    z = np.load(os.path.join(GOLDEN, "evalcore.npz"))
    lifter, dev = _lifter27(), torch.device("cuda:0")
    recorded = [evaluate.Clip(c.camera, c.rays, c.gt_norm, "A", c.clip_id) for c in evalcore_clips()]
    with torch.no_grad():
        named, _, rows = evaluate.evaluate_clips_batched(lifter.forward_clip, recorded, 27, dev, flip=flip, pool_below=10 ** 6,
                                                         kps_left=list(z["kps_left"]), kps_right=list(z["kps_right"]))
    got, ref = np.array(named["A"]), z["metrics_flip%d" % int(flip)]
    print("pool_below flip %d vs evalcore.npz: got" % flip, got, "ref", ref)
    assert torch.isfinite(rows).all()
    assert np.abs(got - ref).max() < 5e-2 and abs(got[0] - ref[0]) < 2e-2, (got, ref)


def _mixed_clips(pixels=False):
    """Clips of 1, 40 and 100 frames (tests/test_gpu_clips_encode.py: raw pixels; or their ray encoding)."""
    from test_clips_encode_host import host_encode
    from test_gpu_clips_encode import _pixel_clips
    px = _pixel_clips()
    if pixels:
        return px
    clips = [evaluate.Clip(c.camera, host_encode(c.camera, c.rays, "ray"), c.gt_norm, c.action, c.clip_id) for c in px]
    _capi.use_hooks(False)
    return clips


@pytest.mark.parametrize("encode", [None, "ray"], ids=["rays", "pixels"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_mixed_shard_keeps_the_bits_of_the_clips_that_are_not_pooled(flip, encode):
    """pool_below=50 on clips of 1, 40 and 100 frames: the 100-frame clip's row has the bits of pool_below=None (and of
    pool_below=0, and of finish=True), the pooled clips' per-frame means agree within the clip-vs-materialised bound."""
    lifter, dev = _lifter27(), torch.device("cuda:0")
    clips = _mixed_clips(pixels=encode is not None)
    lengths = [c.rays.shape[0] for c in clips]
    assert sorted(lengths) == [1, 40, 100]
    kw = dict(flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, encode=encode)
    with torch.no_grad():
        _, _, base = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, finish=True, **kw)
        _, _, none = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, finish=True, pool_below=None, **kw)
        _, _, zero = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, finish=True, pool_below=0, **kw)
        _, _, rows = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, pool_below=50, **kw)
        _, _, alone = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, pool_below=1, **kw)      # nothing is that short
    assert _rows_equal(none, base) and _rows_equal(zero, base) and _rows_equal(alone, base)
    assert torch.isfinite(rows[:, 3:6]).all()
    assert torch.equal(rows[:, :3], base[:, :3])                  # (clip id, action id, frames: the rows' own order)
    long = rows[:, 2].tolist().index(100.0)
    assert _rows_equal(rows[long], base[long])
    got, ref = (t[:, 3:].cpu().numpy() / t[:, 2:3].cpu().numpy() for t in (rows, base))
    fin = np.isfinite(ref)
    check_parity(got[fin], ref[fin], "pooled rows vs the per-clip rows (HIP against HIP)", tol=2e-5 * max(1.0, float(np.abs(ref[fin]).max())))


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_pooled_predictions_agree_with_the_per_clip_path(flip):
    """predict_clips_batched(pool_below=): poses and world poses within the clip-vs-materialised bound of the per-clip path's; the
    clip that is not pooled keeps its bits."""
    lifter, dev = _lifter27(), torch.device("cuda:0")
    clips = _mixed_clips()
    kw = dict(flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    with torch.no_grad():
        want = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, **kw)
        got = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, pool_below=50, **kw)
    torch.cuda.synchronize()
    for c, (p, w), (p0, w0) in zip(clips, got, want):
        n = c.rays.shape[0]
        assert p.shape == p0.shape == (n, 17, 3) and w.shape == w0.shape == (n, 17, 3) and w.dtype == torch.float64
        if n == 100:
            assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and torch.equal(w.view(torch.int64), w0.view(torch.int64))
        for a, b, what in ((p, p0, "poses"), (w, w0, "world poses")):
            b = b.cpu().numpy()
            check_parity(a.cpu().numpy(), b, "%s of the %d-frame clip vs the per-clip path (HIP against HIP)" % (what, n),
                         tol=2e-5 * max(1.0, float(np.abs(b).max())))
