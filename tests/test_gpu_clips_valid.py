"""-m gpu: r3d_clips_valid_losses - a whole shard's validation losses in one launch pair over the device-side clip table - bit
for bit against the per-clip call r3d_clip_valid_losses (the wrap-around of a clip above 128 x 256 frames and the reference's
Inf / NaN included), with invalid descriptors, inside guard bands with a poisoned scratch, captured in a hipGraph, and end to
end: forward_clip(trj_out=) and validate_clips_batched against validate_clips on the smallest model fixture."""
import functools

import numpy as np
import pytest
import torch

from buffers_util import NANS, Arena
from conftest import load_model_fixture, synth_states
import valid_oracle as vo
from test_clips_valid_host import DOUBLES, COUNT, GAP, LENGTHS, VARIANTS, clip_inputs, layout, with_invalid

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
WRAP = (128 * 256 + 257, 1)      # one sweep of the capped per-clip grid and 257 frames more (threads with two frames), next to one frame


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _capi_product():
    from ray3d_amd import _capi
    _capi.use_hooks(False)
    return _capi


def same_bits(a, b):
    """NaN matches NaN; everything else by its 64-bit pattern."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.view(torch.int64)[~na], b.view(torch.int64)[~nb]))


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda() if a is not None else None


def run_batched(J, table, pos, trj, gt, parents, flags, max_frames, row_stride=DOUBLES, frames=True, total=None, scratch_fill=None):
    """One r3d_clips_valid_losses call (product library) on device tensors; every output pre-filled with the sentinel.
    -> (rows (k, row_stride), frame table (total, 7) or None)."""
    _capi = _capi_product()
    k = table.shape[0]
    total = pos.shape[0] if total is None else total
    tab = torch.from_numpy(np.array(table).view(np.uint8)).cuda()
    rows = torch.full((k, row_stride), SENTINEL, dtype=torch.float64, device="cuda")
    fr = torch.full((total, COUNT), SENTINEL, dtype=torch.float64, device="cuda") if frames else None
    nbytes = _capi.clips_valid_scratch_bytes(k, max_frames)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if scratch_fill is not None:
        scratch.fill_(scratch_fill)
    _capi.clips_valid_losses(pos.data_ptr(), trj.data_ptr() if trj is not None else None, gt.data_ptr(), total, J, parents, flags,
                             tab.data_ptr(), k, max_frames, rows.data_ptr() + 8 * (row_stride - DOUBLES), row_stride,
                             fr.data_ptr() if frames else None, scratch.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    return rows, fr


@functools.lru_cache(maxsize=None)
def per_clip(J, variant, bones, lengths=LENGTHS):
    """Every clip alone through r3d_clip_valid_losses: [(the 71 results, the frame table)], on the host."""
    _capi = _capi_product()
    out = []
    for n in lengths:
        pos, trj, gt, flags = clip_inputs(n, J, variant)
        p, t, g = _dev(pos), _dev(trj), _dev(gt)
        sums = torch.full((_capi.VALID_OUT_DOUBLES,), SENTINEL, dtype=torch.float64, device="cuda")
        fr = torch.full((n, COUNT), SENTINEL, dtype=torch.float64, device="cuda")
        _capi.clip_valid_losses(p.data_ptr(), t.data_ptr() if t is not None else None, g.data_ptr(), n, J,
                                vo.tree_for(J) if bones else None, flags, sums.data_ptr(), fr.data_ptr(), _stream())
        torch.cuda.synchronize()
        out.append((sums[:DOUBLES].cpu(), fr.cpu()))
    return out


@functools.lru_cache(maxsize=None)
def batched(J, variant, bones, lengths=LENGTHS):
    table, pos_all, trj_all, gt_all, total, flags = layout(J, variant, lengths)
    rows, fr = run_batched(J, table, _dev(pos_all), _dev(trj_all), _dev(gt_all), vo.tree_for(J) if bones else None, flags, max(lengths))
    return rows.cpu(), fr.cpu()


def _check_equal(J, variant, bones, lengths):
    table, _, _, _, total, _ = layout(J, variant, lengths)
    rows, fr = batched(J, variant, bones, lengths)
    covered = torch.zeros(total, dtype=torch.bool)
    for c, (sums, frames) in enumerate(per_clip(J, variant, bones, lengths)):
        n, at = lengths[c], int(table[c]["first_frame"])
        assert same_bits(rows[c], sums), (J, variant, bones, n, rows[c], sums)
        assert same_bits(fr[at:at + n], frames), (J, variant, bones, n)
        covered[at:at + n] = True
    assert int((~covered).sum()) == GAP * (len(lengths) + 1)
    assert bool((fr[~covered] == SENTINEL).all())                                # the gaps' rows of the frame table: untouched
    return rows


@pytest.mark.parametrize("bones", [True, False], ids=["parents", "noparents"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("J", [1, 14, 17])
def test_bit_equal_to_the_per_clip_call(J, variant, bones):
    """Clips of 1, 2, 63, 64, 65, 255, 256, 257 and 513 frames, shuffled with gaps, max_frames = 513: the 71 results and the frame
    rows of every clip are those of r3d_clip_valid_losses on that clip alone - the Inf of the frame with a zero root depth (the
    65-frame clip), the NaN of the zero-length bone (the 257-frame clip) and of the one-joint tree's empty bone mean included."""
    assert max(LENGTHS) == 513
    rows = _check_equal(J, variant, bones, LENGTHS)
    if variant in ("trj", "sum"):
        assert bool(torch.isinf(rows[LENGTHS.index(65), 3]))                     # TRJ_WSUM: 1 / 0
    if bones and J > 2:
        assert bool(torch.isnan(rows[LENGTHS.index(257), 6])) and bool(torch.isfinite(rows[LENGTHS.index(256)]).all())
    if bones and J == 1:
        assert bool(torch.isnan(rows[:, 5]).all())
    if not bones:
        assert bool((rows[:, 5:] == 0.0).all())


def test_a_clip_above_one_sweep_of_the_per_clip_grid_wraps_the_same_way():
    """128 x 256 + 257 frames next to a one-frame clip, J 17: the per-clip call wraps round its 128 workgroups, the batched one
    assigns frames from the clip's own n_frames - the same partial rows, added in the same order."""
    rows = _check_equal(17, "sum", True, WRAP)
    assert bool(torch.isfinite(rows).all())
    # a larger bound (the same 128 workgroups per clip) moves nothing
    table, pos_all, trj_all, gt_all, total, flags = layout(17, "sum", WRAP)
    loose, _ = run_batched(17, table, _dev(pos_all), _dev(trj_all), _dev(gt_all), vo.H36M, flags, 10 ** 6, frames=False)
    assert same_bits(loose, rows)


def test_invalid_descriptors_are_not_followed():
    """n_frames < 1, n_frames > max_frames, a range past total_frames, a range in front of 0 (and ranges far outside) between
    valid clips, every input inside guard bands of NaN pattern: NaN rows, their frame rows and the columns between the strided
    rows keep the fill, the valid clips as in the first test, nothing outside the buffers touched."""
    table, pos_all, trj_all, gt_all, total, flags = layout(17, "sum")
    keep = [LENGTHS.index(n) for n in (1, 65, 257, 513)]
    mixed, src = with_invalid(table, total, 513, keep)
    arena = Arena("cuda", NANS, Arena.capacity_for([pos_all.nbytes, trj_all.nbytes, gt_all.nbytes, mixed.nbytes]))
    p, t, g = arena.put(pos_all, name="pos")(), arena.put(trj_all, name="trj")(), arena.put(gt_all, name="gt")()
    rows, fr = run_batched(17, mixed, p, t, g, vo.H36M, flags, 513, row_stride=DOUBLES + 3)
    arena.check()
    rows, fr = rows.cpu(), fr.cpu()
    ref_rows, ref_fr = batched(17, "sum", True)
    assert bool((rows[:, :3] == SENTINEL).all())
    touched = torch.zeros(total, dtype=torch.bool)
    for i, c in enumerate(src):
        if c is None:
            assert bool(torch.isnan(rows[i, 3:]).all()), (i, mixed[i], rows[i])
        else:
            at, n = int(table[c]["first_frame"]), LENGTHS[c]
            assert same_bits(rows[i, 3:], ref_rows[c]) and same_bits(fr[at:at + n], ref_fr[at:at + n])
            touched[at:at + n] = True
    assert sum(c is None for c in src) == 8 and bool((fr[~touched] == SENTINEL).all())


def test_guard_bands_strided_rows_and_poisoned_scratch():
    """pos, trj, gt, the table, the strided row matrix, the frame table and the scratch are exact-size regions of one arena (the
    float inputs 4 bytes off their alignment); the scratch is sized by r3d_clips_valid_scratch_bytes and filled with NaNs, then
    with zeros: the same outputs, bit for bit - those of the first test - and not a byte outside the regions written, nor
    between the rows.  One byte less of scratch: R3D_ERR_WORKSPACE, the rows untouched."""
    _capi = _capi_product()
    table, pos_all, trj_all, gt_all, total, flags = layout(17, "trj")
    k, max_frames, stride = len(LENGTHS), max(LENGTHS), DOUBLES + 5
    nbytes = _capi.clips_valid_scratch_bytes(k, max_frames)
    assert nbytes == k * 3 * DOUBLES * 8
    sizes = dict(rows=((k - 1) * stride + DOUBLES) * 8, frames=total * COUNT * 8, scratch=nbytes)
    arena = Arena("cuda", NANS, Arena.capacity_for([pos_all.nbytes, trj_all.nbytes, gt_all.nbytes, table.nbytes] + list(sizes.values())))
    puts = [arena.put(a, skew=4, name=name) for a, name in ((pos_all, "pos"), (trj_all, "trj"), (gt_all, "gt"))]
    put_t = arena.put(np.array(table).view(np.uint8), name="table")
    out = {name: arena.carve(sz, name=name) for name, sz in sizes.items()}
    results = []

    def call(scratch_bytes):
        p, t, g = (w() for w in puts)
        tab = put_t()
        assert p.data_ptr() % 8 == 4 and t.data_ptr() % 8 == 4 and g.data_ptr() % 8 == 4 and tab.data_ptr() % 8 == 0
        return _capi.load().r3d_clips_valid_losses(p.data_ptr(), t.data_ptr(), g.data_ptr(), total, 17, _capi._parent_table(vo.H36M), flags,
                                                   tab.data_ptr(), k, max_frames, out["rows"].data_ptr(), stride, out["frames"].data_ptr(),
                                                   out["scratch"].data_ptr(), scratch_bytes, _stream())

    for word in (-1, 0):                                    # a NaN pattern, then zeros
        arena.refill(NANS)
        for name in ("rows", "frames"):
            out[name].view(torch.float64).fill_(SENTINEL)
        out["scratch"].view(torch.int32).fill_(word)
        assert call(nbytes) == 0                           # exactly r3d_clips_valid_scratch_bytes suffices
        arena.check()
        results.append((out["rows"].view(torch.float64).clone().cpu(), out["frames"].view(torch.float64).clone().cpu()))
    (rows_a, fr_a), (rows_b, fr_b) = results
    assert same_bits(rows_a, rows_b) and same_bits(fr_a, fr_b)
    ref_rows, ref_fr = batched(17, "trj", True)
    assert same_bits(fr_a.view(total, COUNT), ref_fr)
    flat = torch.cat([rows_a, torch.full((stride - DOUBLES,), SENTINEL, dtype=torch.float64)]).view(k, stride)
    assert same_bits(flat[:, :DOUBLES], ref_rows) and bool((flat[:-1, DOUBLES:] == SENTINEL).all())     # nothing between the rows
    # one byte less: refused before any launch
    out["rows"].view(torch.float64).fill_(SENTINEL)
    assert call(nbytes - 1) == _capi.R3D_ERR_WORKSPACE
    arena.check()
    assert bool((out["rows"].view(torch.float64) == SENTINEL).all())


@pytest.mark.parametrize("variant", ("sum", "rel"))
def test_two_runs_are_identical_and_the_frame_table_is_optional(variant):
    table, pos_all, trj_all, gt_all, total, flags = layout(14, variant)
    p, t, g = _dev(pos_all), _dev(trj_all), _dev(gt_all)
    rows, fr = batched(14, variant, True)
    rows2, fr2 = run_batched(14, table, p, t, g, vo.tree_for(14), flags, 513, scratch_fill=0xFF)
    assert same_bits(rows2, rows) and same_bits(fr2, fr)
    rows3, none = run_batched(14, table, p, t, g, vo.tree_for(14), flags, 513, frames=False)      # frame_dev = NULL
    assert none is None and same_bits(rows3, rows)


def test_captured_in_a_hip_graph():
    """r3d_clips_valid_losses captured with torch.cuda.graph (default queue settings) - two launches, no copy, no allocation, no
    synchronisation - and replayed twice: the rows and the frame table of the eager call."""
    _capi = _capi_product()
    table, pos_all, trj_all, gt_all, total, flags = layout(17, "sum")
    k, max_frames = len(LENGTHS), 513
    p, t, g = _dev(pos_all), _dev(trj_all), _dev(gt_all)
    tab = torch.from_numpy(np.array(table).view(np.uint8)).cuda()
    rows = torch.full((k, DOUBLES), SENTINEL, dtype=torch.float64, device="cuda")
    fr = torch.full((total, COUNT), SENTINEL, dtype=torch.float64, device="cuda")
    nbytes = _capi.clips_valid_scratch_bytes(k, max_frames)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    want_rows, want_fr = batched(17, "sum", True)          # (eager: the kernels are loaded before the capture)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            _capi.clips_valid_losses(p.data_ptr(), t.data_ptr(), g.data_ptr(), total, 17, vo.H36M, flags, tab.data_ptr(), k, max_frames,
                                     rows.data_ptr(), DOUBLES, fr.data_ptr(), scratch.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        rows.fill_(SENTINEL)
        fr.fill_(SENTINEL)
        scratch.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(rows, want_rows) and same_bits(fr, want_fr)
    del graph
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end on the smallest model fixture

RF = 9


def _make_lifter():
    import ray3d_amd
    _capi_product()
    z, mc = load_model_fixture("j17_rf9_s1")
    (cp, sp), (ct, st) = synth_states(mc)
    assert cp.receptive_field == RF
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos_m, trj_m = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos_m, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj_m, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos_m.eval(), trj_m.eval()
    return ray3d_amd.Ray3DLifter(pos_m, trj_m).eval(), cp


@functools.lru_cache(maxsize=None)
def _lifter():
    return _make_lifter()


@pytest.mark.parametrize("n", [1, 33, 4200])
def test_forward_clip_trj_out_equals_forward_clip(n):
    """An exact call (1), one rounded up past the clip's end (33 -> 64: through the scratch tensors) and two calls whose second
    overhangs (4200 -> 2176 + 2048): poses and trajectory written into slices have the bits of the call without them."""
    from ray3d_amd import synth
    lifter, cp = _lifter()
    dev = torch.device("cuda:0")
    assert sum(lifter.clip_batch_sizes(n)) == {1: 1, 33: 64, 4200: 4224}[n]
    rays = synth.synth_rays(n + RF - 1, cp, seed=n)[:, 0]
    clip = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
    prow = torch.from_numpy(vo.stub_camera().param()).to(dev)
    buf = torch.full((n + 5, 1, 17, 3), SENTINEL, dtype=torch.float32, device=dev)
    tbuf = torch.full((n + 5, 1, 1, 3), SENTINEL, dtype=torch.float32, device=dev)
    with torch.no_grad():
        want, want_trj = lifter.forward_clip(clip, prow, return_trj=True)
        got, got_trj = lifter.forward_clip(clip, prow, return_trj=True, out=buf[2:2 + n], trj_out=tbuf[3:3 + n])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf[2:].data_ptr() and got_trj.data_ptr() == tbuf[3:].data_ptr()
    assert torch.isfinite(want).all() and torch.isfinite(want_trj).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got_trj.view(torch.int32), want_trj.view(torch.int32))
    assert bool((buf[:2] == SENTINEL).all()) and bool((buf[2 + n:] == SENTINEL).all())
    assert bool((tbuf[:3] == SENTINEL).all()) and bool((tbuf[3 + n:] == SENTINEL).all())
    with pytest.raises(ValueError, match="return_trj"):
        lifter.forward_clip(clip, prow, out=buf[2:2 + n], trj_out=tbuf[3:3 + n])
    with pytest.raises(ValueError, match="trj_out"):
        lifter.forward_clip(clip, prow, return_trj=True, trj_out=tbuf[:n + 1])


E2E_LENGTHS = (1, 12, 33, 40, 64, 100)


def _ray_clips(cp):
    """Six short clips over two actions: seeded rays, ground truth with its root 4 m deep (every figure finite)."""
    from ray3d_amd import evaluate, synth
    rng = np.random.default_rng(21)
    clips = []
    for k, n in enumerate(E2E_LENGTHS):
        rays = np.ascontiguousarray(synth.synth_rays(n, cp, seed=40 + k)[:, 0])
        gt = rng.normal(0, 0.4, (n, 17, 3)).astype(np.float32)
        gt[:, :, 2] += np.float32(4.0)
        clips.append(evaluate.Clip(vo.stub_camera(), rays, gt, "AB"[k % 2], k))
    return clips


def _pair_lift(lifter):
    return functools.partial(lifter.forward_clip, return_trj=True)


def _assert_same_tables(a, b):
    assert a == b, {k: (a[k], b[k]) for k in a if a[k] != b[k]}


def test_validate_clips_batched_equals_validate_clips():
    from ray3d_amd import evaluate, skeleton
    lifter, cp = _lifter()
    dev = torch.device("cuda:0")
    clips = _ray_clips(cp)
    kw = dict(bone_pairs=skeleton.H36M_17_BONE_PAIRS)
    with torch.no_grad():
        table, rows = evaluate.validate_clips(lambda p, q: lifter.forward_clip(p, q, return_trj=True), clips, RF, dev, **kw)
        table_b, rows_b = evaluate.validate_clips_batched(_pair_lift(lifter), clips, RF, dev, **kw)
    torch.cuda.synchronize()
    assert rows_b.is_cuda and rows_b.shape == (6, evaluate.VALID_COLS) and bool(torch.isfinite(rows).all())
    assert torch.equal(rows_b.view(torch.int64), rows.view(torch.int64))
    assert rows_b[:, 2].tolist() == [float(n) for n in E2E_LENGTHS]
    _assert_same_tables(table_b, table)
    assert table["frames"] == sum(E2E_LENGTHS) and table["valid_mm"] > 0.0
    # the separately computed pos (pos_is_sum=False reads the buffer as the pos network's output): both paths alike
    with torch.no_grad():
        t2, r2 = evaluate.validate_clips(lambda p, q: lifter.forward_clip(p, q, return_trj=True), clips, RF, dev, pos_is_sum=False)
        t2b, r2b = evaluate.validate_clips_batched(_pair_lift(lifter), clips, RF, dev, pos_is_sum=False)
    assert torch.equal(r2b.view(torch.int64), r2.view(torch.int64)) and not torch.equal(r2b, rows_b)
    _assert_same_tables(t2b, t2)


def test_validate_clips_batched_on_two_lanes():
    """set_lanes(2): the clips are dealt to the lanes and joined once before the metrics call.  Both lanes have the same number
    of CUs and so the same tile schedules: the rows are, bit for bit, those of validate_clips on the same lifter with its lanes."""
    from ray3d_amd import evaluate
    lifter, cp = _make_lifter()                                      # (a pair of its own: the lanes are an option of its handles)
    dev = torch.device("cuda:0")
    clips = _ray_clips(cp)

    def lift_joined(padded, prow):       # (a forward from the caller's stream is relayed to a lane: its result is ordered behind join_lanes)
        res = lifter.forward_clip(padded, prow, return_trj=True)
        lifter.join_lanes()
        return res

    with torch.no_grad():
        lifter.set_lanes(2, dev)
        try:
            table, rows = evaluate.validate_clips(lift_joined, clips, RF, dev)
            torch.cuda.synchronize()
            table_b, rows_b = evaluate.validate_clips_batched(_pair_lift(lifter), clips, RF, dev)
            torch.cuda.synchronize()
            lifter.check_status()
        finally:
            lifter.set_lanes(0)
    assert bool(torch.isfinite(rows).all()) and torch.equal(rows_b.view(torch.int64), rows.view(torch.int64))
    _assert_same_tables(table_b, table)


def test_validate_clips_batched_from_raw_pixels_of_a_distorted_camera():
    """encode="ray": Clip.rays holds raw pixels of distorted H36M cameras; one r3d_clips_encode call feeds every forward.  The
    per-clip reference is validate_clips on clips that hold THE SAME encoded values: the encoder's own output for the unpadded
    frames (a padding row has the bits of the frame it repeats, tests/test_gpu_clips_encode.py), which the host chain of
    ray3d_amd/camera.py reproduces within one float32 ulp (checked here) - not bit for bit, so the host chain's values
    themselves cannot serve a bit-for-bit comparison of the rows."""
    from ray3d_amd import _capi, evaluate
    from test_clips_encode_host import cameras, host_encode, pixels, ulps
    lifter, cp = _lifter()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(22)
    clips, encoded = [], []
    for k, n in enumerate(E2E_LENGTHS):
        cam = cameras()[k % 4]                                       # the four distorted ones
        assert cam.cam_row(distortion=True)[8:13].any()
        px = pixels("clips_valid.eval.%d" % k, (n, 17, 2))
        gt = rng.normal(0, 0.4, (n, 17, 3)).astype(np.float32)
        gt[:, :, 2] += np.float32(4.0)
        clips.append(evaluate.Clip(cam, px, gt, "AB"[k % 2], k))
        itable = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
        itable[0]["n_frames"], itable[0]["cam"] = n, cam.cam_row(distortion=True)
        x, _, status = evaluate.shard_encode_hip(torch.from_numpy(px).to(dev), torch.from_numpy(itable.view(np.uint8)).to(dev), 1, n, n, "ray")
        assert int(status[0]) == 0
        rays = x.cpu().numpy()
        assert ulps(rays, host_encode(cam, px, "ray")) <= 1
        encoded.append(evaluate.Clip(cam, rays, gt, "AB"[k % 2], k))
    with torch.no_grad():
        table, rows = evaluate.validate_clips(lambda p, q: lifter.forward_clip(p, q, return_trj=True), encoded, RF, dev)
        table_b, rows_b = evaluate.validate_clips_batched(_pair_lift(lifter), clips, RF, dev, encode="ray")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rows).all()) and torch.equal(rows_b.view(torch.int64), rows.view(torch.int64))
    _assert_same_tables(table_b, table)
    with pytest.raises(ValueError, match="encode"):
        evaluate.validate_clips_batched(_pair_lift(lifter), clips, RF, dev, encode="rays")
    with pytest.raises(ValueError, match="forward_clip"):
        evaluate.validate_clips_batched(lambda *a, **k: None, clips, RF, dev, encode="ray")


@pytest.mark.parametrize("gt_root_relative", [False, True], ids=["abs", "rel"])
def test_validate_clips_batched_without_a_trajectory_model(gt_root_relative):
    """lift_clip returns the poses alone (and ignores trj_out): no trajectory buffer reaches the call, POS_IS_SUM is dropped."""
    from ray3d_amd import evaluate
    lifter, cp = _lifter()
    dev = torch.device("cuda:0")
    clips = _ray_clips(cp)
    poses_only = lambda x, p, out=None, trj_out=None, **kw: lifter.forward_clip(x, p, out=out, **kw)
    with torch.no_grad():
        table, rows = evaluate.validate_clips(lambda p, q: lifter.forward_clip(p, q), clips, RF, dev, gt_root_relative=gt_root_relative)
        table_b, rows_b = evaluate.validate_clips_batched(poses_only, clips, RF, dev, gt_root_relative=gt_root_relative)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rows).all()) and torch.equal(rows_b.view(torch.int64), rows.view(torch.int64))
    assert bool((rows_b[:, 3 + 2:3 + 5] == 0.0).all()) and torch.equal(rows_b[:, 3], rows_b[:, 4])      # no trajectory terms; POS == LOSS
    _assert_same_tables(table_b, table)
