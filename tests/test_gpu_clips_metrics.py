"""-m gpu: r3d_clips_metrics - a whole shard of clips measured in one launch pair over a device-side table - bit for bit
against the per-clip calls r3d_clip_metrics / r3d_clip_metrics_detail, against the float64 NumPy oracle (oracle/metrics_oracle.py,
the detail oracle of tests/test_metrics_detail_host.py), with invalid descriptors, inside guard bands with a poisoned scratch,
and end to end through evaluate_clips_batched."""
import functools
import warnings

import numpy as np
import pytest
import torch

from buffers_util import NANS, ZEROS, Arena
from conftest import synth_states
from test_metrics_detail_host import ROW, close, evalcore_clips, make_case, near_clips, threshold_margin

pytestmark = pytest.mark.gpu

# one frame (velocity NaN), one difference, the sizes around a wavefront and a workgroup, more than one workgroup, and a clip
# above the 128 x 256 frames of one sweep of the per-clip grid (the workgroups wrap around)
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 33068)
SHORT = LENGTHS[:-1]
GAP = 37                 # frames between two of the stored clips that belong to no clip (NaN: nothing may read them)
SENTINEL = -7.0


def _bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def layout(J, lengths):
    """The clips (tests/test_metrics_detail_host.make_case: seeded poses, a random rigid transform each, their oracle) stored in
    a shuffled order with a gap behind the second stored one; the table names them in the order of `lengths`."""
    from ray3d_amd import _capi
    cases = [make_case(n, J) for n in lengths]
    store = np.random.default_rng(7 + J).permutation(len(lengths))
    first, at = {}, 0
    for pos, c in enumerate(store):
        first[int(c)] = at
        at += lengths[c] + (GAP if pos == 1 else 0)
    total = at
    pred = np.full((total, J, 3), np.nan, np.float32)
    gt = np.full((total, J, 3), np.nan, np.float32)
    table = np.zeros(len(lengths), dtype=_capi.clip_desc_dtype())
    for c, (p, g, R, T, _) in enumerate(cases):
        pred[first[c]:first[c] + lengths[c]], gt[first[c]:first[c] + lengths[c]] = p, g
        table[c]["first_frame"], table[c]["n_frames"] = first[c], lengths[c]
        table[c]["rn2w"], table[c]["tn2w"] = R.reshape(9), T
    assert sorted(first.values()) != [first[c] for c in range(len(lengths))]          # really shuffled
    for v in (pred, gt, table):
        v.setflags(write=False)
    return cases, table, pred, gt, total


def run_batched(pred, gt, table, J, max_frames, row_stride=5, detail=True, frames=True, total=None):
    """One r3d_clips_metrics call on device tensors; every output pre-filled with the sentinel.
    -> (rows (k, row_stride), detail rows (k, 82) or None, frame table (total, 5) or None)."""
    from ray3d_amd import _capi
    k = table.shape[0]
    total = pred.shape[0] if total is None else total
    tab = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    rows = torch.full((k, row_stride), SENTINEL, dtype=torch.float64, device="cuda")
    det = torch.full((k, _capi.DETAIL_DOUBLES), SENTINEL, dtype=torch.float64, device="cuda") if detail else None
    fr = torch.full((total, 5), SENTINEL, dtype=torch.float64, device="cuda") if frames else None
    nbytes = _capi.clips_metrics_scratch_bytes(k, max_frames, detail)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _capi.clips_metrics(pred.data_ptr(), gt.data_ptr(), total, J, tab.data_ptr(), k, max_frames,
                        rows.data_ptr() + 8 * (row_stride - 5), row_stride, det.data_ptr() if detail else None, _capi.DETAIL_DOUBLES,
                        fr.data_ptr() if frames else None, scratch.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    return rows, det, fr


@functools.lru_cache(maxsize=None)
def per_clip(J, lengths):
    """Every clip alone through r3d_clip_metrics and r3d_clip_metrics_detail: [(plain sums, sums, detail row, frame table)]."""
    from ray3d_amd import _capi
    out = []
    for p, g, R, T, _ in layout(J, lengths)[0]:
        pd, gd = torch.from_numpy(np.array(p)).cuda(), torch.from_numpy(np.array(g)).cuda()
        n = pd.shape[0]
        plain = torch.full((_capi.METRIC_OUT_DOUBLES,), SENTINEL, dtype=torch.float64, device="cuda")
        sums = torch.full((_capi.METRIC_OUT_DOUBLES,), SENTINEL, dtype=torch.float64, device="cuda")
        det = torch.full((_capi.DETAIL_OUT_DOUBLES,), SENTINEL, dtype=torch.float64, device="cuda")
        fr = torch.full((n, 5), SENTINEL, dtype=torch.float64, device="cuda")
        _capi.clip_metrics(pd.data_ptr(), gd.data_ptr(), n, J, R, T, plain.data_ptr(), _stream())
        _capi.clip_metrics_detail(pd.data_ptr(), gd.data_ptr(), n, J, R, T, sums.data_ptr(), fr.data_ptr(), det.data_ptr(), _stream())
        torch.cuda.synchronize()
        out.append((plain[:5].clone(), sums[:5].clone(), det[:_capi.DETAIL_DOUBLES].clone(), fr))
    return out


@functools.lru_cache(maxsize=None)
def batched(J, lengths):
    _, table, pred, gt, _ = layout(J, lengths)
    return run_batched(torch.from_numpy(np.array(pred)).cuda(), torch.from_numpy(np.array(gt)).cuda(), table, J, max(lengths))


CASES = [(17, LENGTHS), (14, SHORT), (15, SHORT)]


@pytest.mark.parametrize("J,lengths", CASES, ids=["J17", "J14", "J15"])
def test_bit_equal_to_the_per_clip_calls(J, lengths):
    _, table, _, _, total = layout(J, lengths)
    rows, det, fr = batched(J, lengths)
    covered = torch.zeros(total, dtype=torch.bool)
    for c, (plain, sums, drow, frames) in enumerate(per_clip(J, lengths)):
        n, at = lengths[c], int(table[c]["first_frame"])
        assert same_bits(rows[c], plain), (J, n, rows[c], plain)                 # the NaN of a one-frame clip has the same bits
        assert same_bits(rows[c], sums), (J, n)
        assert same_bits(det[c], drow), (J, n)
        assert same_bits(fr[at:at + n], frames), (J, n)
        assert bool(torch.isnan(rows[c, 3])) == (n == 1) and not bool(torch.isnan(rows[c, [0, 1, 2, 4]]).any())
        covered[at:at + n] = True
    assert int((~covered).sum()) == GAP
    assert bool((fr.cpu()[~covered] == SENTINEL).all())                          # the gap's rows of the frame table: untouched


def test_five_sums_alone_and_strided_into_the_partial_row_matrix():
    """detail_dev = frame_dev = NULL: the same five sums; row_stride 8 through a pointer to column 3 of a (k, 8) matrix: columns
    0..2 of every row keep what they held."""
    _, table, pred, gt, _ = layout(17, LENGTHS)
    p, g = torch.from_numpy(np.array(pred)).cuda(), torch.from_numpy(np.array(gt)).cuda()
    rows, _, _ = batched(17, LENGTHS)
    only, none_d, none_f = run_batched(p, g, table, 17, max(LENGTHS), detail=False, frames=False)
    assert none_d is None and none_f is None and same_bits(only, rows)
    wide, det8, fr8 = run_batched(p, g, table, 17, max(LENGTHS), row_stride=8)
    assert wide.shape == (len(LENGTHS), 8) and same_bits(wide[:, 3:], rows)
    assert bool((wide[:, :3] == SENTINEL).all())
    assert same_bits(det8, batched(17, LENGTHS)[1]) and same_bits(fr8, batched(17, LENGTHS)[2])
    # a larger max_frames (a larger grid, more scratch per clip) moves nothing
    loose, det_l, _ = run_batched(p, g, table, 17, 40000)
    assert same_bits(loose, rows) and same_bits(det_l, det8)


def _oracle_sums(pw, gw):
    """The five sums of one clip by the reference's formulas (oracle/metrics_oracle.py), frame-count weighted (trainer.py:386-395)."""
    from oracle import metrics_oracle as mo
    n = pw.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                          # the empty mean of a one-frame clip
        vel = mo.mean_velocity_error(pw, gw) if n > 1 else float("nan")
    return np.array([n * mo.mpjpe(pw, gw), n * mo.p_mpjpe(pw, gw), n * mo.n_mpjpe(pw[:, None], gw[:, None]), n * vel,
                     n * mo.mpjpe(pw[:, :1], gw[:, :1])])


@pytest.mark.parametrize("J,lengths", CASES, ids=["J17", "J14", "J15"])
def test_against_the_float64_numpy_oracle(J, lengths):
    """Per clip within 1e-9 * max(1, |want|) - the bound tests/test_gpu_metrics_detail.py uses for the same arithmetic; the
    counts exactly.  Nothing here goes through the per-clip kernels."""
    cases, table, _, _, _ = layout(J, lengths)
    rows, det, fr = (t.cpu().numpy() for t in batched(J, lengths))
    for c, (p, g, R, T, want) in enumerate(cases):
        n, at = lengths[c], int(table[c]["first_frame"])
        pw = p.astype(np.float64) @ R.T + T.reshape(1, 1, 3)
        gw = g.astype(np.float64) @ R.T + T.reshape(1, 1, 3)
        sums = _oracle_sums(pw, gw)
        print("J %d n %5d: five sums |err| %s" % (J, n, np.abs(rows[c] - sums)))
        if n == 1:
            assert np.isnan(rows[c, 3]) and np.isnan(sums[3])
            assert close(np.delete(rows[c], 3), np.delete(sums, 3))
        else:
            assert close(rows[c], sums), (J, n, rows[c], sums)
        assert close(fr[at:at + n], want["frames"]) and fr[at + n - 1, 3] == 0.0
        joints = det[c, :3 * ROW].reshape(3, ROW)
        assert close(joints[:, :J], want["joints"]) and np.all(joints[:, J:] == 0.0)
        assert threshold_margin(want["rel"]) > 1e-12
        assert np.array_equal(det[c, 3 * ROW:], want["counts"].astype(np.float64))


def _arena_for(arrays, extra=()):
    return Arena("cuda", NANS, Arena.capacity_for([a.nbytes for a in arrays] + list(extra)))


def test_invalid_descriptors_are_not_followed():
    """n_frames 0, n_frames > max_frames, a range one frame past total_frames, a negative first_frame (and a negative n_frames, a
    first_frame near INT64_MAX) between valid clips: NaN rows, their frame rows untouched, the valid clips as in the first test,
    nothing outside pred / gt touched (guard bands; a read outside would also meet the arena's NaN pattern)."""
    from ray3d_amd import _capi
    _, table, pred, gt, total = layout(17, LENGTHS)
    keep = [c for c, n in enumerate(LENGTHS) if n in (1, 65, 257, 513)]
    max_frames = 513
    R, T = np.eye(3).reshape(9), np.zeros(3)
    bad = [(5, 0), (0, 514), (total - 99, 100), (-1, 50), (10, -5), (2 ** 63 - 1, 3), (total, 1)]
    is_bad = [True, False, True, False, True, False, True, False, True, True, True]
    mixed = np.zeros(len(is_bad), dtype=table.dtype)
    nb = nv = 0
    for i, b in enumerate(is_bad):
        if b:
            mixed[i]["first_frame"], mixed[i]["n_frames"], mixed[i]["rn2w"], mixed[i]["tn2w"] = bad[nb][0], bad[nb][1], R, T
            nb += 1
        else:
            mixed[i] = table[keep[nv]]
            nv += 1
    assert nb == len(bad) and nv == len(keep) == 4
    arena = _arena_for([pred, gt])
    p, g = arena.put(pred, name="pred")(), arena.put(gt, name="gt")()
    rows, det, fr = run_batched(p, g, mixed, 17, max_frames, total=total)
    arena.check()
    ref_rows, ref_det, ref_fr = batched(17, LENGTHS)
    touched = torch.zeros(total, dtype=torch.bool)
    v = 0
    for i, b in enumerate(is_bad):
        if b:
            assert bool(torch.isnan(rows[i]).all()) and bool(torch.isnan(det[i]).all()), (i, rows[i])
        else:
            c = keep[v]
            v += 1
            at, n = int(table[c]["first_frame"]), LENGTHS[c]
            assert same_bits(rows[i], ref_rows[c]) and same_bits(det[i], ref_det[c]) and same_bits(fr[at:at + n], ref_fr[at:at + n])
            touched[at:at + n] = True
    assert bool((fr.cpu()[~touched] == SENTINEL).all())       # the fill pattern wherever no valid clip lies
    assert _capi.DETAIL_DOUBLES == det.shape[1]


def test_guard_bands_and_poisoned_scratch():
    """Every buffer of the call an exact-size region of one arena (pred and gt 4 bytes off their alignment), the scratch sized
    by r3d_clips_metrics_scratch_bytes and filled with zeros, then with NaNs: the same outputs, bit for bit - those of the first
    test - and not a byte outside the regions written."""
    from ray3d_amd import _capi
    _, table, pred, gt, total = layout(17, LENGTHS)
    k, max_frames = len(LENGTHS), max(LENGTHS)
    nbytes = _capi.clips_metrics_scratch_bytes(k, max_frames, True)
    assert nbytes == k * 128 * (5 + 82) * 8
    sizes = dict(rows=k * 5 * 8, detail=k * _capi.DETAIL_DOUBLES * 8, frames=total * 5 * 8, scratch=nbytes)
    arena = _arena_for([pred, gt, table], sizes.values())
    put_p, put_g = arena.put(pred, skew=4, name="pred"), arena.put(gt, skew=4, name="gt")
    put_t = arena.put(table.view(np.uint8), name="table")
    out = {name: arena.carve(sz, name=name) for name, sz in sizes.items()}
    results = []
    for pattern in (ZEROS, NANS):
        arena.refill(NANS)
        p, g, t = put_p(), put_g(), put_t()
        assert p.data_ptr() % 8 == 4 and g.data_ptr() % 8 == 4
        for name in ("rows", "detail", "frames"):
            out[name].view(torch.float64).fill_(SENTINEL)
        out["scratch"].view(torch.int32).fill_(0 if pattern == ZEROS else -1)
        _capi.clips_metrics(p.data_ptr(), g.data_ptr(), total, 17, t.data_ptr(), k, max_frames, out["rows"].data_ptr(), 5,
                            out["detail"].data_ptr(), _capi.DETAIL_DOUBLES, out["frames"].data_ptr(),
                            out["scratch"].data_ptr(), nbytes, _stream())
        arena.check()
        results.append(tuple(out[name].view(torch.float64).clone() for name in ("rows", "detail", "frames")))
    for a, b in zip(*results):
        assert same_bits(a, b)
    ref = batched(17, LENGTHS)
    for got, want in zip(results[0], ref):
        assert same_bits(got, want.reshape(-1))


# ------------------------------------------------------------------ end to end

H36M_LEFT, H36M_RIGHT = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]


@functools.lru_cache(maxsize=None)
def _lifter():
    import ray3d_amd
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    (_, sp), (_, st) = synth_states(mc)
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos.eval(), trj.eval()
    return ray3d_amd.Ray3DLifter(pos, trj).eval()


@pytest.mark.parametrize("n", [31, 64, 4200])
def test_forward_clip_into_a_slice_equals_forward_clip(n):
    """A call rounded up past the clip's end (31 -> 32), an exact one (64) and two near-equal calls with a surplus (4200)."""
    lifter = _lifter()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(n)
    clip = torch.from_numpy(rng.normal(0, 0.3, (n + 26, 17, 3)).astype(np.float32)).to(dev)
    prow = torch.from_numpy(rng.normal(0, 1, (2,)).astype(np.float32)).to(dev)
    buf = torch.full((n + 10, 1, 17, 3), SENTINEL, dtype=torch.float32, device=dev)
    with torch.no_grad():
        want = lifter.forward_clip(clip, prow)
        got = lifter.forward_clip(clip, prow, out=buf[3:3 + n])
        pair = lifter.forward_clip(clip, prow, return_trj=True)
        buf2 = torch.empty((n, 1, 17, 3), dtype=torch.float32, device=dev)
        pair2 = lifter.forward_clip(clip, prow, return_trj=True, out=buf2)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf[3:].data_ptr() and got.shape == want.shape == (n, 1, 17, 3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool((buf[:3] == SENTINEL).all()) and bool((buf[3 + n:] == SENTINEL).all())
    assert torch.equal(pair2[0].view(torch.int32), pair[0].view(torch.int32)) and torch.equal(pair2[1], pair[1])
    with pytest.raises(ValueError, match="forward_clip"):
        lifter.forward_clip(clip, prow, out=buf[:n + 1])


def _no_swap_mirror(x):
    """A `mirror=` callable that is NOT mirror_input's default: x negated, the keypoints left where they are."""
    from ray3d_amd import evaluate
    return evaluate.mirror_input(x, (), ())


@pytest.mark.parametrize("case", ["plain", "flip", "mirror", "ranks2"])
def test_evaluate_clips_batched_equals_evaluate_clips(case, monkeypatch):
    """Three short clips over two actions through the RF-27 model: the rows of the one-call path are those of the per-clip path.
    `mirror`: the flip pass through a `mirror=` callable, also with finish=True.  `ranks2`: the pass run as rank 0 and as rank 1 of
    two (both shards hold clips; the all_gather replaced by the rows the two ranks made), finish off and on - row for row the
    single-rank result."""
    from ray3d_amd import evaluate
    lifter = _lifter()
    dev = torch.device("cuda:0")
    clips = near_clips(lifter.forward_clip, evalcore_clips(), dev)
    flip = case != "plain"
    kw = dict(flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    if case == "mirror":
        kw["mirror"] = _no_swap_mirror
    with torch.no_grad():
        named, avg, rows = evaluate.evaluate_clips(lifter.forward_clip, clips, 27, dev, **kw)
        named_b, avg_b, rows_b = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, **kw)
        _, _, rows_d, detail = evaluate.evaluate_clips_detail(lifter.forward_clip, clips, 27, dev, **kw)
        named_e, avg_e, rows_e, detail_e = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, detail=True, **kw)
    assert rows_b.is_cuda and rows_b.shape == (3, 8) and torch.equal(rows_b, rows)
    assert named_b == named and avg_b == avg and set(named) == {"A", "B"}
    assert torch.equal(rows_e, rows_d) and torch.equal(detail_e["rows"], detail["rows"]) and detail_e["rows"].shape == (3, 82)
    assert named_e == named and avg_e == avg
    assert set(detail_e) == set(detail) == {"A", "B", "overall", "rows"}
    for key in ("A", "B", "overall"):
        assert detail_e[key] == detail[key], key
    if not flip:     # (the ground truth lies near the plain poses; the synthetic weights are not mirror-symmetric, so the flip average is metres off)
        assert 0.0 < detail_e["overall"]["auc"] < detail_e["overall"]["pck150"] <= 100.0
    if case == "mirror":
        with torch.no_grad():
            _, _, rows_f, detail_f = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, detail=True, finish=True, **kw)
            _, _, rows_default = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, **dict(kw, mirror=None))
        assert same_bits(rows_f, rows_d) and same_bits(detail_f["rows"], detail["rows"])
        assert torch.isfinite(rows_b).all() and not torch.equal(rows_default[:, 3], rows_b[:, 3])      # the callable was used
    if case == "ranks2":
        shards = evaluate.shard_clips([c.rays.shape[0] for c in clips], 2)
        assert all(shards) and sorted(shards[0] + shards[1]) == [0, 1, 2]
        for finish in (False, True):
            made = {}                                    # (rank, cols) -> the rows that rank handed to the exchange

            def gather(local_rows, counts, group=None, cols=evaluate.PARTIAL_COLS, rank=None):
                assert list(counts) == [len(s) for s in shards] and local_rows.shape == (counts[rank], cols)
                made[rank, cols] = local_rows
                return torch.cat([made.get((r, cols), local_rows.new_zeros((counts[r], cols))) for r in range(2)], dim=0)

            got = {}
            for rank in (0, 1, 0):                       # (rank 0 once more, now with rank 1's rows in the exchange)
                monkeypatch.setattr(evaluate, "gather_partials", functools.partial(gather, rank=rank))
                with torch.no_grad():
                    got[rank] = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, rank=rank, world_size=2,
                                                                finish=finish, **kw), \
                        evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, rank=rank, world_size=2, finish=finish,
                                                        detail=True, **kw)
            for rank in (0, 1):
                (_, _, r_plain), (n_det, a_det, r_det, d_det) = got[rank]
                ids = [float(i) for i in shards[0] + shards[1]]
                assert r_plain[:, 0].tolist() == ids                                    # as gathered: rank order, unsorted
                assert same_bits(r_plain[torch.argsort(r_plain[:, 0])], rows_d), (finish, rank)
                assert same_bits(r_det, rows_d) and same_bits(d_det["rows"], detail["rows"]), (finish, rank)
                assert n_det == named_e and a_det == avg_e and all(d_det[k] == detail[k] for k in ("A", "B", "overall"))
