"""CPU suite: the validation losses of Trainer.test (r3d_clip_valid_losses) without a GPU - the kernel's per-frame routines
run on the host by the hooks build (r3d_debug_valid_losses_host) against the NumPy oracle of tests/valid_oracle.py and the
reference's own float32 values (tests/golden/valid.npz), the argument checks, the torch path CPU tensors take, and
validate_clips / reduce_valid over two gloo ranks."""
import os

import numpy as np
import pytest
import torch

from conftest import hooks_library
import valid_oracle as vo

from ray3d_amd import _capi, evaluate, metrics, skeleton

VARIANTS = ("trj", "sum", "abs", "rel")
HOST_CASES = [(1, 17), (2, 17), (37, 17), (65, 14), (257, 15), (300, 17)]


def _run_host(n, J, variant, bones=True, frames=True):
    pos, trj, gt, flags = vo.variant_inputs(n, J, variant)
    rc, out, fr = vo.host_call(hooks_library(), pos, trj, gt, vo.tree_for(J) if bones else None, flags, frames)
    assert rc == 0, _capi.load().r3d_last_error()
    return out, fr, vo.oracle(pos, trj, gt, vo.tree_for(J) if bones else None, flags)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,J", HOST_CASES)
def test_host_routine_matches_the_numpy_oracle(n, J, variant):
    """Sums and per-bone sums within 1e-12 relative, per-frame terms within 1e-9 * max(1, |want|): the bounds
    tests/test_gpu_metrics_detail.py uses for float64 sums (both sides add the same float64 terms, in another order)."""
    out, fr, want = _run_host(n, J, variant)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(fr))
    print("n %d J %d %s: sums max rel err %.3e, frames max abs err %.3e"
          % (n, J, variant, vo.rel_err(out, want["out"]).max(), np.abs(fr - want["frames"]).max()))
    assert vo.sums_close(out, want["out"])
    assert vo.frames_close(fr, want["frames"])
    bones = out[vo.COUNT:].reshape(vo.BONE_ROWS, vo.MAX_BONES)
    assert np.all(bones[:, J - 1:] == 0.0) and np.all(bones[:, :J - 1] > 0.0)
    if variant in ("abs", "rel"):
        assert out[1] == out[0] and np.all(out[2:5] == 0.0)             # POS equals LOSS, no trajectory terms
    # the frame table's columns, added in index order, are the seven sums
    assert vo.sums_close(np.add.reduce(fr, axis=0), out[:vo.COUNT])


def test_no_parent_table_means_no_bone_terms_and_frames_are_optional():
    out, fr, want = _run_host(37, 17, "trj", bones=False)
    assert vo.sums_close(out, want["out"]) and np.all(out[5:] == 0.0) and np.all(fr[:, 5:] == 0.0)
    out2, none, _ = _run_host(37, 17, "trj", bones=False, frames=False)
    assert none is None and out2.tobytes() == out.tobytes()


def test_inputs_are_left_alone_on_the_host():
    pos, trj, gt, flags = vo.variant_inputs(37, 17, "trj")
    p, t, g = np.array(pos), np.array(trj), np.array(gt)
    rc, _, _ = vo.host_call(hooks_library(), p, t, g, vo.H36M, flags)
    assert rc == 0 and np.array_equal(p, pos) and np.array_equal(t, trj) and np.array_equal(g, gt)


@pytest.mark.parametrize("case", ["trj_n37", "trj_n1", "notrj_abs", "notrj_rel"])
def test_host_routine_against_the_reference_fp32_values(case):
    pos, trj, gt, flags, ref = vo.golden_case(case)
    rc, out, _ = vo.host_call(hooks_library(), pos, trj, gt, vo.H36M, flags)
    assert rc == 0
    assert tuple(vo.golden()["parents"]) == vo.H36M == skeleton.H36M_17_PARENTS
    vo.check_against_reference(out, pos.shape[0], ref)


def test_the_test_trj_quirk():
    """Trainer.test's logged test_trj is mean(w) * mean(d) of the clip (its (B,1) weights broadcast against the (B,1,1)
    norms, trainer.py:217-218): WSUM * DSUM / n; TRJ_W is the elementwise figure of Trainer.train (:119-120).  With more
    than one frame the two differ - by far more than the bound."""
    pos, trj, gt, flags, ref = vo.golden_case("trj_n37")
    n = pos.shape[0]
    rc, out, _ = vo.host_call(hooks_library(), pos, trj, gt, vo.H36M, flags)
    assert rc == 0
    rel = 4.0 * float(vo.golden()["ref_fp32_vs_f64_rel"])
    logged, train = out[3] * out[4] / n, out[2]
    print("as logged %.9g (reference %.9g), elementwise %.9g (reference %.9g)" % (logged, ref["trj_logged"], train, ref["trj_train"]))
    assert abs(logged - ref["trj_logged"]) <= rel * ref["trj_logged"]
    assert abs(train - ref["trj_train"]) <= rel * ref["trj_train"]
    assert abs(ref["trj_logged"] - ref["trj_train"]) > 100 * rel * ref["trj_train"]
    assert abs(train - ref["trj_logged"]) > rel * ref["trj_logged"]     # the elementwise sum is NOT the logged figure
    # one frame: an outer product of one element is the elementwise product
    _, _, _, _, ref1 = vo.golden_case("trj_n1")
    assert ref1["trj_logged"] == ref1["trj_train"]


@pytest.mark.parametrize("n,J", [(37, 17), (257, 15)])
def test_pos_is_sum_against_separate_pos(n, J):
    """pos_dev = fl32(pos + trj) with R3D_VALID_POS_IS_SUM against pos and trj given separately.  LOSS sees the same P_abs:
    identical bits.  The recovered root-relative prediction fl32(sum - trj) differs from pos per coordinate by at most
    2^-24 (|sum| + |sum - trj|) <= eps := 2^-23 max|sum| (the clip's largest |sum| coordinate exceeds its largest |pos|
    coordinate: the root is metres away - asserted).  Propagated, with u = 2^-24 the rounding of a float32 difference
    (taken on both sides):
      POS       a joint's difference vector moves by <= e_p = eps + 2 u max|pos - G_rel| per coordinate, its norm by
                sqrt(3) e_p, the frame means by as much, the sum over n frames by n sqrt(3) e_p;
      bones     a bone vector moves by <= e_b = 2 eps + 2 u max|bone| per coordinate, its length by dl = sqrt(3) e_b:
                BONE_LEN and the per-bone sums of |len_p - len_g| and len_p by n dl, of len_p^2 by n (2 Lmax dl + dl^2),
                of len_g by nothing; a unit vector by <= 2 dl / Lmin: BONE_DIR by n 2 dl / Lmin;
    plus 1e-12 relative for the float64 additions."""
    pos, trj, gt, _ = vo.variant_inputs(n, J, "trj")
    total, _, _, flags = vo.variant_inputs(n, J, "sum")
    lib = hooks_library()
    rc_a, a, _ = vo.host_call(lib, pos, trj, gt, vo.tree_for(J), 0)
    rc_b, b, _ = vo.host_call(lib, total, trj, gt, vo.tree_for(J), flags)
    assert rc_a == 0 and rc_b == 0
    assert a[0].tobytes() == b[0].tobytes() and a[2:5].tobytes() == b[2:5].tobytes()
    assert np.abs(total).max() >= np.abs(pos).max()
    u, eps = 2.0 ** -24, 2.0 ** -23 * float(np.abs(total).max())
    g_rel = np.array(gt) - gt[:, :1]
    e_p = eps + 2 * u * float(np.abs(pos - g_rel).max())
    tree = vo.tree_for(J)
    bone = pos[:, list(tree[1:])] - pos[:, 1:]
    length = np.linalg.norm(bone.astype(np.float64), axis=-1)
    dl = np.sqrt(3.0) * (2 * eps + 2 * u * float(np.abs(bone).max()))
    slack = lambda v: 1e-12 * np.abs(v)
    print("eps %.3e: POS differs by %.3e (bound %.3e), BONE_LEN %.3e (%.3e), BONE_DIR %.3e (%.3e)"
          % (eps, abs(a[1] - b[1]), n * np.sqrt(3.0) * e_p, abs(a[5] - b[5]), n * dl, abs(a[6] - b[6]), n * 2 * dl / length.min()))
    assert abs(a[1] - b[1]) <= n * np.sqrt(3.0) * e_p + slack(a[1])
    assert abs(a[5] - b[5]) <= n * dl + slack(a[5])
    assert abs(a[6] - b[6]) <= n * 2 * dl / length.min() + slack(a[6])
    ra, rb = a[vo.COUNT:].reshape(4, 16), b[vo.COUNT:].reshape(4, 16)
    assert np.all(np.abs(ra[0] - rb[0]) <= n * dl + slack(ra[0])) and np.all(np.abs(ra[1] - rb[1]) <= n * dl + slack(ra[1]))
    assert np.all(np.abs(ra[2] - rb[2]) <= n * (2 * length.max() * dl + dl * dl) + slack(ra[2]))
    assert ra[3].tobytes() == rb[3].tobytes()


def _arg_cases():
    pos, trj, gt = (np.array(v) for v in vo.make_inputs(4, 17))
    ok = dict(pos=pos, trj=trj, gt=gt, parents=vo.H36M, flags=0, n=4, J=17)
    bad_root, self_parent, forward_parent = list(vo.H36M), list(vo.H36M), list(vo.H36M)
    bad_root[0], self_parent[5], forward_parent[3] = 0, 5, 9
    return ok, [("null pos", dict(pos=None), "null pointer"), ("null gt", dict(gt=None), "null pointer"),
                ("n = 0", dict(n=0), "n_frames"), ("n < 0", dict(n=-3), "n_frames"),
                ("J = 0", dict(J=0), "num_joints"), ("J = 18", dict(J=18), "num_joints"),
                ("parents[0] != -1", dict(parents=bad_root), "parent table"),
                ("a joint its own parent", dict(parents=self_parent), "parent table"),
                ("a parent after its child", dict(parents=forward_parent), "parent table"),
                ("a negative parent", dict(parents=[-1, -1] + list(vo.H36M[2:])), "parent table"),
                ("POS_IS_SUM without trj", dict(trj=None, flags=vo.POS_IS_SUM), "POS_IS_SUM"),
                ("GT_ROOT_RELATIVE with trj", dict(flags=vo.GT_ROOT_RELATIVE), "GT_ROOT_RELATIVE"),
                ("unknown flag", dict(flags=4), "flags")]


def test_every_argument_error_of_the_host_hook_and_of_the_call():
    lib = hooks_library()
    ok, cases = _arg_cases()
    rc, out, _ = vo.host_call(lib, **ok)
    assert rc == 0 and np.all(np.isfinite(out))
    for label, change, word in cases:
        kw = dict(ok, **change)
        rc, _, _ = vo.host_call(lib, **kw)
        msg = lib.r3d_last_error().decode()
        assert rc == _capi.R3D_ERR_ARG and word in msg and "r3d_debug_valid_losses_host" in msg, (label, rc, msg)
    # the hook's missing result pointer
    assert lib.r3d_debug_valid_losses_host(vo._fptr(ok["pos"]), vo._fptr(ok["trj"]), vo._fptr(ok["gt"]), 4, 17, None, 0, None, None) == _capi.R3D_ERR_ARG
    # r3d_clip_valid_losses itself checks before it launches anything: the same cases on the product library, no device needed
    _capi.use_hooks(False)
    scratch = np.zeros(_capi.VALID_OUT_DOUBLES)
    for label, change, word in cases:
        kw = dict(ok, **change)
        with pytest.raises(_capi.Ray3DHipError, match=word):
            _capi.clip_valid_losses(kw["pos"].ctypes.data if kw["pos"] is not None else None,
                                    kw["trj"].ctypes.data if kw["trj"] is not None else None,
                                    kw["gt"].ctypes.data if kw["gt"] is not None else None, kw["n"], kw["J"], kw["parents"],
                                    kw["flags"], scratch.ctypes.data, None, 0)
    with pytest.raises(_capi.Ray3DHipError, match="null pointer"):
        _capi.clip_valid_losses(ok["pos"].ctypes.data, ok["trj"].ctypes.data, ok["gt"].ctypes.data, 4, 17, vo.H36M, 0, None, None, 0)


def test_constants_follow_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ray3d_hip.h")).read()
    import re
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    assert [val("R3D_VALID_" + k.upper()) for k in _capi.VALID_NAMES] == list(range(7))
    assert (val("R3D_VALID_COUNT"), val("R3D_VALID_MAX_BONES"), val("R3D_VALID_BONE_ROWS")) == (_capi.VALID_COUNT, _capi.VALID_MAX_BONES, _capi.VALID_BONE_ROWS)
    assert (val("R3D_VALID_POS_IS_SUM"), val("R3D_VALID_GT_ROOT_RELATIVE")) == (_capi.R3D_VALID_POS_IS_SUM, _capi.R3D_VALID_GT_ROOT_RELATIVE)
    assert _capi.VALID_DOUBLES == metrics.VALID_DOUBLES == vo.DOUBLES == 71 and evaluate.VALID_COLS == 74
    assert _capi.VALID_OUT_DOUBLES == 71 * (1 + val("R3D_METRIC_MAX_BLOCKS"))


def test_skeleton_validator():
    assert skeleton.validate_parents(list(skeleton.H36M_17_PARENTS), 17) == skeleton.H36M_17_PARENTS
    assert skeleton.validate_parents(vo.chain(14), 14) == vo.chain(14)
    for bad, J in (((0,) + vo.H36M[1:], 17), (vo.H36M, 16), ((-1, 1), 2), ((-1, 0, 3, 1), 4), ((-1,) * 18, 18), ((), 0)):
        with pytest.raises(ValueError):
            skeleton.validate_parents(bad, J)
    assert all(0 <= a < 16 and 0 <= b < 16 for a, b in skeleton.H36M_17_BONE_PAIRS)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,J", [(1, 17), (37, 17), (65, 14)])
def test_clip_valid_on_cpu_tensors_equals_the_hook(n, J, variant):
    pos, trj, gt, flags = vo.variant_inputs(n, J, variant)
    rc, out, fr = vo.host_call(hooks_library(), pos, trj, gt, vo.tree_for(J), flags)
    assert rc == 0
    clip = evaluate.Clip(vo.stub_camera(), np.zeros((n, J, 3), np.float32), np.array(gt), "A", 5)
    p = torch.from_numpy(np.array(pos)).reshape(n, 1, J, 3)
    t = torch.from_numpy(np.array(trj)).reshape(n, 1, 1, 3) if trj is not None else None
    before = p.clone()
    row = evaluate.clip_valid(p, t, clip, parents=vo.tree_for(J), pos_is_sum=bool(flags & vo.POS_IS_SUM),
                              gt_root_relative=bool(flags & vo.GT_ROOT_RELATIVE), action_id=2)
    assert row.dtype == torch.float64 and row.shape == (evaluate.VALID_COLS,) and row[:3].tolist() == [5.0, 2.0, float(n)]
    assert vo.sums_close(row[3:].numpy(), out) and torch.equal(p, before)
    _, frames = metrics.clip_valid(p.reshape(n, J, 3), t.reshape(n, 3) if t is not None else None, torch.from_numpy(np.array(gt)),
                                   vo.tree_for(J), bool(flags & vo.POS_IS_SUM), bool(flags & vo.GT_ROOT_RELATIVE))
    assert vo.frames_close(frames.numpy(), fr)
    filled = torch.zeros(evaluate.VALID_COLS, dtype=torch.float64)
    filled[:3] = torch.tensor([9.0, 1.0, float(n)], dtype=torch.float64)
    got = evaluate.clip_valid(p, t, clip, parents=vo.tree_for(J), pos_is_sum=bool(flags & vo.POS_IS_SUM),
                              gt_root_relative=bool(flags & vo.GT_ROOT_RELATIVE), out=filled)
    assert got is filled and filled[:3].tolist() == [9.0, 1.0, float(n)] and torch.equal(filled[3:], row[3:])
    with pytest.raises(ValueError):
        evaluate.clip_valid(p, None, clip, parents=None, pos_is_sum=True)
    if t is not None:
        with pytest.raises(ValueError):
            evaluate.clip_valid(p, t, clip, parents=None, gt_root_relative=True)


# ------------------------------------------------------------------ validate_clips / reduce_valid

def serial_figures(clips):
    """The figures reduce_valid must give, from the oracle clip by clip."""
    per = []
    for c in clips:
        total, trj = vo.standin_parts(c)
        per.append((c.rays.shape[0], vo.oracle(total, trj, c.gt_norm, vo.H36M, vo.POS_IS_SUM)))
    N = sum(n for n, _ in per)
    s = sum(w["out"] for _, w in per)
    bones = sum(w["bones"] for _, w in per) / N
    return dict(frames=N, valid_mm=s[0] / N * 1e3, pos_mm=s[1] / N * 1e3, trj_mm=s[2] / N * 1e3,
                trj_mm_as_logged=sum(w["out"][3] * w["out"][4] / n for n, w in per) / N * 1e3,
                bone_mm=(s[5] + s[6]) / N * 1e3, bone_len_mm=s[5] / N * 1e3,
                len_err_mm=bones[0] * 1e3, len_pred_mm=bones[1] * 1e3, len_gt_mm=bones[3] * 1e3,
                len_pred_std_mm=np.sqrt(bones[2] - bones[1] ** 2) * 1e3)


def check_table(table, want, tol=1e-9):
    for k in ("valid_mm", "pos_mm", "trj_mm", "trj_mm_as_logged", "bone_mm", "bone_len_mm"):
        assert abs(table[k] - want[k]) <= tol * max(1.0, abs(want[k])), (k, table[k], want[k])
    assert table["frames"] == want["frames"] and len(table["bones"]) == 16
    for k in ("len_err_mm", "len_pred_mm", "len_gt_mm"):
        assert vo.frames_close([b[k] for b in table["bones"]], want[k], tol), k
    # sqrt(E[l^2] - E[l]^2) cancels: lengths of ~0.3 m deviating by centimetres lose ~3 digits
    assert vo.frames_close([b["len_pred_std_mm"] for b in table["bones"]], want["len_pred_std_mm"], 1e-6)


def test_validate_clips_and_reduce_valid_serial():
    clips = vo.valid_clips()
    table, rows = evaluate.validate_clips(vo.standin_lift, clips, vo.RF, "cpu", bone_pairs=skeleton.H36M_17_BONE_PAIRS)
    assert rows.shape == (3, evaluate.VALID_COLS) and rows[:, 0].tolist() == [0.0, 1.0, 2.0] and rows[:, 1].tolist() == [0.0, 1.0, 0.0]
    assert rows[:, 2].tolist() == [23.0, 9.0, 14.0]
    want = serial_figures(clips)
    check_table(table, want)
    assert abs(table["trj_mm"] - table["trj_mm_as_logged"]) > 1e-6          # the quirk shows on these clips
    assert table["bone_mm"] > table["bone_len_mm"] > 0.0
    assert [(a, b) for a, b, _, _ in table["symmetry"]] == list(skeleton.H36M_17_BONE_PAIRS)
    for a, b, dp, dg in table["symmetry"]:
        assert abs(dp - (want["len_pred_mm"][a] - want["len_pred_mm"][b])) <= 1e-9 * 1e3
        assert abs(dg - (want["len_gt_mm"][a] - want["len_gt_mm"][b])) <= 1e-9 * 1e3
    again = evaluate.reduce_valid(rows.flip(0), 17, skeleton.H36M_17_BONE_PAIRS)       # any row order
    assert again == table
    lines = evaluate.format_valid_report(table)
    assert len(lines) == 4 + 16 + 6 and all(isinstance(s, str) for s in lines)
    assert "%.3f mm" % table["valid_mm"] in lines[0] and "%.3f" % table["trj_mm_as_logged"] in lines[2]
    assert evaluate.format_valid_report(table, ["b%d" % b for b in range(16)])[4].startswith("b0: length error ")
    # a lifter without a trajectory: poses alone, no bones asked for
    table2, rows2 = evaluate.validate_clips(lambda p, q: vo.standin_lift(p, q)[0], clips, vo.RF, "cpu", parents=None)
    assert table2["trj_mm"] == 0.0 and table2["pos_mm"] == table2["valid_mm"] and table2["bones"] == [] and table2["bone_mm"] == 0.0
    assert abs(table2["valid_mm"] - want["valid_mm"]) <= 1e-9 * want["valid_mm"]


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        table, rows = evaluate.validate_clips(vo.standin_lift, vo.valid_clips(), vo.RF, "cpu", bone_pairs=skeleton.H36M_17_BONE_PAIRS)
        q.put((rank, table, rows.numpy()))
    finally:
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def test_two_rank_validate_clips_equals_the_serial_evaluation():
    """Two gloo ranks, clips sharded over them, the rows in one all_gather: every rank ends with exactly the single-process
    table (rows are reduced in clip-id order), which matches the oracle's serial evaluation."""
    import torch.multiprocessing as mp
    table1, rows1 = evaluate.validate_clips(vo.standin_lift, vo.valid_clips(), vo.RF, "cpu", bone_pairs=skeleton.H36M_17_BONE_PAIRS)
    check_table(table1, serial_figures(vo.valid_clips()))
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
    for rank, table, rows in res:
        assert np.array_equal(rows, rows1.numpy()), rank
        assert table == table1, rank
