"""CPU suite: the host side of r3d_streams_fuse (one world skeleton per person from several cameras) - the exports, the argument rules
(all checked before any device call: they run without a GPU), and the host hook r3d_debug_streams_fuse_host, bit for bit, against
the NumPy restatement of the header's rule (tests/streams_fuse_cases.py) on seeded cases, plus the rule's properties.  Every buffer
lies inside guard bands with poisoned outputs (tests/buffers_util.py).  tests/test_gpu_streams_fuse.py runs the kernel on the same
cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, hooks_library

import streams_fuse_cases as fc
from streams_fuse_cases import FuseRig, QNAN64, agree, bits64, restate_case, simple_case
from ray3d_amd import _capi

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()


def hook(case, **over):
    rc, out = FuseRig("cpu", case).run(**over)
    return rc, out


def skeleton(seed, J=17, n=1):
    return np.random.RandomState(seed).uniform(-2.0, 2.0, (n, J, 3))


# ------------------------------------------------------------------------------------ header, binding, exports

def test_exports_header_and_abi():
    assert "r3d_streams_fuse" in _capi.EXPORTS and "r3d_debug_streams_fuse_host" in _capi.HOOK_EXPORTS
    assert _capi.FUSE_MAX_MEMBERS == 16 and re.search(r"#define R3D_FUSE_MAX_MEMBERS 16\b", HDR)
    assert re.search(r"\bint r3d_streams_fuse\(", HDR)
    assert HDR.index("int r3d_debug_streams_fuse_host(") > HDR.index("#ifdef R3D_TEST_HOOKS") > HDR.index("int r3d_streams_fuse(")
    block = HDR[HDR.index("one call behind a tick's r3d_streams_poses"):HDR.index("int r3d_streams_fuse(")]
    for word in ("THE WHOLE BOUNDS STORY", "R3D_ERR_ARG", "CANDIDATES", "GATE", "medoid"):
        assert word in block, word
    product = C.CDLL(_capi.LIB_PATH)
    assert hasattr(product, "r3d_streams_fuse") and not hasattr(product, "r3d_debug_streams_fuse_host")
    hooks = hooks_library()
    assert hasattr(hooks, "r3d_streams_fuse") and hasattr(hooks, "r3d_debug_streams_fuse_host")
    assert hooks.r3d_abi_version() == 6 == _capi.ABI_VERSION            # no existing struct changed


# ------------------------------------------------------------------------------------ the hook against the restatement

@pytest.mark.parametrize("M,J", fc.SHAPES)
def test_hook_equals_the_restatement_bit_for_bit(M, J):
    seen = set()
    for rp, sy, gate in fc.VARIANTS:
        case, out = fc.host_run(M, J, rp, sy, gate)
        agree(out, restate_case(case), (M, J, rp, sy, gate))
        seen |= set(out["count"].flatten().tolist())
        assert (out["used"] >> J == 0).all()
    assert (M == 16 or {0, 1} <= seen) and (M == 1 or max(seen) >= 2)      # empty, single and fused joints all occur


@pytest.mark.parametrize("M", [1, 4, 16])
def test_an_all_empty_group_holds_exactly_nan_and_zero(M):
    for g in range(fc.G_CASE):
        case, out = fc.host_run(M, 17, True, True, True, all_empty_group=g)
        agree(out, restate_case(case), (M, g))
        assert (out["fused"][g] == QNAN64).all() and (out["spread"][g] == QNAN64).all()
        assert (out["count"][g] == 0).all() and (out["used"][g] == 0).all()


def test_words_that_name_no_stream_are_not_followed():
    """-1, -2, S and INT32_MAX are empty slots, whatever else the group holds; the result is that of the group without them."""
    x = skeleton(1, n=3)
    a = simple_case(x, [[0, -1, 3, 1, -2, fc.INT32_MAX, 2, -(2 ** 31)]], reproj=np.full((3, 17), 1.5))
    b = simple_case(x, [[0, 1, 2]], reproj=np.full((3, 17), 1.5))
    (_, ga), (_, gb) = hook(a), hook(b)
    assert np.array_equal(ga["fused"], gb["fused"]) and np.array_equal(ga["spread"], gb["spread"]) and np.array_equal(ga["count"], gb["count"])
    assert ga["used"][0].tolist() == [(1 << 17) - 1, 0, 0, (1 << 17) - 1, 0, 0, (1 << 17) - 1, 0]
    agree(ga, restate_case(a))


def test_unfinished_and_refused_members_and_their_stale_rows():
    """A stream with emit < 0 or status != 0 is no candidate, and what its stale rows hold changes no output bit."""
    rng = np.random.RandomState(3)
    x, r = skeleton(2, n=4), rng.uniform(0.5, 4.0, (4, 17))
    emit, status = [3, -1, 5, 0], [0, 0, 1, 0]
    outs = []
    for poison in (None, fc.POISON64, int(np.float64(1e300).view(np.uint64)), 0):
        xx, rr = x.copy(), r.copy()
        if poison is not None:
            xx[[1, 2]] = np.full((2, 17, 3), poison, np.uint64).view(np.float64)
            rr[[1, 2]] = np.full((2, 17), poison, np.uint64).view(np.float64)
        case = simple_case(xx, [[0, 1, 2, 3]], reproj=rr, emit=emit, status=status, max_dist=0.5, synthetic=[0, 0, 0, 0])
        rc, out = hook(case)
        assert rc == 0
        agree(out, restate_case(case))
        outs.append(out)
    assert (outs[0]["used"][0, [1, 2]] == 0).all() and (outs[0]["count"] <= 2).all()
    for o in outs[1:]:
        agree(o, outs[0])


def test_non_finite_components_and_residuals_drop_only_their_joint():
    x, r = skeleton(4, n=3), np.full((3, 17), 2.0)
    x[0, 2, 1], x[1, 3, 0], x[2, 3, 2] = np.nan, np.inf, -np.inf
    r[0, 5], r[1, 6] = np.nan, np.inf
    case = simple_case(x, [[0, 1, 2]], reproj=r)
    rc, out = hook(case)
    agree(out, restate_case(case))
    want = np.full(17, 3)
    want[[2, 5, 6]], want[3] = 2, 1
    assert out["count"][0].tolist() == want.tolist()
    assert out["used"][0].tolist() == [0x1FFFF & ~(1 << 2 | 1 << 5), 0x1FFFF & ~(1 << 3 | 1 << 6), 0x1FFFF & ~(1 << 3)]


def test_a_duplicated_stream_counts_twice():
    x = skeleton(5, n=2)
    twice = simple_case(x, [[0, 1, 0]])
    copy = simple_case(np.concatenate([x, x[:1]]), [[0, 1, 2]])
    (_, a), (_, b) = hook(twice), hook(copy)
    agree(a, b)
    assert (a["count"] == 3).all()
    agree(a, restate_case(twice))


# ------------------------------------------------------------------------------------ properties

@pytest.mark.parametrize("with_reproj", [False, True])
def test_a_one_member_group_returns_the_members_bits(with_reproj):
    x = skeleton(6, n=2)
    r = np.random.RandomState(6).uniform(0.1, 30.0, (2, 17)) if with_reproj else None
    case = simple_case(x, [[1], [0]], reproj=r, max_dist=0.1)
    rc, out = hook(case)
    agree(out, restate_case(case))
    if not with_reproj:                          # w = 1: (1 * x) / 1 is x exactly
        assert np.array_equal(out["fused"], bits64(x[[1, 0]]))
        assert (out["spread"] == 0).all()
    else:                                        # (w * x) / w is x within one rounding of each operation
        assert np.abs(out["fused"].view(np.float64) - x[[1, 0]]).max() <= 4 * 2.2e-16 * np.abs(x).max()
        assert (out["spread"].view(np.float64) <= 4 * 2.2e-16 * np.abs(x).max()).all()
    assert (out["count"] == 1).all() and (out["used"] == 0x1FFFF).all()


def test_a_one_member_group_with_unit_weights_is_exact():
    """Without residuals every weight is 1 and (1 * x) / 1 is x: a one-member group returns the member's world bits, spread 0 and
    count 1 - also with the gate switched on, which needs two candidates."""
    x = skeleton(7, J=14, n=3)
    for max_dist in (0.0, 0.2):
        rc, out = hook(simple_case(x, [[2, -1, -1], [-1, 0, -1]], max_dist=max_dist))
        assert rc == 0 and np.array_equal(out["fused"], bits64(x[[2, 0]])) and (out["spread"] == 0).all() and (out["count"] == 1).all()
        assert out["used"].tolist() == [[0x3FFF, 0, 0], [0, 0x3FFF, 0]]


def test_identical_members_return_that_point():
    x = np.repeat(skeleton(8), 4, axis=0)
    case = simple_case(x, [[0, 1, 2, 3]], max_dist=0.2)
    rc, out = hook(case)
    agree(out, restate_case(case))
    assert np.array_equal(out["fused"][0], bits64(x[0])) and (out["spread"] == 0).all() and (out["count"] == 4).all()
    # with weights the point comes back within the rounding of the weighted mean
    r = np.random.RandomState(8).uniform(0.1, 9.0, (4, 17))
    rc, out = hook(simple_case(x, [[0, 1, 2, 3]], reproj=r, max_dist=0.2))
    assert np.abs(out["fused"][0].view(np.float64) - x[0]).max() <= 8 * 2.2e-16 * np.abs(x).max()


def test_the_gate_drops_a_member_displaced_by_a_metre():
    rng = np.random.RandomState(9)
    base = skeleton(9)[0]
    x = np.stack([base + 0.01 * rng.standard_normal((17, 3)), base + np.array([1.0, 0, 0]), base + 0.01 * rng.standard_normal((17, 3))])
    r = rng.uniform(0.5, 3.0, (3, 17))
    three = simple_case(x, [[0, 1, 2]], reproj=r, max_dist=0.2)
    two = simple_case(x, [[0, -1, 2]], reproj=r, max_dist=0.2)
    (_, a), (_, b) = hook(three), hook(two)
    assert a["used"][0].tolist() == [0x1FFFF, 0, 0x1FFFF] and (a["count"] == 2).all()
    for k in ("fused", "spread", "count"):
        assert np.array_equal(a[k], b[k]), k
    agree(a, restate_case(three))
    _, off = hook(dict(three, max_dist=0.0))     # without the gate the displaced member pulls the mean
    assert (off["count"] == 3).all() and not np.array_equal(off["fused"], a["fused"])


def test_of_two_disagreeing_members_the_smaller_residual_wins():
    base = skeleton(10)[0]
    x = np.stack([base, base + np.array([0.0, 0.6, 0.0])])
    r = np.full((2, 17), 1.0)
    r[0, ::2], r[1, 1::2] = 5.0, 5.0             # even joints: stream 1 is better; odd joints: stream 0
    case = simple_case(x, [[0, 1]], reproj=r, max_dist=0.3)
    rc, out = hook(case)
    agree(out, restate_case(case))
    even, odd = sum(1 << j for j in range(0, 17, 2)), sum(1 << j for j in range(1, 17, 2))
    assert out["used"][0].tolist() == [odd, even] and (out["count"] == 1).all()
    got = out["fused"][0].view(np.float64)
    assert np.abs(got[::2] - x[1, ::2]).max() <= 1e-15 * 4 and np.abs(got[1::2] - x[0, 1::2]).max() <= 1e-15 * 4
    # equal residuals: a tie keeps the earlier slot
    _, tie = hook(simple_case(x, [[0, 1]], reproj=np.full((2, 17), 2.0), max_dist=0.3))
    assert tie["used"][0].tolist() == [0x1FFFF, 0]


def test_the_tier_rule():
    """An observed keypoint outvotes the made-up ones of its joint; where every candidate is made up, all stay."""
    rng = np.random.RandomState(11)
    x = skeleton(11)[0] + 0.01 * rng.standard_normal((3, 17, 3))
    syn = [0b101, 0b110, 0b100]                 # joint 0: stream 0 made up; joint 1: stream 1; joint 2: all three
    case = simple_case(x, [[0, 1, 2]], synthetic=syn)
    rc, out = hook(case)
    agree(out, restate_case(case))
    assert out["count"][0, :4].tolist() == [2, 2, 3, 3]
    assert out["used"][0].tolist() == [0x1FFFF & ~1, 0x1FFFF & ~2, 0x1FFFF]
    _, plain = hook(dict(case, synthetic=None))
    assert (plain["count"] == 3).all() and np.array_equal(plain["fused"][0, 2:], out["fused"][0, 2:])
    # a made-up keypoint is dropped before the gate: it cannot become the medoid
    far = x.copy()
    far[0] += 1.0
    _, gated = hook(simple_case(far, [[0, 1, 2]], synthetic=[0, 0x1FFFF, 0x1FFFF], max_dist=0.2))
    assert gated["used"][0].tolist() == [0x1FFFF, 0, 0]


@pytest.mark.parametrize("M,J", fc.SHAPES)
def test_fused_lies_inside_the_inliers_bounds(M, J):
    """Component-wise, within 32 * 2.2e-16 * max|x|: the rounding bound of a 16-term weighted mean."""
    checked = 0
    for rp, sy, gate in fc.VARIANTS:
        case, out = fc.host_run(M, J, rp, sy, gate)
        fused = out["fused"].view(np.float64)
        for g in range(case["G"]):
            for j in range(J):
                pts = [case["world"][case["member"][g, m], j] for m in range(M) if (out["used"][g, m] >> j) & 1]
                assert len(pts) == out["count"][g, j]
                if not pts:
                    continue
                pts = np.array(pts)
                slack = 32 * 2.2e-16 * np.abs(pts).max()
                assert (fused[g, j] >= pts.min(axis=0) - slack).all() and (fused[g, j] <= pts.max(axis=0) + slack).all(), (g, j)
                checked += 1
    assert checked > 0


# ------------------------------------------------------------------------------------ R3D_ERR_ARG

def test_every_argument_error():
    case = fc.make_case(4, 17, True, True, True)
    rig = FuseRig("cpu", case)
    assert rig.run()[0] == 0
    t = {n: v.data_ptr() for n, v in rig.t.items()}
    bad = [dict(world=None), dict(emit=None), dict(status=None), dict(member=None), dict(fused=None),
           dict(S=0), dict(S=_capi.CLIPS_MAX + 1), dict(G=0), dict(G=_capi.CLIPS_MAX + 1), dict(J=0), dict(J=18), dict(M=0),
           dict(M=_capi.FUSE_MAX_MEMBERS + 1), dict(soft_px=0.0), dict(soft_px=-1.0), dict(soft_px=float("nan")), dict(soft_px=float("inf")),
           dict(max_px=float("nan")), dict(max_dist=float("nan")),
           dict(world=t["world"] + 4), dict(reproj=t["reproj"] + 4), dict(emit=t["emit"] + 4), dict(fused=t["fused"] + 4),
           dict(spread=t["spread"] + 4),
           dict(fused=t["world"]), dict(fused=t["world"] + 8 * (7 * 17 * 3 - 1)), dict(spread=t["reproj"]), dict(count=t["status"]),
           dict(used=t["member"]), dict(count=t["synthetic"] + 4 * 6), dict(spread=t["emit"]), dict(fused=t["reproj"] - 8 * (3 * 17 * 3 - 1))]
    for over in bad:
        before = rig.read()
        rc = _capi.debug_streams_fuse_host(*rig.args(**over))
        assert rc == _capi.R3D_ERR_ARG, over
        assert _capi.load().r3d_last_error()
        agree(rig.read(), before, over)          # nothing is written by a refused call
    ok = [dict(spread=None), dict(count=None), dict(used=None), dict(spread=None, count=None, used=None), dict(max_px=-1.0),
          dict(max_dist=float("-inf")), dict(max_px=float("inf")), dict(M=1), dict(J=1)]
    for over in ok:
        assert _capi.debug_streams_fuse_host(*rig.args(**over)) == 0, over
    rig.arena.check()


def test_the_product_entry_refuses_on_the_host_before_any_device_call():
    """Without a GPU: R3D_ERR_ARG comes back from the product library's r3d_streams_fuse itself."""
    _capi.use_hooks(False)
    bogus = 1 << 20
    with pytest.raises(_capi.Ray3DHipError, match="max_members"):
        _capi.streams_fuse(bogus, None, bogus, bogus, None, 4, 17, bogus, 2, 17, 2.0, 0.0, 0.0, bogus * 2, None, None, None, 0)
    with pytest.raises(_capi.Ray3DHipError, match="soft_px"):
        _capi.streams_fuse(bogus, None, bogus, bogus, None, 4, 17, bogus, 2, 2, 0.0, 0.0, 0.0, bogus * 2, None, None, None, 0)
    with pytest.raises(_capi.Ray3DHipError, match="overlaps"):
        _capi.streams_fuse(bogus, None, bogus * 3, bogus * 4, None, 4, 17, bogus * 5, 2, 2, 2.0, 0.0, 0.0, bogus + 8, None, None, None, 0)
