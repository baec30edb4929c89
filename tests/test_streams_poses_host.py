"""Host suite (no GPU): r3d_streams_poses through its host hook, r3d_debug_streams_poses_host - the argument rules and the
__host__ __device__ routines the kernel runs.  The hook against a NumPy restatement of the stated arithmetic, bit for bit (flip
average, world, residual, quality; J 17 and 14; lag 0 / 4 at RF 9, 13 at RF 27); against the reference's own camera functions
(tests/golden/streams_poses.npz: world within 1e-12 m, residual within 1e-9 px); streams that did not finish keep the fill in every
output; a non-finite raw element touches its own point and its stream's quality words only; every R3D_ERR_ARG rule is refused
before anything is written.  Every buffer sits exact-sized inside guard bands."""
import os

import numpy as np
import pytest

import streams_poses_cases as pc
from conftest import GOLDEN
from ray3d_amd import _capi
from streams_poses_cases import OUTPUTS, Rig, bits, restate, same_bits

SHAPES = [(17, 9, 0), (17, 9, 4), (14, 9, 4), (17, 27, 13), (14, 27, 13)]      # (J, RF, lag)
ERR_ARG = _capi.R3D_ERR_ARG


def _agree(got, want, what):
    assert got["rc"] == 0, what
    for k in want:
        assert same_bits(got[k], want[k]), (what, k, np.argwhere(bits(got[k]) != bits(want[k]))[:4].tolist())


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("J,rf,lag", SHAPES)
def test_hook_equals_the_numpy_restatement_bit_for_bit(J, rf, lag, flip):
    """Six streams, three finished, two idle (emit -1), one refused (status 1); all four outputs, then each output alone."""
    inp = pc.make_inputs(6, J, rf, lag, seed=40 + J + rf + lag, emit=[3, -1, 0, 2 ** 40, -1, 7], status=[0, 0, 0, 0, 0, 1])
    rig = Rig("cpu", inp)
    _agree(rig.call(flip), restate(inp, flip), (J, rf, lag, flip))
    for only in (("pred",), ("world",), ("reproj",), ("reproj", "quality")):
        got = rig.call(flip, only)
        _agree(got, restate(inp, flip, only), (J, rf, lag, flip, only))
        for k in OUTPUTS:                                  # an output that was not given is not written
            assert k in only or (got[k] == (pc.FILL32 if k == "pred" else pc.FILL64)).all(), (only, k)


def test_hook_agrees_with_the_reference_functions():
    """streams_poses.npz: normalized2world within 1e-12 m and the undistorted pixel distance within 1e-9 px of the reference's own
    functions (the derived rounding bound is about 3e-12 px: a dozen float64 operations on values <= 2048 px)."""
    z = np.load(os.path.join(GOLDEN, "streams_poses.npz"))
    tags = [str(t) for t in z["tags"]]
    cams = pc.golden_cameras()
    assert tags == [c.name for c in cams]
    rf, lag, J = 9, 4, 17
    inp = pc.make_inputs(3, J, rf, lag, seed=1)
    worst_w = worst_r = 0.0
    rig = Rig("cpu", inp)
    for f in range(z[tags[0] + "/pose"].shape[0]):
        raw = np.stack([z[t + "/pose"][f] for t in tags])
        x = inp["x"].copy()
        x[:, rf - 1 - lag] = np.stack([z[t + "/ray"][f] for t in tags])
        rig.write(raw=raw, x=x)
        got = rig.call(False)
        assert got["rc"] == 0 and same_bits(got["pred"], raw)
        want_w, want_r = np.stack([z[t + "/world"][f] for t in tags]), np.stack([z[t + "/reproj"][f] for t in tags])
        worst_w, worst_r = max(worst_w, np.abs(got["world"] - want_w).max()), max(worst_r, np.abs(got["reproj"] - want_r).max())
        assert np.allclose(got["quality"][:, 0], want_r.mean(1), rtol=0, atol=1e-9) and np.array_equal(got["quality"][:, 1], got["reproj"].max(1))
    print("worst |world - reference| %.3g m, worst |residual - reference| %.3g px" % (worst_w, worst_r))
    assert float(min(z[t + "/zc_min"] for t in tags)) >= 1.0
    assert worst_w <= 1e-12 and worst_r <= 1e-9, (worst_w, worst_r)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_streams_that_did_not_finish_keep_the_fill(flip):
    """emit -1 or status 1 - and nothing else of the stream's rows is read: they hold NaNs with a payload."""
    inp = pc.make_inputs(4, 17, 9, 4, seed=3, emit=[-1, 5, -1, 0], status=[0, 1, 1, 1])
    for k in ("raw", "raw_m", "x"):
        inp[k].view(np.uint32)[:] = 0x7FC00BAD
    inp["desc"][:], inp["cam"][:] = np.nan, np.nan
    got = Rig("cpu", inp).call(flip)
    assert got["rc"] == 0 and pc.untouched(got)
    inp["status"][1] = 0                                   # ... and one that did: its rows alone are written
    got = Rig("cpu", inp).call(flip)
    assert got["rc"] == 0
    for k in OUTPUTS:
        fill = pc.FILL32 if k == "pred" else pc.FILL64
        assert (got[k][[0, 2, 3]] == fill).all() and not (got[k][1] == fill).any(), k
    _agree(got, restate(inp, flip), flip)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("poison", [0x7FC00BAD, 0x7F800000, 0xFF800000], ids=["nan", "inf", "-inf"])
def test_a_non_finite_raw_element_touches_its_point_and_its_quality_words_only(poison, flip):
    inp = pc.make_inputs(3, 17, 9, 0, seed=5)
    clean = Rig("cpu", inp).call(flip)
    for (s, j, k) in ((1, 6, 0), (1, 6, 1), (2, 16, 2)):
        bad = dict(inp, raw=inp["raw"].copy())
        bad["raw"].view(np.uint32)[s, j, k] = poison
        got = Rig("cpu", bad).call(flip)
        _agree(got, restate(bad, flip), (hex(poison), flip, s, j, k))
        for name in ("pred", "world", "reproj"):
            differs = np.argwhere((bits(got[name]) != bits(clean[name])).reshape(3, 17, -1).any(-1)).tolist()
            assert differs == [[s, j]], (name, differs)
        assert same_bits(np.delete(got["quality"], s, 0), np.delete(clean["quality"], s, 0)) and not same_bits(got["quality"][s], clean["quality"][s])
        if not flip:                                       # raw bits that are only copied keep their payload
            assert bits(got["pred"])[s, j, k] == poison
        elif poison == 0x7FC00BAD:                         # a NaN the arithmetic produced is the canonical one
            assert bits(got["pred"])[s, j, k] == 0x7FC00000
        if poison == 0x7FC00BAD:
            assert (bits(got["quality"][s]) == pc.QNAN64).all() and bits(got["reproj"])[s, j] == pc.QNAN64


def test_a_point_behind_the_camera_or_in_its_plane_is_followed():
    """Zc < 0: a mirrored, finite residual; Zc == 0 with Yc == 0: an infinite a and a NaN b - the canonical NaN, not an error."""
    inp = pc.make_inputs(2, 17, 9, 4, seed=6)
    h = inp["desc"][:, 12]
    inp["raw"][0, 3] = (0.25, np.float32(-h[0]) + np.float32(0.5), -4.0)
    inp["desc"][1, 12] = np.float64(np.float32(h[1]))      # a height float32 holds: yy = p[1] + h can be exactly zero
    inp["raw"][1, 8] = (0.25, -np.float32(h[1]), 0.0)
    got = Rig("cpu", inp).call(False)
    _agree(got, restate(inp, False), "behind")
    assert np.isfinite(got["reproj"][0, 3]) and bits(got["reproj"])[1, 8] == pc.QNAN64
    assert np.isfinite(got["quality"][0]).all() and (bits(got["quality"][1]) == pc.QNAN64).all()
    assert np.isfinite(np.delete(got["reproj"][1], 8)).all()


def test_every_argument_rule_is_refused_before_anything_is_written():
    J, rf, lag = 17, 9, 4
    inp = pc.make_inputs(3, J, rf, lag, seed=7)
    rig = Rig("cpu", inp)
    t = rig.t
    ptr = {k: v.data_ptr() for k, v in t.items()}
    not_perm = list(inp["perm"])
    not_perm[2] = not_perm[3]
    span = lambda k: ptr[k] + t[k].numel() * t[k].element_size()      # noqa: E731
    refused = [
        ("raw null", True, OUTPUTS, dict(raw=None)), ("emit null", False, OUTPUTS, dict(emit=None)),
        ("status null", False, OUTPUTS, dict(status=None)), ("desc null with world", False, ("world",), dict(desc=None)),
        ("all outputs null", False, (), {}), ("quality alone", False, ("quality",), {}),
        ("raw_mirror without perm", True, OUTPUTS, dict(perm=None)), ("perm without raw_mirror", False, OUTPUTS, dict(perm=inp["perm"])),
        ("not a permutation", True, OUTPUTS, dict(perm=not_perm)), ("perm entry out of range", True, OUTPUTS, dict(perm=[J] + list(inp["perm"])[1:])),
        ("S = 0", False, OUTPUTS, dict(S=0)), ("S above the maximum", False, OUTPUTS, dict(S=_capi.CLIPS_MAX + 1)),
        ("J = 0", False, OUTPUTS, dict(J=0, perm=None)), ("J = 18", False, OUTPUTS, dict(J=18)),
        ("reproj without cam", False, OUTPUTS, dict(cam=None)), ("reproj without x", False, OUTPUTS, dict(x=None)),
        ("reproj without desc", False, ("reproj",), dict(desc=None)), ("quality without reproj", False, ("pred", "world", "quality"), {}),
        ("RF = 0", False, OUTPUTS, dict(rf=0, lag=0)), ("lag = -1", False, OUTPUTS, dict(lag=-1)), ("lag = RF", False, OUTPUTS, dict(lag=rf)),
        ("S * RF * J too large", False, OUTPUTS, dict(rf=_capi.ENCODE_MAX_POINTS // (3 * J) + 1, lag=0)),
        ("world unaligned", False, OUTPUTS, dict(world=ptr["world"] + 4)), ("reproj unaligned", False, OUTPUTS, dict(reproj=ptr["reproj"] + 4)),
        ("quality unaligned", False, OUTPUTS, dict(quality=ptr["quality"] + 4)), ("cam unaligned", False, OUTPUTS, dict(cam=ptr["cam"] + 4)),
        ("desc unaligned", False, OUTPUTS, dict(desc=ptr["desc"] + 4)), ("emit unaligned", False, OUTPUTS, dict(emit=ptr["emit"] + 4)),
        ("pred on raw", False, OUTPUTS, dict(pred=ptr["raw"])), ("pred ends in raw_mirror", True, OUTPUTS, dict(pred=ptr["raw_m"] - 3 * J * 3 * 4 + 4)),
        ("world starts in x", False, OUTPUTS, dict(world=span("x") - 8)), ("reproj in raw", False, OUTPUTS, dict(reproj=ptr["raw"] + 4)),
        ("quality on raw_mirror", True, OUTPUTS, dict(quality=span("raw_m") - 8)),
    ]
    for what, flip, which, over in refused:
        got = rig.call(flip, which, **over)
        assert got["rc"] == ERR_ARG and pc.untouched(got), what
        assert _capi.load().r3d_last_error(), what
    assert rig.call(True)["rc"] == 0 and rig.call(False, ("pred",), desc=None, cam=None, x=None, rf=0, lag=-3)["rc"] == 0


def test_descriptor_layout_and_the_camera_row():
    cam = pc.golden_cameras()[1]
    row = cam.stream_pose_row()
    assert row.dtype == np.float64 and row.shape == (14,) and _capi.stream_pose_desc_dtype().itemsize == _capi.STREAM_POSE_DESC_BYTES == 112
    d = row.view(_capi.stream_pose_desc_dtype())[0]
    assert np.array_equal(d["rn2w"].reshape(3, 3), cam.Rn2w) and np.array_equal(d["tn2w"], cam.Tn2w.reshape(3))
    assert d["height"] == cam.height and d["reserved"] == 0.0
