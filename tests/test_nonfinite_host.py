"""CPU suite: what a non-finite keypoint does - the helper of the GPU tests must fail when it should, the reference's behaviour
(torch port and C oracle: every output of the window that holds the element is NaN, every other window keeps its bits) pinned
on five configurations, and the pixel pre-pass's per-keypoint routines on the host hooks (r3d_debug_undistort_host,
r3d_debug_encode_px_host, r3d_debug_clips_encode_host): one bad pixel coordinate stays inside its keypoint."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import hooks_library, synth_states
import nonfinite_util as nf
from test_clips_encode_host import FILL, cameras, host_encode, mirror_perm, pixels, run_hook

import ray3d_amd
from ray3d_amd import _capi, synth


# ------------------------------------------------------------------ the helper fails when it should

@pytest.fixture
def unrecorded():
    """The helper's failures are wanted here: keep their figures out of the run's parity table."""
    import conftest
    n = len(conftest.PARITY)
    yield
    del conftest.PARITY[n:]


def _helper_case():
    rng = np.random.default_rng(3)
    clean = rng.normal(0, 1, (6, 1, 17, 3)).astype(np.float32)
    got = clean.copy()
    got[2] = np.nan
    return got, clean


def test_helper_accepts_a_poisoned_window_and_identical_clean_windows(unrecorded):
    got, clean = _helper_case()
    nf.check_poisoned(got, clean, clean.copy(), [2], "helper")
    inf = got.copy()
    inf[2, 0, 5, 1] = np.inf                                    # non-finite, not only NaN
    nf.check_poisoned(inf, clean, clean.copy(), [2], "helper")
    nf.check_poisoned(torch.from_numpy(got), torch.from_numpy(clean), clean.copy(), [2], "helper, tensors")


def test_helper_fails_on_a_finite_value_in_a_poisoned_window(unrecorded):
    got, clean = _helper_case()
    got[2, 0, 16, 2] = 0.25
    with pytest.raises(AssertionError, match="finite output"):
        nf.check_poisoned(got, clean, clean.copy(), [2], "helper")


def test_helper_fails_on_a_nan_in_a_clean_window(unrecorded):
    got, clean = _helper_case()
    got[4, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="differ from the call on finite input"):
        nf.check_poisoned(got, clean, clean.copy(), [2], "helper")


def test_helper_fails_on_one_bit_in_a_clean_window(unrecorded):
    got, clean = _helper_case()
    got.view(np.uint32)[5, 0, 3, 1] ^= 1
    assert np.abs(got[5] - clean[5]).max() < 1e-6                # far inside the parity bound: only the bit comparison sees it
    with pytest.raises(AssertionError, match="differ from the call on finite input"):
        nf.check_poisoned(got, clean, clean.copy(), [2], "helper")


def test_helper_fails_when_the_clean_windows_miss_the_reference(unrecorded):
    got, clean = _helper_case()
    ref = clean.copy()
    ref[0, 0, 0, 0] += 2e-4
    with pytest.raises(AssertionError, match="max abs err"):
        nf.check_poisoned(got, clean, ref, [2], "helper")


def test_put_bits_keeps_signalling_and_payload_bits():
    a = np.zeros(4, np.float32)
    for k, bits in enumerate((0x7FA00000, nf.ACT_SENTINEL, 0xFFC5A1E7, 0xFF800000)):
        nf.put_bits(a, k, bits)
    assert a.view(np.uint32).tolist() == [0x7FA00000, 0x7FC5A1E7, 0xFFC5A1E7, 0xFF800000]
    assert np.isnan(a[:3]).all() and a[3] == -np.inf
    assert nf.windows_to_poison(1) == [0] and nf.windows_to_poison(2) == [0, 1] and nf.windows_to_poison(97) == [0, 48, 96]
    assert nf.positions(27, 17, 3) == [(0, 0, 0), (9, 0, 0), (26, 16, 2)] and nf.positions(27, 17, 2)[1] == (13, 0, 0)
    for rows, elements in nf.rotations(5, 9, 17, 3):
        assert rows == [0, 2, 4] and [e[0] for e in elements] == rows
    assert {e[1:] for _, els in nf.rotations(5, 9, 17, 3) for e in els if e[0] == 2} == set(nf.positions(9, 17, 3))


# ------------------------------------------------------------------ the reference contract

CONFIGS = [pytest.param(dict(ARCHITECTURE="3,3"), id="rf9"),
           pytest.param(dict(ARCHITECTURE="3,3,3", NUM_KPTS=14, STAGE=2), id="rf27-j14-s2"),
           pytest.param(dict(ARCHITECTURE="3,3,3", INPUT_DIM=2, CAMERA_EMBDDING=False), id="rf27-f2-noemb"),
           pytest.param(dict(ARCHITECTURE="3,3,3,3", DISABLE_OPTIMIZATIONS=True, CAUSAL=True), id="rf81-causal-dilated"),
           pytest.param(dict(ARCHITECTURE="3,3", NUM_KPTS=15), id="rf9-j15")]


@pytest.mark.parametrize("over", CONFIGS)
def test_reference_turns_one_bad_element_into_one_all_nan_window(over):
    """torch port and C oracle (both pinned to the reference fixtures): one element of window 2 of 6 set to each value at each of
    five positions - every pos and trj output of that window is NaN (for +-Inf too: NaN, not Inf), the other five windows have
    the bits of the clean run.  The experiments (one group of six windows each) run side by side in one batch per checker:
    windows are independent, and a group that leaked into another would show there."""
    from oracle import oracle, torch_port
    mc = ray3d_amd.default_model_config(**over)
    (cp, sp), (ct, st) = synth_states(mc)
    G, rf, J, F = 6, cp.receptive_field, cp.num_joints, cp.in_features
    x6 = synth.synth_rays(G, cp, seed=601)
    p6 = synth.synth_param(G, seed=602)
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]

    def port(xx, pp):
        with torch.no_grad():
            return [torch_port.forward(c, sd, torch.from_numpy(xx), torch.from_numpy(pp)).numpy() for c, sd in ((cp, sds[0]), (ct, sds[1]))]

    def c_oracle(xx, pp):
        return [oracle.forward(c, s, xx, pp) for c, s in ((cp, sp), (ct, st))]
    spots = nf.positions(rf, J, F) + [(1, 1, F - 1), (rf // 2, J // 2, 0)]
    for name, run, values in (("torch port", port, list(nf.VALUES)), ("C oracle", c_oracle, ["nan", "sentinel", "+inf", "-inf"])):
        cases = [(v, s) for v in values for s in spots]
        x = np.tile(x6, (len(cases), 1, 1, 1))
        p = np.tile(p6, (len(cases), 1))
        bad = x.copy()
        for g, (value, spot) in enumerate(cases):
            nf.put_bits(bad, (G * g + 2,) + spot, nf.VALUES[value])
        hit = np.arange(x.shape[0]) % G == 2
        clean, outs = run(x, p), run(bad, p)
        for o, c in zip(outs, clean):
            assert np.isfinite(c).all()
            nan_rows = np.isnan(o.reshape(o.shape[0], -1)).all(axis=1)
            assert nan_rows[hit].all(), (name, [cases[g] for g in np.flatnonzero(~nan_rows[hit])])
            assert nf.same_bits(o[~hit], c[~hit]), name


# ------------------------------------------------------------------ the pixel pre-pass on the host hooks

BAD_PIXELS = [pytest.param(float("nan"), id="nan"), pytest.param(float("inf"), id="+inf")]
CAM_ROWS = [pytest.param(1, id="distorted"), pytest.param(5, id="zero-coefficients")]     # test_clips_encode_host.cameras()


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _only_this_keypoint(got, clean, k, what):
    """got / clean (n, F) per-keypoint outputs: keypoint k holds a non-finite float, nothing else changed a bit."""
    assert not np.isfinite(got[k]).all(), what
    keep = np.ones(got.shape[0], bool)
    keep[k] = False
    assert np.isfinite(clean).all() and nf.same_bits(got[keep], clean[keep]), what


@pytest.mark.parametrize("cam", CAM_ROWS)
@pytest.mark.parametrize("bad", BAD_PIXELS)
def test_undistort_hook_keeps_a_bad_pixel_inside_its_keypoint(bad, cam):
    lib = hooks_library()
    camera = cameras()[cam]
    row = _f64(camera.cam_row(distortion=True))
    uv = _f64(pixels("nonfinite.undistort", (40, 2)))

    def run(u):
        out_uv, out_rays = np.full_like(u, -7.0), np.full((u.shape[0], 3), -7.0)
        assert lib.r3d_debug_undistort_host(_ptr(row), _ptr(u), u.shape[0], _ptr(out_uv), _ptr(out_rays)) == 0
        return out_uv, out_rays
    clean_uv, clean_rays = run(uv)
    for k, comp in ((0, 0), (17, 1), (39, 0)):
        u = uv.copy()
        u[k, comp] = bad
        got_uv, got_rays = run(u)
        _only_this_keypoint(got_uv, clean_uv, k, (k, comp))
        _only_this_keypoint(got_rays, clean_rays, k, (k, comp))
        # the same floats as the host chain finds non-finite (the reference's arithmetic in NumPy)
        want = camera.rays_from_uv(u)
        assert np.array_equal(np.isfinite(got_rays), np.isfinite(want)), (k, comp, got_rays[k], want[k])


@pytest.mark.parametrize("encoding", ["intrinsic", "screen"])
@pytest.mark.parametrize("cam", CAM_ROWS)
@pytest.mark.parametrize("bad", BAD_PIXELS)
def test_encode_px_hook_keeps_a_bad_pixel_inside_its_keypoint(bad, cam, encoding):
    from ray3d_amd import evaluate
    lib = hooks_library()
    camera = cameras()[cam]
    row = _f64(camera.cam_row(distortion=True))
    uv = _f64(pixels("nonfinite.encode_px", (40, 2)))

    def run(u):
        out = np.full_like(u, -7.0)
        assert lib.r3d_debug_encode_px_host(_ptr(row), _ptr(u), u.shape[0], evaluate.ENCODINGS[encoding], _ptr(out)) == 0
        return out
    clean = run(uv)
    for k, comp in ((0, 1), (17, 0), (39, 1)):
        u = uv.copy()
        u[k, comp] = bad
        got = run(u)
        _only_this_keypoint(got, clean, k, (k, comp))
        want = camera.intrinsic_from_uv(u) if encoding == "intrinsic" else camera.screen_from_uv(u)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (k, comp, got[k], want[k])


@functools.lru_cache(maxsize=None)
def three_clips(J=17):
    """Three clips on three camera rows - two distorted H36M ones, the last with zero coefficients - with pads (and extra
    surplus rows behind) and gaps between them: (table, px (total, J, 2), out_rows, max_rows)."""
    specs = ((20, 13, 0, 0), (31, 13, 5, 1), (9, 4, 0, 6))          # (frames, pad, extra rows behind, camera)
    table = np.zeros(len(specs), dtype=_capi.clip_input_desc_dtype())
    first, ofirst, parts = 2, 1, []
    for c, (n, pad, extra, cam) in enumerate(specs):
        table[c]["first_frame"], table[c]["n_frames"], table[c]["out_first"] = first, n, ofirst
        table[c]["pad_front"], table[c]["pad_back"] = pad, pad + extra
        table[c]["cam"] = cameras()[cam].cam_row(distortion=True)
        parts.append((first, pixels("nonfinite.clips.%d" % c, (n, J, 2))))
        first += n + 3
        ofirst += n + 2 * pad + extra + 2
    px = np.full((first, J, 2), -1.0e3, np.float32)                   # (finite gaps: nothing reads them, and nothing may leak)
    for at, part in parts:
        px[at:at + part.shape[0]] = part
    rows = [int(d["pad_front"] + d["n_frames"] + d["pad_back"]) for d in table]
    for v in (table, px):
        v.setflags(write=False)
    return table, px, ofirst, max(rows)


def bad_clip_pixels(frame, joint, comp, value):
    """three_clips() with one coordinate of the MIDDLE clip set to `value`; -> (px, the output rows that repeat that frame)."""
    table, px, _, _ = three_clips()
    d = table[1]
    n, pf, pb, at = int(d["n_frames"]), int(d["pad_front"]), int(d["pad_back"]), int(d["out_first"])
    bad = np.array(px)
    bad[int(d["first_frame"]) + frame, joint, comp] = value
    rows = [at + pf + frame]
    if frame == 0:
        rows += [at + r for r in range(pf)]
    if frame == n - 1:
        rows += [at + pf + n + r for r in range(pb)]
    return bad, sorted(rows)


def check_clips_encode_outputs(x, xm, clean_x, clean_xm, rows, joint, J=17):
    """Only keypoint `joint` of `rows` (its mirror_perm destination in the mirrored buffer) is non-finite; every other float has
    the bits of the clean run (FILL rows included)."""
    dest = mirror_perm(J).index(joint)                                 # x_mirror[row, dest] = x[row, joint]
    for buf, clean, j in ((x, clean_x, joint), (xm, clean_xm, dest)):
        hit = np.zeros(buf.shape[:2], bool)
        hit[rows, j] = True
        assert not np.isfinite(buf[hit]).all(axis=1).any(), "a repeated row of the bad frame came out finite"
        assert np.isfinite(buf[~hit]).all() and nf.same_bits(buf[~hit], clean[~hit])


CLIP_SPOTS = [(0, 0, 0), (15, 4, 1), (30, 16, 0)]                     # (frame of the middle clip, joint, coordinate)


@pytest.mark.parametrize("encoding", ["ray", "intrinsic", "screen"])
@pytest.mark.parametrize("bad", BAD_PIXELS)
def test_clips_encode_hook_keeps_a_bad_pixel_inside_its_keypoint_and_its_mirrored_slot(bad, encoding):
    """Three clips, flip buffers on: the first frame (repeated into the front pad), a middle one and the last frame (repeated
    into the back pad and the surplus rows) of the middle clip; the status words stay 0."""
    table, px, out_rows, max_rows = three_clips()
    rc, cx, cxm, status = run_hook(17, encoding, table, px, out_rows, max_rows)
    assert rc == 0 and not status.any()
    for frame, joint, comp in CLIP_SPOTS:
        bad_px, rows = bad_clip_pixels(frame, joint, comp, bad)
        assert len(rows) == {0: 14, 15: 1, 30: 19}[frame]
        rc, x, xm, status = run_hook(17, encoding, table, bad_px, out_rows, max_rows)
        assert rc == 0 and not status.any(), (frame, status)
        check_clips_encode_outputs(x, xm, cx, cxm, rows, joint)
        assert (x[0] == FILL).all() and (xm[0] == FILL).all()
        # the host chain finds the same floats non-finite
        cam = cameras()[1]
        want = host_encode(cam, bad_px[int(table[1]["first_frame"]) + frame], encoding)
        assert np.array_equal(np.isfinite(x[rows[0]]), np.isfinite(want)), (frame, x[rows[0], joint], want[joint])
