"""CPU suite, part 2: host logic of the product (no GPU, no compute calls into the HIP library):
C-ABI surface, weight grammar, module shim contract, camera constants, metrics, clip evaluation
logic, clip sharding and the world_size-2 gather over gloo."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, MODEL_CASES, ROOT, dev_switch, hooks_library, load_model_fixture, synth_states

import ray3d_amd
from ray3d_amd import _capi, evaluate, metrics, synth
from ray3d_amd.spec import config_from_dicts, default_model_config, state_entries


# ------------------------------------------------------------------ C ABI surface

def test_library_exports_every_declared_symbol():
    """The product library exports exactly what include/ray3d_hip.h declares outside its R3D_TEST_HOOKS block; the hooks
    build (tests / tools only) the r3d_debug_* entry points on top."""
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
    m = re.search(r"#ifdef R3D_TEST_HOOKS(.*?)#endif /\* R3D_TEST_HOOKS \*/", hdr, flags=re.S)
    assert m, "the header keeps its test hooks in an #ifdef R3D_TEST_HOOKS block"
    hooks_declared = set(re.findall(r"\b(r3d_[a-z_]+)\s*\(", m.group(1)))
    declared = set(re.findall(r"\b(r3d_[a-z_]+)\s*\(", hdr.replace(m.group(0), "")))
    assert declared == set(_capi.EXPORTS), declared ^ set(_capi.EXPORTS)
    assert hooks_declared == set(_capi.HOOK_EXPORTS), hooks_declared ^ set(_capi.HOOK_EXPORTS)
    for path, want in ((_capi.LIB_PATH, declared), (_capi.HOOKS_LIB_PATH, declared | hooks_declared)):
        lib = ctypes.CDLL(path)
        for name in want:
            assert hasattr(lib, name), (path, name)
        # ... and nothing else under the r3d_ prefix
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r"\b[TW] (r3d_[a-z_0-9]+)$", out, flags=re.M))
        assert exported == want, (path, exported ^ want)
    assert b"gfx950" in _capi.load().r3d_version()
    # the product library reads no development switch: none of their names is in its strings
    blob = open(_capi.LIB_PATH, "rb").read()
    for name in (b"R3D_FAULT_TILE", b"R3D_NO_SMALL_PLAN", b"R3D_NO_GEMV", b"R3D_NO_LAT", b"R3D_SCHED_DUMP", b"R3D_COST"):
        assert name not in blob, name


# one kernel per elementwise entry point (ray3d_amd/csrc/r3d_k_elementwise.hip) -> the bytes of static LDS it declares.  The sizes are
# the kernels' own constants, restated from the limits of include/ray3d_hip.h that size them:
#   res[17] doubles                                     (streams_poses_body)
#   STREAMS_FUSE_STAGE * STREAMS_FUSE_JOINTS doubles    (r3d_streams_fuse.hpp)
#   STREAMS_ASSIGN_LDS_BYTES                            (r3d_streams_assign.hpp)
#   STREAMS_LINK_LDS_BYTES                              (r3d_streams_link.hpp)
#   CLIPS_REPAIR_LDS_BYTES                              (r3d_clips_repair.hpp)
ELEMENTWISE_KERNELS = {
    "r3d_undistort_rays_f64": 0, "r3d_k_clips_encode": 0, "r3d_k_clips_poses": 0, "r3d_k_clips_project": 0, "r3d_k_clips_windows": 0,
    "r3d_k_pack": 0, "r3d_k_streams_advance": 0, "r3d_k_streams_gather": 0, "r3d_k_streams_repair": 0, "r3d_k_streams_peek": 0,
    "r3d_k_streams_poses": 136, "r3d_k_streams_fuse": 8704, "r3d_k_streams_assign": 8576, "r3d_k_streams_link": 8320,
    "r3d_k_clips_repair": 8272,
}

PRODUCT_KERNELS = {
    "r3d_bind_f32", "r3d_decode_f32", "r3d_decode_w4_f32", "r3d_clip_metrics_f64", "r3d_clip_metrics_sum_f64",
    "r3d_gemm_f32", "r3d_gemm_uv_f32", "r3d_gemm_b3", "r3d_gemm_uv_b3", "r3d_gemm_enc_f32", "r3d_gemm_enc_uv_f32",
    "r3d_forward_f32", "r3d_forward_uv_f32", "r3d_forward_b3", "r3d_forward_uv_b3", "r3d_forward_lat", "r3d_forward_uv_lat",
    "r3d_forward_clip_f32", "r3d_forward_clip_uv_f32",
} | set(ELEMENTWISE_KERNELS)


def _gfx950_kernels(path, tmp_path):
    """(name, metadata record) of the kernels in the gfx950 code object(s) of a shared library: the offload bundle's entries of
    that target, their metadata notes read with the ROCm LLVM's llvm-readelf (the toolchain build() compiles with)."""
    import struct
    import subprocess
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), readelf
    data = open(path, "rb").read()
    magic, kernels, pos, k = b"__CLANG_OFFLOAD_BUNDLE__", [], 0, 0
    while (i := data.find(magic, pos)) >= 0:
        n, = struct.unpack_from("<Q", data, i + 24)
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                co = tmp_path / ("%s.%d.co" % (os.path.basename(path), k))
                k += 1
                co.write_bytes(data[i + off:i + off + size])
                txt = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
                rec = {}
                for key, val in re.findall(r"^\s+-?\s*\.(\w+):\s+'?([\w.$]+?)'?\s*$", txt, flags=re.M):
                    rec[key] = val
                    if key != "wavefront_size" or "symbol" not in rec:      # .wavefront_size ends a kernel's record
                        continue
                    assert rec["symbol"].endswith(".kd"), rec["symbol"]
                    sym = rec["symbol"][:-3]
                    # extern "C" kernels carry their own name; the metrics kernels sit in an anonymous namespace: the last
                    # <length><identifier> of the Itanium nested name _ZN...E
                    rest = sym[3:] if sym.startswith("_ZN") else ""
                    while (m := re.match(r"\d+", rest)):
                        sym, rest = rest[m.end():m.end() + int(m.group())], rest[m.end() + int(m.group()):]
                    kernels.append((sym, rec))
                    rec = {}
        pos = i + 24
    return kernels


def test_libraries_hold_exactly_the_documented_kernels(tmp_path):
    """The gfx950 code object of the product library holds the documented kernels and nothing else - no experiment's kernel
    rides along (one did: a rejected first-level tile was linked in and had its LDS attribute set in every process) - and the
    hooks library, which links the same kernel objects, holds the same set.  Each elementwise kernel takes what its own body
    needs: no scratch, no spilled register, and exactly the LDS it declares.
    (No assertion on scratch for the others: r3d_forward_lat, the r3d_gemm_* kernels of the level-by-level form and
    r3d_clip_metrics_f64 do use a few bytes of it - tools/kernel_resources.py prints the figures.)"""
    hdr = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
    lim = {n: int(v) for n, v in re.findall(r"#define R3D_(ASSIGN_MAX_SLOTS|ASSIGN_MAX_DETECTIONS|LINK_MAX_PEOPLE|FUSE_MAX_MEMBERS|REPAIR_MAX_ROWS) (\d+)", hdr)}
    slots, dets, people = lim["ASSIGN_MAX_SLOTS"], lim["ASSIGN_MAX_DETECTIONS"], lim["LINK_MAX_PEOPLE"]
    assert ELEMENTWISE_KERNELS["r3d_k_streams_fuse"] == 8 * 4 * lim["FUSE_MAX_MEMBERS"] * 17
    assert ELEMENTWISE_KERNELS["r3d_k_streams_assign"] == 8 * slots * dets + 8 * dets + 4 * dets
    assert ELEMENTWISE_KERNELS["r3d_k_streams_link"] == 8 * people * slots + 4 * slots
    assert ELEMENTWISE_KERNELS["r3d_k_clips_repair"] == lim["REPAIR_MAX_ROWS"] // 8 + 4 * 4 + 4 * 4 * 4
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        kernels = _gfx950_kernels(path, tmp_path)
        names = [name for name, _ in kernels]
        assert len(names) == len(set(names)), (path, sorted(names))
        assert set(names) == PRODUCT_KERNELS, (path, set(names) ^ PRODUCT_KERNELS)
        for name, rec in kernels:
            if name in ELEMENTWISE_KERNELS:
                assert int(rec["private_segment_fixed_size"]) == 0, (path, name, rec["private_segment_fixed_size"])
                assert int(rec["vgpr_spill_count"]) == 0, (path, name, rec["vgpr_spill_count"])
                assert int(rec["group_segment_fixed_size"]) == ELEMENTWISE_KERNELS[name], (path, name, rec["group_segment_fixed_size"])


@pytest.mark.parametrize("name", MODEL_CASES)
def test_c_grammar_equals_python_spec(name):
    _, mc = load_model_fixture(name)
    for kind in ("pos", "trj"):
        cfg = config_from_dicts(mc, kind)
        h = _capi.Handle(cfg)
        want = {e.key: tuple(e.shape) for e in state_entries(cfg) if e.role != "bn_count"}
        keys = h.keys()
        assert set(keys) == set(want)
        for i, k in enumerate(keys):
            assert h.shape(i) == want[k], k
        h.close()


def test_set_weight_is_strict_and_loud():
    cfg = config_from_dicts(default_model_config(), "trj")
    h = _capi.Handle(cfg)
    w = np.zeros((256, 153, 3), np.float32)
    h.set_weight("LocalLayer.expand_conv.weight", w)
    h.set_weight("module.LocalLayer.expand_conv.weight", w)            # DataParallel prefix accepted
    with pytest.raises(_capi.Ray3DHipError, match="unexpected key"):
        h.set_weight("LocalLayer.nonexistent.weight", w)
    with pytest.raises(_capi.Ray3DHipError, match="size mismatch"):
        h.set_weight("LocalLayer.expand_conv.weight", np.zeros((256, 153, 1), np.float32))
    with pytest.raises(_capi.Ray3DHipError, match="Missing key"):
        h.finalize()                                                    # most tensors were never set
    h.close()


def test_create_rejects_unsupported_configs():
    for over in (dict(NUM_KPTS=16), dict(INPUT_DIM=4), dict(CHANNELS=250)):
        with pytest.raises((ValueError, _capi.Ray3DHipError)):
            _capi.Handle(config_from_dicts(default_model_config(**over), "pos"))
    # CAUSAL with the strided convolutions is the pairing the reference's own forward raises on (rie.py:94-97)
    for over in (dict(CAUSAL=True), dict(ARCHITECTURE="3,5")):
        with pytest.raises(NotImplementedError):
            config_from_dicts(default_model_config(**over), "pos")
    # DENSE is read and ignored by the strided constructor branch (rie.py:54-55); with DISABLE_OPTIMIZATIONS it is the
    # dense-convolution ablation: 2 * 3^i + 1 taps per level (:49-53)
    plain = config_from_dicts(default_model_config(DENSE=True), "pos")
    assert not plain.dense_convs and plain.level_taps(1) == 3
    dense = config_from_dicts(default_model_config(ARCHITECTURE="3,3,3", DENSE=True, DISABLE_OPTIMIZATIONS=True), "trj")
    assert dense.dense_convs and (dense.level_taps(1), dense.level_taps(2)) == (7, 19)
    h = _capi.Handle(dense)
    shapes = {k: h.shape(i) for i, k in enumerate(h.keys())}
    assert shapes["LocalLayer.layers_conv.0.weight"] == (256, 256, 7) and shapes["LocalLayer.layers_conv.2.weight"] == (256, 256, 19)
    h.close()
    with pytest.raises(_capi.Ray3DHipError, match="num_levels"):       # evaluated at every position: short receptive fields only
        _capi.Handle(config_from_dicts(default_model_config(ARCHITECTURE="3,3,3,3,3", DENSE=True, DISABLE_OPTIMIZATIONS=True), "pos"))
    assert config_from_dicts(default_model_config(DISABLE_OPTIMIZATIONS=True), "pos").residual_tap == 1
    assert config_from_dicts(default_model_config(DISABLE_OPTIMIZATIONS=True, CAUSAL=True), "trj").residual_tap == 2
    bad = _capi.Config(_capi.C.sizeof(_capi.Config), 0, 17, 3, 2, 256, 256, 3, 2, 64, 7, 0, 0)
    with pytest.raises(_capi.Ray3DHipError, match="causal"):
        _capi.check(_capi.load().r3d_create(_capi.C.byref(bad), _capi.C.byref(_capi.C.c_void_p())), "r3d_create")
    # a binding built against an older, shorter r3d_config (no struct_size / fewer fields) is refused, not mis-read
    old = _capi.Config(0, 17, 3, 2, 256, 256, 3, 2, 64, 0, 0, 0, 0)
    with pytest.raises(_capi.Ray3DHipError, match="struct_size"):
        _capi.check(_capi.load().r3d_create(_capi.C.byref(old), _capi.C.byref(_capi.C.c_void_p())), "r3d_create")
    assert _capi.load().r3d_abi_version() == _capi.ABI_VERSION and ("ABI %d" % _capi.ABI_VERSION).encode() in _capi.load().r3d_version()


def test_forward_before_finalize_fails():
    cfg = config_from_dicts(default_model_config(), "trj")
    h = _capi.Handle(cfg)
    inp = _capi.make_input(_capi.R3D_INPUT_RAYS, 1 << 20, 9, 1 << 20, 2)
    with pytest.raises(_capi.Ray3DHipError, match="finalize"):
        _capi.forward(h, inp, 4, 1 << 20, 1 << 20, 1 << 30, 0)
    h.close()


# ------------------------------------------------------------------ nn.Module shim

def test_module_state_dict_contract():
    mc = default_model_config(ARCHITECTURE="3,3,3")
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    assert pos.receptive_field() == 27 and trj.receptive_field() == 27
    (cp, sp), (ct, st) = synth_states(mc)
    pre = "module." if torch.cuda.is_available() else ""     # with a GPU the factory returns the reference's DataParallel face
    assert set(pos.state_dict().keys()) == {pre + k for k in sp}
    assert set(trj.state_dict().keys()) == {pre + k for k in st}
    for k, v in pos.state_dict().items():
        assert tuple(v.shape) == tuple(np.asarray(sp[k[len(pre):]]).shape), k
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()}
    pos.load_state_dict(sd, strict=True)
    pos.load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)   # DataParallel checkpoint
    bad = dict(sd)
    bad.pop("GlobalInfo.fc_1.weight")
    with pytest.raises(RuntimeError, match="Missing key"):
        ray3d_amd.load_weight(pos, bad)
    assert sum(p.numel() for p in pos.parameters()) > 39e6          # 39.5 M parameters at RF 27
    assert len(list(pos.named_parameters())) > 100
    assert fac.get_trj_model() is trj
    fac2 = ray3d_amd.Model(default_model_config(TRAJECTORY_MODEL=False), {}, is_train=True)
    assert fac2.get_trj_model() is None


def test_module_forward_guards():
    mc = default_model_config()
    pos = ray3d_amd.RIEModel(config_from_dicts(mc, "pos"))
    x = torch.zeros(2, 9, 17, 3)
    p = torch.zeros(2, 2)
    with pytest.raises(RuntimeError, match="inference-only"):
        pos.train()(x, p)
    with pytest.raises(RuntimeError, match="no.*CPU fallback|AMD GPU"):
        pos.eval()(x, p)
    with pytest.raises(AssertionError):
        pos(torch.zeros(2, 9, 16, 3), p)
    with pytest.raises(RuntimeError, match="9-frame"):
        pos(torch.zeros(2, 27, 17, 3), p)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "ray3d_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f
                assert "ray3d_oracle" not in text or f == "spec.py", f


# ------------------------------------------------------------------ synthetic generator pin

def test_synth_generator_is_pinned():
    u = synth.hash_uniform("pin", (4,), seed=7)
    assert np.allclose(u, synth.hash_uniform("pin", (4,), seed=7))
    assert not np.allclose(u, synth.hash_uniform("pin", (4,), seed=8))
    z, mc = load_model_fixture("j17_rf27_s3")
    cfg = config_from_dicts(mc, "pos")
    assert np.array_equal(synth.synth_rays(3, cfg, seed=3), z["x"])          # inputs regenerate bit-exactly
    assert np.array_equal(synth.synth_param(3, seed=4), z["param"])


# ------------------------------------------------------------------ camera + metrics

def test_camera_matches_reference():
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    for tag in z["tags"]:
        cam = ray3d_amd.Camera(z[tag + "/K"], z[tag + "/R"], z[tag + "/t"])
        assert abs(cam.height - float(z[tag + "/height"])) < 1e-12
        assert abs(cam.pitch - float(z[tag + "/pitch"])) < 1e-12
        for n in ("Rc2n", "Tc2n", "Rn2w", "Tn2w", "Rw2n", "Tw2n"):
            assert np.abs(getattr(cam, n) - z[tag + "/" + n]).max() < 1e-12, (tag, n)
        assert np.abs(cam.rays_from_uv(z[tag + "/uv"]) - z[tag + "/rays"]).max() < 1e-12
        assert np.abs(cam.uv_from_rays(z[tag + "/rays"]) - z[tag + "/uv"]).max() < 1e-9
        assert np.abs(cam.world2normalized(z[tag + "/Xw"]) - z[tag + "/Xn"]).max() < 1e-12
        assert np.abs(cam.normalized2world(z[tag + "/Xn"]) - z[tag + "/Xw_back"]).max() < 1e-12
        assert np.abs(cam.project(z[tag + "/Xw"]) - z[tag + "/proj"]).max() < 1e-8
        assert cam.param().dtype == np.float32 and cam.cam_row().shape == (8,)
    s9 = ray3d_amd.Camera(z["h36m_S9_0/K"], z["h36m_S9_0/R"], z["h36m_S9_0/t"])
    assert np.allclose(s9.param(), [1.4812, 0.18404], atol=2e-4)    # the constants BASELINE.md quotes
    with pytest.raises(ValueError):
        ray3d_amd.Camera(z["h36m_S9_0/K"], z["h36m_S9_0/R"], z["h36m_S9_0/t"], undistort=True)   # no coefficients given


def test_camera_undistortion_is_unpinned_but_consistent():
    """undistort=True (H36M default): no reference vector exists (OpenCV absent) - the product code must agree
    with the oracle's restatement and satisfy the weak known-answer relations of SURVEY 8c."""
    import ray3d_amd
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    K = z["h36m_S9_0/K"]
    dist = np.array([-0.207098910824901, 0.247775183068982, -0.00142447157470321, -0.000975698859470499,
                     -0.00307515035078854])                                  # (rad0, rad1, tan0, tan1, rad2): h36m_dataset.py:378-380
    cam = ray3d_amd.Camera(K, z["h36m_S9_0/R"], z["h36m_S9_0/t"], dist_coeff=dist, undistort=True)
    pts = np.stack(np.meshgrid(np.linspace(100, 900, 9), np.linspace(100, 900, 9)), -1).reshape(-1, 2)
    und = cam.undistort_points(pts)
    assert np.abs(und - oracle.undistort_points(K, dist, pts)).max() < 1e-9
    assert np.abs(cam.distort_points(und) - pts).max() < 2e-2              # centi-pixel round trip after 5 iterations
    pp = np.array([[K[0, 2], K[1, 2]]])
    assert np.abs(cam.undistort_points(pp) - pp).max() < 1e-9             # the principal point is a fixed point
    plain = ray3d_amd.Camera(K, z["h36m_S9_0/R"], z["h36m_S9_0/t"])
    assert np.abs(cam.rays_from_uv(pts) - plain.rays_from_uv(und)).max() < 1e-12   # encode = undistort, then the usual rays
    assert np.abs(cam.rays_from_uv(pts) - plain.rays_from_uv(pts)).max() > 1e-4    # ... and it is not a no-op


def test_3dhp_cameras_match_reference():
    """All 14 MPI-INF-3DHP cameras (BASELINE configs[3] draws one per window): product and oracle against the
    reference's CameraInfoPacket (tests/golden/cameras_3dhp.npz)."""
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "cameras_3dhp.npz"))
    assert len(z["tags"]) == 14
    seen = set()
    for tag in z["tags"]:
        for cam in (ray3d_amd.Camera(z[tag + "/K"], z[tag + "/R"], z[tag + "/t"]),
                    oracle.Camera(z[tag + "/K"], z[tag + "/R"], z[tag + "/t"])):
            assert abs(cam.height - float(z[tag + "/height"])) < 1e-12
            assert abs(cam.pitch - float(z[tag + "/pitch"])) < 1e-12
            assert np.abs(cam.Rn2w - z[tag + "/Rn2w"]).max() < 1e-12 and np.abs(cam.Tn2w - z[tag + "/Tn2w"]).max() < 1e-12
            assert np.abs(cam.rays_from_uv(z[tag + "/uv"]) - z[tag + "/rays"]).max() < 1e-12
        seen.add((round(float(z[tag + "/height"]), 6), round(float(z[tag + "/pitch"]), 6)))
    assert len(seen) >= 10          # they really are different cameras (heights / pitches)


def test_undistortion_inverts_the_references_distortion_model():
    """The undistortion is cv2.undistortPoints in the reference (camera.py:412-421; OpenCV absent: PARITY UNPINNED vs cv2).
    What the reference itself holds is the forward model, distortPoint (data/camera_augmentation.py:502-542): its outputs
    on a pixel grid for the four H36M coefficient sets are in undistort.npz, and undistorting them must give the grid
    back - for the product and for the oracle - and the product's own forward model must BE distortPoint."""
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "undistort.npz"))
    worst = 0.0
    for i in range(int(z["n"])):
        K, dist, ideal, distorted = z["cam%d/K" % i], z["cam%d/dist" % i], z["cam%d/ideal" % i], z["cam%d/distorted" % i]
        cam = ray3d_amd.Camera(K, np.eye(3), np.zeros(3) + [0, 0, 4.0], dist_coeff=dist, undistort=True)
        assert np.abs(cam.distort_points(ideal) - distorted).max() < 1e-9
        assert np.abs(oracle.distort_points(K, dist, ideal) - distorted).max() < 1e-9
        # the image's inner 80 %: where the fixed five iterations have converged to a centi-pixel (H36M keypoints live there)
        w, h = 2 * K[0, 2], 2 * K[1, 2]
        inner = (np.abs(ideal[:, 0] - K[0, 2]) < 0.4 * w) & (np.abs(ideal[:, 1] - K[1, 2]) < 0.4 * h)
        for und in (cam.undistort_points(distorted), oracle.undistort_points(K, dist, distorted)):
            err = np.abs(und - ideal)
            worst = max(worst, err[inner].max())
            assert err[inner].max() < 1e-2, (i, err[inner].max())
            assert err.max() < 0.5, (i, err.max())              # corners: still sub-pixel after five iterations
        assert np.abs(distorted - ideal).max() > 5.0            # ... of a distortion of many pixels
    print("undistort(distortPoint_ref(p)) - p: worst inner-grid error %.2e px" % worst)


# What five iterations leave on the dense grid, per H36M coefficient set (pixels; tests/golden/make_golden.py gen_undistort,
# INTEGRATION.md section 5): the residual a maintainer with OpenCV should also see from
# cv2.undistortPoints(distortPoint(grid), K, dist, P=K) against the grid.
UNDISTORT_RES5_PX = {0: (4.3e-6, 5.6e-6), 1: (3.9e-6, 5.0e-6), 2: (4.1e-6, 5.2e-6), 3: (5.7e-6, 8.4e-6)}   # (inner 80 %, whole image)


def test_undistortion_is_opencvs_five_iteration_inverse_on_a_dense_grid():
    """The ALGORITHM pin of the one boundary that stays unpinned against cv2 itself (opencv-python 4.4.0.42 is not in the
    image and cannot be installed): the reference's distortPoint on a dense 65 x 65 grid over the whole image for the four
    H36M coefficient sets, and - restated a third time, in the fixture generator, independently of product and oracle - what
    cv2.undistortPoints(pts, K, dist, P=K) is documented to compute: exactly five fixed-point iterations
    (cvUndistortPointsInternal, default TermCriteria(MAX_ITER, 5, 0.01)).  Product and oracle must reproduce that result
    point by point, the residual against the true inverse must be the documented one per camera (micro-pixels: five
    iterations are converged for H36M's lenses), and the iteration itself must converge to the grid (200 iterations)."""
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "undistort.npz"))
    for i in range(int(z["n"])):
        K, dist = z["cam%d/K" % i], z["cam%d/dist" % i]
        ideal, distorted, und5, inner = (z["cam%d/dense_%s" % (i, k)] for k in ("ideal", "distorted", "und5", "inner"))
        assert ideal.shape == (65 * 65, 2) and inner.sum() > 2000
        cam = ray3d_amd.Camera(K, np.eye(3), np.zeros(3) + [0, 0, 4.0], dist_coeff=dist, undistort=True)
        assert np.abs(cam.distort_points(ideal) - distorted).max() < 1e-9          # the product's forward model IS distortPoint
        for und in (cam.undistort_points(distorted), oracle.undistort_points(K, dist, distorted)):
            assert np.abs(und - und5).max() < 1e-9, i                               # the same five iterations, point by point
            res = np.abs(und - ideal).max(axis=1)
            want_inner, want_all = UNDISTORT_RES5_PX[i]
            assert res[inner].max() <= want_inner and res.max() <= want_all, (i, res[inner].max(), res.max())
            assert abs(res[inner].max() - float(z["cam%d/res5_inner_max" % i])) < 1e-9
            assert abs(res.max() - float(z["cam%d/res5_all_max" % i])) < 1e-9
        assert float(z["cam%d/res200_max" % i]) < 1e-9                              # ... of an iteration that converges to the grid
        assert np.abs(distorted - ideal).max() > 20.0                               # (a distortion of tens of pixels at the corners)


def test_metrics_match_reference():
    z = np.load(os.path.join(GOLDEN, "losses.npz"))
    a, b = torch.from_numpy(z["pred"]), torch.from_numpy(z["target"])
    assert abs(float(metrics.mpjpe(a, b)) - float(z["mpjpe"])) < 1e-12
    assert abs(float(metrics.n_mpjpe(a, b)) - float(z["n_mpjpe"])) < 1e-12
    assert abs(float(metrics.p_mpjpe(a.reshape(-1, 17, 3), b.reshape(-1, 17, 3))) - float(z["p_mpjpe"])) < 1e-10
    assert abs(float(metrics.mean_velocity_error(a.reshape(-1, 17, 3), b.reshape(-1, 17, 3))) - float(z["mpjve"])) < 1e-12


# ------------------------------------------------------------------ evaluation loop (oracle as the lifter)

def _evalcore_clips():
    z = np.load(os.path.join(GOLDEN, "evalcore.npz"))
    clips = []
    for ci in range(3):
        cam = ray3d_amd.Camera(z["clip%d/K" % ci], z["clip%d/R" % ci], z["clip%d/t" % ci])
        clips.append(evaluate.Clip(cam, z["clip%d/rays" % ci], z["clip%d/gt_norm" % ci], action="A", clip_id=ci))
    return z, clips


def _oracle_lift_clip():
    """CPU stand-in for Ray3DLifter.forward_clip built on the oracle (checker role only)."""
    from oracle import oracle
    mc = default_model_config(ARCHITECTURE="3,3,3")
    (cp, sp), (ct, st) = synth_states(mc)

    def lift(padded, prow):
        pad = padded.numpy()
        n = pad.shape[0] - 27 + 1
        win = np.stack([pad[i:i + 27] for i in range(n)])
        par = np.tile(prow.numpy(), (n, 1))
        return torch.from_numpy(oracle.forward(cp, sp, win, par) + oracle.forward(ct, st, win, par))
    return lift


@pytest.mark.parametrize("flip", [False, True])
def test_evaluate_reproduces_reference_evaluate_core(flip):
    z, clips = _evalcore_clips()
    lift = _oracle_lift_clip()
    named, avg, rows = evaluate.evaluate_clips(lift, clips, 27, "cpu", flip=flip,
                                               kps_left=list(z["kps_left"]), kps_right=list(z["kps_right"]))
    ref = z["metrics_flip%d" % int(flip)]
    got = np.array(named["A"])
    assert np.abs(got - ref).max() < 2e-2, (got, ref)     # millimetres; reference works in fp32
    per_clip = evaluate.reduce_partials(torch.cat([rows[:, :1] * 0 + 0, rows[:, 0:1], rows[:, 2:]], dim=1))
    for ci in range(3):
        assert np.abs(np.array(per_clip[ci]) - z["clip%d/metrics_flip%d" % (ci, int(flip))]).max() < 2e-2
    if not flip:
        pred0 = evaluate.predict_clip(lift, clips[0], 27, "cpu").numpy()
        assert np.abs(pred0 - z["clip0/predictions"]).max() < 5e-5


def test_pad_clip_is_edge_padding():
    a = np.arange(24, dtype=np.float32).reshape(4, 2, 3)
    assert np.array_equal(evaluate.pad_clip(a, 3), np.pad(a, ((3, 3), (0, 0), (0, 0)), "edge"))
    assert np.array_equal(evaluate.pad_clip(a, 3, 3), np.pad(a, ((6, 0), (0, 0), (0, 0)), "edge"))   # causal


def test_shard_clips_partitions_and_balances():
    rng = np.random.default_rng(0)
    lengths = rng.integers(1000, 6000, size=236).tolist()
    for world in (1, 2, 4, 8):
        shards = evaluate.shard_clips(lengths, world)
        flat = sorted(i for s in shards for i in s)
        assert flat == list(range(236))
        loads = [sum(lengths[i] for i in s) for s in shards]
        assert max(loads) - min(loads) <= max(lengths)
    assert evaluate.shard_clips([5, 5], 4) == [[0], [1], [], []]


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _, clips = _evalcore_clips()
        clips[1].action = "B"
        named, avg, rows = evaluate.evaluate_clips(_oracle_lift_clip(), clips, 27, "cpu", rank=rank, world_size=world)
        q.put((rank, named, avg, rows.numpy()))
    finally:
        dist.destroy_process_group()


def _free_port():
    """A TCP port nobody listens on right now (a fixed port derived from the pid can collide between parallel test runs)."""
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


def test_two_rank_gather_matches_single_process():
    import torch.multiprocessing as mp
    _, clips = _evalcore_clips()
    clips[1].action = "B"
    named1, avg1, rows1 = evaluate.evaluate_clips(_oracle_lift_clip(), clips, 27, "cpu")
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
    for rank, named, avg, rows in res:
        assert avg == avg1
        for a in named1:
            assert np.allclose(named[a], named1[a], rtol=0, atol=1e-9)
        assert sorted(rows[:, 0].tolist()) == [0.0, 1.0, 2.0]


def _standin_pred(clip):
    """A cheap deterministic stand-in for the lifted poses of a clip (the arithmetic under test is the sharding, the
    per-rank rows and the gather, not the forward): ground truth plus a smooth function of the rays."""
    n = clip.rays.shape[0]
    return torch.from_numpy((clip.gt_norm + 0.01 * np.sin(7.0 * clip.rays[..., :3])).astype(np.float32)).reshape(n, 1, -1, 3)


def _bench_eval_rows(world, rank, n_clips, length_div, gather):
    """bench.py --mode eval's pass with the stand-in above: the same partition (bench.eval_partition), the same
    once-per-evaluation header upload (evaluate.partial_rows), the same gather, the same summary."""
    import bench
    part = bench.eval_partition(n_clips, world, length_div=length_div)
    mine = [bench.make_clip(idx, part["lengths"][idx], part["cams"]) for idx in part["shards"][rank]]
    local = evaluate.partial_rows([(c.clip_id, part["aid"][c.action], c.rays.shape[0]) for c in mine], "cpu")
    for k, c in enumerate(mine):
        local[k, 3:8] = evaluate.clip_partials(_standin_pred(c), c, part["aid"][c.action])[3:8]
    return gather(local, [len(s) for s in part["shards"]]), part


def _gloo_eval_worker(rank, world, port, q, n_clips, length_div):
    import torch.distributed as dist
    import bench
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        rows, _ = _bench_eval_rows(world, rank, n_clips, length_div, evaluate.gather_partials)
        q.put((rank, bench.eval_summary(rows), sorted(int(v) for v in rows[:, 0].tolist())))
    finally:
        dist.destroy_process_group()


def test_bench_eval_sharding_and_gather_at_world_size_8_matches_world_size_1():
    """bench.py --mode eval --gpus 8 on CPU over gloo: the 240-clip set (shortened clips) sharded longest-first over EIGHT
    ranks, every rank's rows built as the bench builds them, one all_gather - the gathered MPJPE, the other four action
    averages and the checksum equal the single-process values exactly, on every rank; every clip appears once."""
    import torch.multiprocessing as mp
    import bench
    n_clips, div = 240, 40
    rows1, part1 = _bench_eval_rows(1, 0, n_clips, div, lambda local, counts: local)
    want = bench.eval_summary(rows1)
    assert sorted(len(s) for s in bench.eval_partition(n_clips, 8)["shards"]) == [30] * 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_eval_worker, args=(r, 8, port, q, n_clips, div)) for r in range(8)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(8)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(r for r, _, _ in res) == list(range(8))
    for rank, got, ids in res:
        assert ids == list(range(n_clips)), rank
        for k in want:
            # the per-clip sums are computed by the same code on the same data whatever the rank; only the row ORDER of the
            # gathered matrix differs, and the summary sorts / groups before it adds
            assert abs(got[k] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), (rank, k, got[k], want[k])


def _gloo_eval_pass_worker(rank, world, port, q, n_clips, length_div):
    import torch.distributed as dist
    import bench
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)

        def max_over_ranks(v):
            t = torch.tensor([v], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())

        def all_ranks(v):
            t = torch.tensor([v], dtype=torch.float64)
            bucket = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(bucket, t)
            return [float(b.item()) for b in bucket]

        def lift(c, out_row):
            out_row[3:8] = evaluate.clip_partials(_standin_pred(c), c, 0)[3:8]

        res = bench.eval_pass(None, "cpu", dist, world, rank, n_clips, 1, 0, dist.barrier, max_over_ranks, all_ranks,
                              length_div=length_div, lift=lift)
        res.pop("_mine")
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


def test_bench_dump_outputs_keeps_small_arrays_and_samples_large_ones_under_the_cap(tmp_path):
    """bench.py --dump-outputs: float32 / float64 kept as they are, other types as float64; an output beyond its share of the
    64 MB budget becomes a fixed sample of its rows - the same rows on every run - and all files together stay within it."""
    import bench
    small = np.random.default_rng(1).random((256, 1, 17, 3)).astype(np.float32)
    big = np.random.default_rng(2).random((600000, 1, 17, 3)).astype(np.float32)       # 122 MB
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"poses": small, "big": big, "ids": np.arange(10)})
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_LIMIT_BYTES
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("poses", "big", "ids")}
    assert np.array_equal(a["poses"], small) and a["ids"].dtype == np.float64 and np.array_equal(a["ids"], np.arange(10))
    assert a["big"].dtype == np.float32 and a["big"].shape[1:] == big.shape[1:] and 0 < a["big"].shape[0] < big.shape[0]
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
    idx = [int(np.flatnonzero(big[:, 0, 0, 0] == r[0, 0, 0])[0]) for r in a["big"][:100]]       # (the sample is rows of the output, in order)
    assert idx == sorted(idx) and all(np.array_equal(big[i], r) for i, r in zip(idx, a["big"]))
    bench.dump_outputs(str(tmp_path / "r"), {"poses": big}, world=2, rank=1)
    assert [f.name for f in (tmp_path / "r").iterdir()] == ["poses_rank1.npy"]
    assert (tmp_path / "r" / "poses_rank1.npy").stat().st_size <= bench.DUMP_LIMIT_BYTES // 2


def test_bench_eval_pass_object_at_world_size_8_over_gloo():
    """bench.eval_pass - the object the driver's `bench.py --gpus N` line carries under a process group (north_star's split:
    whole clips sharded over the ranks, ONE all_gather of the per-clip rows) - run as the bench runs it, on eight CPU ranks
    over gloo with a stand-in for the lifted poses: the gathered MPJPE / checksum equal the single-process values, every
    rank's re-lift of a neighbour's clip equals the gathered row bit for bit, and the line's fields are there."""
    import torch.multiprocessing as mp
    import bench
    n_clips, div, world = 240, 40, 8
    rows1, part1 = _bench_eval_rows(1, 0, n_clips, div, lambda local, counts: local)
    want = bench.eval_summary(rows1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_eval_pass_worker, args=(r, world, port, q, n_clips, div)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    r0 = res[0]
    for k in ("value", "ms_per_pass", "shard_frames", "shard_imbalance", "pass_ms_per_rank", "pass_ms_imbalance", "all_gather_ms",
              "world_size_observed", "cross_rank_rows_bit_equal", "mpjpe_mm", "frames", "clips"):
        assert k in r0, k
    assert r0["world_size_observed"] == world and r0["backend"] == "gloo" and r0["scaling"] == "strong"
    assert len(r0["shard_frames"]) == world and sum(r0["shard_frames"]) == r0["frames"] == sum(part1["lengths"])
    assert len(r0["pass_ms_per_rank"]) == world and r0["pass_ms_imbalance"] >= 1.0
    assert all(res[r]["cross_rank_rows_bit_equal"] is True for r in range(world))
    for k in want:
        assert abs(r0["mpjpe_mm"][k] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), (k, r0["mpjpe_mm"][k], want[k])
    assert "mpjpe_mm" not in res[3]                      # (the gathered summary is rank 0's to print)


def test_partial_rows_header_is_uploaded_once_and_kept():
    hdr = [(5, 2, 100), (7, 0, 33)]
    rows = evaluate.partial_rows(hdr, "cpu")
    assert rows.shape == (2, evaluate.PARTIAL_COLS) and rows.dtype == torch.float64
    assert rows[:, :3].tolist() == [[5.0, 2.0, 100.0], [7.0, 0.0, 33.0]] and float(rows[:, 3:].abs().sum()) == 0.0
    assert evaluate.partial_rows([], "cpu").shape == (0, evaluate.PARTIAL_COLS)


# ----------------------------------------------------------------- static tile schedule (host code, no GPU)

def _schedule_check(probs, nwg=256, enc=False):
    """probs: list of (M, N, nk, max_ks, max_units).  Calls the library's own checker
    (r3d_debug_schedule_check, r3d_hooks.cpp): exact cover + tile-shape rules."""
    import ctypes as C
    from ray3d_amd import _capi
    lib = hooks_library()
    fn = lib.r3d_debug_schedule_check
    fn.restype = C.c_int
    n = len(probs)
    cols = [(C.c_int * n)(*[p[i] for p in probs]) for i in range(5)]
    grid, tiles, imb = C.c_int(), C.c_int(), C.c_double()
    rc = fn(n, cols[0], cols[1], cols[2], cols[3], cols[4], nwg, int(enc), C.byref(grid), C.byref(tiles), C.byref(imb))
    return rc, grid.value, tiles.value, imb.value


def test_schedule_covers_every_launch_of_the_plan_exactly_once():
    for B in (1, 3, 8, 100, 256, 1000, 1024):
        launches = {
            "pyramid 1a + GlobalInfo": [(B * 27, 256, 24, 4, 0)] * 6 + [(B, 1024, 32, 4, 0)] * 2,
            "pyramid 3a": [(B * 3, 256, 24, 4, 0)] * 6 + [(B, 256, 32, 4, 0)] * 2,
            "pyramid top": [(B, 256, 8, 4, 0)] * 6,
            "fuse fc_1": [(B, 1024, 32, 4, 0)] * 5 + [(B, 1024, 18, 2, 0)],
            "integration fc_1": [(B, 1024, 26, 4, 0)] * 5,
            "embedding": [(B, 32, 1, 4, 0), (B, 64, 1, 4, 0)],
            "ragged N": [(B * 9, 96, 3, 4, 0), (B, 15, 32, 4, 0)],
        }
        for name, probs in launches.items():
            rc, grid, tiles, imb = _schedule_check(probs)
            assert rc == 0, (B, name, rc)
            assert 1 <= grid <= 256 and tiles >= 1
        rc, grid, tiles, imb = _schedule_check([(B * 81, 256, 5, 1, 3)] + [(B * 81, 256, 3, 1, 3)] * 4 +
                                               [(B * 81, 256, 15, 1, 1), (B, 1024, 2, 1, 3), (B, 1024, 2, 1, 3)], enc=True)
        assert rc == 0, (B, "first layers", rc)


def test_schedule_random_problem_sets():
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 13))
        probs = []
        for _ in range(n):
            M = int(rng.integers(1, 9000))
            N = int(rng.choice([3, 15, 32, 64, 256, 512, 1024]))
            nk = int(rng.integers(1, 40))
            probs.append((M, N, nk, int(rng.choice([1, 2, 4])), int(rng.choice([0, 0, 1, 3]))))
        nwg = int(rng.choice([1, 7, 64, 256, 304]))
        rc, grid, tiles, imb = _schedule_check(probs, nwg=nwg)
        assert rc == 0, (trial, probs, nwg, rc)


def test_schedule_balances_the_headline_launch():
    # level-1 3-tap convolutions of all six branches at B = 256: 1296 + 64 units on 256 CUs
    rc, grid, tiles, imb = _schedule_check([(256 * 27, 256, 24, 4, 0)] * 6 + [(256, 1024, 32, 4, 0)] * 2)
    assert rc == 0 and grid == 256
    assert imb < 1.08          # longest chunk within 8 % of the mean (it was 19 % with whole 6-unit tiles only)


# ------------------------------------------------------------------ real-data front end

def _dataset_fixture_archives(tmp_path):
    z = np.load(os.path.join(GOLDEN, "dataset.npz"))
    acts = [str(a) for a in z["actions"]]
    pos3d = {"TS1": {a: z["in3d/%d" % i] for i, a in enumerate(acts)}}
    pos2d = {"TS1": {a: [z["in2d/%d" % i]] for i, a in enumerate(acts)}}
    meta = {"layout_name": "3dhp", "num_joints": 17, "keypoints_symmetry": [[4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]]}
    p3, p2 = str(tmp_path / "d3.npz"), str(tmp_path / "d2.npz")
    np.savez_compressed(p3, positions_3d=pos3d)
    np.savez_compressed(p2, positions_2d=pos2d, metadata=meta)
    table = {"TS1": [{"R": z["table_R"], "translation": z["table_translation"],
                      "focal_length": z["table_focal_length"], "center": z["table_center"]}]}
    return z, acts, p3, p2, table


def test_pose_archives_load_like_the_reference_front_end(tmp_path):
    """ray3d_amd.dataset vs lib/dataset/__init__.py (Data + fetch_via_action) on the same archive pair
    (tests/golden/dataset.npz holds the reference's per-clip outputs)."""
    from ray3d_amd import dataset
    z, acts, p3, p2, table = _dataset_fixture_archives(tmp_path)
    cams = dataset.cameras_from_tables(table)
    pd = dataset.load_pose_data(p3, p2, cams, ["TS1"])
    assert len(pd.clips) == len(acts)
    for i, (a, c) in enumerate(zip(acts, pd.clips)):
        ref_gt, ref_rays = z["gt_norm/%d" % i], z["rays/%d" % i]
        assert c.rays.shape == ref_rays.shape and c.gt_norm.shape == ref_gt.shape      # 2D cut to the mocap length
        assert np.array_equal(c.rays, ref_rays.astype(np.float32))                      # what trainer.py:298 feeds
        assert np.array_equal(c.gt_norm, ref_gt.astype(np.float32))
        assert c.action == a.split(" ")[0]
        assert abs(c.camera.pitch - float(z["pitch/%d" % i])) < 1e-15
    assert pd.actions == {"Seq": [0, 1], "Other": [2]}
    assert pd.kps_left == list(z["kps_left"]) and pd.kps_right == list(z["kps_right"])
    assert pd.joints_left == list(z["joints_left"]) and pd.joints_right == list(z["joints_right"])
    assert list(dataset.H36M_32_TO_17) == list(z["h36m_kept_17"])
    # filters, the 14-joint layout, and the sanity checks
    only = dataset.load_pose_data(p3, p2, cams, ["TS1"], action_filter=["Other"], downsample=2)
    assert len(only.clips) == 1 and only.clips[0].rays.shape[0] == 12
    # ACTIONS entries are exact action keys, as Trainer.evaluate uses them (trainer.py:412-417): a prefix is not a match
    second = [a for a in acts if a.split(" ")[0] == "Seq"][1]
    exact = dataset.load_pose_data(p3, p2, cams, ["TS1"], action_filter=[second])
    assert len(exact.clips) == 1 and exact.actions == {"Seq": [0]}
    assert np.array_equal(exact.clips[0].rays, pd.clips[1].rays)
    with pytest.raises(KeyError, match="exact"):
        dataset.load_pose_data(p3, p2, cams, ["TS1"], action_filter=["Se"])
    uni = dataset.load_pose_data(p3, p2, cams, ["TS1"], joints_3d=dataset.KEEP_UNIVERSAL_14_OF_17,
                                 joints_2d=dataset.KEEP_UNIVERSAL_14_OF_17)
    assert uni.clips[0].rays.shape[1] == 14 and (uni.kps_left, uni.kps_right) == ([4, 5, 6, 8, 9, 10], [1, 2, 3, 11, 12, 13])
    assert (uni.joints_left, uni.joints_right) == ([4, 5, 6, 8, 9, 10], [1, 2, 3, 11, 12, 13])
    assert np.array_equal(uni.clips[0].rays, pd.clips[0].rays[:, list(dataset.KEEP_UNIVERSAL_14_OF_17)])
    with pytest.raises(KeyError, match="missing"):
        dataset.load_pose_data(p3, p2, cams, ["TS2"])
    with pytest.raises(ValueError, match="Camera count mismatch"):
        dataset.load_pose_data(p3, p2, {"TS1": cams["TS1"] * 2}, ["TS1"])
    short = dict(np.load(p2, allow_pickle=True))
    k2 = short["positions_2d"].item()
    k2["TS1"]["Other"] = [k2["TS1"]["Other"][0][:5]]
    np.savez_compressed(str(tmp_path / "short.npz"), positions_2d=k2, metadata=short["metadata"].item())
    with pytest.raises(ValueError, match="keypoint frames"):
        dataset.load_pose_data(p3, str(tmp_path / "short.npz"), cams, ["TS1"])


def test_h36m_table_conventions():
    """Millimetre translations divided in float32, (k1,k2,p1,p2,k3) coefficient order (h36m_dataset.py:355-381)."""
    from ray3d_amd import dataset
    ext = {"S0": [{"R": np.eye(3), "translation": [1841.1070556640625, 4955.28466796875, 1563.4454345703125]}, {}]}
    intr = [{"focal_length": [1145.0494384765625, 1143.7811279296875], "center": [512.54150390625, 515.4514770507812],
             "radial_distortion": [-0.2, 0.24, -0.002], "tangential_distortion": [-0.0009, -0.0016]}, {}]
    cam = dataset.cameras_from_tables(ext, intr, translation_divisor=1000, undistort=True)["S0"]
    assert len(cam) == 1                                               # the entry without a translation is skipped
    want_t = (np.array(ext["S0"][0]["translation"], dtype="float32") / 1000).astype(np.float64)
    assert np.array_equal(cam[0].Tw2c.ravel(), want_t)
    assert np.allclose(cam[0].dist_coeff, [-0.2, 0.24, -0.0009, -0.0016, -0.002], atol=1e-7)
    assert cam[0].undistort and cam[0].fx == np.float32(1145.0494384765625)


def test_checkpoint_file_in_the_trainers_format(tmp_path):
    """A file as Trainer.train saves it (trainer.py:232-249): DataParallel-prefixed state dicts next to training state."""
    mc = default_model_config(ARCHITECTURE="3,3")
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    (cp, sp), (ct, st) = synth_states(mc)
    as_dp = lambda st_: {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in st_.items()}
    path = str(tmp_path / "epoch_10.bin")
    torch.save({"epoch": 10, "lr": 1e-4, "best_performance": 41.5, "random_state": np.random.RandomState(3),
                "optimizer": {"state": {}}, "model_pos": as_dp(sp), "model_trj": as_dp(st)}, path)
    rest = ray3d_amd.load_checkpoint(path, pos, trj)
    assert rest["epoch"] == 10 and "optimizer" not in rest and "model_pos" not in rest
    k = "GlobalInfo.fc_1.weight"
    pre = "module." if torch.cuda.is_available() else ""     # with a GPU the factory returns the reference's DataParallel face
    assert np.array_equal(pos.state_dict()[pre + k].cpu().numpy(), np.asarray(sp[k]))
    kt = "shrink.weight" if "shrink.weight" in st else next(iter(st))
    assert np.array_equal(trj.state_dict()[pre + kt].cpu().numpy(), np.asarray(st[kt]))
    torch.save({"epoch": 1, "model_pos": as_dp(sp)}, path)
    with pytest.raises(KeyError, match="model_trj"):
        ray3d_amd.load_checkpoint(path, pos, trj)
    ray3d_amd.load_checkpoint(path, pos)


def _plan_check(mc, batches, nwg=256):
    """Whole-forward tile lists built on the host (r3d_debug_plan_check): every 32 x 64 cell of every problem once,
    producers' tiles in earlier launches than their consumers', spilled rows only in the launch that lists them."""
    lib = hooks_library()
    fn = lib.r3d_debug_plan_check
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    hp, ht = _capi.Handle(config_from_dicts(mc, "pos")), _capi.Handle(config_from_dicts(mc, "trj"))
    out = []
    for B in batches:
        n, sp = ctypes.c_int(), ctypes.c_int()
        rc = fn(hp.ptr, ht.ptr, B, nwg, ctypes.byref(n), ctypes.byref(sp))
        assert rc == 0, (B, rc)
        out.append((n.value, sp.value))
    hp.close()
    ht.close()
    return out


def test_plan_tile_lists_cover_every_problem_once(monkeypatch):
    mc = default_model_config(ARCHITECTURE="3,3,3,3,3")
    res = _plan_check(mc, [1, 2, 31, 100, 255, 256, 257, 600, 1024, 2048])
    # (shrink folded into its consumers: one launch fewer than DAG levels of the reference; calls of <= 48 windows use the
    # un-fused small plan - expand_conv, every 3-tap and every 1x1 convolution a launch of its own -, calls of <= 96
    # windows the medium one: first level fused, pairs not)
    assert [n for n, _ in res] == [16, 16, 16] + [12] * 5 + [11, 11]     # (from 1024 windows on the top level is a fused pair too)
    assert [n for n, _ in _plan_check(mc, [48, 49, 64, 96, 97])] == [16, 14, 14, 14, 12]
    assert dict(zip([1, 2, 31, 100, 255, 256, 257, 600, 1024, 2048], [s for _, s in res]))[256] == 512
    # 1296 equal-row tiles on 256 CUs: the 16 that would open a sixth round run with the next launch
    for arch in ("3,3,3", "3,3", "3"):
        _plan_check(default_model_config(ARCHITECTURE=arch), [1, 64, 256, 1000, 4096])
    _plan_check(mc, [256, 1000], nwg=64)
    _plan_check(default_model_config(ARCHITECTURE="3,3,3,3", CHANNELS=512), [3, 256])
    _plan_check(default_model_config(ARCHITECTURE="3,3,3", DENSE=True, DISABLE_OPTIMIZATIONS=True), [1, 50, 256])
    dev_switch(monkeypatch, "R3D_NO_SPILL", "1")
    assert all(s == 0 for _, s in _plan_check(mc, [100, 256, 1024]))


def test_workspace_bytes_is_monotonic_in_the_batch():
    """A C caller sizes its workspace once for its largest batch: r3d_workspace_bytes(B) must cover every call of fewer
    windows too, although those select less fused plans with larger intermediates (the plan switches at 48 / 96 / 1024)."""
    for mc in (default_model_config(ARCHITECTURE="3,3,3,3,3"), default_model_config(ARCHITECTURE="3,3", NUM_KPTS=14),
               default_model_config(ARCHITECTURE="3,3,3", CHANNELS=512)):
        hp, ht = _capi.Handle(config_from_dicts(mc, "pos")), _capi.Handle(config_from_dicts(mc, "trj"))
        for pair in ((hp, ht), (hp, None), (None, ht)):
            prev = 0
            for B in list(range(1, 130)) + [255, 256, 511, 1000, 1023, 1024, 1025, 4096]:
                need = _capi.workspace_bytes(pair[0], pair[1], B)
                assert need >= prev > -1, (mc["ARCHITECTURE"], B, need, prev)
                prev = need
        hp.close()
        ht.close()


def test_pairs_with_different_channel_counts_get_one_first_level_kind():
    """The first level is fused for the pair or for neither model: pos with 256 channels (fusable) next to a trajectory
    model with 512 (not) must not put r3d_gemm_f32 and r3d_gemm_enc_f32 problems into one launch."""
    lib = hooks_library()
    fn = lib.r3d_debug_plan_check
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    mc = default_model_config(ARCHITECTURE="3,3,3")
    n, sp = ctypes.c_int(), ctypes.c_int()
    for cp, ct in ((256, 512), (512, 256), (128, 256)):
        hp = _capi.Handle(config_from_dicts(dict(mc, CHANNELS=cp), "pos"))
        ht = _capi.Handle(config_from_dicts(dict(mc, CHANNELS=ct), "trj"))
        for B in (8, 64, 200, 1024):
            assert fn(hp.ptr, ht.ptr, B, 256, ctypes.byref(n), ctypes.byref(sp)) == 0, (cp, ct, B)
        hp.close()
        ht.close()


def test_single_launch_forward_is_a_sound_dependency_machine():
    """The whole forward as ONE persistent launch (r3d_forward_f32): tiles of every level in one list per workgroup,
    ordered by ready counters instead of kernel boundaries.  r3d_debug_forward_check builds those lists and executes
    them on the host: every tile gets to run (no waiting cycle with all workgroups resident), every counter ends full,
    and - independently of the dependency ranges the scheduler wrote - whenever a tile runs, every earlier problem that
    writes what it reads or touches what it writes (same buffer, overlapping columns) is complete for its windows.  For the
    plan of calls of <= 48 windows it also checks that no workspace element is written twice in a call and that every
    element read is written - what the GEMV / latency tiles' "data as its own ready flag" mode relies on."""
    lib = hooks_library()
    fn = lib.r3d_debug_forward_check
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    cases = [(default_model_config(ARCHITECTURE="3,3,3,3,3"), (1, 2, 4, 5, 16, 33, 48, 64, 97, 128, 255, 256, 257, 600, 1024, 2048)),
             (default_model_config(ARCHITECTURE="3,3"), (64, 256, 1024, 4096)),
             (default_model_config(ARCHITECTURE="3,3", NUM_KPTS=14), (512, 4096)),
             (default_model_config(ARCHITECTURE="3,3,3", STAGE=1, CAMERA_EMBDDING=False), (100, 300)),
             (default_model_config(ARCHITECTURE="3,3,3,3", DISABLE_OPTIMIZATIONS=True, CAUSAL=True), (130,)),
             (default_model_config(ARCHITECTURE="3,3,3", CHANNELS=128, LATENT_FEATURES_DIM=160, STAGE=2), (256,))]
    for mc, batches in cases:
        hp, ht = _capi.Handle(config_from_dicts(mc, "pos")), _capi.Handle(config_from_dicts(mc, "trj"))
        for pair in ((hp, ht), (hp, None), (None, ht)):
            for B in batches:
                n, c = ctypes.c_int(), ctypes.c_int()
                rc = fn(pair[0].ptr if pair[0] else None, pair[1].ptr if pair[1] else None, B, 256, ctypes.byref(n), ctypes.byref(c))
                assert rc in (0, 1), (mc["ARCHITECTURE"], B, rc)
                if B > 96:
                    assert rc == 0 and n.value > 0 and c.value > 0, (mc["ARCHITECTURE"], B, rc)    # the fused plans run as one launch
        assert fn(hp.ptr, ht.ptr, 256, 64, ctypes.byref(n), ctypes.byref(c)) == 0                   # a smaller chip
        hp.close()
        ht.close()
    # plans with r3d_gemm_enc_f32 launches (the small plan, more than 256 channels) stay launch by launch
    hp = _capi.Handle(config_from_dicts(default_model_config(ARCHITECTURE="3,3,3", CHANNELS=512), "pos"))
    assert fn(hp.ptr, None, 256, 256, ctypes.byref(n), ctypes.byref(c)) == 1
    hp.close()


def test_narrow_column_tiles_and_the_cu_limit_option_on_the_host():
    """(i) One-tile-deep M = B launches are re-tiled with gemm_tile_nb's narrower single-unit tiles (tile codes 64 + 4 .. 7):
    exact cover by the library's own checker, and fewer modelled cycles than the whole-tile packing it replaces.
    (ii) R3D_OPT_CU_LIMIT is accepted (0 .. 4096), rejected outside, and the single-launch lists for a 128-CU stream are a
    sound dependency machine."""
    lib = hooks_library()
    # 6 problems of 256 x 1024 (K = 1024): the Integration levels of a 256-window call - 192 whole tiles for 256 CUs
    probs = [(256, 1024, 32, 4, 0)] * 6
    rc, grid, tiles, imb = _schedule_check(probs)
    assert rc == 0 and tiles == 240 and grid == 240, (rc, grid, tiles)        # five tiles per row of 32 blocks: 7 + 7 + 6 + 6 + 6
    # seven problems: 7 x 8 x 5 narrow tiles would be 280 > 256 - the whole tiles stay
    rc, grid, tiles, imb = _schedule_check([(256, 1024, 32, 4, 0)] * 7)
    assert rc == 0 and tiles == 224, (rc, tiles)
    # 128 windows (four units): the split-K pieces of the classic packing stay where they are modelled shorter
    assert _schedule_check([(128, 1024, 32, 4, 0)] * 7)[0] == 0
    assert _schedule_check([(192, 1024, 32, 4, 0)] * 7)[0] == 0
    fn = lib.r3d_debug_forward_check
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    mc = default_model_config(ARCHITECTURE="3,3,3,3,3")
    hp, ht = _capi.Handle(config_from_dicts(mc, "pos")), _capi.Handle(config_from_dicts(mc, "trj"))
    n, c = ctypes.c_int(), ctypes.c_int()
    for h in (hp, ht):
        h.set_option(_capi.R3D_OPT_CU_LIMIT, 128)
        with pytest.raises(_capi.Ray3DHipError):
            h.set_option(_capi.R3D_OPT_CU_LIMIT, -1)
    for B in (192, 256, 512):
        assert fn(hp.ptr, ht.ptr, B, 128, ctypes.byref(n), ctypes.byref(c)) == 0, B
    for h in (hp, ht):
        h.set_option(_capi.R3D_OPT_CU_LIMIT, 0)
        h.close()


def test_plans_do_not_outlive_a_partner_model():
    """A (pos, trj) plan holds the partner's layer indices and K paddings.  It is keyed by model ids that are never
    reused and dropped when either model is destroyed: a new trajectory model - which malloc may well place at the old
    one's address - gets a plan built for ITS configuration."""
    lib = hooks_library()
    fn = lib.r3d_debug_plan_check
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    mc = default_model_config(ARCHITECTURE="3,3,3")
    hp = _capi.Handle(config_from_dicts(mc, "pos"))
    n, sp = ctypes.c_int(), ctypes.c_int()
    for over in (dict(), dict(CHANNELS=128), dict(LATENT_FEATURES_DIM=128), dict(CHANNELS=512), dict()):
        ht = _capi.Handle(config_from_dicts(dict(mc, **over), "trj"))
        assert fn(hp.ptr, ht.ptr, 200, 256, ctypes.byref(n), ctypes.byref(sp)) == 0, over
        ht.close()                                     # the plan goes with it
    hp.close()


def test_schedule_build_stays_cheap_at_large_batches():
    """The host search that builds a batch size's tile lists runs inside the first forward at that size (or r3d_prepare):
    tens of milliseconds, not seconds - a filler-placement loop once made it quadratic in the batch (1 s at 2048 windows)."""
    import time
    mc = default_model_config(ARCHITECTURE="3,3,3,3,3")
    _plan_check(mc, [8])                                   # (library load, plan construction)
    for B in (2048, 4096):
        t0 = time.perf_counter()
        _plan_check(mc, [B])
        assert time.perf_counter() - t0 < 0.5, B           # schedule + the exact-cover check of every cell


# ------------------------------------------------------------------ camera-augmented H36M and HumanEva front ends

def test_h36m_aug_json_cameras_and_per_camera_fetch(tmp_path):
    """ray3d_amd.dataset.cameras_from_json + load_pose_data vs the reference's h36m_aug front end
    (lib/dataset/h36m_aug_dataset.py through lib/dataset/__init__.py Data; tests/golden/frontends.npz): one JSON camera
    list for the original and the scaled subjects, 32-joint mocap reduced to 17 joints, per-camera clips."""
    import json
    from ray3d_amd import dataset
    z = np.load(os.path.join(GOLDEN, "frontends.npz"))
    meta = json.loads(str(z["aug/cams_json"]))
    pj = str(tmp_path / "cams.json")
    json.dump(meta, open(pj, "w"))
    cams, ids = dataset.cameras_from_json(pj)
    assert list(cams.keys()) == [str(s) for s in z["aug/subjects_all"]] == list(dataset.H36M_AUG_SUBJECTS)
    assert ids == [str(c) for c in z["aug/camera_dist"]]
    for ci in range(3):
        c = cams["S9_0.9"][ci]
        assert c is not cams["S9"][ci] and np.array_equal(c.Rn2w, cams["S9"][ci].Rn2w)      # same calibration for every subject
        assert np.abs(c.Rn2w - z["aug/cam%d/Rn2w" % ci]).max() < 1e-12
        assert np.abs(c.Tn2w - z["aug/cam%d/Tn2w" % ci]).max() < 1e-12
        assert np.abs(np.array([c.height, c.pitch]) - z["aug/cam%d/height_pitch" % ci]).max() < 1e-12
    subjects, acts = [str(s) for s in z["aug/subjects"]], [str(a) for a in z["aug/actions"]]
    pos3d = {s: {a: z["aug/in3d/%d/%d" % (si, ai)] for ai, a in enumerate(acts)} for si, s in enumerate(subjects)}
    pos2d = {s: {a: [z["aug/in2d/%d/%d/%d" % (si, ai, ci)] for ci in range(3)] for ai, a in enumerate(acts)}
             for si, s in enumerate(subjects)}
    p3, p2 = str(tmp_path / "d3.npz"), str(tmp_path / "d2.npz")
    np.savez_compressed(p3, positions_3d=pos3d)
    np.savez_compressed(p2, positions_2d=pos2d, metadata={"layout_name": "h36m", "num_joints": 17,
                                                          "keypoints_symmetry": [[4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]]})
    pd = dataset.load_pose_data(p3, p2, cams, subjects, joints_3d=dataset.H36M_32_TO_17)
    assert len(pd.clips) == len(subjects) * len(acts) * 3 and pd.camera_index == [0, 1, 2] * (len(subjects) * len(acts))
    k = 0
    for si in range(len(subjects)):
        for ai in range(len(acts)):
            for ci in range(3):
                c = pd.clips[k]
                assert np.array_equal(c.gt_norm, z["aug/gt_norm/%d/%d/%d" % (si, ai, ci)].astype(np.float32))
                assert np.array_equal(c.rays, z["aug/rays/%d/%d/%d" % (si, ai, ci)].astype(np.float32))
                k += 1
    assert set(pd.actions) == {"Walk", "Sit"}


def test_camera_wise_reduction_follows_the_reference_loop():
    """evaluate.reduce_camera_wise vs a literal restatement of lib/train_val/trainer.py:425-446 (cumulative means)."""
    rng = np.random.default_rng(5)
    n_clips, n_cam, n_act = 24, 3, 4
    rows = np.zeros((n_clips, evaluate.PARTIAL_COLS))
    cam_of = [i % n_cam for i in range(n_clips)]
    for i in range(n_clips):
        n = int(rng.integers(50, 200))
        rows[i] = [i, (i // n_cam) % n_act, n] + list(n * rng.uniform(0.02, 0.08, 5))
    got = evaluate.reduce_camera_wise(torch.from_numpy(rows[rng.permutation(n_clips)]), cam_of, ["a", "b", "c"])
    lists = [[] for _ in range(5)]
    want = []
    for ci, cid in enumerate(["a", "b", "c"]):
        for a in range(n_act):                                         # evaluate_core per (camera, action): trainer.py:399-403
            sel = [r for i, r in enumerate(rows) if cam_of[i] == ci and int(r[1]) == a]
            n = sum(r[2] for r in sel)
            for m in range(5):
                lists[m].append(sum(r[3 + m] for r in sel) / n * 1000.0)
        want.append((cid, tuple(round(float(np.mean(l)), 1) for l in lists)))
    assert got == want
    assert evaluate.format_camera_report(got)[0].startswith("CAM ID a, ")


def test_humaneva_camera_layout_and_joint_conventions():
    """ray3d_amd.dataset.cameras_humaneva / SYMMETRY_HUMANEVA_15 / HUMANEVA_15_TO_UNIVERSAL_14 vs
    lib/dataset/humaneva_dataset.py (tests/golden/frontends.npz)."""
    import json
    from ray3d_amd import dataset
    z = np.load(os.path.join(GOLDEN, "frontends.npz"))
    ext, intr = json.loads(str(z["he/ext_json"])), json.loads(str(z["he/int_json"]))
    cams = dataset.cameras_humaneva(ext, intr)
    assert list(cams.keys()) == [str(k) for k in z["he/keys"]]
    for k, cl in cams.items():
        tag = "he/" + k.replace("/", "_")
        assert len(cl) == int(z[tag + "/n"])
        c = cl[0]
        assert c.undistort and np.abs(c.dist_coeff - z[tag + "/dist"]).max() < 1e-12
        assert np.abs(c.K - z[tag + "/K"]).max() < 1e-12
        assert np.abs(c.Rn2w - z[tag + "/Rn2w"]).max() < 1e-12 and np.abs(c.Tn2w - z[tag + "/Tn2w"]).max() < 1e-12
        assert np.abs(np.array([c.height, c.pitch]) - z[tag + "/height_pitch"]).max() < 1e-12
    assert list(dataset.SYMMETRY_HUMANEVA_15[0]) == list(z["he/joints_left"])
    assert list(dataset.SYMMETRY_HUMANEVA_15[1]) == list(z["he/joints_right"])
    assert np.array_equal(z["he/universal_in"][:, list(dataset.HUMANEVA_15_TO_UNIVERSAL_14)], z["he/universal_out"])
    assert [list(v) for v in dataset.SYMMETRY_14] == z["he/universal_symmetry"].tolist()


def test_camera_augmentation_grid_matches_the_reference_script():
    """ray3d_amd.augment_camera vs data/camera_augmentation.py's camera_translation / rotate_camera chain (:416-466,
    :696-718) on the script's base camera, and the size / order of the 'Train' grid (:637-642)."""
    z = np.load(os.path.join(GOLDEN, "frontends.npz"))
    R0, T0 = z["grid/R0"], z["grid/T0"]
    for i, (yaw, ratio, pitch) in enumerate(z["grid/combos"]):
        R, T = ray3d_amd.augment_camera(R0, T0, yaw, ratio, pitch)
        assert np.abs(R - z["grid/R/%d" % i]).max() < 1e-12 and np.abs(T - z["grid/T/%d" % i]).max() < 1e-12
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6          # (the float32 table itself is orthogonal to ~5e-8)
    K = np.array([[1145.0, 0, 512.0], [0, 1144.0, 515.0], [0, 0, 1.0]])
    cams = ray3d_amd.camera_grid(K, R0, T0)
    assert len(cams) == 3 * 6 * 19 and cams[0].name == "yaw60_d2_p-26" and cams[-1].name == "yaw300_d3_p10"
    R, T = ray3d_amd.augment_camera(R0, T0, 60, 2.0, -26)
    assert np.array_equal(cams[0].Rw2c, R) and np.array_equal(cams[0].Tw2c, T)


def test_clip_batch_sizes_share_a_handful_of_schedules():
    """Ray3DLifter.clip_batch_sizes: ceil(n / 4096) near-equal calls, each rounded up to a multiple of 128 - a short clip to
    1, 2, 4 ... 64 when it is that short (the GEMV / latency schedules of calls of a few windows) - so that clips of any
    length use at most 39 batch sizes and none ends in a short rest call; CLIP_ROUND = 0 lifts exact sizes; CLIP_BALANCED =
    False is the chunking of rounds 1-5 (4096 at a time + the rest)."""
    mc = default_model_config(ARCHITECTURE="3,3")
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    lifter = ray3d_amd.Ray3DLifter(fac.get_pos_model(), fac.get_trj_model())
    assert lifter.clip_batch_sizes(1) == [1] and lifter.clip_batch_sizes(3) == [4] and lifter.clip_batch_sizes(17) == [32]
    assert lifter.clip_batch_sizes(33) == [64] and lifter.clip_batch_sizes(65) == [128]
    assert lifter.clip_batch_sizes(128) == [128] and lifter.clip_batch_sizes(129) == [256]
    assert lifter.clip_batch_sizes(4096) == [4096] and lifter.clip_batch_sizes(4097) == [2176, 2048]
    assert lifter.clip_batch_sizes(5000) == [2560, 2560] and lifter.clip_batch_sizes(9000) == [3072, 3072, 2944]
    assert lifter.clip_batch_sizes(8192) == [4096, 4096] and lifter.clip_batch_sizes(12288) == [4096] * 3
    seen = set()
    for n in range(1, 13000, 7):
        sizes = lifter.clip_batch_sizes(n)
        assert sum(sizes) >= n and sum(sizes) - n < 128
        assert len(sizes) == -(-n // 4096) and max(sizes) <= 4096
        assert len(sizes) == 1 or min(sizes) >= max(sizes) - 128 * (len(sizes) - 1)     # near-equal: no short rest call
        seen.update(sizes)
    assert len(seen) <= 39
    lifter.CLIP_ROUND = 0
    assert lifter.clip_batch_sizes(5000) == [2500, 2500] and lifter.clip_batch_sizes(4097) == [2049, 2048]
    lifter.CLIP_ROUND, lifter.CLIP_BALANCED = 128, False
    assert lifter.clip_batch_sizes(4097) == [4096, 1] and lifter.clip_batch_sizes(5000) == [4096, 1024]
    assert lifter.clip_batch_sizes(9000) == [4096, 4096, 896]


# ------------------------------------------------------------------ sanitizers on the host code

def test_host_schedule_plan_and_model_code_under_asan_and_ubsan():
    """SURVEY section 5 promised sanitizers on the host code: `make -C ray3d_amd/csrc san` builds the hooks library with its four
    host objects (weight packing, plans, tile schedules, the C ABI: ~3000 lines of index arithmetic) under
    -fsanitize=address,undefined, and the host-side schedule / plan / dependency-machine / model tests of this file run
    against it in a subprocess (the ASan runtime has to be the first library loaded: LD_PRELOAD).  Any report fails the run
    (halt_on_error; UBSan does not recover).  Skipped when hipcc or the ASan runtime are absent (the GPU box has both)."""
    import glob
    import shutil
    import subprocess
    import sys
    hipcc = "/opt/rocm/bin/hipcc"
    rts = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    if not os.path.exists(hipcc) or not rts or shutil.which("make") is None:
        pytest.skip("hipcc / the ASan runtime / make are not here")
    csrc = os.path.join(ROOT, "ray3d_amd", "csrc")
    if not all(os.path.exists(os.path.join(csrc, "build", f)) for f in ("r3d_kernels.o", "r3d_k_fwd_f32.o")):
        pytest.skip("the device objects have not been built yet (python -c 'import __graft_entry__ as g; g.build()')")
    r = subprocess.run(["make", "-C", csrc, "san", "ARCH=gfx950"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    san = os.path.join(ROOT, "ray3d_amd", "libray3d_hip_san.so")
    # the ASan runtime first; a preload the environment already has stays in the list behind it.  Host code only: the child
    # sees no GPU (HIP_VISIBLE_DEVICES=-1), as on a machine without one - the HIP runtime is never started under the sanitizers
    env = dict(os.environ, R3D_HOOKS_LIB=san, LD_PRELOAD=":".join([rts[-1]] + ([os.environ["LD_PRELOAD"]] if os.environ.get("LD_PRELOAD") else [])),
               HIP_VISIBLE_DEVICES="-1",
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0:exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=67")
    sel = ("schedule or plan or forward_check or dependency or single_launch or narrow or tiles or workspace or pairs or grammar or "
           "set_weight or create_rejects or before_finalize")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_host.py"), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "(%s) and not asan" % sel], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    m = __import__("re").search(r"(\d+) passed", out)
    assert m and int(m.group(1)) >= 9, out[-2000:]       # (the selection really ran the host-side tests)


# ------------------------------------------------------------------ profile tooling

def test_pmc_summary_picks_the_timed_kernel_by_name(tmp_path):
    """profiles/summarize_pmc.py: one row per kernel NAME (the last dispatch of that name in each pass), the timed kernel taken
    from the run's bench line - a pixel-keypoint run also launches the rays mode's kernel, which must not stand in for it -
    with the gfx950 unit corrections (SQ quad-cycle counters x4, FETCH_SIZE x2, KiB); profiles/make_pmc_json.py keys the
    result by workload for bench.py."""
    import csv
    import json
    import subprocess
    import sys
    root = tmp_path / "r99_cfg4_rf9"
    passes = {1: ["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"],
              2: ["GRBM_GUI_ACTIVE", "SQ_LDS_IDX_ACTIVE"], 3: ["FETCH_SIZE"], 4: ["WRITE_SIZE", "TCC_HIT_sum", "TCC_MISS_sum"]}
    # dispatches: uv kernel (id 1, 3) and rays kernel (id 2, 4: the LAST one - what round 3's summary took); 1000 us each
    val = {"SQ_VALU_MFMA_BUSY_CYCLES": {"r3d_forward_uv_f32": 1.2e9, "r3d_forward_f32": 0.6e9}, "GRBM_GUI_ACTIVE": 8 * 2.4e6,
           "FETCH_SIZE": {"r3d_forward_uv_f32": 400000.0, "r3d_forward_f32": 100000.0}, "WRITE_SIZE": 200000.0,
           "TCC_HIT_sum": 3.0, "TCC_MISS_sum": 1.0}
    for i, ctrs in passes.items():
        d = root / ("pmc%d" % i) / "host"
        d.mkdir(parents=True)
        with open(d / "1_counter_collection.csv", "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Dispatch_Id", "Kernel_Name", "Grid_Size", "Start_Timestamp", "End_Timestamp", "Counter_Name", "Counter_Value"])
            for did, name in ((1, "r3d_forward_uv_f32"), (2, "r3d_forward_f32"), (3, "r3d_forward_uv_f32.kd"), (4, "r3d_forward_f32(FwdArgs)")):
                for c in ctrs:
                    v = val.get(c, 1.0)
                    v = v[name.split("(")[0].split(".")[0]] if isinstance(v, dict) else v
                    w.writerow([did, name, 131072, 1000000 * did, 1000000 * did + 1000000, c, v])
    (root / "bench_line.json").write_text(json.dumps({"dtype": "f32", "config": {"batch_per_gpu": 1024, "receptive_field": 9, "joints": 17,
                                                      "workload": "cfg4"}, "roofline": {"kernel": "r3d_forward_uv_f32"}}))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "summarize_pmc.py"), str(root)], capture_output=True, text=True, check=True).stdout
    assert "timed kernel r3d_forward_uv_f32" in out and "RF 9" in out
    sm = json.load(open(root / "pmc_summary.json"))
    assert sm["timed_kernel"] == "r3d_forward_uv_f32" and set(sm["kernels"]) == {"r3d_forward_uv_f32", "r3d_forward_f32"}
    uv, rays = sm["kernels"]["r3d_forward_uv_f32"], sm["kernels"]["r3d_forward_f32"]
    assert uv["fetch_bytes"] == 800000000 and rays["fetch_bytes"] == 200000000 and uv["write_bytes"] == 200000000   # x2, KiB -> bytes
    assert abs(uv["clk_ghz_pmc_pass"] - 2.4) < 1e-9
    assert abs(uv["mfma_busy_frac"] - 1.2e9 / (1024 * 1000e3 * 2.4)) < 1e-4 and abs(uv["executed_flops"] - 1.2e9 * 64) < 1.0
    assert uv["l2_hit_pct"] == 75.0
