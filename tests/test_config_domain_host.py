"""The configuration domain model_create accepts (r3d_model.cpp: 1 .. 6 levels; channels, latent size and embedding width any
multiple of 32, the embedding up to 128; up to 8 camera parameters) beyond the configurations the census of kernel specialisations
sweeps - on the host (hooks library, no GPU).  Nineteen configurations, both precisions, every B of the census's thinned range
(specialisation_cases.sweep_batches: every value to 140, every fourth to 300, the large sizes; the six-level models stop at 300):

  r3d_debug_plan_check == 0        the launch-by-launch tile lists cover every problem exactly once, producers before consumers;
  r3d_debug_forward_check in 0, 1  the single-launch lists are a sound dependency machine (1: the plan runs launch by launch);
  r3d_workspace_bytes              monotonic in B (a C caller sizes its workspace once, for its largest batch);
  r3d_debug_forward_census         succeeds for every form and call shape the configuration allows, and every (kernel, tile kind)
                                   pair it returns is one that a case of specialisation_cases.CASES reaches - a configuration of
                                   the accepted domain that selects an instantiation no GPU case runs fails HERE, by name.

At 128 and 64 workgroups (a lane of R3D_OPT_LANES = 2 / 4) the plan check and the census are repeated for every B up to 64 - where
the small, latency and medium plans live -, every fourth to 140, and 192, 256, 1024 (1024: not the six-level models).

Wall time, one core: about three minutes, two thirds of it r3d_debug_forward_check executing the single-launch lists of the 38
(configuration, precision) pairs at 256 workgroups."""
import ctypes

import pytest

import specialisation_cases as sc
from conftest import hooks_library

_L6 = "3,3,3,3,3,3"
DOMAIN = {
    # the four the census sweeps itself (specialisation_cases._DOMAIN), and six levels with 14 joints at stage 1
    "six-levels": dict(ARCHITECTURE=_L6),
    "six-levels-j14-s1": dict(ARCHITECTURE=_L6, NUM_KPTS=14, STAGE=1),
    "latent-512": dict(ARCHITECTURE="3,3,3", LATENT_FEATURES_DIM=512),
    "c640-n320": dict(ARCHITECTURE="3,3,3", CHANNELS=640, LATENT_FEATURES_DIM=320),
    "c768-n512-rf9": dict(ARCHITECTURE="3,3", CHANNELS=768, LATENT_FEATURES_DIM=512),
    # channels / latent size
    "c32-n32": dict(CHANNELS=32, LATENT_FEATURES_DIM=32), "c160-n96": dict(CHANNELS=160, LATENT_FEATURES_DIM=96),
    "c192-n192": dict(CHANNELS=192, LATENT_FEATURES_DIM=192), "c224-n224": dict(CHANNELS=224, LATENT_FEATURES_DIM=224),
    "c288-n288": dict(CHANNELS=288, LATENT_FEATURES_DIM=288), "c320-n64": dict(CHANNELS=320, LATENT_FEATURES_DIM=64),
    # latent size at 256 channels
    "n32": dict(LATENT_FEATURES_DIM=32), "n96": dict(LATENT_FEATURES_DIM=96), "n224": dict(LATENT_FEATURES_DIM=224),
    "n1024": dict(LATENT_FEATURES_DIM=1024),
    # embedding width / camera parameters
    "e128-x8": dict(EMBEDD_DIM=128, EXTRINSIC_DIM=8), "e32-x1": dict(EMBEDD_DIM=32, EXTRINSIC_DIM=1),
    # two input features (no pixel input), dense
    "f2-c160-n192-j15": dict(INPUT_DIM=2, CHANNELS=160, LATENT_FEATURES_DIM=192, NUM_KPTS=15),
    "dense-c192-n96": dict(DENSE=True, CHANNELS=192, LATENT_FEATURES_DIM=96),
}
LANE_BATCHES = list(range(1, 65)) + list(range(68, 141, 4)) + [192, 256, 1024]


def _model_config(name, b3):
    import ray3d_amd
    kw = dict(DOMAIN[name])
    kw.setdefault("ARCHITECTURE", "3,3,3")
    mc = {str(k): v for k, v in ray3d_amd.default_model_config(**kw).items()}
    mc["BF16X3"] = bool(b3)
    return mc


@pytest.fixture(scope="module")
def table_pairs():
    """{(kernel, tile kind)} over specialisation_cases.CASES: what the GPU suite runs against the oracle."""
    census = sc.Census()
    out = set()
    for case in sc.CASES:
        out |= census.pairs(case)
    census.close()
    return out


def test_the_domain_is_the_nineteen_configurations():
    assert len(DOMAIN) == 19 and len({tuple(sorted(v.items())) for v in DOMAIN.values()}) == 19


@pytest.mark.parametrize("b3", [False, True], ids=["f32", "bf16x3"])
@pytest.mark.parametrize("name", list(DOMAIN))
def test_accepted_configuration_plans_check_and_select_only_tested_specialisations(name, b3, table_pairs):
    from ray3d_amd import _capi
    from ray3d_amd.spec import config_from_dicts
    lib = hooks_library()
    sig = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    plan_check, forward_check = lib.r3d_debug_plan_check, lib.r3d_debug_forward_check
    plan_check.argtypes, plan_check.restype = sig, ctypes.c_int
    forward_check.argtypes, forward_check.restype = sig, ctypes.c_int
    mc = _model_config(name, b3)
    cp, ct = config_from_dicts(mc, "pos"), config_from_dicts(mc, "trj")
    hp, ht = _capi.Handle(cp), _capi.Handle(ct)
    rf = cp.receptive_field
    deep = rf > 243
    shapes = sc.shapes_of(mc)
    n0, n1 = ctypes.c_int(), ctypes.c_int()
    untested = {}
    try:
        for nwg in sc.NWGS:
            batches = [b for b in sc.sweep_batches("n512", nwg) if b <= 300 or not deep] if nwg == sc.NWG else \
                      [b for b in LANE_BATCHES if b <= 300 or not deep]
            prev = 0
            for B in batches:
                assert plan_check(hp.ptr, ht.ptr, B, nwg, ctypes.byref(n0), ctypes.byref(n1)) == 0, (name, b3, B, nwg)
                if nwg == sc.NWG:
                    rc = forward_check(hp.ptr, ht.ptr, B, nwg, ctypes.byref(n0), ctypes.byref(n1))
                    assert rc in (0, 1), (name, b3, B, nwg, rc)
                    need = _capi.workspace_bytes(hp, ht, B)
                    assert need >= prev > -1 and need > 0, (name, b3, B, need, prev)
                    prev = need
                for staged in (False, True):
                    for shape in shapes:
                        uv, per_window, stride = sc.SHAPES[shape]
                        launches = _capi.debug_forward_census(hp, ht, B, stride or rf, nwg=nwg, uv=uv, cam_stride=8 if per_window else 0,
                                                              staged=staged)
                        assert launches, (name, b3, B, nwg, shape, staged)
                        for kernel, _, hist in launches:
                            for pair in ([(kernel, kind) for kind in hist] or [(kernel, "")]):
                                if pair not in table_pairs:
                                    untested.setdefault(pair, (B, nwg, shape, "staged" if staged else "single"))
    finally:
        hp.close()
        ht.close()
    assert not untested, "%s %s selects (kernel, tile kind) pairs that no case of specialisation_cases.CASES runs on the GPU " \
        "(pair: the first B, workgroups, shape, form): %s" % (name, "bf16x3" if b3 else "f32", sorted(untested.items()))
