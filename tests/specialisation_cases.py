"""Shared by tests/test_specialisations_host.py, tests/test_gpu_specialisations.py and tools/specialisation_cover.py: the domain
the census of kernel specialisations (r3d_debug_forward_census, hooks library, host only) is swept over, and CASES - the small
table of calls that reaches every (kernel, tile kind) pair the sweep reaches.  A tile kind is what the persistent loop's dispatch
selects for a tile (r3d_tiles.hpp, gemm_persistent): the tile function and its template arguments as the switches clamp them.

A case is (config, bf16x3, form, shape, B):
  config  a name of CONFIGS: the eleven reference fixtures' model_configs, the default RF 9 model, the channel counts 64 / 96 / 128 /
          384 / 512 and a one-level model (weights are synthetic at scale 1 whatever the fixture's)
  bf16x3  model_config['BF16X3']
  form    "single" (one persistent launch where the plan allows it), "staged" (R3D_OPT_STAGED), "captured" (single, on a stream
          under capture - swept at CAPTURED_BATCHES only: one small and one large size)
  shape   a name of SHAPES: rays windows, UV windows with one camera row / a row per window, rays clip, UV clip (one camera)
  B       windows

When a tile kind is added: add it to the dispatch and to census_tile_kind (r3d_hooks.cpp); test_specialisations_host.py then fails
until `python tools/specialisation_cover.py` has been run and the CASES it prints are pasted below (or the kind is listed in
UNREACHABLE there with the reason the code gives)."""
import functools

from conftest import MODEL_CASES, load_model_fixture

NWG = 256                                     # CUs of the device the table is computed for (MI355X)

_WIDTHS = {"c64": dict(CHANNELS=64, LATENT_FEATURES_DIM=128), "c96": dict(CHANNELS=96, LATENT_FEATURES_DIM=128),
           "c128": dict(CHANNELS=128, LATENT_FEATURES_DIM=160), "c384": dict(CHANNELS=384, LATENT_FEATURES_DIM=128),
           "c512": dict(CHANNELS=512, LATENT_FEATURES_DIM=128)}
CONFIGS = list(MODEL_CASES) + ["rf9"] + list(_WIDTHS) + ["one-level"]
DEFAULT_CONFIGS = ("j17_rf27_s3", "rf9", "j17_rf243_s3")              # (swept over every B; the others: see sweep_batches)

# shape -> (UV input, a camera row per window, window stride in frames - None: independent windows, RF apart; 1: a clip call)
SHAPES = {"rays": (False, False, None), "uv-cam0": (True, False, None), "uv-cam8": (True, True, None),
          "rays-clip": (False, False, 1), "uv-clip": (True, False, 1),
          "uv-overlap": (True, True, 5)}      # (windows that share frames but not the camera: not swept - it selects what uv-cam8 selects)
SWEPT_SHAPES = ("rays", "uv-cam0", "uv-cam8", "rays-clip", "uv-clip")
FORMS = ("single", "staged", "captured")
CAPTURED_BATCHES = (12, 203)
EXTRA_BATCHES = (511, 512, 513, 700, 1023, 1024, 1025, 1100, 4096)


@functools.lru_cache(maxsize=None)
def model_config(name, bf16x3=False):
    """The model_config dict of a CONFIGS name."""
    import ray3d_amd
    if name in MODEL_CASES:
        mc = dict(load_model_fixture(name)[1])
    elif name == "one-level":
        mc = ray3d_amd.default_model_config(ARCHITECTURE="3")
    elif name == "rf9":
        mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3")
    else:
        mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3", **_WIDTHS[name])
    mc = {str(k): v for k, v in mc.items()}
    mc["BF16X3"] = bool(bf16x3)
    return mc


def shapes_of(mc):
    """The call shapes a configuration allows: pixel input needs the three ray features (check_call, r3d_forward.cpp)."""
    return [s for s in SWEPT_SHAPES if not SHAPES[s][0] or int(mc["INPUT_DIM"]) == 3]


def sweep_batches(config):
    """Every B of the sweep for a configuration.  The three DEFAULT_CONFIGS (RF 27, 9 and 243 of the default model): every value
    1 ... 300 and EXTRA_BATCHES, as the census was specified.  The other configurations, thinned to keep the host test under a
    minute: every value 1 ... 140 (all plan switches - 4 / 16 / 32 / 48 / 96 / 128 windows - and the first 32-row units), every
    fourth value from there to 300, and EXTRA_BATCHES."""
    full = list(range(1, 301)) + list(EXTRA_BATCHES)
    if config in DEFAULT_CONFIGS:
        return full
    return [b for b in full if b <= 140 or b > 300 or b % 4 == 0]


def domain():
    """Every case of the sweep, grouped so that consecutive cases share a schedule: (config, bf16x3, B, [(form, shape)])."""
    for config in CONFIGS:
        for b3 in (False, True):
            shapes = shapes_of(model_config(config, b3))
            for B in sweep_batches(config):
                forms = [f for f in FORMS if f != "captured" or B in CAPTURED_BATCHES]
                yield config, b3, B, [(f, s) for f in forms for s in shapes]
            for B in CAPTURED_BATCHES:
                if B not in sweep_batches(config):
                    yield config, b3, B, [("captured", s) for s in shapes]


class Census:
    """Handles of the hooks library per (config, bf16x3), made once, and the census of a case on them (host only)."""

    def __init__(self):
        self._handles = {}

    def handles(self, config, b3):
        from ray3d_amd import _capi
        from ray3d_amd.spec import config_from_dicts
        key = (config, bool(b3))
        if key not in self._handles:
            _capi.use_hooks(True)
            mc = model_config(config, b3)
            cp, ct = config_from_dicts(mc, "pos"), config_from_dicts(mc, "trj")
            self._handles[key] = (_capi.Handle(cp), _capi.Handle(ct), cp.receptive_field)
        return self._handles[key]

    def launches(self, case, nwg=NWG):
        """[(kernel, blocks, {tile kind: tiles})] of the call, in launch order."""
        from ray3d_amd import _capi
        config, b3, form, shape, B = case
        hp, ht, rf = self.handles(config, b3)
        uv, per_window, stride = SHAPES[shape]
        return _capi.debug_forward_census(hp, ht, B, stride or rf, nwg=nwg, uv=uv, cam_stride=8 if per_window else 0,
                                          staged=form == "staged", captured=form == "captured")

    def pairs(self, case, nwg=NWG):
        """{(kernel, tile kind)} of the call; a launch without tile lists counts as (kernel, "")."""
        out = set()
        for kernel, _, hist in self.launches(case, nwg):
            out.update((kernel, kind) for kind in hist) if hist else out.add((kernel, ""))
        return out

    def close(self):
        for hp, ht, _ in self._handles.values():
            hp.close()
            ht.close()
        self._handles = {}


def sweep(census):
    """{case: {(kernel, tile kind)}} over the whole domain."""
    out = {}
    for config, b3, B, calls in domain():
        for form, shape in calls:
            case = (config, b3, form, shape, B)
            out[case] = frozenset(census.pairs(case))
    return out


def receptive_field(config):
    from ray3d_amd.spec import config_from_dicts
    return config_from_dicts(model_config(config), "pos").receptive_field


def case_cost(case, fixed_cost=64):
    """What a case costs on the GPU and in its CPU reference, in windows of the default RF 27 model: B * RF / 27, plus a fixed cost
    for what every case pays whatever its size (modules, schedule, reference set-up)."""
    return case[4] * receptive_field(case[0]) / 27.0 + fixed_cost


def smallest_cover(reached, start=()):
    """Greedy cover of the union of `reached` (sweep()) that prefers the smallest B: the case added next is the one with the most
    pairs still open per unit of case_cost - ties to the smaller B, then to the first in CONFIGS / FORMS / SHAPES order.  `start`:
    cases that are in the table whatever the cover picks.  Returns (cases, {pair: the smallest case of the table that reaches it})."""
    order = {c: i for i, c in enumerate(reached)}
    chosen, covered = list(start), set()
    for case in start:
        covered |= reached.get(case, frozenset())
    open_of = {c: set(p) - covered for c, p in reached.items()}
    open_of = {c: p for c, p in open_of.items() if p}
    cost = {c: case_cost(c) for c in open_of}
    while open_of:
        best = max(open_of, key=lambda c: (len(open_of[c]) / cost[c], -c[4], -order[c]))
        chosen.append(best)
        new = open_of.pop(best)
        for c in list(open_of):
            open_of[c] -= new
            if not open_of[c]:
                del open_of[c]
    first = {}
    for case in sorted(chosen, key=lambda c: (c[4], chosen.index(c))):
        for p in reached.get(case, ()):
            first.setdefault(p, case)
    return chosen, first


# ---- the holes known before the census existed (in the table whatever the cover picks): UV input on bf16x3 handles.  bf16x3 tiles
# start at 96 windows; the pos branches have K <= 64 and the trajectory model K = 153 > 64, so one pair call runs both K kinds of
# first_level_taps_b3<.., UV>; RF 9 and RF 27, one camera row and a row per window, single launch (r3d_forward_uv_b3) and staged
# (r3d_gemm_uv_b3), once with overlapping windows (stride 5); more than 256 channels and one-level models keep
# r3d_gemm_enc_uv_f32 in front of bf16x3 levels.
KNOWN_HOLES = [
    ("rf9", True, "single", "uv-cam0", 97), ("rf9", True, "single", "uv-cam8", 97),
    ("rf9", True, "single", "uv-cam0", 130), ("rf9", True, "single", "uv-cam8", 130),
    ("j17_rf27_s3", True, "single", "uv-cam0", 97), ("j17_rf27_s3", True, "single", "uv-cam8", 97),
    ("j17_rf27_s3", True, "single", "uv-cam0", 130), ("j17_rf27_s3", True, "single", "uv-cam8", 130),
    ("j17_rf27_s3", True, "single", "uv-overlap", 130),
    ("rf9", True, "staged", "uv-cam8", 97), ("j17_rf27_s3", True, "staged", "uv-cam0", 97),
    ("c512", True, "single", "uv-cam8", 97), ("one-level", True, "single", "uv-cam0", 97),
    ("j17_rf81_s2_big", True, "single", "uv-clip", 200),     # (a bf16x3 clip call keeps the gathered first level: DESIGN 4.4)
]

# ---- a captured forward binds inside its graph and keeps its control region in the caller's workspace (no polled activation banks at
# 12 windows): the same kernels and tile kinds as the eager call, so the cover never needs one - one small and one large size
CAPTURED = [("j17_rf27_s3", False, "captured", "rays", 12), ("j17_rf27_s3", True, "captured", "uv-cam0", 203)]
ALWAYS = KNOWN_HOLES + CAPTURED

# ---- the cover: printed by `python tools/specialisation_cover.py`, pasted here
COVER = [
    ('j17_rf9_s1', False, 'single', 'rays', 65),
    ('j17_rf9_s1', False, 'single', 'uv-cam0', 65),
    ('j14_rf9_s3', True, 'single', 'rays', 96),
    ('c96', False, 'single', 'rays-clip', 65),
    ('c96', False, 'single', 'uv-clip', 65),
    ('j17_rf81_s2_big', False, 'single', 'uv-cam0', 4),
    ('j14_rf9_s3', False, 'staged', 'uv-cam0', 129),
    ('c64', True, 'staged', 'rays', 107),
    ('j17_rf9_s1', False, 'staged', 'rays', 228),
    ('c64', True, 'single', 'rays', 97),
    ('j14_rf9_dense_causal_s2', False, 'single', 'rays', 1),
    ('c64', True, 'single', 'uv-cam0', 97),
    ('one-level', False, 'single', 'rays', 97),
    ('rf9', False, 'single', 'rays', 161),
    ('rf9', False, 'single', 'uv-cam0', 161),
    ('c64', True, 'staged', 'uv-cam0', 96),
    ('one-level', False, 'single', 'rays', 1),
    ('j14_rf9_dense_causal_s2', True, 'single', 'rays', 1025),
    ('j17_rf9_s1', False, 'single', 'rays', 228),
    ('j17_rf9_s1', False, 'single', 'uv-cam0', 228),
    ('c64', False, 'single', 'rays', 11),
    ('c64', False, 'single', 'uv-cam0', 11),
    ('c64', False, 'single', 'rays-clip', 513),
    ('c64', False, 'single', 'uv-clip', 513),
    ('j14_rf9_s3', False, 'single', 'rays', 97),
    ('j14_rf9_s3', False, 'single', 'uv-cam0', 97),
    ('c128', True, 'staged', 'uv-cam0', 1025),
    ('j17_rf27_s3', False, 'staged', 'rays-clip', 49),
    ('j17_rf27_s3', False, 'staged', 'uv-clip', 49),
    ('j17_rf9_s1', True, 'single', 'rays', 513),
    ('j17_rf9_s1', True, 'single', 'uv-cam0', 513),
    ('j17_rf27_s3', False, 'single', 'rays-clip', 193),
    ('j17_rf27_s3', False, 'single', 'uv-clip', 193),
    ('j17_rf27_dense_s3', False, 'single', 'uv-cam0', 196),
    ('j17_rf9_s1', False, 'staged', 'uv-cam0', 1025),
    ('c64', False, 'single', 'rays', 513),
    ('c64', False, 'single', 'uv-cam0', 513),
    ('j17_rf243_s3', False, 'single', 'rays', 17),
    ('j17_rf243_s3', False, 'single', 'uv-cam0', 17),
    ('j17_rf27_s3', False, 'staged', 'uv-cam0', 1025),
    ('c96', True, 'single', 'rays', 1025),
    ('c64', False, 'staged', 'rays', 511),
    ('c64', False, 'staged', 'uv-clip', 1100),
    ('j17_rf81_s2_big', False, 'single', 'rays', 97),
    ('j17_rf81_s2_big', False, 'single', 'uv-cam0', 97),
    ('j17_rf81_s2_big', False, 'single', 'rays-clip', 97),
    ('j17_rf81_s2_big', False, 'single', 'uv-clip', 97),
    ('c64', True, 'single', 'uv-cam0', 1025),
    ('j17_rf243_s3', False, 'staged', 'rays-clip', 50),
    ('j17_rf81_s2_big', False, 'single', 'rays', 1025),
    ('j17_rf81_s2_big', False, 'single', 'uv-cam0', 1025),
    ('j17_rf27_s3', False, 'single', 'rays-clip', 1024),
    ('j17_rf27_s3', False, 'single', 'uv-clip', 1024),
    ('j17_rf27_s3', False, 'staged', 'uv-cam0', 1024),
    ('c64', True, 'staged', 'rays', 1025),
    ('j17_rf243_s3', False, 'staged', 'rays', 513),
    ('j17_rf243_s3', False, 'single', 'rays-clip', 513),
    ('j17_rf243_s3', False, 'single', 'uv-clip', 513),
    ('j17_rf243_s3', False, 'staged', 'uv-cam0', 1024),
    ('j17_rf81_s2_big', True, 'staged', 'uv-cam0', 1023),
    ('j17_rf81_s2_big', True, 'single', 'rays', 1025),
    ('j17_rf81_s2_big', True, 'single', 'uv-cam0', 1025),
    ('j17_rf81_s2_big', True, 'staged', 'rays', 1025),
    ('j17_rf81_s2_big', True, 'staged', 'uv-cam0', 1025),
    ('j17_rf243_s3', False, 'single', 'rays', 511),
    ('j17_rf243_s3', False, 'single', 'uv-cam0', 511),
]

CASES = ALWAYS + [c for c in COVER if c not in ALWAYS]


def case_id(case):
    config, b3, form, shape, B = case
    return "%s-%s-%s-%s-%d" % (config, "bf16x3" if b3 else "f32", form, shape, B)
