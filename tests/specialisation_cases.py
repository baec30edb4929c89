"""Shared by tests/test_specialisations_host.py, tests/test_gpu_specialisations.py and tools/specialisation_cover.py: the domain
the census of kernel specialisations (r3d_debug_forward_census, hooks library, host only) is swept over, and CASES - the small
table of calls that reaches every (kernel, tile kind) pair the sweep reaches.  A tile kind is what the persistent loop's dispatch
selects for a tile (r3d_tiles.hpp, gemm_persistent): the tile function and its template arguments as the switches clamp them.

A case is (config, bf16x3, form, shape, B, nwg):
  config  a name of CONFIGS: the eleven reference fixtures' model_configs, the default RF 9 model, the channel counts 64 / 96 / 128 /
          384 / 512, a one-level model, and four more of the domain model_create accepts: six levels (RF 729), a latent size of
          512 at 256 channels, 640 channels, 768 channels at RF 9 (weights are synthetic at scale 1 whatever the fixture's)
  bf16x3  model_config['BF16X3']
  form    "single" (one persistent launch where the plan allows it), "staged" (R3D_OPT_STAGED), "captured" (single, on a stream
          under capture - swept at CAPTURED_BATCHES only: one small and one large size)
  shape   a name of SHAPES: rays windows, UV windows with one camera row / a row per window, rays clip, UV clip (one camera)
  B       windows
  nwg     workgroups the tile lists are cut for: 256 (the whole chip), 128 (a lane of R3D_OPT_LANES = 2, or R3D_OPT_CU_LIMIT = 128),
          64 (a lane of R3D_OPT_LANES = 4): r3d_forward.cpp, schedule keys

When a tile kind is added: add it to the dispatch and to census_tile_kind (r3d_hooks.cpp); test_specialisations_host.py then fails
until `python tools/specialisation_cover.py` has been run and the CASES it prints are pasted below (or the kind is listed in
UNREACHABLE there with the reason the code gives)."""
import functools

from conftest import MODEL_CASES, load_model_fixture

NWG = 256                                     # CUs of the device the table is computed for (MI355X)
NWGS = (256, 128, 64)                         # ... and what a lane of two / of four gets of them (device CUs / lanes)

_WIDTHS = {"c64": dict(CHANNELS=64, LATENT_FEATURES_DIM=128), "c96": dict(CHANNELS=96, LATENT_FEATURES_DIM=128),
           "c128": dict(CHANNELS=128, LATENT_FEATURES_DIM=160), "c384": dict(CHANNELS=384, LATENT_FEATURES_DIM=128),
           "c512": dict(CHANNELS=512, LATENT_FEATURES_DIM=128)}
# (more of what model_create accepts - 1 .. 6 levels, channels and latent size any multiple of 32: keyword arguments of default_model_config)
_DOMAIN = {"rf729": dict(ARCHITECTURE="3,3,3,3,3,3"), "n512": dict(ARCHITECTURE="3,3,3", LATENT_FEATURES_DIM=512),
           "c640": dict(ARCHITECTURE="3,3,3", CHANNELS=640, LATENT_FEATURES_DIM=320),
           "c768_rf9": dict(ARCHITECTURE="3,3", CHANNELS=768, LATENT_FEATURES_DIM=512)}
CONFIGS = list(MODEL_CASES) + ["rf9"] + list(_WIDTHS) + ["one-level"] + list(_DOMAIN)
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
    elif name in _DOMAIN:
        mc = ray3d_amd.default_model_config(**_DOMAIN[name])
    else:
        mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3", **_WIDTHS[name])
    mc = {str(k): v for k, v in mc.items()}
    mc["BF16X3"] = bool(bf16x3)
    return mc


def shapes_of(mc):
    """The call shapes a configuration allows: pixel input needs the three ray features (check_call, r3d_forward.cpp)."""
    return [s for s in SWEPT_SHAPES if not SHAPES[s][0] or int(mc["INPUT_DIM"]) == 3]


LANE_EXTRA_BATCHES = (1024, 1025)             # (the sizes above 300 kept on the 128- and 64-workgroup axes)


def sweep_batches(config, nwg=NWG):
    """Every B of the sweep for a configuration and a workgroup count.  The three DEFAULT_CONFIGS (RF 27, 9 and 243 of the default
    model) at 256 workgroups: every value 1 ... 300 and EXTRA_BATCHES, as the census was specified.  The other configurations,
    thinned: every value 1 ... 140 (all plan switches - 4 / 16 / 32 / 48 / 96 / 128 windows -, the small and latency plans and the
    first 32-row units), every fourth value from there to 300, and EXTRA_BATCHES.  At 128 and 64 workgroups every configuration
    keeps every value to 140, then every eighth to 300 (192, 224, 256 among them), and of the sizes above 300
    LANE_EXTRA_BATCHES.  The six-level model (RF 729) stops at 300 windows on every axis: a 4096-window call of it (3 million
    frames) is no test shape."""
    full = list(range(1, 301)) + list(EXTRA_BATCHES if nwg == NWG else LANE_EXTRA_BATCHES)
    if config in DEFAULT_CONFIGS and nwg == NWG:
        return full
    step = 4 if nwg == NWG else 8
    return [b for b in full if b <= 140 or (b % step == 0 and b <= 300) or (b > 300 and config != "rf729")]


def domain():
    """Every case of the sweep, grouped so that consecutive cases share a schedule: (config, bf16x3, B, nwg, [(form, shape)]).
    Captured calls are swept at 256 workgroups only (KNOWN_HOLES and CAPTURED stay there)."""
    for config in CONFIGS:
        for b3 in (False, True):
            shapes = shapes_of(model_config(config, b3))
            for nwg in NWGS:
                for B in sweep_batches(config, nwg):
                    forms = [f for f in FORMS if f != "captured" or (B in CAPTURED_BATCHES and nwg == NWG)]
                    yield config, b3, B, nwg, [(f, s) for f in forms for s in shapes]
            for B in CAPTURED_BATCHES:
                if B not in sweep_batches(config):
                    yield config, b3, B, NWG, [("captured", s) for s in shapes]


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

    def launches(self, case, nwg=None):
        """[(kernel, blocks, {tile kind: tiles})] of the call, in launch order (nwg: instead of the case's own)."""
        from ray3d_amd import _capi
        config, b3, form, shape, B = case[:5]
        nwg = nwg or case[5]
        hp, ht, rf = self.handles(config, b3)
        uv, per_window, stride = SHAPES[shape]
        return _capi.debug_forward_census(hp, ht, B, stride or rf, nwg=nwg, uv=uv, cam_stride=8 if per_window else 0,
                                          staged=form == "staged", captured=form == "captured")

    def pairs(self, case, nwg=None):
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
    for config, b3, B, nwg, calls in domain():
        for form, shape in calls:
            case = (config, b3, form, shape, B, nwg)
            out[case] = frozenset(census.pairs(case))
    return out


def receptive_field(config):
    from ray3d_amd.spec import config_from_dicts
    return config_from_dicts(model_config(config), "pos").receptive_field


def case_cost(case, fixed_cost=64):
    """What a case costs on the GPU and in its CPU reference, in windows of the default RF 27 model: B * RF / 27, plus a fixed cost
    for what every case pays whatever its size (modules, schedule, reference set-up)."""
    return case[4] * receptive_field(case[0]) / 27.0 + fixed_cost


def cover_tier(case):
    """The order the cover is built in: calls on the whole chip of the configurations the census began with, then the whole chip
    on the rest of the accepted domain, then 128 workgroups, then 64.  A case of a later tier joins the table only for pairs no
    earlier tier reaches - so the table of an earlier tier, and its test ids, stay when an axis is added behind it."""
    config, nwg = case[0], case[5]
    return NWGS.index(nwg) + 1 if nwg != NWG else (1 if config in _DOMAIN else 0)


def smallest_cover(reached, start=()):
    """Greedy cover of the union of `reached` (sweep()) that prefers the smallest B, tier by tier (cover_tier): the case added next
    is the one of the tier with the most pairs still open per unit of case_cost - ties to the smaller B, then to the first in
    CONFIGS / FORMS / SHAPES order.  `start`: cases that are in the table whatever the cover picks.  Returns (cases, {pair: the
    smallest case of the table that reaches it})."""
    order = {c: i for i, c in enumerate(reached)}
    chosen, covered = list(start), set()
    for case in start:
        covered |= reached.get(case, frozenset())
    for tier in range(len(NWGS) + 1):
        open_of = {c: set(p) - covered for c, p in reached.items() if cover_tier(c) == tier}
        open_of = {c: p for c, p in open_of.items() if p}
        cost = {c: case_cost(c) for c in open_of}
        while open_of:
            best = max(open_of, key=lambda c: (len(open_of[c]) / cost[c], -c[4], -order[c]))
            chosen.append(best)
            new = open_of.pop(best)
            covered |= new
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
KNOWN_HOLES = [c + (NWG,) for c in [
    ("rf9", True, "single", "uv-cam0", 97), ("rf9", True, "single", "uv-cam8", 97),
    ("rf9", True, "single", "uv-cam0", 130), ("rf9", True, "single", "uv-cam8", 130),
    ("j17_rf27_s3", True, "single", "uv-cam0", 97), ("j17_rf27_s3", True, "single", "uv-cam8", 97),
    ("j17_rf27_s3", True, "single", "uv-cam0", 130), ("j17_rf27_s3", True, "single", "uv-cam8", 130),
    ("j17_rf27_s3", True, "single", "uv-overlap", 130),
    ("rf9", True, "staged", "uv-cam8", 97), ("j17_rf27_s3", True, "staged", "uv-cam0", 97),
    ("c512", True, "single", "uv-cam8", 97), ("one-level", True, "single", "uv-cam0", 97),
    ("j17_rf81_s2_big", True, "single", "uv-clip", 200),     # (a bf16x3 clip call keeps the gathered first level: DESIGN 4.4)
]]

# ---- a captured forward binds inside its graph and keeps its control region in the caller's workspace (no polled activation banks at
# 12 windows): the same kernels and tile kinds as the eager call, so the cover never needs one - one small and one large size
CAPTURED = [("j17_rf27_s3", False, "captured", "rays", 12, NWG), ("j17_rf27_s3", True, "captured", "uv-cam0", 203, NWG)]
ALWAYS = KNOWN_HOLES + CAPTURED

# ---- the cover: printed by `python tools/specialisation_cover.py`, pasted here
COVER = [
    ('j17_rf9_s1', False, 'single', 'rays', 65, 256),
    ('j17_rf9_s1', False, 'single', 'uv-cam0', 65, 256),
    ('j14_rf9_s3', True, 'single', 'rays', 96, 256),
    ('c96', False, 'single', 'rays-clip', 65, 256),
    ('c96', False, 'single', 'uv-clip', 65, 256),
    ('j17_rf81_s2_big', False, 'single', 'uv-cam0', 4, 256),
    ('j14_rf9_s3', False, 'staged', 'uv-cam0', 129, 256),
    ('c64', True, 'staged', 'rays', 107, 256),
    ('j17_rf9_s1', False, 'staged', 'rays', 228, 256),
    ('c64', True, 'single', 'rays', 97, 256),
    ('j14_rf9_dense_causal_s2', False, 'single', 'rays', 1, 256),
    ('c64', True, 'single', 'uv-cam0', 97, 256),
    ('one-level', False, 'single', 'rays', 97, 256),
    ('rf9', False, 'single', 'rays', 161, 256),
    ('rf9', False, 'single', 'uv-cam0', 161, 256),
    ('c64', True, 'staged', 'uv-cam0', 96, 256),
    ('one-level', False, 'single', 'rays', 1, 256),
    ('j14_rf9_dense_causal_s2', True, 'single', 'rays', 1025, 256),
    ('j17_rf9_s1', False, 'single', 'rays', 228, 256),
    ('j17_rf9_s1', False, 'single', 'uv-cam0', 228, 256),
    ('c64', False, 'single', 'rays', 11, 256),
    ('c64', False, 'single', 'uv-cam0', 11, 256),
    ('c64', False, 'single', 'rays-clip', 513, 256),
    ('c64', False, 'single', 'uv-clip', 513, 256),
    ('j14_rf9_s3', False, 'single', 'rays', 97, 256),
    ('j14_rf9_s3', False, 'single', 'uv-cam0', 97, 256),
    ('c128', True, 'staged', 'uv-cam0', 1025, 256),
    ('j17_rf27_s3', False, 'staged', 'rays-clip', 49, 256),
    ('j17_rf27_s3', False, 'staged', 'uv-clip', 49, 256),
    ('j17_rf9_s1', True, 'single', 'rays', 513, 256),
    ('j17_rf9_s1', True, 'single', 'uv-cam0', 513, 256),
    ('j17_rf27_s3', False, 'single', 'rays-clip', 193, 256),
    ('j17_rf27_s3', False, 'single', 'uv-clip', 193, 256),
    ('j17_rf27_dense_s3', False, 'single', 'uv-cam0', 196, 256),
    ('j17_rf9_s1', False, 'staged', 'uv-cam0', 1025, 256),
    ('c64', False, 'single', 'rays', 513, 256),
    ('c64', False, 'single', 'uv-cam0', 513, 256),
    ('j17_rf243_s3', False, 'single', 'rays', 17, 256),
    ('j17_rf243_s3', False, 'single', 'uv-cam0', 17, 256),
    ('j17_rf27_s3', False, 'staged', 'uv-cam0', 1025, 256),
    ('c96', True, 'single', 'rays', 1025, 256),
    ('c64', False, 'staged', 'rays', 511, 256),
    ('c64', False, 'staged', 'uv-clip', 1100, 256),
    ('j17_rf81_s2_big', False, 'single', 'rays', 97, 256),
    ('j17_rf81_s2_big', False, 'single', 'uv-cam0', 97, 256),
    ('j17_rf81_s2_big', False, 'single', 'rays-clip', 97, 256),
    ('j17_rf81_s2_big', False, 'single', 'uv-clip', 97, 256),
    ('c64', True, 'single', 'uv-cam0', 1025, 256),
    ('j17_rf243_s3', False, 'staged', 'rays-clip', 50, 256),
    ('j17_rf81_s2_big', False, 'single', 'rays', 1025, 256),
    ('j17_rf81_s2_big', False, 'single', 'uv-cam0', 1025, 256),
    ('j17_rf27_s3', False, 'single', 'rays-clip', 1024, 256),
    ('j17_rf27_s3', False, 'single', 'uv-clip', 1024, 256),
    ('j17_rf27_s3', False, 'staged', 'uv-cam0', 1024, 256),
    ('c64', True, 'staged', 'rays', 1025, 256),
    ('j17_rf243_s3', False, 'staged', 'rays', 513, 256),
    ('j17_rf243_s3', False, 'single', 'rays-clip', 513, 256),
    ('j17_rf243_s3', False, 'single', 'uv-clip', 513, 256),
    ('j17_rf243_s3', False, 'staged', 'uv-cam0', 1024, 256),
    ('j17_rf81_s2_big', True, 'staged', 'uv-cam0', 1023, 256),
    ('j17_rf81_s2_big', True, 'single', 'rays', 1025, 256),
    ('j17_rf81_s2_big', True, 'single', 'uv-cam0', 1025, 256),
    ('j17_rf81_s2_big', True, 'staged', 'rays', 1025, 256),
    ('j17_rf81_s2_big', True, 'staged', 'uv-cam0', 1025, 256),
    ('j17_rf243_s3', False, 'single', 'rays', 511, 256),
    ('j17_rf243_s3', False, 'single', 'uv-cam0', 511, 256),
    ('c768_rf9', True, 'single', 'rays', 196, 256),
    ('n512', True, 'single', 'rays', 292, 256),
    ('n512', True, 'single', 'uv-cam0', 292, 256),
    ('c640', True, 'single', 'rays', 292, 256),
    ('rf729', False, 'single', 'rays', 26, 256),
    ('rf729', False, 'single', 'uv-cam0', 26, 256),
    ('rf729', False, 'single', 'rays', 31, 128),
    ('rf729', False, 'single', 'uv-cam0', 31, 128),
    ('j17_rf243_s3', True, 'staged', 'uv-cam0', 96, 128),
    ('c512', False, 'single', 'rays', 22, 64),
    ('c512', False, 'single', 'uv-cam0', 22, 64),
    ('c640', True, 'single', 'rays', 22, 64),
    ('c640', True, 'single', 'uv-cam0', 22, 64),
    ('rf729', False, 'single', 'rays', 23, 64),
    ('rf729', False, 'single', 'uv-cam0', 23, 64),
    ('j17_rf243_s3', True, 'staged', 'uv-cam0', 96, 64),
]

CASES = ALWAYS + [c for c in COVER if c not in ALWAYS]


def case_id(case):
    config, b3, form, shape, B, nwg = case
    return "%s-%s-%s-%s-%d" % (config, "bf16x3" if b3 else "f32", form, shape, B) + ("" if nwg == NWG else "-nwg%d" % nwg)
