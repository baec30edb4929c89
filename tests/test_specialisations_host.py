"""Census of kernel specialisations, on the host (hooks library, no GPU): which (kernel, tile kind) pairs the library's calls
run, by r3d_debug_forward_census - the driver's own plan / schedule / kernel / call-form selection plus ONE restatement of the
persistent loop's dispatch (r3d_hooks.cpp, census_tile_kind) - swept over the domain of tests/specialisation_cases.py at 256,
128 and 64 workgroups (the whole chip; a lane of R3D_OPT_LANES = 2 or an R3D_OPT_CU_LIMIT of 128; a lane of four).  At 256
workgroups B runs over every value 1 ... 300 plus 511, 512, 513, 700, 1023, 1024, 1025, 1100 and 4096 for the default model at
RF 9, 27 and 243; for the other configurations (fixtures, channel counts, one level, and the four of the wider accepted domain:
six levels, latent 512, 640 and 768 channels) the range is thinned to every value up to 140, every fourth from there to 300, and
the same large sizes.  At 128 and 64 workgroups every configuration runs every value up to 140 (the small and latency plans, all
plan switches), every eighth from there to 300 (192, 224 and 256 among them), 1024 and 1025.  The six-level model stops at 300
windows everywhere (specialisation_cases.sweep_batches).

Wall time of the module, one core: 36 s before the workgroup axis (18 configurations, 256 workgroups only); 119 s with it (22
configurations, three workgroup counts) - within three times the old time plus the added configurations' share (3 x 36 s x 22 / 18
= 133 s).  With every fourth value kept to 300 on the two new axes the sweep alone took 128 s: hence every eighth there.

tests/test_gpu_specialisations.py holds every case of the table to the oracle on the GPU, and the census to the launch records."""
import fnmatch

import pytest

import specialisation_cases as sc

# Kernels of the launch records' name table that no call of the domain launches.
UNREACHABLE_KERNELS = {
    # the pre-pass of the pixel modes (R3D_INPUT_UV_DIST / PX_INTRINSIC / PX_SCREEN, redirect_px): the forward behind it is the
    # rays one, which the domain holds; the census's call shapes are rays and R3D_INPUT_UV
    "r3d_undistort_rays_f64",
}

# Instantiations of the dispatch that no call of the domain selects: (kernel pattern, tile-kind pattern, why).  "code": the
# selection code excludes it; "domain": a call outside the domain reaches it; "packer": nothing excludes it, but the tile packer
# (r3d_schedule.cpp, pack / assign) produces it for no swept size at 256, 128 or 64 workgroups.
UNREACHABLE = [
    # --- code
    ("r3d_forward_clip_*", "first_level_taps<*",
     "code: a plan with a per-frame buffer gives EVERY fused first level its block of it (r3d_plan.cpp: frame_col of all or none), so in "
     "a clip call they all run first_level_shared"),
    ("r3d_gemm_*b3", "first_level_shared<*", "code: call_shares_first_layers refuses calls with bf16x3 tiles (b3_call)"),
    ("r3d_gemm_*b3", "gemv_tile", "code: bf16x3 tiles start at 96 windows (b3_min_batch); GEMV tiles need a layer of <= 4 rows"),
    ("r3d_gemm_*b3", "lat_tile", "code: bf16x3 tiles start at 96 windows (b3_min_batch); latency tiles need a layer of <= 32 rows"),
    ("r3d_gemm_uv_f32", "gemv_tile",
     "code: r3d_gemm_uv_f32 runs the launch that gathers inside r3d_gemm_f32 - the fused first level, plans of more than 48 windows "
     "(the small plan gathers in r3d_gemm_enc_uv_f32); every layer then has more than 32 rows"),
    ("r3d_gemm_uv_f32", "lat_tile", "code: as gemv_tile there"),
    ("r3d_forward_*lat", "first_level_taps<*",
     "code: the _lat kernels run lists with GEMV / latency tiles - a layer of <= 32 rows, so at most 32 windows: the small plan "
     "(plan_kind, <= 48 windows), which fuses no first level (only R3D_NO_SMALL_PLAN, a development switch, gets there)"),
    ("r3d_forward_*lat", "gemm_tile<?,1,pair>", "code: ... and no pairs"),
    # --- domain
    ("r3d_*b3", "first_level_taps<*",
     "domain: in a bf16x3 call the fused first levels of a bf16x3 model carry bf16x3 weights (Layer::bf3_conv); fp32 ones beside "
     "them need a pair with ONE bf16x3 handle - model_config['BF16X3'] sets both"),
    ("r3d_*b3", "gemm_tile<?,1,pair>", "domain: as the first level: the fused pairs of a bf16x3 model run gemm_tile_b3t"),
    # --- packer
    ("r3d_*", "gemm_tile<2,2>", "packer: assign() may give a workgroup two split-K-2 units of a column block; no swept size does"),
    ("r3d_forward_*b3", "gemm_tile_nb<[47]>",
     "packer: a bf16x3 model's 1024-wide Linears run gemm_tile_b3; its other layers wide enough for gemm_tile_nb (N >= 512: a latent "
     "size of 512 or more at <= 256 channels - wider models run launch by launch) are cut into 5- and 6-block tiles at every swept size"),
    ("r3d_gemm_uv_*", "gemm_tile_nb<?>",
     "packer: the launch that gathers is the plan's first; the wide plain layers (N >= 512, K >= 256) read the pyramids' outputs "
     "and sit in later launches"),
    ("r3d_gemm_uv_b3", "gemm_tile_b3<4>",
     "packer: the bf16x3 Linears beside a gathering first level get tiles of <= 3 units at every swept size and workgroup count"),
]


@pytest.fixture(scope="module")
def census():
    c = sc.Census()
    yield c
    c.close()


@pytest.fixture(scope="module")
def reached(census):
    return sc.sweep(census)


def _union(sets):
    out = set()
    for s in sets:
        out |= s
    return out


def test_the_table_reaches_every_pair_the_sweep_reaches(census, reached):
    """The union of (kernel, tile kind) pairs over CASES equals the union over the sweep: a specialisation added later fails here
    until a case reaches it.  Prints the census table: per kernel and tile kind, the smallest case of the table that reaches it."""
    table = {case: reached[case] if case in reached else frozenset(census.pairs(case)) for case in sc.CASES}
    swept, covered = _union(reached.values()), _union(table.values())
    first = {}
    for case in sorted(table, key=lambda c: (c[4], sc.CASES.index(c))):        # (ties in B: the whole chip first - the table's order)
        for p in table[case]:
            first.setdefault(p, case)
    print("\ncensus: %d cases swept, %d (kernel, tile kind) pairs, %d cases in the table" % (len(reached), len(swept), len(sc.CASES)))
    for (kernel, kind), case in sorted(first.items()):
        print("census %-26s %-36s %s" % (kernel, kind or "-", sc.case_id(case)))
    assert not swept - covered, "no case of specialisation_cases.CASES reaches %s: run tools/specialisation_cover.py" % sorted(swept - covered)
    assert not covered - swept, "cases outside the sweep's domain reach %s" % sorted(covered - swept)
    assert len(set(sc.CASES)) == len(sc.CASES)
    for case in sc.ALWAYS:
        assert case in sc.CASES
    assert {c[4] for c in sc.CASES if c[2] == "captured"} == set(sc.CAPTURED_BATCHES)


def test_the_table_is_the_greedy_cover(reached, census):
    """CASES is what tools/specialisation_cover.py prints: the known holes and the two captured calls, then the greedy cover that prefers the smallest B."""
    full = dict(reached)
    for case in sc.ALWAYS:
        full.setdefault(case, frozenset(census.pairs(case)))
    cases, _ = sc.smallest_cover(full, sc.ALWAYS)
    assert cases == sc.CASES


def test_every_kernel_and_every_instantiation_is_reached_or_explained(reached):
    """Every kernel of the launch records' name table and every instantiation of the dispatch (r3d_debug_census_domain: the same
    restatement over all header values) appears in the sweep, or in the commented lists above - and nothing listed there is
    reached after all."""
    from ray3d_amd import _capi
    _capi.use_hooks(True)
    names, dispatch = _capi.debug_census_domain()
    swept = _union(reached.values())
    launched = {k for k, _ in swept}
    assert len(set(names)) == len(names) and launched <= set(names), sorted(launched - set(names))
    assert set(names) - launched == UNREACHABLE_KERNELS, (sorted(set(names) - launched), sorted(UNREACHABLE_KERNELS))
    tiled = {p for p in swept if p[1]}
    assert tiled <= dispatch, sorted(tiled - dispatch)

    def why(pair):
        return [r for r in UNREACHABLE if fnmatch.fnmatchcase(pair[0], r[0]) and fnmatch.fnmatchcase(pair[1], r[1])]
    unexplained = sorted(p for p in dispatch - tiled if not why(p))
    assert not unexplained, "instantiations neither reached nor listed in UNREACHABLE: %s" % unexplained
    stale = sorted(p for p in tiled if why(p))
    assert not stale, "listed in UNREACHABLE, but reached: %s" % stale
    for rule in UNREACHABLE:
        assert any(fnmatch.fnmatchcase(k, rule[0]) and fnmatch.fnmatchcase(t, rule[1]) for k, t in dispatch), rule
    print("\ncensus: %d instantiations of the dispatch, %d reached, %d listed as unreachable" % (len(dispatch), len(tiled), len(dispatch - tiled)))


def test_the_census_names_the_launches_of_known_calls(census):
    """A few calls whose launches the GPU suite has asserted from launch records for a long time (test_gpu_parity.py), asked of
    the census: the hook agrees with them without a device."""
    kernels = lambda case: [k for k, _, _ in census.launches(case)]
    # a clip call: the per-frame launch, the bind, r3d_forward_clip_f32, the decoder tail (test_clip_calls_run_the_per_frame_first_layers)
    assert kernels(("j17_rf81_causal_s3", False, "single", "rays-clip", 200, sc.NWG)) == ["r3d_gemm_f32", "r3d_bind_f32", "r3d_forward_clip_f32", "r3d_decode_w4_f32"]
    assert kernels(("j17_rf81_causal_s3", False, "single", "uv-clip", 200, sc.NWG))[:3] == ["r3d_gemm_uv_f32", "r3d_bind_f32", "r3d_forward_clip_uv_f32"]
    # ... which a bf16x3 handle does not take: the gathered first level on the bf16 matrix cores
    assert kernels(("j17_rf81_s2_big", True, "single", "uv-clip", 200, sc.NWG)) == ["r3d_bind_f32", "r3d_forward_uv_b3", "r3d_decode_w4_f32"]
    # more than 256 channels: launch by launch, r3d_gemm_enc_* in front (test_forward_uv_on_the_unfused_first_layer_kernel)
    ks = kernels(("c512", True, "single", "uv-cam8", 97, sc.NWG))
    assert ks[0] == "r3d_gemm_enc_uv_f32" and "r3d_gemm_b3" in ks and not any(k.startswith("r3d_forward") for k in ks)
    # calls of a few windows: the _lat kernel with GEMV tiles, one block of the decoder per wavefront
    launches = census.launches(("j17_rf27_s3", False, "single", "rays", 3, sc.NWG))
    assert [k for k, _, _ in launches] == ["r3d_bind_f32", "r3d_forward_lat", "r3d_decode_f32"] and "gemv_run" in launches[1][2]
    # both K kinds of the bf16x3 first level in one pair call, with pixel input
    hist = census.launches(("j17_rf27_s3", True, "single", "uv-cam8", 97, sc.NWG))[1][2]
    assert {"first_level_taps_b3<1,K<=64,UV>", "first_level_taps_b3<1,K>64,UV>"} <= set(hist)
