"""CPU suite: the trained-checkpoint weight statistics of tests/trained_stats.py - what the profile is, the conditions the GPU
file (tests/test_gpu_trained_stats.py) rests on, why these weights see an eps that the synthetic ones cannot, and both oracles
against the reference's own outputs on them (tests/golden/model_trained_*.npz, written by tests/golden/make_golden_trained.py)."""
import numpy as np
import pytest
import torch

import trained_stats as ts
from conftest import load_model_fixture, synth_states
from oracle import oracle, torch_port
from test_oracle import ORACLE_ATOL, _tap_from_oracle

LITERAL = 1e-4


def _mc(over):
    import ray3d_amd
    return ray3d_amd.default_model_config(**over)


def _bn_arrays(state):
    var = np.concatenate([v for k, v in state.items() if k.endswith(".running_var")])
    gamma = np.concatenate([state[k[:-len("running_var")] + "weight"] for k in state if k.endswith(".running_var")])
    return var, gamma


# ---------------------------------------------------------------- the profile

def test_profile_is_deterministic_and_keeps_keys_shapes_and_dtypes():
    (cp, sp), (ct, st) = synth_states(_mc(ts.RF27))
    for state, seed in ((sp, 11), (st, 12)):
        before = {k: np.array(v, copy=True) for k, v in state.items()}
        a, b = ts.trained_like(state, seed), ts.trained_like(state, seed)
        assert list(a) == list(state)
        for k, v in state.items():
            assert np.array_equal(v, before[k]), k                      # pure: the input is left alone
            assert a[k].shape == np.shape(v) and a[k].dtype == np.asarray(v).dtype, k
            assert np.array_equal(a[k], b[k]), k
        assert a["GlobalInfo.bn_1.num_batches_tracked"].dtype == np.int64
        other = ts.trained_like(state, seed + 1)
        assert not np.array_equal(other["GlobalInfo.bn_1.running_var"], a["GlobalInfo.bn_1.running_var"])
        # layers without a BatchNorm behind them (shrink, fc_2) are untouched
        untouched = [k for k in state if ".shrink." in k or ".fc_2." in k]
        assert untouched and all(np.array_equal(a[k], state[k]) for k in untouched)


def test_profile_rescales_the_partner_row_with_the_variance():
    (_, sp), _ = synth_states(_mc(ts.RF27))
    a = ts.trained_like(sp, 11)
    from ray3d_amd import synth
    for p, w in (("LocalLayer_Torso.expand_bn", "LocalLayer_Torso.expand_conv"), ("LocalLayer_Torso.layers_bn.3", "LocalLayer_Torso.layers_conv.3"),
                 ("GlobalInfo.bn_1", "GlobalInfo.fc_1"), ("GlobalInfo.layers.1.batch_norm2", "GlobalInfo.layers.1.w2"),
                 ("embedder.b1", "embedder.w1"), ("embedder.b2", "embedder.w2")):
        assert ts.partner(p) == w
        C = sp[p + ".running_var"].shape[0]
        f = 10.0 ** (-7.0 + 9.0 * synth.hash_uniform("trained.var." + p, (C,), 11))
        r = np.sqrt(f)
        assert np.array_equal(a[p + ".running_var"], (sp[p + ".running_var"].astype(np.float64) * f).astype(np.float32))
        assert np.array_equal(a[p + ".running_mean"], (sp[p + ".running_mean"].astype(np.float64) * r).astype(np.float32))
        wt = sp[w + ".weight"].astype(np.float64)
        assert np.array_equal(a[w + ".weight"], (wt * r.reshape((C,) + (1,) * (wt.ndim - 1))).astype(np.float32))
        if w + ".bias" in sp:
            assert np.array_equal(a[w + ".bias"], (sp[w + ".bias"].astype(np.float64) * r).astype(np.float32))
        assert np.array_equal(np.abs(a[p + ".weight"])[a[p + ".weight"] != 0], sp[p + ".weight"][a[p + ".weight"] != 0])
        assert np.array_equal(a[p + ".bias"], sp[p + ".bias"])


def test_a_batchnorm_without_a_partner_layer_is_an_error():
    with pytest.raises(KeyError):
        ts.trained_like({"odd.norm.running_var": np.ones(4, np.float32)}, 1)
    with pytest.raises(KeyError):          # the grammar names a partner, the state has none
        ts.trained_like({"x.bn_1.running_var": np.ones(4, np.float32)}, 1)


@pytest.mark.parametrize("name", list(ts.TRAINED_CASES))
def test_profile_has_the_shares_of_a_trained_checkpoint(name):
    """Per network: dead channels (variance below eps), variances far above 1, negative and pruned gammas."""
    for cfg, st in ts.trained_states(_mc(ts.TRAINED_CASES[name][0])):
        var, gamma = _bn_arrays(st)
        shares = ((var < 1e-5).mean(), (var < 1e-4).mean(), (var > 10).mean(), (gamma < 0).mean(), (gamma == 0).mean())
        print("%s %s: %d channels, var < 1e-5 %.3f, < 1e-4 %.3f, > 10 %.3f, gamma < 0 %.3f, == 0 %.3f" % ((name, cfg.kind, var.size) + shares))
        assert shares[0] >= 0.15 and shares[2] >= 0.05
        assert 0.20 <= shares[3] <= 0.30
        assert shares[4] >= 0.01
        assert var.min() > 0 and np.isfinite(var).all()


def test_product_modules_load_the_trained_like_state_strictly():
    pos, trj, (_, sp), (_, st) = ts.build_trained_modules(_mc(ts.RF27))
    for module, state in ((pos, sp), (trj, st)):
        sd = {k[7:] if k.startswith("module.") else k: v for k, v in module.state_dict().items()}
        assert sorted(sd) == sorted(state)
        for k, v in state.items():
            assert np.array_equal(sd[k].numpy(), v), k


# ---------------------------------------------------------------- the conditions the GPU tests rest on

def _condition_cases():
    """(id, model_config overrides, decoder scale, how to build (x, param)): every trained fixture and every further
    configuration of tests/test_gpu_trained_stats.py at its size (calls of fewer windows of the same seed are the first rows)."""
    for name in ts.TRAINED_CASES:
        yield name, None, 1.0, ("fixture", name)
    for k, over in ts.SHRINK_CONFIGS.items():                      # (also the few-window and re-fold calls: RF 27, <= 75 windows)
        yield "windows-" + k, over, 1.0, ("windows", ts.SHRINK_WINDOWS, 21)
    for k, over in ts.WIDTH_CONFIGS.items():
        yield "width-" + k, over, 1.0, ("windows", ts.WIDTH_WINDOWS, 21)
    yield "rf243", ts.RF243, ts.RF243_SCALE, ("windows", ts.RF243_WINDOWS, 21)
    for k, over in ts.CLIP_CONFIGS.items():
        yield "clip-" + k, over, 1.0, ("clip",)
    for k, over in ts.UV_CONFIGS.items():
        yield "uv-" + k, over, 1.0, ("uv",)
    for seed in ts.RANDOM_SEEDS:
        over, B = ts.random_configuration(seed)
        yield "random-%d" % seed, over, 1.0, ("windows", B, seed)


_CONDITIONS = list(_condition_cases())


@pytest.mark.parametrize("case", _CONDITIONS, ids=[c[0] for c in _CONDITIONS])
def test_outputs_stay_below_10_m_and_the_cpu_fp32_error_below_a_tenth_of_the_bound(case):
    """What lets the GPU file hold every case to the literal 1e-4: each network's float64 output is at most 10 m (the scale
    the bound is meant at), and the reference's own arithmetic - the torch port in fp32 on the CPU - is within 1e-5 of the
    float64 evaluation (4.2e-6 was the worst when the profile was designed; 7.5e-6 is the worst here, the 130-window
    causal-dilated clip).  Two trained fixtures have |pos + trj| above 10 m (10.09 and 11.99 m) although neither network
    is: their sums are held to the same literal bound, which only asks more."""
    ident, over, scale, how = case
    if how[0] == "fixture":
        z, mc = load_model_fixture(how[1])
        x, p = z["x"], z["param"]
    else:
        mc = _mc(over)
    states = ts.trained_states(mc, scale)
    cp = states[0][0]
    if how[0] == "windows":
        x, p = ts.window_inputs(cp, how[1], seed=how[2])
    elif how[0] == "clip":
        _, x, _, p = ts.clip_inputs(cp)
    elif how[0] == "uv":
        from test_gpu_parity import _reference_cameras
        cams, ocams, _, _ = _reference_cameras()
        _, x, _, p = ts.uv_inputs(cp, cams, ocams)
        p = p.astype(np.float32)
    ref, cpu = ts.f64_and_cpu(states, x, p)
    per_network = [float(np.abs(ts.f64_and_cpu((s,), x, p)[0]).max()) for s in states]
    e_cpu = float(np.abs(cpu.astype(np.float64) - ref).max())
    print("%s: %d windows, max |pos| %.3f, |trj| %.3f, |pos + trj| %.3f m, torch-CPU fp32 error %.2e"
          % (ident, x.shape[0], per_network[0], per_network[1], np.abs(ref).max(), e_cpu))
    assert max(per_network) <= 10.0
    assert e_cpu <= 0.1 * LITERAL


# ---------------------------------------------------------------- teeth

def _f64_sum(states, x, p, var_plus=0.0):
    tot = 0
    for cfg, st in states:
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}
        sd = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}
        sd = {k: (v + var_plus if k.endswith(".running_var") else v) for k, v in sd.items()}
        with torch.no_grad():
            tot = tot + torch_port.forward(cfg, sd, torch.from_numpy(x).double(), torch.from_numpy(p).double())
    return tot.numpy()


@pytest.mark.parametrize("name", list(ts.TRAINED_CASES))
def test_an_eps_off_by_one_percent_misses_the_bound_fifty_times_over(name):
    """running_var + 1e-7 everywhere (in float64: an eps of 1.01e-5) moves the float64 outputs by >= 5e-3 m on the trained-like
    weights (5.9e-3 is the smallest here, 1.5e-2 the largest).  On the synthetic weights of the same models even a DOUBLED
    eps (running_var + 1e-5) moves them by < 1e-3 m: an eps wrong by a third passes every other forward test in the suite."""
    z, mc = load_model_fixture(name)
    x, p = z["x"], z["param"]
    trained = ts.trained_states(mc)
    moved = float(np.abs(_f64_sum(trained, x, p, 1e-7) - _f64_sum(trained, x, p)).max())
    synthetic = synth_states(mc)
    moved_synth = float(np.abs(_f64_sum(synthetic, x, p, 1e-5) - _f64_sum(synthetic, x, p)).max())
    print("%s: trained-like, var + 1e-7 moves the outputs by %.3e m; synthetic, eps doubled: %.3e m" % (name, moved, moved_synth))
    assert moved >= 5e-3 == 50 * LITERAL
    assert moved_synth < 1e-3


# ---------------------------------------------------------------- both oracles against the reference on these weights

@pytest.mark.parametrize("name", list(ts.TRAINED_CASES))
def test_c_oracle_matches_the_reference_on_trained_like_weights(name):
    z, mc = load_model_fixture(name)
    assert mc == _mc(ts.TRAINED_CASES[name][0]) and z["x"].shape[0] == ts.TRAINED_CASES[name][1]
    for kind, (cfg, st) in zip(("pos", "trj"), ts.trained_states(mc)):
        taps = {}
        out = oracle.forward(cfg, st, z["x"], z["param"], taps=taps)
        ref = z["out_" + kind]
        assert out.shape == ref.shape
        assert np.abs(out - ref).max() <= ORACLE_ATOL * max(1.0, np.abs(ref).max() / 10.0)
        checked = 0
        for k in z.files:
            if k.startswith(kind + "/"):
                r = z[k]
                o = _tap_from_oracle(taps, k.split("/", 1)[1]).reshape(r.shape)
                assert np.abs(o - r).max() <= 5e-5 * max(1.0, np.abs(r).max()), k
                checked += 1
        assert checked >= (5 if not mc["DISABLE_OPTIMIZATIONS"] else 4)
    assert int(z["receptive_field"]) == cfg.receptive_field


def _torch_port_taps(cfg, sd, x, p):
    """The torch port's value at every tap the fixtures record whole: block outputs by the name of their state prefix."""
    taps = {}
    real_fc, real_tb, real_tbd, real_emb = torch_port.fc_block, torch_port.temporal_block, torch_port.temporal_block_dense, torch_port.embedding

    def fc(sd_, pfx, *a):
        taps[pfx] = real_fc(sd_, pfx, *a)
        return taps[pfx]

    def tb(sd_, pfx, *a):
        taps[pfx] = real_tb(sd_, pfx, *a)
        return taps[pfx]

    def tbd(sd_, pfx, *a):
        taps[pfx] = real_tbd(sd_, pfx, *a)
        return taps[pfx]

    def emb(sd_, pfx, *a):
        taps[pfx] = real_emb(sd_, pfx, *a)
        return taps[pfx]

    torch_port.fc_block, torch_port.temporal_block, torch_port.temporal_block_dense, torch_port.embedding = fc, tb, tbd, emb
    try:
        with torch.no_grad():
            out = torch_port.forward(cfg, sd, x, p)
    finally:
        torch_port.fc_block, torch_port.temporal_block, torch_port.temporal_block_dense, torch_port.embedding = real_fc, real_tb, real_tbd, real_emb
    return out.numpy(), {k: v.numpy() for k, v in taps.items()}


@pytest.mark.parametrize("name", list(ts.TRAINED_CASES))
def test_torch_port_matches_the_reference_on_trained_like_weights(name):
    """Outputs and every block-level tap (the per-level BatchNorm taps are inside the port's fused expressions: the C oracle
    is held to those above)."""
    z, mc = load_model_fixture(name)
    x, p = torch.from_numpy(z["x"]), torch.from_numpy(z["param"])
    for kind, (cfg, st) in zip(("pos", "trj"), ts.trained_states(mc)):
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}
        out, taps = _torch_port_taps(cfg, sd, x, p)
        ref = z["out_" + kind]
        assert np.abs(out - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
        checked = 0
        for k in z.files:
            tap = k.split("/", 1)[1] if k.startswith(kind + "/") else None
            if tap in taps:
                r = z[k]
                assert np.abs(taps[tap].reshape(r.shape) - r).max() <= 1e-6 * max(1.0, np.abs(r).max()), k
                checked += 1
        assert checked >= 3
