"""Shared helper of tests/test_trained_stats_host.py, tests/test_gpu_trained_stats.py and tests/golden/make_golden_trained.py:
weights with the BatchNorm statistics of a TRAINED checkpoint.  ray3d_amd.synth draws every running_var from [0.5, 1.5] and every
gamma from [0.8, 1.2]: there `var + eps` is `var` to 1e-5, no gamma is negative or zero, and an eps that is wrong by a third
moves no output by 1e-4.  trained_like() spreads the variances over nine decades (1e-7 ... 1e2 times the synthetic ones: dead
channels far below eps, a few far above 1), flips a quarter of the gammas and prunes 2 % of them, and rescales the row of the
layer that feeds each BatchNorm channel so that its pre-BN output really has the variance the BN claims - activations stay O(1),
and the eps under the square root decides the output of every small-variance channel.  The profile itself is numpy only (torch and
the package are imported inside the helpers that need them)."""
import numpy as np

# running_var prefix suffix -> the same suffix of the layer whose output the BatchNorm reads
_PARTNER_LAST = {"expand_bn": "expand_conv", "bn_1": "fc_1", "batch_norm1": "w1", "batch_norm2": "w2", "b1": "w1", "b2": "w2"}

NEG_SHARE, ZERO_ABOVE = 0.25, 0.98

# name -> (model_config overrides, windows): tests/golden/model_<name>.npz, written by tests/golden/make_golden_trained.py
TRAINED_CASES = {
    "trained_j17_rf27_s3": (dict(ARCHITECTURE="3,3,3"), 3),
    "trained_j14_rf9_s2": (dict(ARCHITECTURE="3,3", NUM_KPTS=14, STAGE=2), 4),
    "trained_j17_rf81_causal_s3": (dict(ARCHITECTURE="3,3,3,3", DISABLE_OPTIMIZATIONS=True, CAUSAL=True), 3),
    "trained_j17_f2_rf27_noemb_s3": (dict(ARCHITECTURE="3,3,3", INPUT_DIM=2, CAMERA_EMBDDING=False), 3),
}


def partner(bn_prefix):
    """'<...>.expand_bn' -> '<...>.expand_conv', '<...>.layers_bn.3' -> '<...>.layers_conv.3', bn_1 -> fc_1,
    batch_norm1 / batch_norm2 -> w1 / w2 (the residual units), b1 / b2 -> w1 / w2 (the Embedding)."""
    parts = bn_prefix.split(".")
    if len(parts) >= 2 and parts[-2] == "layers_bn" and parts[-1].isdigit():
        return ".".join(parts[:-2] + ["layers_conv", parts[-1]])
    if parts[-1] in _PARTNER_LAST:
        return ".".join(parts[:-1] + [_PARTNER_LAST[parts[-1]]])
    raise KeyError("no partner layer for BatchNorm %r" % bn_prefix)


def trained_like(state, seed):
    """A new state dict (same keys, shapes, dtypes): per BatchNorm `p` with C channels and partner layer `w`,
      f = 10 ** (-7 + 9 u),  u = hash_uniform("trained.var." + p, (C,), seed),  r = sqrt(f);
      w.weight[o] *= r[o] (float64, rounded once to float32), w.bias *= r, running_mean *= r, running_var *= f;
      gamma negated where s < 0.25, zero where s > 0.98,  s = hash_uniform("trained.sign." + p, (C,), seed)."""
    from ray3d_amd import synth
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    done = 0
    for key in state:
        if not key.endswith(".running_var"):
            continue
        p = key[:-len(".running_var")]
        w = partner(p)
        if w + ".weight" not in state:
            raise KeyError("BatchNorm %r: partner %r is not in the state" % (p, w))
        C = state[key].shape[0]
        f = 10.0 ** (-7.0 + 9.0 * synth.hash_uniform("trained.var." + p, (C,), seed))
        r = np.sqrt(f)
        wt = state[w + ".weight"]
        assert wt.shape[0] == C, (p, w, wt.shape, C)
        out[w + ".weight"] = (wt.astype(np.float64) * r.reshape((C,) + (1,) * (wt.ndim - 1))).astype(np.float32)
        if w + ".bias" in state:
            out[w + ".bias"] = (state[w + ".bias"].astype(np.float64) * r).astype(np.float32)
        out[p + ".running_mean"] = (state[p + ".running_mean"].astype(np.float64) * r).astype(np.float32)
        out[key] = (state[key].astype(np.float64) * f).astype(np.float32)
        s = synth.hash_uniform("trained.sign." + p, (C,), seed)
        g = state[p + ".weight"].astype(np.float64)
        g = np.where(s < NEG_SHARE, -g, g)
        out[p + ".weight"] = np.where(s > ZERO_ABOVE, 0.0, g).astype(np.float32)
        done += 1
    assert done == sum(k.endswith(".running_var") for k in state)
    for k, v in state.items():
        assert out[k].shape == np.shape(v) and out[k].dtype == np.asarray(v).dtype, k
    return out


def trained_states(mc, out_scale=1.0):
    """((cfg_pos, state_pos), (cfg_trj, state_trj)) like conftest.synth_states: synth_state seeds 1 / 2, trained_like seeds 11 / 12."""
    from conftest import synth_states
    (cp, sp), (ct, st) = synth_states(mc, out_scale)
    return (cp, trained_like(sp, 11)), (ct, trained_like(st, 12))


def load_states(pos, trj, sp, st):
    import torch
    import ray3d_amd
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})


def build_trained_modules(mc, out_scale=1.0):
    """test_gpu_parity.build_modules with the trained-like weights: (pos, trj, (cfg_pos, state_pos), (cfg_trj, state_trj))."""
    import ray3d_amd
    (cp, sp), (ct, st) = trained_states(mc, out_scale)
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    load_states(pos, trj, sp, st)
    pos.eval(), trj.eval()
    return pos, trj, (cp, sp), (ct, st)


# ---------------------------------------------------------------- the inputs the host and the GPU file share

RF27 = dict(ARCHITECTURE="3,3,3")
CLIP_WINDOWS = 130
CLIP_CONFIGS = {"rf27": RF27, "rf81-causal-dilated": TRAINED_CASES["trained_j17_rf81_causal_s3"][0],
                "f2-noemb": TRAINED_CASES["trained_j17_f2_rf27_noemb_s3"][0]}
UV_WINDOWS = 24
UV_CONFIGS = {"rf9": dict(ARCHITECTURE="3,3"), "rf27": RF27}
SHRINK_WINDOWS = 75
SHRINK_CONFIGS = {"default": RF27, "c128-l160-s2": dict(RF27, CHANNELS=128, LATENT_FEATURES_DIM=160, STAGE=2)}
WIDTH_WINDOWS = 70
WIDTH_CONFIGS = {"c64": dict(RF27, CHANNELS=64, LATENT_FEATURES_DIM=128), "c96": dict(RF27, CHANNELS=96, LATENT_FEATURES_DIM=128),
                 "c128": dict(RF27, CHANNELS=128, LATENT_FEATURES_DIM=160), "c384": dict(RF27, CHANNELS=384),
                 "c512": dict(RF27, CHANNELS=512)}
RF243_WINDOWS = 40
RF243 = dict(ARCHITECTURE="3,3,3,3,3")
RF243_SCALE = 0.5        # decoder scale: at 1.0 the RF-243 trajectory output reaches 10.4 m on these 40 windows, at 0.5 it is 7.3 m
RANDOM_SEEDS = [2000, 2001, 2002, 2003, 2004]


def window_inputs(cfg, B, seed=21):
    """(x (B, RF, J, F), param (B, 2)); the first rows of a larger call with the same seed are the smaller call's."""
    from ray3d_amd import synth
    return synth.synth_rays(B, cfg, seed=seed), synth.synth_param(B, seed=seed + 1)


def clip_inputs(cfg, n=CLIP_WINDOWS):
    """A clip of n + RF - 1 frames in the distribution of synth_rays (no two windows alike), its n sliding windows, the clip's
    parameter row and that row per window."""
    from ray3d_amd import synth
    rf = cfg.receptive_field
    frames = n + rf - 1
    clip = np.concatenate(list(synth.synth_rays(-(-frames // rf), cfg, seed=5)), axis=0)[:frames].copy()
    clip += (0.001 * np.arange(frames, dtype=np.float32))[:, None, None]
    windows = np.stack([clip[i:i + rf] for i in range(n)])
    prow = np.array([1.5, 0.2], np.float32)
    return clip, windows, prow, np.tile(prow, (n, 1))


def uv_inputs(cfg, cams, ocams, B=UV_WINDOWS):
    """Pixels with one of the reference cameras per window: (uv, rays encoded by the oracle cameras in float64 and cast, camera
    rows, parameter rows).  cams / ocams: test_gpu_parity._reference_cameras()."""
    from ray3d_amd import synth
    rf = cfg.receptive_field
    uv = (1000.0 * synth.hash_uniform("uvtrained%d" % rf, (B, rf, cfg.num_joints, 2), 9)).astype(np.float32)
    pick = [i % len(cams) for i in range(B)]
    rays = np.stack([ocams[c].rays_from_uv(uv[i].astype(np.float64)) for i, c in enumerate(pick)]).astype(np.float32)
    return uv, rays, np.stack([cams[c].cam_row() for c in pick]), np.stack([cams[c].param() for c in pick])


def random_configuration(seed):
    """(model_config overrides, windows) drawn as test_gpu_parity.test_random_configurations_match_the_oracle_chain draws them
    (joints, input dimension, depth, channels, latent size, stage, camera embedding, geometry); the precision is the caller's."""
    rng = np.random.default_rng(seed)
    levels = int(rng.integers(1, 5))
    over = dict(ARCHITECTURE=",".join(["3"] * levels), NUM_KPTS=int(rng.choice([14, 15, 17])),
                INPUT_DIM=int(rng.choice([2, 3])), CHANNELS=int(rng.choice([64, 96, 128, 256, 256, 384])),
                LATENT_FEATURES_DIM=int(rng.choice([64, 128, 256])), STAGE=int(rng.choice([1, 2, 3])),
                CAMERA_EMBDDING=bool(rng.integers(0, 2)), EMBEDD_DIM=int(rng.choice([32, 64])))
    geom = int(rng.integers(0, 4))                  # strided | dilated | dilated + causal | dense (short receptive fields)
    if geom >= 1:
        over["DISABLE_OPTIMIZATIONS"] = True
    if geom == 2:
        over["CAUSAL"] = True
    if geom == 3 and levels <= 3:
        over["DENSE"] = True
    return over, int(rng.choice([1, 7, 33, 100]))


def f64_and_cpu(states, x, p):
    """(float64 evaluation of the torch port, its fp32 evaluation) of pos + trj: test_gpu_parity._f64_and_cpu_errors."""
    import torch
    from oracle import torch_port
    out = []
    for dt in (torch.float64, torch.float32):
        tot = 0
        for cfg, st in states:
            sd = {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}
            sd = {k: (v.to(dt) if v.dtype == torch.float32 else v) for k, v in sd.items()}
            with torch.no_grad():
                tot = tot + torch_port.forward(cfg, sd, torch.from_numpy(x).to(dt), torch.from_numpy(p).to(dt))
        out.append(tot.numpy())
    return out[0], out[1]
