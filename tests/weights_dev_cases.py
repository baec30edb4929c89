"""Shared by tests/test_weights_dev_host.py and tests/test_gpu_weights_dev.py: the configurations r3d_finalize_dev is checked on and
the two kinds of weights.  Each name is a configuration of tests/specialisation_cases.py; what it adds to the pack:
  j17_rf9_s1            stage 1: the Integration blocks' shrink fold alone;
  j14_rf9_s3            FuseBlocks' four folded ranges, groups with and without the root joint, per-frame [E | V] layers;
  j17_f2_rf27_noemb_s3  two input features, no embedding;
  j17_rf27_dense_s3     the dense ablation's wide taps, no per-frame layers;
  c384                  more channels than the latent size: no shrink fold at all;
  j17_rf27_s3 + bf16x3  the copies in bf16-MFMA operand order."""
import numpy as np

import specialisation_cases
import trained_stats
from conftest import synth_states

CASES = [("j17_rf9_s1", False), ("j14_rf9_s3", False), ("j17_f2_rf27_noemb_s3", False), ("j17_rf27_dense_s3", False), ("c384", False),
         ("j17_rf27_s3", True)]
GPU_EXTRA = [("j17_rf81_causal_s3", False), ("j15_rf9_s3", False)]
WEIGHTS = ("synth", "trained")


def case_id(case):
    return case[0] + ("-bf16x3" if case[1] else "")


def states_of(case, weights):
    """(model_config, (cfg_pos, state_pos), (cfg_trj, state_trj)): conftest.synth_states or trained_stats.trained_states."""
    from conftest import case_out_scale
    mc = dict(specialisation_cases.model_config(case[0], case[1]))
    make = synth_states if weights == "synth" else trained_stats.trained_states
    sp, st = make(mc, case_out_scale(case[0]))
    return mc, sp, st


def set_host_weights(handle, state):
    for key in handle.keys():
        handle.set_weight(key, np.ascontiguousarray(state[key], dtype=np.float32))
