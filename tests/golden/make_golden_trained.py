#!/usr/bin/env python3
"""Generate tests/golden/model_trained_*.npz by IMPORTING the reference on CPU: the reference's pos and trj modules under
weights with the BatchNorm statistics of a trained checkpoint (tests/trained_stats.py: variances over nine decades, dead
channels far below eps, negative and pruned gammas), loaded with load_state_dict(strict=True).

Needs a checkout of the reference (RAY3D_REFERENCE, as make_golden.py); the tests only read the .npz files it writes:

    python tests/golden/make_golden_trained.py

Cases: trained_stats.TRAINED_CASES (RF 27 default, 14 joints RF 9 stage 2, causal-dilated RF 81, two input features without
the camera embedding).  Inputs synth_rays(B, seed 3) / synth_param(B, seed 4), keys and taps exactly those of make_golden.py's
model fixtures, so conftest.load_model_fixture reads them.  The archives carry a fixed time stamp: a second run writes the
same bytes.  Only numbers leave this script; no reference source text is stored.
"""
import os
import sys
import zipfile

import numpy as np
import torch

import make_golden as mg                      # puts the reference and the repository on sys.path (cv2 stubbed)
from make_golden import default_model_config, synth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from trained_stats import TRAINED_CASES, trained_like   # noqa: E402


def load_trained(module, cfg, seed):
    state = trained_like(synth.synth_state(cfg, seed=seed), 10 + seed)
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    module.eval()


def restamp(path):
    """Rewrite an .npz with every member dated 1980-01-01 (np.savez stamps the wall clock): same arrays, reproducible bytes."""
    with np.load(path) as z:
        arrays = [(k, z[k]) for k in z.files]
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays:
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


if __name__ == "__main__":
    for name, (over, batch) in TRAINED_CASES.items():
        mg.write_model_fixture(name, default_model_config(**over), batch, load_trained)
        path = os.path.join(HERE, "model_%s.npz" % name)
        restamp(path)
        print("model_%s.npz: %d bytes" % (name, os.path.getsize(path)))
