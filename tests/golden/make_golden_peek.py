#!/usr/bin/env python3
"""Generate tests/golden/peek.npz by IMPORTING the reference on CPU: the windows r3d_streams_peek writes for a live stream - what
the reference builds when a clip ENDS at the newest frame.

Run in the build container only (needs the reference; the GPU box never has it):

    python tests/golden/make_golden_peek.py

The two cases and the six seeded clips of windows.npz (make_golden_windows.py: the same seeds, so the same numbers; checked here
against that file when it is present): RF 27 (pad 13) on (N, 17, 3) and RF 9 (pad 4) on (N, 14, 2), clips of 1, 2, 5, 13, 14 and
40 frames.  For a fixed list of (clip k, prefix length c, look L) - every clip at its full length, the longest clip at c = 1, 2,
lag / 2, lag / 2 + 1, lag, lag + 1, RF, RF + 1, RF + 6 and 40, each with the looks 0, lag / 2 and lag - 1 - what
UnchunkedGenerator (lib/dataloader/generators.py:209-234: np.pad(..., 'edge'), causal_shift 0, with augment=True its mirrored
second sequence) and Trainer.eval_data_prepare (lib/train_val/trainer.py:47-58) make of clip[:c], window c - 1 - L of it:
  * ``<case>_pairs``: (P, 4) int64 rows (k, c, L, row): `row` indexes the two arrays below, or is -1 where c <= L (frame c - 1 - L
    does not exist: there is no preview);
  * ``<case>_plain`` / ``<case>_mirror``: (rows, RF, J, F) float32, the straight and the mirrored sequence's window.
Only numbers leave this script; no reference source text is stored.
"""
import os

import numpy as np
import torch

import make_golden as mg                      # noqa: F401  puts the reference on sys.path (cv2 stubbed)
from lib.dataloader.generators import UnchunkedGenerator    # noqa: E402
from lib.train_val.trainer import Trainer                   # noqa: E402

from make_golden_windows import CASES, KPS, LENGTHS          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def looks_of(lag):
    return (0, lag // 2, lag - 1)


def prefixes(rf, lag):
    """-> [(clip, c)]: every clip whole, the longest clip at the lengths where the window's shape changes."""
    longest = len(LENGTHS) - 1
    cs = sorted({1, 2, lag // 2, lag // 2 + 1, lag, lag + 1, rf, rf + 1, rf + 6, LENGTHS[longest]})
    return [(k, n) for k, n in enumerate(LENGTHS[:-1])] + [(longest, c) for c in cs]


def main():
    out = {"lengths": np.asarray(LENGTHS, dtype=np.int64)}
    have = os.path.join(HERE, "windows.npz")
    pinned = np.load(have) if os.path.exists(have) else None
    for name, (pad, J, F) in CASES.items():
        rf, lag = 2 * pad + 1, pad
        rng = np.random.RandomState(100 + rf)
        clips = [rng.standard_normal((n, J, F)).astype(np.float32) for n in LENGTHS]
        if pinned is not None:
            assert np.array_equal(np.concatenate(clips, axis=0).view(np.uint32), pinned[name + "_src"].view(np.uint32))
        left, right = KPS[J]
        pairs, plain, mirror = [], [], []
        for k, c in prefixes(rf, lag):
            gen = UnchunkedGenerator(None, None, [clips[k][:c]], pad=pad, causal_shift=0, augment=True, kps_left=left, kps_right=right)
            (_, _, batch_2d), = list(gen.next_epoch())
            x = torch.from_numpy(batch_2d.astype("float32"))
            wins = [Trainer.eval_data_prepare(rf, x[f:f + 1], None)[0].numpy().astype(np.float32).reshape(c, rf, J, F) for f in (0, 1)]
            for L in looks_of(lag):
                p = c - 1 - L
                pairs.append((k, c, L, len(plain) if p >= 0 else -1))
                if p >= 0:
                    plain.append(wins[0][p])
                    mirror.append(wins[1][p])
        out[name + "_pairs"] = np.asarray(pairs, dtype=np.int64)
        out[name + "_plain"], out[name + "_mirror"] = np.stack(plain), np.stack(mirror)
    path = os.path.join(HERE, "peek.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
