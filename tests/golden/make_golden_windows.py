#!/usr/bin/env python3
"""Generate tests/golden/windows.npz by IMPORTING the reference on CPU: the materialised evaluation windows and training chunks
that r3d_clips_windows gathers on the device.

Run in the build container only (needs the reference; the GPU box never has it):

    python tests/golden/make_golden_windows.py

What is pinned, for two cases - RF 27 (pad 13) on (N, 17, 3) inputs and RF 9 (pad 4) on (N, 14, 2) inputs - over clips of
1, 2, 5, 13, 14 and 40 frames of seeded float32 noise:
  * ``<case>_src``: the clips back to back, ``<case>_lengths``;
  * ``<case>_eval_s<shift>_f<flip>``: for causal_shift 0 and pad, what UnchunkedGenerator (lib/dataloader/generators.py:209-234:
    np.pad(..., 'edge'), with augment=True its mirrored second sequence) and Trainer.eval_data_prepare
    (lib/train_val/trainer.py:47-58) make of every clip, concatenated in clip order: (sum N, RF, J, F).  The mirrored sequence of
    the generator is checked here against the flip lines of Trainer.evaluate_core (trainer.py:299-302) applied to the padded clip;
  * ``<case>_chunk_s<shift>``: every chunk of a ChunkedGenerator (chunk_length 1, augment=True, unshuffled) over the same clips,
    (chunks, RF, J, F), with ``<case>_chunk_s<shift>_pairs``: (sequence, start_3d, flip) per chunk.
Only numbers leave this script; no reference source text is stored.
"""
import os

import numpy as np
import torch

import make_golden as mg                      # noqa: F401  puts the reference on sys.path (cv2 stubbed)
from lib.dataloader.generators import ChunkedGenerator, UnchunkedGenerator    # noqa: E402
from lib.train_val.trainer import Trainer                                     # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (1, 2, 5, 13, 14, 40)
KPS = {17: ([4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]), 14: ([4, 5, 6, 10, 11], [1, 2, 3, 12, 13])}
CASES = {"rf27": (13, 17, 3), "rf9": (4, 14, 2)}


def main():
    out = {"lengths": np.asarray(LENGTHS, dtype=np.int64)}
    for name, (pad, J, F) in CASES.items():
        rf = 2 * pad + 1
        rng = np.random.RandomState(100 + rf)
        clips = [rng.standard_normal((n, J, F)).astype(np.float32) for n in LENGTHS]
        left, right = KPS[J]
        out[name + "_src"] = np.concatenate(clips, axis=0)
        out[name + "_kps_left"], out[name + "_kps_right"] = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
        for shift in (0, pad):
            gen = UnchunkedGenerator(None, None, clips, pad=pad, causal_shift=shift, augment=True, kps_left=left, kps_right=right)
            plain, flipped = [], []
            for _, _, batch_2d in gen.next_epoch():
                x = torch.from_numpy(batch_2d.astype("float32"))
                # trainer.py:299-302 on the straight sequence gives the generator's mirrored one
                xf = x[:1].clone()
                xf[:, :, :, 0] *= -1
                xf[:, :, left + right, :] = xf[:, :, right + left, :]
                assert torch.equal(xf[0], x[1])
                for dst, seq in ((plain, x[0:1]), (flipped, x[1:2])):
                    w, _ = Trainer.eval_data_prepare(rf, seq.reshape(1, *seq.shape[1:]), None)
                    dst.append(w.numpy().astype(np.float32).reshape(-1, rf, J, F))
            out["%s_eval_s%d_f0" % (name, shift)] = np.concatenate(plain, axis=0)
            out["%s_eval_s%d_f1" % (name, shift)] = np.concatenate(flipped, axis=0)
            cams = [[None] * n for n in LENGTHS]
            total = 2 * sum(LENGTHS)
            cg = ChunkedGenerator(total, cams, None, clips, 1, pad=pad, causal_shift=shift, shuffle=False, augment=True,
                                  kps_left=left, kps_right=right)
            batches = list(cg.next_epoch())
            assert len(batches) == 1 and batches[0][2].shape[0] == total
            keep = np.arange(0, total, 5)                                  # a handful: every fifth chunk, both flip halves
            out["%s_chunk_s%d" % (name, shift)] = batches[0][2][keep].astype(np.float32)
            out["%s_chunk_s%d_pairs" % (name, shift)] = np.asarray([[int(cg.pairs[i][0]), int(cg.pairs[i][1]), int(bool(cg.pairs[i][3]))]
                                                                    for i in keep], dtype=np.int64)
    path = os.path.join(HERE, "windows.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
