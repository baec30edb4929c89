#!/usr/bin/env python3
"""A/B of the validation pass (Trainer.test): one r3d_clip_valid_losses call per clip against ONE r3d_clips_valid_losses call per
shard, on the H36M-shaped synthetic set of tools/clips_metrics_ab.py (240 clips, lengths U(1000, 6000), seed 0; weights from
ray3d_amd.synth).

  (a) `losses`: the losses only, on resident predictions - evaluate.clip_valid per clip (resident ground truth, rows written on
                the device) against evaluate.shard_valid_hip; the rows of both must be equal bit for bit.
  (b) `pass`:   the whole pass, evaluate.validate_clips against evaluate.validate_clips_batched (RF 243), without lanes.

Device-event times, 5 repetitions of each side, the two sides alternating; mean, min, max and standard deviation are kept.
No speed threshold: the ratio batched / per-clip and whether the two ranges overlap are recorded.
usage:  python tools/clips_valid_ab.py              every step in a fresh process of its own under its own time limit, stopping at
                                                    the first that fails, then profiles/clips_valid_ab.json is written
        python tools/clips_valid_ab.py --step S     one step (losses | pass): writes measure_out/clips_valid_ab.S.json
        --per-clip-only   time the per-clip side alone (alternating with nothing): runs on a build that has no
                          r3d_clips_valid_losses - the parent commit's, whose per-clip path is the yardstick
        --baseline FILE.. the --out files of --per-clip-only runs of another build in the same session (e.g. one before and one
                          after this run): stored as `baseline` beside every step, with whether this build's per-clip mean
                          lies within the range of their repetitions
        [--out FILE] [--clips N] [--reps R] another result file; a smaller run (rehearsals) - tools/clips_ab_common.py."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_ab_common as ab
from clips_ab_common import alternate, make_set, ranges_overlap, verdict

TOOL = "clips_valid_ab"
STEPS = (("losses", 300), ("pass", 420))      # (step, its time limit in seconds)


def result(what, timed, per_clip_only, equal, extra=None):
    res = {"what": what, "per_clip": timed[0]}
    if not per_clip_only:
        a, b = timed
        res.update({"batched": b, "ratio_batched_over_per_clip": round(b["mean_ms"] / a["mean_ms"], 4),
                    "ranges_overlap": ranges_overlap(a, b),
                    "rows_bit_equal": equal, "verdict": verdict(a, b)})
    res.update(extra or {})
    if not per_clip_only and not equal:
        raise SystemExit("the rows of the two paths differ: %s" % json.dumps(res))
    return res


def step_losses(n_clips, reps, per_clip_only):
    import numpy as np
    import torch
    from ray3d_amd import _capi, evaluate
    dev = torch.device("cuda", 0)
    clips = make_set(n_clips)
    lengths = [c.rays.shape[0] for c in clips]
    first = [int(v) for v in np.cumsum([0] + lengths[:-1])]
    total, longest = sum(lengths), max(lengths)
    gt_all = torch.from_numpy(np.concatenate([c.gt_norm for c in clips], axis=0)).to(dev)
    noise = torch.from_numpy(np.random.default_rng(1).normal(0, 0.03, tuple(gt_all.shape)).astype(np.float32)).to(dev)
    sum_all = (gt_all + noise).reshape(total, 1, 17, 3).contiguous()            # pos + trj, as the lifter writes it
    trj_all = (gt_all[:, :1] + noise[:, 1:2]).reshape(total, 1, 1, 3).contiguous()
    headers = torch.tensor([[float(k), float(k % 15), float(n)] for k, n in enumerate(lengths)], dtype=torch.float64)
    rows_a = torch.zeros((len(clips), evaluate.VALID_COLS), dtype=torch.float64)
    rows_a[:, :3] = headers
    rows_a = rows_a.to(dev)
    rows_b = rows_a.clone()
    sl = [slice(first[k], first[k] + n) for k, n in enumerate(lengths)]

    def per_clip():
        for k, c in enumerate(clips):
            evaluate.clip_valid(sum_all[sl[k]], trj_all[sl[k]], c, pos_is_sum=True, gt_dev=gt_all[sl[k]], out=rows_a[k])

    sides = [per_clip]
    if not per_clip_only:
        table, _, _, _ = evaluate.clip_frame_table(lengths)
        table_dev = evaluate._to_device_bytes(table, dev)
        sides.append(lambda: evaluate.shard_valid_hip(sum_all, trj_all, gt_all, table_dev, len(clips), total, longest, rows_b,
                                                      flags=_capi.R3D_VALID_POS_IS_SUM))
    timed = alternate(sides, reps, dev)
    equal = bool(torch.equal(rows_a.view(torch.int64), rows_b.view(torch.int64)))
    return result("validation losses only, predictions resident: %d clips, %d frames, J 17" % (len(clips), total), timed, per_clip_only, equal,
                  {"launches": {"per_clip": "%d x (losses + sum + row copy)" % len(clips), "batched": "2"}})


def step_pass(n_clips, reps, per_clip_only):
    import functools
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = make_set(n_clips)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter = ab.make_lifter(clips, dev)
    keep = {}

    def per_clip():
        keep["a"] = evaluate.validate_clips(lambda x, p: lifter.forward_clip(x, p, return_trj=True), clips, 243, dev)

    def batched():
        keep["b"] = evaluate.validate_clips_batched(functools.partial(lifter.forward_clip, return_trj=True), clips, 243, dev)

    with torch.no_grad():
        timed = alternate([per_clip] if per_clip_only else [per_clip, batched], reps, dev)
    lifter.check_status(dev)
    equal = per_clip_only or bool(torch.equal(keep["a"][1].view(torch.int64), keep["b"][1].view(torch.int64)))
    extra = {"valid_mm": {k: keep[k][0]["valid_mm"] for k in sorted(keep)}}
    for k, t in zip(("per_clip", "batched"), timed):
        t["poses_per_s"] = round(frames / t["mean_ms"] * 1e3, 1)
    return result("whole pass (upload, lift, losses, reduce), RF 243: %d clips, %d frames, no lanes" % (len(clips), frames), timed,
                  per_clip_only, equal, extra)


def main():
    ap = ab.parser(__doc__, TOOL, STEPS)
    ap.add_argument("--per-clip-only", action="store_true")
    ap.add_argument("--baseline", nargs="+")
    args = ap.parse_args()
    if args.step:
        return ab.run_step(TOOL, args, (step_losses if args.step == "losses" else step_pass)(args.clips, args.reps, args.per_clip_only))
    baseline = [json.load(open(f)) for f in args.baseline] if args.baseline else None

    def add_baseline(step, res):
        if baseline is not None:
            res["baseline"] = ab.baseline_entry(res["per_clip"], [b[step]["per_clip"] for b in baseline])

    return ab.run_steps(TOOL, STEPS, args, dict(ab.header(args), sides="per-clip only" if args.per_clip_only else "per-clip and batched"),
                        ["--per-clip-only"] if args.per_clip_only else [], add_baseline)


if __name__ == "__main__":
    sys.exit(main())
