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
        [--out FILE] [--clips N] [--reps R] another result file; a smaller run (rehearsals)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("losses", 300), ("pass", 420))      # (step, its time limit in seconds)
PART_DIR = os.path.join(ROOT, "measure_out")
OUT = os.path.join(ROOT, "profiles", "clips_valid_ab.json")


def stats(ms):
    import numpy as np
    a = np.asarray(ms, dtype=np.float64)
    return {"mean_ms": round(float(a.mean()), 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
            "std_ms": round(float(a.std(ddof=1)) if a.size > 1 else 0.0, 4), "reps_ms": [round(float(v), 4) for v in a]}


def verdict(a, b):
    """b against a, beyond the spread of the repetitions: the ranges of the two sides must not overlap."""
    if b["max_ms"] < a["min_ms"]:
        return "batched faster (ranges do not overlap)"
    if b["min_ms"] > a["max_ms"]:
        return "batched SLOWER (ranges do not overlap)"
    return "no difference beyond the spread (ranges overlap)"


def baseline_entry(mine, runs):
    """This build's per-clip side against the per-clip side of another build's runs (their repetitions' range taken together)."""
    lo, hi = min(r["min_ms"] for r in runs), max(r["max_ms"] for r in runs)
    return {"what": "the per-clip path on a build of the parent commit, same session", "per_clip_runs": runs,
            "range_ms": [lo, hi], "per_clip_mean_within_baseline_range": lo <= mine["mean_ms"] <= hi,
            "per_clip_mean_not_above_baseline_range": mine["mean_ms"] <= hi,
            "per_clip_ranges_overlap": not (mine["max_ms"] < lo or mine["min_ms"] > hi)}


def make_set(n_clips, seed=0):
    """bench.py's evaluation stand-in (tools/clips_metrics_ab.py's set): clip lengths ~ U(1000, 6000), four cameras, 15 actions."""
    import numpy as np
    import ray3d_amd
    from ray3d_amd import evaluate
    rng = np.random.default_rng(seed)
    lengths = [int(rng.integers(1000, 6001)) for _ in range(n_clips)]
    cams = [ray3d_amd.synthetic_camera(yaw, 4.5, -12.0, name="cam%d" % i) for i, yaw in enumerate((20, 110, 200, 290))]
    clips = []
    for i, n in enumerate(lengths):
        r = np.random.default_rng([seed, i])
        cam = cams[i % 4]
        world = r.normal(0, 0.3, (1, 17, 3)) + np.array([0, 0, 1.0]) + 0.02 * np.cumsum(r.normal(0, 1.0, (n, 1, 3)), axis=0) \
            + r.normal(0, 0.02, (n, 17, 3))
        rays = cam.rays_from_uv(cam.project(world)).astype(np.float32)
        clips.append(evaluate.Clip(cam, rays, cam.world2normalized(world).astype(np.float32), "A%d" % (i % 15), i))
    return clips


def alternate(sides, reps, dev):
    """reps x (every side in turn), each timed by a pair of device events on the current stream; one untimed round first."""
    import torch
    for run in sides:
        run()
    torch.cuda.synchronize(dev)
    times = [[] for _ in sides]
    for _ in range(reps):
        for run, acc in zip(sides, times):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(dev))
            run()
            e1.record(torch.cuda.current_stream(dev))
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return [stats(t) for t in times]


def result(what, timed, per_clip_only, equal, extra=None):
    res = {"what": what, "per_clip": timed[0]}
    if not per_clip_only:
        a, b = timed
        res.update({"batched": b, "ratio_batched_over_per_clip": round(b["mean_ms"] / a["mean_ms"], 4),
                    "ranges_overlap": not (b["max_ms"] < a["min_ms"] or b["min_ms"] > a["max_ms"]),
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
        table_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
        sides.append(lambda: evaluate.shard_valid_hip(sum_all, trj_all, gt_all, table_dev, len(clips), total, longest, rows_b,
                                                      flags=_capi.R3D_VALID_POS_IS_SUM))
    timed = alternate(sides, reps, dev)
    equal = bool(torch.equal(rows_a.view(torch.int64), rows_b.view(torch.int64)))
    return result("validation losses only, predictions resident: %d clips, %d frames, J 17" % (len(clips), total), timed, per_clip_only, equal,
                  {"launches": {"per_clip": "%d x (losses + sum + row copy)" % len(clips), "batched": "2"}})


def step_pass(n_clips, reps, per_clip_only):
    import functools
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import evaluate, synth
    from ray3d_amd.spec import config_from_dicts
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    for m, kind, seed in ((pos, "pos", 1), (trj, "trj", 2)):
        cfg = config_from_dicts(mc, kind)
        ray3d_amd.load_weight(m, {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(cfg, seed=seed).items()})
        m.eval()
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    clips = make_set(n_clips)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter.prepare(sorted(set(b for c in clips for b in lifter.clip_batch_sizes(c.rays.shape[0]))), dev)
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--clips", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--per-clip-only", action="store_true")
    ap.add_argument("--baseline", nargs="+")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    os.makedirs(PART_DIR, exist_ok=True)
    part = lambda s: os.path.join(PART_DIR, "clips_valid_ab.%s.json" % s)
    if args.step:
        res = (step_losses if args.step == "losses" else step_pass)(args.clips, args.reps, args.per_clip_only)
        with open(part(args.step), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({args.step: res}))
        return 0
    merged = {"set": "%d clips, lengths U(1000, 6000), seed 0" % args.clips, "repetitions": args.reps,
              "timing": "device events around each side, sides alternating, one untimed round first",
              "sides": "per-clip only" if args.per_clip_only else "per-clip and batched"}
    baseline = [json.load(open(f)) for f in args.baseline] if args.baseline else None
    for step, limit in STEPS:                     # a fresh process per step; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--clips", str(args.clips), "--reps", str(args.reps)] + (["--per-clip-only"] if args.per_clip_only else [])).returncode
        if rc != 0:
            print("step %s ended with status %d: stopping" % (step, rc), file=sys.stderr)
            return rc
        merged[step] = json.load(open(part(step)))
        if baseline is not None:
            merged[step]["baseline"] = baseline_entry(merged[step]["per_clip"], [b[step]["per_clip"] for b in baseline])
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
