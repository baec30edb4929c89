#!/usr/bin/env python3
"""A/B of a synthetic camera sweep (the reference's data/camera_augmentation.py + scripts/synthetic/test_aug.py: the world-frame
ground truth seen through a grid of virtual cameras, one whole evaluation per camera): the HOST path - per camera and clip
Camera.project, Camera.rays_from_uv and Camera.world2normalized in NumPy float64, Clip objects, evaluate_clips_batched(finish=True):
everything the parent commit has - against evaluate.evaluate_camera_sweep, which uploads the world poses once and makes every
camera's inputs and ground truth on the device (r3d_clips_project).  The set has the `Translation` set's shape: 36 cameras
(6 yaws x 6 distance ratios around one base camera), H36M-shaped clips as bench.py --mode eval builds them (lengths U(1000, 6000),
seed 0, 15 actions), RF 243, flip off, no lanes.

  (a) `input`: the input step alone, per camera - host: projection + encoding + edge padding + the uploads of inputs and ground
               truth, clip by clip; device: ONE evaluate.shard_project_hip call per pass of --cameras-per-pass cameras, world poses
               resident.  Also the project call's own device time and the bytes it moves against the device's memory rate (it is a
               streaming kernel: 12 bytes read, 12 + 12 written per point with the ground truth, 12 more with the mirrored copy).
  (b) `pass`:  the whole sweep - host path against evaluate_camera_sweep; the per-camera, per-action errors of the two must agree
               to 1e-3 mm (the inputs differ by at most one float32 ulp: the host path rounds the same float64 chain in another
               operation order).

Times are host-clock times with the device synchronised before and after (both sides do host work), --reps repetitions of each
side, the two sides alternating, one untimed round first; mean, min, max and standard deviation are kept.  No speed threshold: the
ratio and whether the two ranges overlap are recorded.
usage:  python tools/camera_sweep_ab.py              every step in a fresh process of its own under its own time limit, stopping at
                                                     the first that fails, then profiles/camera_sweep_ab.json is written
        python tools/camera_sweep_ab.py --step S     one step (input | pass): writes measure_out/camera_sweep_ab.S.json
        [--out FILE] [--clips N] [--reps R] [--cameras C] [--cameras-per-pass P]   (tools/clips_ab_common.py)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_ab_common as ab
from clips_ab_common import alternate, ranges_overlap, verdict

TOOL = "camera_sweep_ab"
STEPS = (("input", 420), ("pass", 560))       # (step, its time limit in seconds)
RF = 243
HBM_GBPS = 8000.0                             # the MI355X's memory rate (8 TB/s), the yardstick of a streaming kernel


def make_sweep(n_clips, n_cameras, seed=0):
    """(world clips, cameras): bench.py's evaluation stand-in in WORLD coordinates and a yaw x distance grid of virtual cameras
    around one synthetic base camera, 1000 x 1000 frame."""
    import numpy as np
    import ray3d_amd
    from ray3d_amd import camera, evaluate
    rng = np.random.default_rng(seed)
    lengths = [int(rng.integers(1000, 6001)) for _ in range(n_clips)]
    clips = []
    for i, n in enumerate(lengths):
        r = np.random.default_rng([seed, i])
        world = r.normal(0, 0.3, (1, 17, 3)) + np.array([0, 0, 1.0]) + 0.002 * np.cumsum(r.normal(0, 1.0, (n, 1, 3)), axis=0) \
            + r.normal(0, 0.02, (n, 17, 3))
        clips.append(evaluate.WorldClip(world.astype(np.float32), "A%d" % (i % 15), i))
    base = ray3d_amd.synthetic_camera(20, 4.5, -12.0)
    yaws = tuple(60 * k for k in range(6))
    ratios = tuple(1.0 + 0.1 * k for k in range(-(-n_cameras // 6)))
    cams = camera.camera_grid(base.K, base.Rw2c, base.Tw2c, (yaws, ratios, (0,)), center=(0.0, 0.0, 1.0))[:n_cameras]
    return clips, [ray3d_amd.Camera(c.K, c.Rw2c, c.Tw2c, name=c.name, res_w=1000, res_h=1000) for c in cams]


def host_clips(world_clips, cam):
    """What the parent commit offers for one camera: NumPy float64 projection, encoding and ground truth, one Clip per clip."""
    import numpy as np
    from ray3d_amd import evaluate
    out = []
    for c in world_clips:
        w = c.world.astype(np.float64)
        out.append(evaluate.Clip(cam, cam.rays_from_uv(cam.project(w)).astype(np.float32), cam.world2normalized(w).astype(np.float32),
                                 c.action, c.clip_id))
    return out


def compare(a, b, extra=None):
    res = {"host": a, "device": b, "ratio_device_over_host": round(b["mean_ms"] / a["mean_ms"], 4), "ranges_overlap": ranges_overlap(a, b),
           "verdict": verdict(a, b, "device")}
    res.update(extra or {})
    return res


def step_input(args):
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    wc, cams = make_sweep(args.clips, args.cameras)
    frames = sum(c.world.shape[0] for c in wc)
    pad = (RF - 1) // 2
    sizes_of = ray3d_amd.Ray3DLifter.clip_batch_sizes.__get__(ray3d_amd.Ray3DLifter)      # (the class defaults: CLIP_CHUNK, CLIP_ROUND)
    surplus = lambda n: sum(sizes_of(n)) - n
    per_pass = args.cameras_per_pass
    world_all = torch.from_numpy(np.concatenate([c.world for c in wc], axis=0)).to(dev)
    passes = []
    for at in range(0, len(cams), per_pass):
        pairs = [(k, ci) for ci in range(at, min(at + per_pass, len(cams))) for k in range(len(wc))]
        table, _, out_rows, max_rows, _, gt_rows = evaluate.clip_project_table(wc, pairs, cams, RF, False, surplus)
        passes.append((evaluate._to_device_bytes(table, dev), len(pairs), out_rows, max_rows, gt_rows))
    most_out, most_gt = max(p[2] for p in passes), max(p[4] for p in passes)
    x = torch.empty((most_out, 17, 3), device=dev)
    gt = torch.empty((most_gt, 17, 3), device=dev)
    outside = torch.empty(max(p[1] for p in passes), dtype=torch.int32, device=dev)
    status = torch.empty_like(outside)
    keep = {}

    def host():
        for cam in cams:
            held = []
            for c in host_clips(wc, cam):
                held.append((torch.from_numpy(evaluate.pad_clip(c.rays, pad)).to(dev), torch.from_numpy(c.gt_norm).to(dev)))
            keep["host"] = held

    def device():
        for tab, k, out_rows, max_rows, gt_rows in passes:
            evaluate.shard_project_hip(world_all, tab, k, out_rows, max_rows, gt_rows, "ray", None, x_all=x[:out_rows], gt_all=gt[:gt_rows],
                                       outside=outside[:k], status=status[:k])

    a, b = alternate([host, device], args.reps, dev, wall=True)
    for t in (a, b):
        t["per_camera_ms"] = round(t["mean_ms"] / len(cams), 4)
    if status[:passes[-1][1]].any().item():
        raise SystemExit("r3d_clips_project refused descriptors")
    # the call alone, by device events: one pass, with the ground truth and the counts (12 B read, 24 B written per point)
    tab, k, out_rows, max_rows, gt_rows = passes[0]
    (alone,) = alternate([lambda: evaluate.shard_project_hip(world_all, tab, k, out_rows, max_rows, gt_rows, "ray", None, x_all=x[:out_rows],
                                                             gt_all=gt[:gt_rows], outside=outside[:k], status=status[:k])], max(args.reps, 5), dev)
    cams_in_pass = k // len(wc)
    # (per output point 12 bytes are read - a padding row reads its edge frame again, from the caches - and 12 written; per
    # unpadded point 12 more for the ground truth)
    moved = out_rows * 17 * (12 + 12) + gt_rows * 17 * 12
    alone.update({"what": "one r3d_clips_project call: %d cameras x %d clips, %d output rows, %d ground-truth rows, J 17, ray encoding, "
                          "ground truth and counts, no mirrored copy" % (cams_in_pass, len(wc), out_rows, gt_rows),
                  "bytes_moved": moved, "gb_per_s": round(moved / alone["mean_ms"] / 1e6, 1),
                  "share_of_memory_rate": round(moved / alone["mean_ms"] / 1e6 / HBM_GBPS, 4), "memory_rate_gb_per_s": HBM_GBPS})
    return compare(a, b, {"what": "input step of the sweep, %d cameras x %d clips (%d frames), RF %d: host = NumPy projection + encoding + "
                                  "padding + per-clip uploads; device = one launch per pass of %d cameras, world poses resident"
                                  % (len(cams), len(wc), frames, RF, per_pass), "project_call_alone": alone})


def step_pass(args):
    import numpy as np
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    wc, cams = make_sweep(args.clips, args.cameras)
    frames = sum(c.world.shape[0] for c in wc)
    lengths = [types_clip(c) for c in wc]
    lifter = ab.make_lifter(lengths, dev)
    keep = {}

    def host():
        out = []
        for cam in cams:
            named, avg, _ = evaluate.evaluate_clips_batched(lifter.forward_clip, host_clips(wc, cam), RF, dev, finish=True)
            out.append((cam.name, named, avg))
        keep["host"] = out

    def device():
        keep["device"] = evaluate.evaluate_camera_sweep(lifter.forward_clip, wc, cams, RF, dev, cameras_per_pass=args.cameras_per_pass)[0]

    with torch.no_grad():
        a, b = alternate([host, device], args.reps, dev, wall=True)
    lifter.check_status(dev)
    worst = 0.0
    for (hn, hnamed, _), (dn, dnamed, _, _) in zip(keep["host"], keep["device"]):
        assert hn == dn and set(hnamed) == set(dnamed)
        worst = max(worst, max(float(np.max(np.abs(np.array(hnamed[k]) - np.array(dnamed[k])))) for k in hnamed))
    for t in (a, b):
        t["poses_per_s"] = round(frames * len(cams) / t["mean_ms"] * 1e3, 1)
        t["per_camera_ms"] = round(t["mean_ms"] / len(cams), 4)
    res = compare(a, b, {"what": "whole sweep (inputs, lift, finish, metrics, reduce), %d cameras x %d clips (%d frames), RF %d, flip off, "
                                 "no lanes, %d cameras per pass; host = the parent commit's path" % (len(cams), len(wc), frames, RF, args.cameras_per_pass),
                         "max_abs_diff_per_action_mm": worst, "outside_points": [r[3] for r in keep["device"]]})
    if not worst <= 1e-3:
        raise SystemExit("pass: the two paths' per-camera errors differ by more than 1e-3 mm: %s" % json.dumps(res))
    return res


def types_clip(c):
    """A stand-in with the `.rays.shape[0]` clips_ab_common.make_lifter reads (it prepares the batch sizes of these lengths)."""
    import types
    return types.SimpleNamespace(rays=c.world)


def main():
    ap = ab.parser(__doc__, TOOL, STEPS)
    ap.add_argument("--cameras", type=int, default=36)
    ap.add_argument("--cameras-per-pass", type=int, default=4)
    args = ap.parse_args()
    if args.step:
        return ab.run_step(TOOL, args, (step_input if args.step == "input" else step_pass)(args))
    head = ab.header(args)
    head.update({"cameras": args.cameras, "cameras_per_pass": args.cameras_per_pass,
                 "timing": "host clock, device synchronised before and after each side, sides alternating, one untimed round first"})
    return ab.run_steps(TOOL, STEPS, args, head, extra=["--cameras", str(args.cameras), "--cameras-per-pass", str(args.cameras_per_pass)])


if __name__ == "__main__":
    sys.exit(main())
