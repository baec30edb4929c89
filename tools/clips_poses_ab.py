#!/usr/bin/env python3
"""A/B of the step between a clip pass's forwards and its measurement: the per-clip torch code of evaluate_clips_batched (the tail
copy of forward_clip(out=) and, with flip, mirror_output + torch.add + mul_) against ONE r3d_clips_poses call per shard, on the
H36M-shaped synthetic set of tools/clips_metrics_ab.py (240 clips, lengths U(1000, 6000), seed 0; weights from ray3d_amd.synth).

  (a) `finish`: the finishing step alone, raw poses resident in the layout forward_clip(raw_out=) leaves - per clip, what
                evaluate_clips_batched runs behind a clip's forwards (the tail call's rows copied in; with flip
                torch.add(raw, mirror_output(raw_m), out=dst) and dst.mul_(0.5)) against evaluate.shard_poses_hip; the
                prediction buffers of both must be equal bit for bit.
  (b) `pass`:   the whole pass, evaluate_clips_batched(finish=False) - the parent commit's code, the baseline - against
                evaluate_clips_batched(finish=True) (RF 243, no lanes); the rows of both must be equal bit for bit.

Both with flip off and on.  Device-event times, 5 repetitions of each side, the two sides alternating; mean, min, max and standard
deviation are kept.  No speed threshold: the ratio and whether the two ranges overlap are recorded.
usage:  python tools/clips_poses_ab.py              every step in a fresh process of its own under its own time limit, stopping at
                                                    the first that fails, then profiles/clips_poses_ab.json is written
        python tools/clips_poses_ab.py --step S     one step (finish | pass): writes measure_out/clips_poses_ab.S.json
        --resources AFTER.log [BEFORE.log]          no GPU needed: read the compiler's resource remarks (a build log made with
                                                    -Rpass-analysis=kernel-resource-usage) of this build and, optionally, of the
                                                    parent's, and store the figures of the kernel r3d_clips_poses runs on and the
                                                    list of kernels whose figures differ in the --out file (kept if it exists)
        [--out FILE] [--clips N] [--reps R] another result file; a smaller run (rehearsals) - tools/clips_ab_common.py."""
import json
import os
import re
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_ab_common as ab
from clips_ab_common import H36M_LEFT, H36M_RIGHT, alternate, make_set, ranges_overlap, verdict

TOOL = "clips_poses_ab"
STEPS = (("finish", 300), ("pass", 560))      # (step, its time limit in seconds)
KERNEL = "r3d_k_clips_poses"                  # the kernel r3d_clips_poses launches


def compare(a, b, equal, what):
    res = {"per_clip": a, "one_call": b, "ratio_one_call_over_per_clip": round(b["mean_ms"] / a["mean_ms"], 4),
           "ranges_overlap": ranges_overlap(a, b), "bit_equal": equal, "verdict": verdict(a, b, "one call")}
    if not equal:
        raise SystemExit("%s: the results of the two paths differ: %s" % (what, json.dumps(res)))
    return res


def step_finish(n_clips, reps):
    import torch
    import ray3d_amd
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = make_set(n_clips)
    sizes_of = types.MethodType(ray3d_amd.Ray3DLifter.clip_batch_sizes, ray3d_amd.Ray3DLifter)   # (the class defaults: CLIP_CHUNK, CLIP_ROUND)
    lengths = [c.rays.shape[0] for c in clips]
    table, first, total, longest = evaluate.clip_table(clips)
    raw_first, raw_rows = evaluate.clip_raw_table(lengths, sizes_of)
    table_dev = evaluate._to_device_bytes(table, dev)
    raw_first_dev = torch.tensor(raw_first, dtype=torch.int64).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    raw = torch.randn((raw_rows, 1, 17, 3), generator=g, device=dev)
    raw_m = torch.randn((raw_rows, 1, 17, 3), generator=g, device=dev)
    perm = evaluate.mirror_permutation(17, H36M_LEFT, H36M_RIGHT)
    out = {"what": "finishing step only, raw poses resident: %d clips, %d frames, %d raw rows, J 17" % (len(clips), total, raw_rows)}
    for flip in (False, True):
        pred_a = torch.empty((total, 1, 17, 3), device=dev)
        pred_b = torch.empty((total, 1, 17, 3), device=dev)
        for k, n in enumerate(lengths):           # untimed: the calls that fit wrote straight into the clip's rows
            pred_a[first[k]:first[k] + n] = raw[raw_first[k]:raw_first[k] + n]
        tails = [n - (sum(sizes_of(n)) - sizes_of(n)[-1]) for n in lengths]     # rows of the clip the last, rounded-up call holds

        def per_clip():
            for k, n in enumerate(lengths):
                dst, src = pred_a[first[k]:first[k] + n], raw[raw_first[k]:raw_first[k] + n]
                if sum(sizes_of(n)) > n:          # forward_clip(out=): the tail call went through a scratch tensor
                    dst[n - tails[k]:] = src[n - tails[k]:]
                if flip:
                    torch.add(src, evaluate.mirror_output(raw_m[raw_first[k]:raw_first[k] + n], H36M_LEFT, H36M_RIGHT), out=dst)
                    dst.mul_(0.5)

        def one_call():
            evaluate.shard_poses_hip(raw, table_dev, raw_first_dev, len(clips), total, longest, raw_m if flip else None,
                                     perm if flip else None, pred_all=pred_b)

        a, b = alternate([per_clip, one_call], reps, dev)
        equal = bool(torch.equal(pred_a.view(torch.int32), pred_b.view(torch.int32)))
        out["flip%d" % flip] = compare(a, b, equal, "finish flip %d" % flip)
        out["flip%d" % flip]["torch_ops_per_clip"] = "tail copy" + (", clone + negation + indexed copy (mirror_output), add, mul_" if flip else "")
    return out


def step_pass(n_clips, reps):
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = make_set(n_clips)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter = ab.make_lifter(clips, dev)
    out = {"what": "whole pass (upload, lift, finish, metrics, reduce), RF 243: %d clips, %d frames, no lanes; per_clip = finish=False, "
                   "the parent commit's code" % (len(clips), frames)}
    for flip in (False, True):
        keep = {}
        kw = dict(flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)

        def per_clip():
            keep["a"] = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 243, dev, **kw)

        def one_call():
            keep["b"] = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 243, dev, finish=True, **kw)

        with torch.no_grad():
            a, b = alternate([per_clip, one_call], reps, dev)
        lifter.check_status(dev)
        equal = bool(torch.equal(keep["a"][2].view(torch.int64), keep["b"][2].view(torch.int64)))
        for t in (a, b):
            t["poses_per_s"] = round(frames / t["mean_ms"] * 1e3, 1)
        out["flip%d" % flip] = compare(a, b, equal, "pass flip %d" % flip)
        out["flip%d" % flip]["average_mm"] = {k: [float(v) for v in keep[k][1]] for k in sorted(keep)}
    return out


def read_remarks(path):
    """{kernel: {figure: value}} from a build log with -Rpass-analysis=kernel-resource-usage."""
    kernels, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: (?:[^:]*: )?\s*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels.setdefault(name, {})
            continue
        m = re.search(r"remark: (?:[^:]*: )?\s*([A-Za-z][A-Za-z /\[\]]*?): (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    return kernels


def resources(after, before):
    a = read_remarks(after)
    res = {"kernel": KERNEL, "what": "compiler resource remarks (-Rpass-analysis=kernel-resource-usage, gfx950) of the kernel "
                                     "r3d_clips_poses launches", "after": a.get(KERNEL)}
    if before:
        b = read_remarks(before)
        res["before"] = b.get(KERNEL)
        res["kernels_compared"] = len(set(a) | set(b))
        res["kernels_whose_figures_differ"] = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    return res


def main():
    ap = ab.parser(__doc__, TOOL, STEPS)
    ap.add_argument("--resources", nargs="+", metavar="LOG")
    args = ap.parse_args()
    if args.step:
        return ab.run_step(TOOL, args, (step_finish if args.step == "finish" else step_pass)(args.clips, args.reps))
    if args.resources:
        merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
        merged["kernel_resources"] = resources(args.resources[0], args.resources[1] if len(args.resources) > 1 else None)
        return ab.write_out(args.out, merged)
    return ab.run_steps(TOOL, STEPS, args, ab.header(args))


if __name__ == "__main__":
    sys.exit(main())
