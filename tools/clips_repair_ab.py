#!/usr/bin/env python3
"""Measurements of r3d_clips_repair on the H36M-shaped synthetic set of the other clip A/B tools (240 clips, lengths U(1000, 6000),
seed 0, raw pixels of four distorted cameras, RF 243, flip on; weights from ray3d_amd.synth):

  1. NO COST WHEN OFF.  `off`: wall time of evaluate_clips_batched(encode="ray", flip=True) WITHOUT repair=; `live`: one tick of
     tools/online_ab.py's smallest (RF 9, 1 stream) and largest (RF 243, 1 024 streams) configuration - the live calls' kernels
     come from the same file, r3d_k_elementwise.hip.  With --parent DIR (a checkout of the parent commit, built on the same box) both steps run in
     DIR as well, the two trees alternating, ROUNDS times each: this tree's means must lie inside the range the parent's own
     repetitions span in the same session.
  2. COST WHEN ON.  `on`: device-event time of the ONE r3d_clips_repair launch on the shard at 0 %, 1 % and 10 % dropped points
     (NaN runs of 1 - 10 frames, max_gap 10; the buffers restored before every launch, outside the timing), beside the shard's
     r3d_clips_encode launch and the whole pass with repair=10.  Recorded, not gated.
  3. AGAINST THE HOST ALTERNATIVE.  What a user has without the call: download x_all, the rule in vectorised NumPy, mirror, upload.
     Its wall time is measured on the same buffers (and its bits compared with the device's) and added to the pass without repair.
  Pathological pattern: one clip of R3D_REPAIR_MAX_ROWS rows whose joints are observed once and then missing for 65 535 rows,
  max_gap 10, against a gap-free clip of the same length: a per-point scan would show as a launch time far above the gap-free one.

usage:  python tools/clips_repair_ab.py [--parent DIR] [--rounds N]   every step in a fresh process under its own time limit, then
                                                                     profiles/clips_repair_ab.json is written (--out: elsewhere)
        python tools/clips_repair_ab.py --step off|live|on [--tree DIR]   one step (in the tree DIR): measure_out/clips_repair_ab.<step>.json
        [--clips N] [--reps R] shrink the run (rehearsals) - tools/clips_ab_common.py."""
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_ab_common as ab

TOOL = "clips_repair_ab"
LIMITS = {"off": 420, "live": 420, "on": 600}
MAX_GAP = 10


def drop_points(clips, fraction, seed=1):
    """Copies of the pixel clips with about `fraction` of their keypoints NaN, in runs of 1 - 10 frames."""
    import numpy as np
    from ray3d_amd import evaluate
    rng = np.random.default_rng(seed)
    out = []
    for c in clips:
        px = c.rays.copy()
        n, J = px.shape[:2]
        for _ in range(int(round(fraction * n * J / 5.5))):
            run = int(rng.integers(1, 11))
            start = int(rng.integers(0, max(n - run, 1)))
            px[start:start + run, int(rng.integers(0, J))] = np.nan
        out.append(evaluate.Clip(c.camera, px, c.gt_norm, c.action, c.clip_id))
    return out


def host_rule(x, max_gap):
    """The rule of include/ray3d_hip.h on one clip's rows (R, J, F) float32, vectorised NumPy -> the repaired rows."""
    import numpy as np
    R, J, _ = x.shape
    obs = np.isfinite(x).all(-1)
    idx = np.arange(R)[:, None]
    prev = np.maximum.accumulate(np.where(obs, idx, -1), axis=0)
    nxt = np.minimum.accumulate(np.where(obs, idx, R)[::-1], axis=0)[::-1]
    miss, has_p, has_q = ~obs, prev >= 0, nxt < R
    g = nxt - prev - 1
    interp = miss & has_p & has_q & (g <= max_gap)
    jj = np.arange(J)[None, :]
    a, e = x[np.clip(prev, 0, R - 1), jj], x[np.clip(nxt, 0, R - 1), jj]
    with np.errstate(all="ignore"):
        t = ((idx - prev) / (g + 1.0))[..., None]
        val = (a.astype(np.float64) + (e.astype(np.float64) - a.astype(np.float64)) * t).astype(np.float32)
    out = x.copy()
    out[interp] = val[interp]
    out[miss & has_p & ~interp] = a[miss & has_p & ~interp]
    out[miss & ~has_p & has_q] = e[miss & ~has_p & has_q]
    out[miss & ~has_p & ~has_q] = np.nan
    return out


def step_off(args):
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = ab.make_set(args.clips, pixels=True)
    lifter = ab.make_lifter(clips, dev)
    kw = dict(flip=True, kps_left=ab.H36M_LEFT, kps_right=ab.H36M_RIGHT, encode="ray")
    with torch.no_grad():
        (a,) = ab.alternate([lambda: evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 243, dev, **kw)], args.reps, dev, wall=True)
    lifter.check_status(dev)
    return {"what": "evaluate_clips_batched(encode='ray', flip=True) without repair=, wall ms per pass", "tree": "parent" if args.tree else "this", "pass": a}


def step_live(args):
    """tools/online_ab.py of the tree, its smallest and its largest configuration."""
    tree = args.tree or ab.ROOT
    rows = []
    for config, S in (("rf9", 1), ("rf243", 1024)):
        out = os.path.join(ab.PART_DIR, "%s.online.%s.json" % (TOOL, config))
        os.makedirs(ab.PART_DIR, exist_ok=True)
        rc = subprocess.run(["timeout", "-k", "10", "200", sys.executable, os.path.join(tree, "tools", "online_ab.py"), "--out", out, "--streams", str(S),
                             "--configs", config, "--ticks", "50", "--reps", str(args.reps)], stdout=subprocess.DEVNULL).returncode
        if rc != 0:
            raise SystemExit("online_ab.py of %s ended with status %d" % (tree, rc))
        r = json.load(open(out))["rows"][0]
        rows.append({k: r[k] for k in ("config", "streams", "streams_step", "streams_step_captured", "step_alone")})
    return {"what": "tools/online_ab.py: ms per live tick, smallest and largest configuration", "tree": "parent" if args.tree else "this", "rows": rows}


def step_on(args):
    import numpy as np
    import torch
    from ray3d_amd import _capi, evaluate
    dev = torch.device("cuda", 0)
    base = ab.make_set(args.clips, pixels=True)
    lifter = ab.make_lifter(base, dev)
    perm = evaluate.mirror_permutation(17, ab.H36M_LEFT, ab.H36M_RIGHT)
    kw = dict(flip=True, kps_left=ab.H36M_LEFT, kps_right=ab.H36M_RIGHT, encode="ray")
    sizes_of = lifter.clip_batch_sizes
    res = {"what": "the one r3d_clips_repair launch (device events), the shard's r3d_clips_encode launch, the whole pass (wall)",
           "max_gap": MAX_GAP, "repetitions": args.reps, "fractions": []}

    def launch_ms(run, restore):
        ms = []
        for k in range(args.reps + 1):
            restore()
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(dev))
            run()
            e1.record(torch.cuda.current_stream(dev))
            e1.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        return ab.stats(ms)

    with torch.no_grad():
        for fraction in (0.0, 0.01, 0.1):
            clips = drop_points(base, fraction) if fraction else base
            itable, first, out_rows, max_rows = evaluate.clip_input_table(clips, 243, False, lambda n: sum(sizes_of(n)) - n)
            tab = evaluate._to_device_bytes(itable, dev)
            px_all = torch.from_numpy(np.concatenate([c.rays for c in clips])).to(dev)
            x_all, xm_all, _ = evaluate.shard_encode_hip(px_all, tab, len(clips), out_rows, max_rows, "ray", perm)
            x0, xm0 = x_all.clone(), xm_all.clone()
            state = torch.empty((out_rows, 17), dtype=torch.uint8, device=dev)
            stats = torch.empty((len(clips), 17, 4), dtype=torch.int32, device=dev)
            status = torch.empty((len(clips),), dtype=torch.int32, device=dev)

            def restore():
                x_all.copy_(x0), xm_all.copy_(xm0)
            enc = launch_ms(lambda: evaluate.shard_encode_hip(px_all, tab, len(clips), out_rows, max_rows, "ray", perm, x_all, xm_all, status),
                            lambda: None)
            rep = launch_ms(lambda: evaluate.shard_repair_hip(x_all, tab, len(clips), out_rows, max_rows, MAX_GAP, xm_all, perm, state=state,
                                                              stats=stats, status=status), restore)
            counts = stats.sum(dim=(0, 1)).tolist()
            # the host alternative on the same buffers: download, the NumPy rule clip by clip, mirror, upload
            restore()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            hx = x_all.cpu().numpy()
            for d in itable:
                at, R = int(d["out_first"]), int(d["pad_front"] + d["n_frames"] + d["pad_back"])
                hx[at:at + R] = host_rule(hx[at:at + R], MAX_GAP)
            hxm = hx[:, perm].copy()
            hxm[..., 0] = -hxm[..., 0]
            ux, uxm = torch.from_numpy(hx).to(dev), torch.from_numpy(hxm).to(dev)
            torch.cuda.synchronize(dev)
            host_ms = (time.perf_counter() - t0) * 1e3
            evaluate.shard_repair_hip(x_all, tab, len(clips), out_rows, max_rows, MAX_GAP, xm_all, perm, state=state, stats=stats, status=status)
            same = bool(torch.equal(ux.view(torch.int32), x_all.view(torch.int32)) and torch.equal(uxm.view(torch.int32), xm_all.view(torch.int32)))
            off, on = ab.alternate([lambda: evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 243, dev, **kw),
                                    lambda: evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 243, dev, repair=MAX_GAP, **kw)],
                                   args.reps, dev, wall=True)
            res["fractions"].append({
                "dropped_fraction_asked": fraction, "points": out_rows * 17, "rows": out_rows,
                "points_interpolated_held_backfilled_never": counts, "encode_launch": enc, "repair_launch": rep,
                "pass_without_repair": off, "pass_with_repair": on,
                "host_alternative_step_ms": round(host_ms, 2), "host_alternative_pass_ms": round(off["mean_ms"] + host_ms, 2),
                "host_rule_bits_equal_device": same})
        # the pathological pattern against a gap-free clip of the same length
        R = _capi.REPAIR_MAX_ROWS
        table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
        table[0]["n_frames"] = R
        tab = evaluate._to_device_bytes(table, dev)
        full = torch.randn((R, 17, 3), device=dev)
        once = full.clone()
        once[1:] = float("nan")
        x = torch.empty_like(full)
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        rows = {}
        for name, src in (("gap_free", full), ("observed_once_then_65535_missing", once)):
            rows[name] = launch_ms(lambda: evaluate.shard_repair_hip(x, tab, 1, R, R, MAX_GAP, status=status), lambda: x.copy_(src))
        res["pathological"] = dict(rows, rows_of_the_clip=R, joints=17,
                                   ratio=round(rows["observed_once_then_65535_missing"]["mean_ms"] / rows["gap_free"]["mean_ms"], 3))
    lifter.check_status(dev)
    return res


def run(step, args, tree=None):
    """One step as a fresh process of this tool under its time limit -> its result."""
    cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--clips", str(args.clips),
           "--reps", str(args.reps)] + (["--tree", tree] if tree else [])
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL).returncode
    if rc != 0:
        raise SystemExit("step %s%s ended with status %d: stopping, nothing written" % (step, " in " + tree if tree else "", rc))
    return json.load(open(os.path.join(ab.PART_DIR, "%s.%s.json" % (TOOL, step))))


def inside(mine, theirs):
    """This tree's means against the range the parent's repetitions span."""
    lo, hi = min(t["min_ms"] for t in theirs), max(t["max_ms"] for t in theirs)
    mean = sum(m.get("mean_ms", m.get("median_ms")) for m in mine) / len(mine)
    return {"parent_range_ms": [lo, hi], "this_mean_ms": round(mean, 4), "this_mean_not_above_parent_range": mean <= hi,
            "this_mean_inside_parent_range": lo <= mean <= hi}


def main():
    ap = ab.parser(__doc__, TOOL, tuple(LIMITS.items()))
    ap.add_argument("--tree", help="with --step: the checkout whose ray3d_amd and tools are measured (default: this one)")
    ap.add_argument("--parent", help="a checkout of the parent commit, built on this box: `off` and `live` run there as well")
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if args.step:
        if args.tree:
            sys.path.insert(0, os.path.abspath(args.tree))      # (in front of this tree: its ray3d_amd is the one imported)
        return ab.run_step(TOOL, args, {"off": step_off, "live": step_live, "on": step_on}[args.step](args))
    merged = {"set": "%d clips, lengths U(1000, 6000), seed 0, raw pixels of four distorted cameras, J 17, RF 243, flip on" % args.clips,
              "repetitions": args.reps, "rounds": args.rounds, "off": {"this": [], "parent": []}, "live": {"this": [], "parent": []}}
    for _ in range(args.rounds):                                    # the two trees alternate
        for side, tree in (("parent", args.parent), ("this", None)):
            if side == "parent" and not args.parent:
                continue
            merged["off"][side].append(run("off", args, tree))
            merged["live"][side].append(run("live", args, tree))
    if args.parent:
        merged["off"]["verdict"] = inside([r["pass"] for r in merged["off"]["this"]], [r["pass"] for r in merged["off"]["parent"]])
        merged["live"]["verdict"] = {
            "%s S %d %s" % (merged["live"]["this"][0]["rows"][k]["config"], merged["live"]["this"][0]["rows"][k]["streams"], key):
                inside([r["rows"][k][key] for r in merged["live"]["this"]], [r["rows"][k][key] for r in merged["live"]["parent"]])
            for k in range(2) for key in ("streams_step", "step_alone")}
    merged["on"] = run("on", args)
    return ab.write_out(args.out, merged)


if __name__ == "__main__":
    sys.exit(main())
