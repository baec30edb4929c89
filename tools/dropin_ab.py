"""What the reference's literal seam costs through Model(...): the sequence ``pos(x, p); trj(x, p); add`` of
lib/train_val/trainer.py:337-353 at RF 243, J 17, timed three ways on the same device inputs in one process -

  separate   Model(..., fuse_pair=False): two whole-chip launches per step (the behaviour before the pair seam; the baseline) -
             timed TWICE per round, first and last, so that the spread between its two series is the noise of the session;
  fused      Model(..., fuse_pair=True): one r3d_forward_pair_split launch, the trj call served from the park;
  lifter     Ray3DLifter.forward: one r3d_forward_pair launch, the sum made in the decode kernel.

The sides alternate (--reps rounds); every timed window is --window-ms of back-to-back steps (the step count comes from a short
pilot), between device events; before the first round the pair runs for --settle-s seconds so that the shader clock has settled.
Before anything is timed the three results are compared: fused == lifter bit for bit (include/ray3d_hip.h), separate within 1e-4.
Writes profiles/dropin_ab.json (--out): ms per step, poses / s and the two ratios per batch size.  Needs the GPU; nothing is
asserted about the speeds."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def build(fuse, dev):
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import synth
    from ray3d_amd.spec import config_from_dicts
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    fac = ray3d_amd.Model(mc, {}, is_train=False, fuse_pair=fuse)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    cfgs = {}
    for m, kind, seed in ((pos, "pos", 1), (trj, "trj", 2)):
        cfgs[kind] = config_from_dicts(mc, kind)
        ray3d_amd.load_weight(m, {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(cfgs[kind], seed=seed).items()})
        m.eval()
    return fac, pos, trj, cfgs["pos"]


def timed(run, steps, dev):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.current_stream(dev))
    for _ in range(steps):
        run()
    e1.record(torch.cuda.current_stream(dev))
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def measure(B, args, dev):
    import torch
    import ray3d_amd
    from ray3d_amd import synth
    from clips_ab_common import stats
    _, spos, strj, cfg = build(False, dev)
    _, fpos, ftrj, _ = build(True, dev)
    lifter = ray3d_amd.Ray3DLifter(spos, strj).eval()
    x = torch.from_numpy(synth.synth_rays(B, cfg, seed=3)).to(dev)
    p = torch.from_numpy(synth.synth_param(B, seed=4)).to(dev)

    def separate():
        return spos(x, p) + strj(x, p)

    def fused():
        return fpos(x, p) + ftrj(x, p)

    def lift():
        return lifter(x, p)

    with torch.no_grad():
        a, b, c = separate(), fused(), lift()
        torch.cuda.synchronize(dev)
        lifter.check_status(dev)
        same = {"fused_equals_lifter_bit_for_bit": bool(torch.equal(b, c)),
                "separate_vs_fused_max_abs": float((a - b).abs().max())}
        if not same["fused_equals_lifter_bit_for_bit"] or not same["separate_vs_fused_max_abs"] <= 1e-4:
            raise SystemExit("results differ: %s" % same)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.settle_s:      # the clock settles under the load that is timed afterwards
            for _ in range(10):
                lift()
            torch.cuda.synchronize(dev)
        steps = max(10, min(2000, int(math.ceil(args.window_ms / timed(separate, 10, dev)))))
        sides = (("separate", separate), ("fused", fused), ("lifter", lift), ("separate_again", separate))
        for _, run in sides:
            timed(run, max(2, steps // 10), dev)
        series = {name: [] for name, _ in sides}
        for _ in range(args.reps):
            for name, run in sides:
                series[name].append(timed(run, steps, dev))
    res = {name: stats(v) for name, v in series.items()}
    for r in res.values():
        r["poses_per_s"] = round(B / (r["mean_ms"] * 1e-3), 1)
    base = 0.5 * (res["separate"]["mean_ms"] + res["separate_again"]["mean_ms"])
    noise = abs(res["separate"]["mean_ms"] - res["separate_again"]["mean_ms"]) / base
    return dict(res, batch=B, steps_per_window=steps, outputs=same,
                noise_between_the_two_separate_series=round(noise, 4),
                separate_over_fused=round(base / res["fused"]["mean_ms"], 4),
                fused_throughput_over_lifter=round(res["lifter"]["mean_ms"] / res["fused"]["mean_ms"], 4),
                fused_faster_than_separate_beyond_noise=bool(
                    res["fused"]["max_ms"] < min(res["separate"]["min_ms"], res["separate_again"]["min_ms"])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="256,2048")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=500.0)
    ap.add_argument("--settle-s", type=float, default=3.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropin_ab.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dropin_ab needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"what": "pos(x,p); trj(x,p); add through Model(...) at RF 243, J 17: fuse_pair off (twice) / on, and Ray3DLifter.forward",
           "timing": "device events around windows of back-to-back steps, sides alternating, %d rounds, %.0f ms windows, %.0f s of "
                     "forwards before the first round" % (args.reps, args.window_ms, args.settle_s),
           "device": torch.cuda.get_device_name(dev), "results": [measure(int(b), args, dev) for b in args.batches.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for r in out["results"]:
        print(json.dumps({k: (v["mean_ms"] if isinstance(v, dict) and "mean_ms" in v else v) for k, v in r.items()}))
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
