"""What a weight refresh costs when the parameters already live on the device: the RF-243 pos + trj pair (561 tensors), parameters
on the GPU, ``refresh_weights()`` on both networks followed by one forward of --batch windows and a synchronisation - the step a
validation pass after every epoch starts with - timed two ways in one process:

  host     set_device_weights(False): 561 tensor.to("cpu") copies, r3d_set_weight, the float64 fold and pack on the host, a device
           synchronisation and the upload (r3d_finalize; the parent commit's only path);
  device   set_device_weights(True): r3d_finalize_dev - one copy of the pointer table and two launches per network on the stream.

Wall time (host clock) from refresh_weights() to the synchronised forward, the sides alternating, best and median of --reps after a
warm-up round; the same forward without a refresh for scale; the device path's pack alone between device events.  Before anything
is timed the two pairs' outputs are compared bit for bit.  Writes profiles/weights_dev_ab.json (--out).  Needs the GPU; nothing is
asserted about the speeds."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(device_weights):
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import synth
    from ray3d_amd.spec import config_from_dicts
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    fac = ray3d_amd.Model(mc, {}, is_train=False, device_weights=device_weights)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    cfgs = {}
    for m, kind, seed in ((pos, "pos", 1), (trj, "trj", 2)):
        cfgs[kind] = config_from_dicts(mc, kind)
        ray3d_amd.load_weight(m, {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(cfgs[kind], seed=seed).items()})
        m.eval()
    return ray3d_amd.Ray3DLifter(pos, trj).eval(), cfgs["pos"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weights_dev_ab.json"))
    args = ap.parse_args()
    import torch
    from ray3d_amd import synth
    dev = torch.device("cuda:0")
    sides = {"host": build(False), "device": build(True)}
    cfg = sides["host"][1]
    x = torch.from_numpy(synth.synth_rays(args.batch, cfg, seed=3)).to(dev)
    p = torch.from_numpy(synth.synth_param(args.batch, seed=4)).to(dev)

    def refresh_and_forward(lifter):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        lifter.pos.refresh_weights()
        lifter.trj.refresh_weights()
        out = lifter(x, p)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3, out

    def forward_only(lifter):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        lifter(x, p)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3

    def pack_only(lifter):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        lifter.pos.refresh_weights()
        lifter.trj.refresh_weights()
        st = torch.cuda.current_stream(dev)
        e0.record(st)
        lifter.pos.handle(dev)
        lifter.trj.handle(dev)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with torch.no_grad():
        outs = {}
        for name, (lifter, _) in sides.items():          # warm-up round: first finalize, schedules, the clock
            refresh_and_forward(lifter)
            _, outs[name] = refresh_and_forward(lifter)
        same = bool(torch.equal(outs["host"], outs["device"]))
        if not same:
            raise SystemExit("the two paths' outputs differ: nothing timed")
        times = {"host": [], "device": []}
        fwd, pack = [], []
        for _ in range(args.reps):
            for name, (lifter, _) in sides.items():
                times[name].append(refresh_and_forward(lifter)[0])
            fwd.append(forward_only(sides["device"][0]))
            pack.append(pack_only(sides["device"][0]))
        sides["device"][0].check_status(dev)
    res = {"what": "refresh_weights() on pos and trj -> one synchronised forward, RF 243, J 17, parameters on the device; ms, host clock",
           "device": torch.cuda.get_device_name(dev), "date": datetime.date.today().isoformat(), "batch": args.batch, "reps": args.reps,
           "outputs_bit_equal": same,
           "host_path_ms": {"best": min(times["host"]), "median": statistics.median(times["host"]), "all": times["host"]},
           "device_path_ms": {"best": min(times["device"]), "median": statistics.median(times["device"]), "all": times["device"]},
           "forward_without_refresh_ms": {"best": min(fwd), "median": statistics.median(fwd)},
           "pack_both_networks_event_ms": {"best": min(pack), "median": statistics.median(pack), "all": pack},
           "host_over_device_best": min(times["host"]) / min(times["device"])}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
