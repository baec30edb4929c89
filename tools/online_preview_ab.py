#!/usr/bin/env python3
"""A/B of one tick of a live caller that also wants EARLY poses from a centred model - S cameras, one new frame of raw pixel
keypoints each; back come the final pose of the frame `lag` ticks old and, for K looks, a preview pose of the frame L ticks old -
on synthetic weights (ray3d_amd.synth), distorted synthetic cameras, the RF-243 pair (ARCHITECTURE 3,3,3,3,3, lag 121), S in
{1, 32, 256}, K in {1, 3} (looks (60,) and (0, 60, 120)):

  `history`:  what a live caller could do before r3d_streams_peek - the `history` side of tools/online_ab.py (a device-resident
              (S, RF, J, 2) pixel history rolled with torch ops every tick, forward_uv on it for the final pose) plus the back
              padding: the K * S edge-padded preview windows built from the history with one torch index op, then forward_uv on them;
  `previews`: OnlineLifter(previews=looks).step(check=False) - r3d_streams_step, the final forward, r3d_streams_peek, one forward
              over the K * S preview windows;
  `plain`:    the same build's OnlineLifter(previews=None).step(check=False): `previews` less `plain` is what a preview tick adds.

All three eager and captured into a hipGraph.  `peek_alone`: the r3d_streams_peek launch without a forward.  After RF + 2 ticks
on the same frames the sides' poses are compared (the same encoding routine and the same forwards: expected equal bit for bit; the
result is recorded, not asserted).  NOT measured here: the flip pass, `repair`, S above 256.

Timing: a side's run is TICKS ticks on a host clock with the device synchronised before it starts and before it stops; the sides
alternate, one untimed round first, REPS repetitions; the MEDIAN, min and max of ms per tick are kept.  The shader clock of the
last single-launch forward (r3d_last_clock) is recorded before and after each configuration.  No ratio is a pass condition.
usage:  python tools/online_preview_ab.py [--out FILE] [--streams 1,32,256] [--looks 1,3] [--ticks N] [--reps R]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clips_ab_common import write_out                           # noqa: E402
from online_ab import CONFIGS, J, cameras, make_lifter, timed   # noqa: E402


def looks_of(K, lag):
    return (lag // 2,) if K == 1 else tuple(round(i * (lag - 1) / (K - 1)) for i in range(K))


def one(lifter, S, looks, ticks, reps, dev):
    import torch
    import ray3d_amd
    from ray3d_amd import _capi
    rf, K = lifter.receptive_field(), len(looks)
    lag = (rf - 1) // 2
    rows, params = cameras(S, dev)
    rows_k, params_k = rows.repeat(K, 1), params.repeat(K, 1)
    gen = torch.Generator(device="cpu").manual_seed(S)
    frames = (1024.0 * torch.rand((rf + 4, S, J, 2), generator=gen)).to(dev)      # the ticks' new frames, device-resident
    at = [0]

    def new_frame():
        at[0] = (at[0] + 1) % frames.shape[0]
        return frames[at[0]]

    # ---- the history side.  h[:, RF - 1] is the newest frame c - 1; row i of the window of frame c - 1 - L is frame
    # min(c - 1 - L - (RF - 1 - lag) + i, c - 1): history row min(lag - L + i, RF - 1) (the front padding is the history's own)
    idx = torch.stack([torch.clamp(torch.arange(rf) + (lag - L), max=rf - 1) for L in looks]).reshape(-1).to(dev)      # (K * RF)
    hist = frames[0].unsqueeze(1).repeat(1, rf, 1, 1).contiguous()
    lifter.prepare([S, K * S], dev)

    def history_tick(fresh, h=hist):
        h.copy_(torch.roll(h, -1, 1))
        h[:, -1] = fresh
        final = lifter.forward_uv(h, rows, params)
        w = h.index_select(1, idx).view(S, K, rf, J, 2).transpose(0, 1).reshape(K * S, rf, J, 2)
        return final, lifter.forward_uv(w, rows_k, params_k)

    hist_c, fresh_c = hist.clone(), frames[0].clone()
    with torch.no_grad():
        history_tick(fresh_c, hist_c)                      # (the workspace exists before the capture)
        torch.cuda.synchronize(dev)
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out_c = history_tick(fresh_c, hist_c)
    torch.cuda.synchronize(dev)

    def history_captured():
        fresh_c.copy_(new_frame())
        g.replay()
        return out_c

    # ---- the streams sides: with previews, and the same build without
    def online(previews, captured):
        ol = ray3d_amd.OnlineLifter(lifter, S, encoding="ray", device=dev, previews=previews)
        ol.set_cameras(rows, params)
        if captured:
            ol.capture()
        return ol
    pv, pv_c, plain, plain_c = online(looks, False), online(looks, True), online(None, False), online(None, True)

    # ---- the same RF + 2 frames through all of them: final and preview poses (the windows are full after RF ticks)
    hist.copy_(frames[0].unsqueeze(1).expand(-1, rf, -1, -1))
    hist_c.copy_(hist)
    with torch.no_grad():
        for t in range(rf + 2):
            f = frames[t]
            a_final, a_prev = history_tick(f)
            fresh_c.copy_(f)
            g.replay()
            b_final, b_emit, b_extras = pv.step(f, check=False)
            c_final, _, c_extras = pv_c.step(f, check=False)
            d_final, _ = plain.step(f, check=False)
            plain_c.step(f, check=False)
    torch.cuda.synchronize(dev)
    assert all(int(o.status.abs().sum()) == 0 for o in (pv, pv_c, plain, plain_c)) and bool((b_emit >= 0).all())
    stack = lambda extras: torch.stack([p["poses"] for p in extras["previews"]]).reshape(K * S, J, 3)      # noqa: E731
    assert all(bool((p["frames"] == rf + 1 - p["look"]).all()) for p in b_extras["previews"])
    same = {"final_previews_vs_history": bool(torch.equal(a_final[:, 0], b_final)), "final_previews_vs_plain": bool(torch.equal(d_final, b_final)),
            "final_captured_vs_eager": bool(torch.equal(c_final, b_final)), "previews_vs_history": bool(torch.equal(a_prev[:, 0], stack(b_extras))),
            "previews_captured_vs_eager": bool(torch.equal(stack(c_extras), stack(b_extras))),
            "history_captured_vs_eager": bool(torch.equal(out_c[0], a_final) and torch.equal(out_c[1], a_prev))}
    worst = float(max((a_final[:, 0] - b_final).abs().max(), (a_prev[:, 0] - stack(b_extras)).abs().max()))

    clock0 = lifter.last_clock_ghz(dev)
    with torch.no_grad():
        res = timed([lambda: history_tick(new_frame()), history_captured, lambda: pv.step(new_frame(), check=False),
                     lambda: pv_c.step(new_frame(), check=False), lambda: plain.step(new_frame(), check=False),
                     lambda: plain_c.step(new_frame(), check=False)], ticks, reps, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def peek_alone():
            _capi.streams_peek(pv.state.data_ptr(), S, rf, lag, J, 3, looks, pv.action.data_ptr(), pv.status.data_ptr(), pv.px.data_ptr(), None,
                               None, pv.pemit.data_ptr(), pv.pstatus.data_ptr(), stream)
        (alone,) = timed([peek_alone], ticks, reps, dev)
    lifter.check_status(dev)
    for ol in (pv_c, plain_c):
        ol.release()
    del g
    torch.cuda.synchronize(dev)
    lifter.release_prepared()
    h, hc, p, pc, q, qc = res
    return {"config": "rf243", "receptive_field": rf, "lag": lag, "streams": S, "looks": list(looks), "history": h, "history_captured": hc,
            "previews": p, "previews_captured": pc, "plain": q, "plain_captured": qc, "peek_alone": alone,
            "ratio_previews_over_history": round(p["median_ms"] / h["median_ms"], 4),
            "ratio_captured_previews_over_captured_history": round(pc["median_ms"] / hc["median_ms"], 4),
            "added_ms_over_plain": round(p["median_ms"] - q["median_ms"], 4),
            "added_ms_over_plain_captured": round(pc["median_ms"] - qc["median_ms"], 4),
            "poses_equal": same, "worst_pose_difference_m": worst,
            "preview_window_bytes_rebuilt_per_tick_history": K * S * rf * J * 2 * 4,
            "shader_clock_ghz_before_after": [clock0, lifter.last_clock_ghz(dev)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_preview_ab.json"))
    ap.add_argument("--streams", default="1,32,256")
    ap.add_argument("--looks", default="1,3", help="numbers of looks K")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("online_preview_ab.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lifter = make_lifter(CONFIGS["rf243"], dev)
    lag = (lifter.receptive_field() - 1) // 2
    rows = []
    for S in (int(v) for v in args.streams.split(",")):
        for K in (int(v) for v in args.looks.split(",")):
            rows.append(one(lifter, S, looks_of(K, lag), args.ticks, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    head = {"what": "ms per tick of a live caller that wants early poses from a centred model: pixel history rolled with torch ops, the "
                    "edge-padded preview windows by a torch index op and forward_uv, against OnlineLifter(previews=).step, and against the "
                    "same build's previews=None tick; eager and captured",
            "timing": "host clock around %d ticks, device synchronised before start and stop, the sides alternating, one untimed round first, "
                      "%d repetitions: median / min / max of ms per tick" % (args.ticks, args.reps),
            "not_measured": ["the flip pass", "repair=", "S above 256"],
            "device": torch.cuda.get_device_name(dev), "rows": rows}
    return write_out(args.out, head)


if __name__ == "__main__":
    sys.exit(main())
