"""-m gpu: a forward's result does not depend on the calls before it.

Every per-form test of this suite runs on handles built for it.  Here ONE long-lived pair runs generated sequences of every
forward form, window count and option change (tests/call_history_cases.py; the generator's coverage is checked on the host,
tests/test_call_history_host.py), and every output is compared BIT FOR BIT with the same call as the only call of a fresh pair
in the same configuration - the cold reference, which is itself held to the float64 / torch-port oracle at the literal 1e-4
(conftest.check_parity) and asserted to be reproducible (two fresh pairs, same bits).  No tolerance is introduced here."""
import time

import numpy as np
import pytest
import torch

import call_history_cases as ch
from conftest import check_parity

pytestmark = pytest.mark.gpu


def _names(recs):
    return [r["kernel"] for r in recs]


@pytest.mark.parametrize("seed", ch.SEEDS)
def test_a_call_gives_the_bits_of_the_same_call_on_fresh_handles(seed):
    """One pair, one seeded sequence of forwards and mutators: every forward has the bits of its cold reference; a mismatch
    names the step, the operation and the three operations before it."""
    rig = ch.rig()
    steps = ch.sequence(seed)
    t0 = time.perf_counter()
    lifter, cfg = rig.new_lifter(ch.COLD), ch.COLD
    n_fwd = 0
    for i, op in enumerate(steps):
        if isinstance(op, ch.Mutator):
            rig.mutate(lifter, op)
            cfg = ch.after(cfg, op)
            continue
        outs = rig.run(lifter, op, cfg)
        n_fwd += 1
        rig.compare(outs, op, cfg, "seed %d step %d: %s in %s after [%s]"
                    % (seed, i, ch.describe(op), cfg, " -> ".join(ch.describe(s) for s in steps[max(i - 3, 0):i])))
    lifter.join_lanes()
    lifter.check_status(rig.dev)
    lifter.trj.check_status(rig.dev)                 # (the trajectory module's forwards alone raise their own handle's word)
    print("call history seed %d: %d operations, %d forwards, %.2f s (cold references included), %d cold results cached, unstable: %s"
          % (seed, len(steps), n_fwd, time.perf_counter() - t0, len(rig._cold), sorted(map(str, rig.unstable))))


def test_each_bound_key_field_changing_alone_rebinds():
    """Pairs of eager calls at one window count that differ in one BoundKey field (tests/call_history_cases.py, DIRECTED - and in
    the two or three fields that cannot move alone), each run as A, A, B, B, A on one pair: both the call that skips r3d_bind_f32
    and the one that binds again run on both counter banks.  Every call has the bits of its cold reference; the second A and the
    second B ran without the bind kernel, the first B and the last A with it."""
    from ray3d_amd.modules import _Workspace
    rig = ch.rig()
    lifter = rig.new_lifter(ch.COLD)
    other = _Workspace()
    for name, a, b, fields in ch.DIRECTED:
        for at, (call, binds) in enumerate(((a, None), (a, False), (b, True), (b, False), (a, True))):
            got = []
            recs = lifter.profile_call(lambda: got.append(rig.run_call(lifter, call, other)), rig.dev)
            what = "pair '%s' (key fields %s), call %d of A A B B A: %s" % (name, sorted(fields), at, ch.describe(call))
            rig.compare(got[0], call, ch.COLD, what)
            names = _names(recs)
            single = [k for k in names if k.startswith("r3d_forward")]
            if not single:
                continue                                         # (R3D_STAGED=1: one launch per level, nothing to bind)
            # the host restatement of the variant (bound_key) against the kernel that ran
            variant = ch.bound_key(call)["variant"]
            if "_b3" in single[0]:
                variant %= 2                                     # (bf16x3 handles keep the gathered first level)
            assert ("clip" in single[0]) == (variant >= 2) and ("uv" in single[0]) == (variant % 2 == 1), (what, single, variant)
            if binds is not None:
                assert ("r3d_bind_f32" in names) == binds, "%s: expected %s r3d_bind_f32, launches %s" % (what, "a" if binds else "no", names)
    lifter.check_status(rig.dev)


def test_more_than_64_sizes_evict_and_rebuild_without_changing_a_result():
    """The schedule cache keeps 64 unpinned sizes per plan kind (r3d_schedule.cpp, schedule_get): 70 window counts of the fused plan
    evict, the evicted sizes are rebuilt with the bits they had, a prepared (pinned) size under a captured graph is never the
    victim, and a released one is."""
    from ray3d_amd import synth, _capi
    rig = ch.rig()
    edges = sorted(ch_edges())                                   # (before this test creates handles: they belong to one library)
    lifter = rig.new_lifter(ch.COLD._replace(device_weights=False))     # (the host weight path: r3d_finalize)
    dev = rig.dev
    first, pinned, n_sweep, n_more = 100, 130, 70, 65
    top = first + n_sweep + n_more
    xnp, pnp = synth.synth_rays(top, rig.cp, seed=321), synth.synth_param(top, seed=322)
    x, p = torch.from_numpy(xnp).to(dev), torch.from_numpy(pnp).to(dev)
    assert all(not (first <= e < top) for e in edges), "the sweep must stay inside one plan kind: %s" % edges
    t0 = time.perf_counter()
    with torch.no_grad():
        lifter.prepare([pinned], dev)
        hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
        lifter._ws.get(_capi.workspace_bytes(hp, ht, top), dev)          # (one workspace for every size: no reallocation under the graph)
        out = torch.empty((pinned, 1, ch.J, 3), dtype=torch.float32, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(rig.side_stream):
            with torch.cuda.graph(g, stream=rig.side_stream):
                lifter._run(_capi.R3D_INPUT_RAYS, x, ch.RF, pinned, p, ch.E, out=out)

        def replay():
            out.zero_()
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(rig.side_stream):
                g.replay()
            torch.cuda.synchronize(dev)
            return out.clone()

        want_pinned = replay()
        seen = {}
        sizes = [b for b in range(first, first + n_sweep)]
        for k, b in enumerate(sizes):
            seen[b] = lifter(x[:b], p[:b]).clone()
            if (k + 1) % 16 == 0:
                assert ch.bits_equal(replay(), want_pinned), "replay of the pinned size after %d new sizes" % (k + 1)
        assert ch.bits_equal(replay(), want_pinned), "replay of the pinned size after the sweep"
        assert ch.bits_equal(seen[pinned], want_pinned), "the eager call of the pinned size against its replay"
        t_sweep = time.perf_counter() - t0
        # the first sizes were evicted (69 unpinned sizes passed through 64 places): rebuilt, the same bits
        for b in sizes[:8]:
            assert ch.bits_equal(lifter(x[:b], p[:b]), seen[b]), "%d windows, rebuilt after eviction" % b
        assert ch.bits_equal(replay(), want_pinned), "replay of the pinned size after the rebuilds"
        # three sizes over the range against the oracle (windows are independent: one evaluation of the longest prefix)
        from test_gpu_parity import _oracle_lift
        check = (sizes[0], sizes[len(sizes) // 2], sizes[-1])
        ref = _oracle_lift(((rig.cp, rig.states[0][0]), (rig.ct, rig.states[0][1])), xnp[:check[-1]], pnp[:check[-1]])
        for b in check:
            check_parity(seen[b], ref[:b], "%d windows of the sweep" % b)
        # the graph goes, the size is released: 65 further sizes make it the victim; called again it has the same bits
        g.reset()
        lifter.release_prepared()
        for b in range(first + n_sweep, top):
            lifter(x[:b], p[:b])
        assert ch.bits_equal(lifter(x[:pinned], p[:pinned]), want_pinned), "the released size, rebuilt after eviction"
        ghz = lifter.last_clock_ghz(dev)
        assert np.isfinite(ghz) and 0.0 <= ghz < 3.0, ghz              # (0: a level-by-level forward; MI355X: 2.4 GHz maximum)
    lifter.check_status(dev)
    print("schedule-cache eviction: %d + 8 + %d + 1 schedule builds at %d..%d windows, sweep %.2f s, whole test %.2f s"
          % (n_sweep, n_more, first, top - 1, t_sweep, time.perf_counter() - t0))


def ch_edges():
    from conftest import hooks_library
    from ray3d_amd import _capi
    try:
        hooks_library()
        return _capi.debug_plan_kind_edges()
    finally:
        _capi.use_hooks(False)
