"""The generator of the call-history tests (tests/call_history_cases.py), checked on the host: conditions on the INPUTS of
tests/test_gpu_call_history.py, so that a later edit cannot shrink what those tests cover without a test noticing."""
import itertools

import call_history_cases as ch
from conftest import hooks_library


def _forwards(steps):
    return [s for s in steps if isinstance(s, ch.Forward)]


def test_a_seed_gives_the_same_sequence_twice():
    for seed in ch.SEEDS:
        a, b = ch.sequence(seed), ch.sequence(seed)
        assert a == b and len(a) > 20
        assert all(isinstance(s, (ch.Forward, ch.Mutator)) for s in a)
        assert all(s in ch.MUTATORS for s in a if isinstance(s, ch.Mutator))
        hash(tuple(a))                                            # descriptors are hashable ...
        assert all(ch.describe(s) for s in a)                     # ... and printable
    assert len({tuple(ch.sequence(s)) for s in ch.SEEDS}) == len(ch.SEEDS)


def test_sequences_stay_short():
    """A seed's test builds two fresh pairs per distinct call: the sequences stay near a hundred operations."""
    for seed in ch.SEEDS:
        assert len(ch.sequence(seed)) <= 160, (seed, len(ch.sequence(seed)))


def test_every_ordered_pair_of_forward_forms_occurs():
    seen = set()
    for seed in ch.SEEDS:
        steps = ch.sequence(seed)
        for a, b in zip(steps, steps[1:]):
            if isinstance(a, ch.Forward) and isinstance(b, ch.Forward):
                seen.add((a.form, b.form))
    missing = set(itertools.product(ch.FORMS, ch.FORMS)) - seen
    assert not missing, sorted(missing)


def test_every_mutator_is_followed_by_every_forward_form():
    seen = set()
    for seed in ch.SEEDS:
        steps = ch.sequence(seed)
        for a, b in zip(steps, steps[1:]):
            if isinstance(a, ch.Mutator) and isinstance(b, ch.Forward):
                seen.add((a, b.form))
    missing = set(itertools.product(ch.MUTATORS, ch.FORMS)) - seen
    assert not missing, sorted(missing, key=str)
    assert {m.name for m in ch.MUTATORS} == {"set_staged", "refresh_weights", "load_state_dict", "set_device_weights", "prepare",
                                              "release_prepared", "set_lanes"}


def test_every_window_count_occurs_with_every_form():
    seen = {(f.form, f.B) for seed in ch.SEEDS for f in _forwards(ch.sequence(seed))}
    want = {(form, B) for form in ch.FORMS for B in ch.WINDOW_COUNTS if ch.accepts(form, B)}
    assert len(want) == len(ch.FORMS) * len(ch.WINDOW_COUNTS)
    assert not want - seen, sorted(want - seen)
    assert not seen - want


def test_sequences_repeat_a_call_at_once_and_come_back_to_earlier_ones():
    """The two ways a schedule's bound state is met again: the same call twice in a row (the bind is skipped), and the same call
    after other operations - mutators among them - ran in between."""
    for seed in ch.SEEDS:
        steps = ch.sequence(seed)
        assert any(a == b for a, b in zip(steps, steps[1:]) if isinstance(a, ch.Forward)), seed
        back = 0
        for i, s in enumerate(steps):
            if isinstance(s, ch.Forward) and s in steps[:max(i - 1, 0)]:
                between = steps[steps.index(s) + 1:i]
                back += any(isinstance(b, ch.Mutator) for b in between)
        assert back >= 2, seed


def test_every_option_is_on_and_off_under_forwards_and_every_seed_ends_with_options_off():
    configs = set()
    for seed in ch.SEEDS:
        cfg = ch.COLD
        for s in ch.sequence(seed):
            if isinstance(s, ch.Mutator):
                cfg = ch.after(cfg, s)
            else:
                configs.add(cfg)
        assert cfg == ch.COLD, (seed, cfg)
    for field in ch.Config._fields:
        assert len({getattr(c, field) for c in configs}) == 2, field


def test_the_window_counts_straddle_every_plan_kind_edge_the_library_reports():
    """The plan kind switches behind r3d_debug_plan_kind_edges' counts (hooks library, read at run time): every edge below the
    pool's 150 windows has both of its sides in the list; so have the limits of the gemv tiles (4) and of the polled banks (16)."""
    from ray3d_amd import _capi
    hooks_library()
    edges = _capi.debug_plan_kind_edges()
    assert edges == sorted(edges) and len(edges) >= 2
    inside = [e for e in edges if e < ch.BMAX]
    assert len(inside) >= 2, edges
    for e in inside + [4, 16]:
        assert e in ch.WINDOW_COUNTS and e + 1 in ch.WINDOW_COUNTS, (e, edges)
    assert ch.BMAX in ch.WINDOW_COUNTS and 1 in ch.WINDOW_COUNTS and 32 in ch.WINDOW_COUNTS


def test_every_view_fits_the_buffer_it_is_taken_from():
    calls = {ch.call_of(f) for seed in ch.SEEDS for f in _forwards(ch.sequence(seed))}
    calls |= {c for _, a, b, _ in ch.DIRECTED for c in (a, b)}
    # what the oracle evaluates: the same call at the pool's full window count
    calls |= {c._replace(B=ch.BMAX) for c in calls}
    assert len(calls) > 100
    for c in calls:
        for name, (need, have) in ch.extents(c).items():
            assert name in ch.POOL and 0 < need <= have, (c, name, need, have)
    # the largest index read, spelt out for one call of each layout
    assert ch.extents(ch.call_of(ch.Forward("clip", 150, 1, 0, 0)))["x1"] == ((149 + 27) * 51, 150 * 27 * 51)
    assert ch.extents(ch.call_of(ch.Forward("uv_rows", 97, 0, 1, 0))) == {"x0": (97 * 27 * 34, 150 * 27 * 51), "p1": (97 * 2, 300), "c1": (97 * 8, 1200)}
    assert ch.extents(ch.call_of(ch.Forward("uv_bcast", 5, 0, 0, 0))) == {"x0": (5 * 27 * 34, 150 * 27 * 51), "pb": (2, 2), "c0": (8, 1200)}
    # same-sized alternatives: a stale table reads a wrong but valid address
    for a, b in (("x0", "x1"), ("x0", "xn"), ("p0", "p1"), ("c0", "c1"), ("d0", "d1")):
        assert ch.POOL[a] == ch.POOL[b]


def test_the_directed_list_changes_the_key_fields_it_names_and_no_other():
    covered = set()
    for name, a, b, fields in ch.DIRECTED:
        assert a.B == b.B == ch.DIRECTED_B, name                  # one schedule: the two calls meet each other's bound table
        assert ch.key_diff(a, b) == set(fields), (name, ch.key_diff(a, b))
        assert set(fields) <= set(ch.KEY_FIELDS)
        covered |= set(fields)
    assert covered == set(ch.KEY_FIELDS), set(ch.KEY_FIELDS) - covered
    # the fields that CAN change alone at a fixed window count each have a pair of their own
    alone = {next(iter(f)) for _, _, _, f in ch.DIRECTED if len(f) == 1}
    assert alone == {"x", "param", "param_stride", "cam", "cam_stride", "workspace"}
    # ... and the rest cannot: frames = (B - 1) * stride + RF ties enc_ws to enc_bytes, the floats per frame tie the variant to them
    for a, b in itertools.combinations({c for _, x, y, _ in ch.DIRECTED for c in (x, y)}, 2):
        d = ch.key_diff(a, b)
        assert d not in ({"enc_ws"}, {"enc_bytes"}, {"variant"}), (a, b)
    assert [n for n, _, _, _ in ch.DIRECTED] == ["x", "param", "param_stride", "cam", "cam_stride", "window_stride", "variant-rays-uv",
                                                 "variant-batch-clip", "workspace"]
    assert {ch.bound_key(a)["variant"] for _, a, b, _ in ch.DIRECTED} | {ch.bound_key(b)["variant"] for _, a, b, _ in ch.DIRECTED} == {0, 1, 2}
