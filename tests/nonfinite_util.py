"""Shared helper of tests/test_nonfinite_host.py and tests/test_gpu_nonfinite.py: non-finite input elements as bit patterns,
where to put them, and the three assertions every such call is held to (the reference's behaviour, pinned on the CPU by
tests/test_nonfinite_host.py): every output of a window that reads a non-finite element is non-finite, every other window has
the bits of the same call on finite input, and those windows are within the literal 1e-4 of the torch port."""
import numpy as np

from conftest import check_parity

ACT_SENTINEL = 0x7FC5A1E7            # r3d_tiles.hpp: "not there yet" in the activation banks of calls of up to 16 windows
# name -> float32 bits
VALUES = {"nan": 0x7FC00000, "sentinel": ACT_SENTINEL, "neg-sentinel": 0xFFC5A1E7, "snan": 0x7FA00000,
          "+inf": 0x7F800000, "-inf": 0xFF800000}


def current_frame(rf, F):
    """rie.py:290 (quirk Q1): the frame GlobalInfo reads and the temporal difference subtracts."""
    return rf // F


def positions(rf, J, F):
    """(frame, joint, feature): the first element, the one both folded differences subtract, the last element."""
    return [(0, 0, 0), (current_frame(rf, F), 0, 0), (rf - 1, J - 1, F - 1)]


def windows_to_poison(B):
    """The first window, one in the middle, the last one (the last valid row of a partial tile): at most 3, at B = 1 the one."""
    return sorted({0, B // 2, B - 1})


def put_bits(arr, index, bits):
    """arr[index] = the float32 with exactly these bits (a signalling NaN or a payload survives: no float passes through)."""
    assert arr.dtype == np.float32 and arr.flags["C_CONTIGUOUS"] and arr.flags["WRITEABLE"]
    arr.view(np.uint32)[index] = np.uint32(bits)
    return arr


def poisoned_copy(x, elements, bits):
    """A copy of x (B, RF, J, F) - or any float32 array - with `bits` at every index tuple of `elements`."""
    out = np.array(x, dtype=np.float32, copy=True, order="C")
    for idx in elements:
        put_bits(out, tuple(idx), bits)
    return out


def rotations(B, rf, J, F):
    """Three element sets per call size: window k of windows_to_poison(B) gets position (k + r) % 3 - over r = 0, 1, 2 every
    poisoned window meets every position.  -> [(rows, [(window, frame, joint, feature), ...])]."""
    rows, pos = windows_to_poison(B), positions(rf, J, F)
    return [(rows, [(w,) + pos[(k + r) % 3] for k, w in enumerate(rows)]) for r in range(3)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def check_poisoned(got, got_clean, ref_clean, poisoned_rows, label=""):
    """got: the outputs (B, ...) of a call with non-finite input; got_clean: the same call (same B, same handle) with each bad
    element replaced by a finite value; ref_clean: the torch port on that finite input; poisoned_rows: the windows that read
    a non-finite element.
      * rows in poisoned_rows hold no finite element,
      * every other row is bit-identical to got_clean (none is left out),
      * those rows pass check_parity against ref_clean at the literal 1e-4."""
    got, got_clean, ref_clean = _np(got), _np(got_clean), _np(ref_clean)
    assert got.shape == got_clean.shape == ref_clean.shape, (label, got.shape, got_clean.shape, ref_clean.shape)
    B = got.shape[0]
    bad = np.zeros(B, dtype=bool)
    bad[list(poisoned_rows)] = True
    assert bad.any(), label
    g = got.reshape(B, -1)
    finite_in_bad = np.isfinite(g[bad])
    assert not finite_in_bad.any(), "%s: %d finite output(s) in poisoned window(s) %s" % (
        label, int(finite_in_bad.sum()), np.flatnonzero(bad)[finite_in_bad.any(axis=1)].tolist())
    clean = ~bad
    if clean.any():
        gc = got_clean.reshape(B, -1)
        differs = (g[clean].view(np.uint32) != gc[clean].view(np.uint32)).any(axis=1)
        assert not differs.any(), "%s: clean window(s) %s differ from the call on finite input" % (
            label, np.flatnonzero(clean)[differs].tolist())
        check_parity(got[clean], ref_clean[clean], label)
