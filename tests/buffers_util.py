"""Guard-band helper of tests/test_gpu_buffers.py: every device buffer of one library call is carved, exact-sized, out of ONE
allocation that is filled with a 32-bit pattern, with at least 1 MiB of pattern in front of, behind and between the carved
regions.  A read past a buffer's end then returns the pattern (a NaN pattern poisons the result), a write past it lands in
a guard - it is found by check() as data, and never reaches memory the process does not own."""
import numpy as np
import torch

GUARD = 1 << 20                     # bytes of pattern in front of, behind and between carved regions (at least)

ZEROS, NANS, INF, ACT_SENTINEL = 0x00000000, 0xFFFFFFFF, 0x7F800000, 0x7FC5A1E7    # (ACT_SENTINEL: r3d_tiles.hpp)
PATTERNS = (ZEROS, NANS, INF, ACT_SENTINEL)
PATTERN_IDS = ("zeros", "nan", "inf", "act-sentinel")


def _i32(pattern):
    return int(np.array([pattern & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)[0])


def fill_pattern(view, pattern):
    """Fill a uint8 view that starts on a 4-byte boundary of its allocation with the little-endian bytes of `pattern`."""
    assert view.dtype == torch.uint8 and view.dim() == 1 and view.data_ptr() % 4 == 0
    n4 = view.numel() // 4 * 4
    if n4:
        view[:n4].view(torch.int32).fill_(_i32(pattern))
    for k in range(n4, view.numel()):
        view[k] = (pattern >> (8 * (k - n4))) & 0xFF


class DirtyGuard(AssertionError):
    pass


class Arena:
    """One torch.uint8 device allocation of `capacity` bytes filled with `pattern`; carve() hands out exact-sized views."""

    def __init__(self, device, pattern, capacity):
        self.device = torch.device(device)
        self.buf = torch.empty(int(capacity), dtype=torch.uint8, device=self.device)
        self.regions = []           # (name, start, end) in carve order
        self.cursor = 0
        self.refill(pattern)

    @staticmethod
    def capacity_for(sizes, align=256):
        """Bytes that hold regions of these sizes (each with its guard in front, alignment and skew slack) and the last guard."""
        return sum(int(s) + GUARD + 2 * max(align, 256) for s in sizes) + GUARD + 256

    def refill(self, pattern):
        """The whole allocation - guards AND carved regions - back to `pattern` (the regions stay carved)."""
        self.pattern = pattern & 0xFFFFFFFF
        fill_pattern(self.buf, self.pattern)

    def carve(self, nbytes, align=256, skew=0, name=None):
        """A view of exactly `nbytes` bytes that starts `skew` bytes behind an `align`-aligned address, >= GUARD behind the last region."""
        assert skew % 4 == 0 and align % 4 == 0 and nbytes >= 0
        base = self.buf.data_ptr()                     # (aligned addresses, not aligned offsets)
        start = -(-(base + self.cursor + GUARD) // align) * align - base + skew
        end = start + int(nbytes)
        assert end + GUARD <= self.buf.numel(), "arena too small: capacity_for() the sizes first"
        self.regions.append((name or "region%d" % len(self.regions), start, end))
        self.cursor = end
        view = self.buf[start:end]
        assert (view.data_ptr() - skew) % align == 0 and view.numel() == nbytes
        return view

    def put(self, array, align=256, skew=0, name=None):
        """carve() a region of exactly array.nbytes; -> a function that (re)writes the array into it and returns the typed view."""
        array = np.ascontiguousarray(array)
        raw = self.carve(array.nbytes, align, skew, name)
        host = torch.from_numpy(array.reshape(-1).view(np.uint8).copy())
        dtype = torch.from_numpy(array.reshape(-1)[:0].copy()).dtype

        def write():
            raw.copy_(host)
            return raw.view(dtype).view(array.shape)
        return write

    def _dirty(self, a, b):
        """(first, last) dirty absolute byte offset in [a, b), or None."""
        if b <= a:
            return None
        got = self.buf[a:b]
        a4, b4 = -(-a // 4) * 4, b // 4 * 4
        if a4 >= b4:
            cand = list(range(a, b))
        else:
            ne = got[a4 - a:b4 - a].view(torch.int32) != _i32(self.pattern)
            edge = list(range(a, a4)) + list(range(b4, b))
            if not bool(ne.any()) and not edge:
                return None
            idx = ne.nonzero().flatten()
            words = [int(idx[0]), int(idx[-1])] if idx.numel() else []
            cand = edge + [a4 + 4 * w + k for w in words for k in range(4)]
        host = self.buf.new_tensor(cand, dtype=torch.long)
        vals = self.buf[host].cpu().tolist()
        bad = sorted(o for o, v in zip(cand, vals) if v != (self.pattern >> (8 * (o % 4))) & 0xFF)
        return (bad[0], bad[-1]) if bad else None

    def check(self):
        """Every byte outside the carved regions still holds the pattern - or DirtyGuard names the region the dirty bytes lie
        behind (offsets relative to that region's END: +0 is the first byte past it) or, in the first guard, in front of."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        problems = []
        edges = [(None, 0, 0)] + self.regions + [(None, self.buf.numel(), self.buf.numel())]
        for (pname, _, pend), (nname, nstart, _) in zip(edges[:-1], edges[1:]):
            d = self._dirty(pend, nstart)
            if d is None:
                continue
            if pname is not None:
                problems.append("guard behind '%s': dirty bytes from +%d to +%d past its end (pattern 0x%08X)%s"
                                % (pname, d[0] - pend, d[1] - pend, self.pattern,
                                   "" if nname is None else "; that is -%d to -%d in front of '%s'" % (nstart - d[0], nstart - d[1], nname)))
            else:
                problems.append("guard in front of '%s': dirty bytes from -%d to -%d before its start (pattern 0x%08X)"
                                % (nname, nstart - d[0], nstart - d[1], self.pattern))
        if problems:
            raise DirtyGuard("; ".join(problems))


class ExactWorkspace:
    """What Ray3DLifter._run(..., workspace=) and LiftModule._ws expect (`.get(nbytes, device)`): hands the library a carved
    view of exactly the number of bytes it asked for."""

    def __init__(self, arena, name="workspace"):
        self.arena, self.name, self.view = arena, name, None

    def get(self, nbytes, device):
        if self.view is None:
            self.view = self.arena.carve(int(nbytes), 256, 0, self.name)
        assert self.view.numel() == int(nbytes), (self.view.numel(), nbytes)
        return self.view
