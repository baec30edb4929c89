"""The guard-band helper of tests/test_gpu_buffers.py on host memory: what it hands out and what check() finds."""
import numpy as np
import pytest
import torch

from buffers_util import GUARD, PATTERNS, Arena, DirtyGuard, ExactWorkspace


@pytest.mark.parametrize("pattern", PATTERNS)
def test_carved_regions_are_exact_aligned_and_a_megabyte_apart(pattern):
    sizes = [12, 4 * 37 * 2, 1000, 7]
    a = Arena("cpu", pattern, Arena.capacity_for(sizes, align=4096))
    views = [a.carve(sizes[0], name="a"), a.carve(sizes[1], skew=4, name="b"), a.carve(sizes[2], align=4096, name="c"), a.carve(sizes[3], name="d")]
    for v, n in zip(views, sizes):
        assert v.numel() == n and v.dtype == torch.uint8
    assert views[0].data_ptr() % 256 == 0 and views[1].data_ptr() % 256 == 4 and views[2].data_ptr() % 4096 == 0
    base = a.buf.data_ptr()
    assert views[0].data_ptr() - base >= GUARD
    for u, v in zip(views[:-1], views[1:]):
        assert v.data_ptr() - (u.data_ptr() + u.numel()) >= GUARD
    assert base + a.buf.numel() - (views[-1].data_ptr() + views[-1].numel()) >= GUARD
    want = np.frombuffer(np.uint32(pattern).tobytes(), dtype=np.uint8)
    assert np.array_equal(a.buf[:8].numpy(), np.tile(want, 2))
    for v in views:                                  # writing INSIDE the regions is nobody's business
        v.fill_(0x5A)
    a.check()
    a.refill(pattern)
    assert int(views[2][5]) == int(want[(views[2].data_ptr() - base + 5) % 4])
    a.check()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_check_names_the_region_and_the_dirty_offsets(pattern):
    a = Arena("cpu", pattern, Arena.capacity_for([64, 30]))
    x = a.carve(64, name="x_dev")
    o = a.carve(30, name="out_dev")                  # (ends off a word boundary)
    xs, oe = x.data_ptr() - a.buf.data_ptr(), o.data_ptr() - a.buf.data_ptr() + 30
    a.buf[xs + 64 + 5] ^= 0x01                       # one flipped bit 5 bytes behind x ...
    a.buf[xs + 64 + 4099] ^= 0x80                    # ... and another 4099 bytes behind it
    with pytest.raises(DirtyGuard, match=r"behind 'x_dev': dirty bytes from \+5 to \+4099 past its end"):
        a.check()
    a.refill(pattern)
    a.buf[oe] ^= 0xFF                                # the very first byte behind out
    with pytest.raises(DirtyGuard, match=r"behind 'out_dev': dirty bytes from \+0 to \+0 past"):
        a.check()
    a.refill(pattern)
    a.buf[xs - 1] ^= 0xFF                            # the byte in front of the first region
    with pytest.raises(DirtyGuard, match=r"in front of 'x_dev': dirty bytes from -1 to -1"):
        a.check()
    a.refill(pattern)
    a.buf[a.buf.numel() - 1] ^= 0x10                 # the last byte of the allocation
    with pytest.raises(DirtyGuard, match="behind 'out_dev'"):
        a.check()


def test_put_round_trips_and_the_workspace_adapter_is_exact():
    a = Arena("cpu", 0xFFFFFFFF, Arena.capacity_for([4 * 6, 8 * 16, 1001]))
    arr = np.arange(6, dtype=np.float32).reshape(2, 3)
    cam = np.arange(16, dtype=np.float64)
    wx, wc = a.put(arr, skew=4, name="x"), a.put(cam, name="cam")
    x, c = wx(), wc()
    assert x.shape == (2, 3) and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 256 == 4
    assert np.array_equal(x.numpy(), arr) and np.array_equal(c.numpy(), cam)
    a.refill(0x7F800000)
    assert torch.isinf(x).all()
    assert np.array_equal(wx().numpy(), arr)
    ws = ExactWorkspace(a)
    v = ws.get(1001, a.device)
    assert v.numel() == 1001 and v.data_ptr() % 256 == 0 and ws.get(1001, a.device) is v
    with pytest.raises(AssertionError):
        ws.get(1002, a.device)
    a.check()
