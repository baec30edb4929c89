"""The single-launch tile lists of a call as the library builds them on the host (hooks build, no GPU): r3d_debug_forward_check under
R3D_FWD_DUMP, parsed.  Shared by tests/test_run_tiles_host.py and tests/test_gpu_run_tiles.py."""
import ctypes
import os

NB_CODE = 64          # r3d_internal.hpp: tile code NB_CODE + nb = one 32-row unit x nb column blocks (gemm_tile_nb)


def forward_lists(mc, B, tmp_path, pair="both", nwg=256):
    """(problems, tiles, rc) of the call of B windows: problems[i] = dict(name, M, N, K, nseg, deps); tiles = dicts(wg, prob, units,
    row0, col0, code, src2) in workgroup order; rc = r3d_debug_forward_check's verdict (0: a sound dependency machine)."""
    from conftest import hooks_library
    from ray3d_amd import _capi
    from ray3d_amd.spec import config_from_dicts
    lib = hooks_library()
    fn = lib.r3d_debug_forward_check
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    hp = _capi.Handle(config_from_dicts(mc, "pos")) if pair in ("both", "pos") else None
    ht = _capi.Handle(config_from_dicts(mc, "trj")) if pair in ("both", "trj") else None
    path = os.path.join(str(tmp_path), "fwd_%s_%d.txt" % (pair, B))
    old = os.environ.get("R3D_FWD_DUMP")
    os.environ["R3D_FWD_DUMP"] = path
    try:
        n, c = ctypes.c_int(), ctypes.c_int()
        rc = fn(hp.ptr if hp else None, ht.ptr if ht else None, B, nwg, ctypes.byref(n), ctypes.byref(c))
    finally:
        if old is None:
            del os.environ["R3D_FWD_DUMP"]
        else:
            os.environ["R3D_FWD_DUMP"] = old
        for h in (hp, ht):
            if h:
                h.close()
    probs, tiles = {}, []
    with open(path) as f:
        for line in f:
            w = line.split()
            if w[0] == "P":
                val = lambda key: int(w[w.index(key) + 1])
                probs[int(w[1])] = dict(name=w[2], M=val("M"), N=val("N"), K=val("K"), nseg=val("nseg"), deps=[int(v) for v in w[w.index("deps") + 1:]])
            elif w[0] == "T":
                tiles.append(dict(wg=int(w[1]), prob=int(w[3]), units=int(w[4]), row0=int(w[5]), col0=int(w[6]), code=int(w[7]), src2=int(w[8])))
    os.remove(path)
    return probs, tiles, rc


def sources_of(tile, probs):
    """[(problem, unit, first block, blocks)] of a gemm_tile_nb tile: one source, or the rest of a row and the start of the next."""
    nb = tile["code"] - NB_CODE
    if tile["src2"] < 0:
        return [(tile["prob"], tile["row0"] // 32, tile["col0"] // 32, nb)]
    n0 = (probs[tile["prob"]]["N"] - tile["col0"]) // 32
    same = tile["src2"] == tile["prob"]
    return [(tile["prob"], tile["row0"] // 32, tile["col0"] // 32, n0), (tile["src2"], tile["row0"] // 32 + 1 if same else 0, 0, nb - n0)]
