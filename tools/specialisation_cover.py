"""The table of tests/specialisation_cases.py: sweeps the census of kernel specialisations (r3d_debug_forward_census, hooks library,
host only - no GPU) over the domain defined there and prints the COVER list to paste into that module - a greedy cover of every
(kernel, tile kind) pair the sweep reaches that prefers the smallest B, tier by tier (256 workgroups, then 128, then 64) - and, with --table, the census table: per pair the smallest
case that reaches it.

    python tools/specialisation_cover.py [--table]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import specialisation_cases as sc      # noqa: E402


def main():
    t0 = time.time()
    census = sc.Census()
    reached = sc.sweep(census)
    for case in sc.ALWAYS:
        reached.setdefault(case, frozenset(census.pairs(case)))
    cases, first = sc.smallest_cover(reached, sc.ALWAYS)
    census.close()
    print("# %d cases swept in %.1f s, %d (kernel, tile kind) pairs, %d cases in the table" % (len(reached), time.time() - t0, len(first), len(cases)),
          file=sys.stderr)
    print("COVER = [")
    for c in cases:
        if c not in sc.ALWAYS:
            print("    %r," % (c,))
    print("]")
    if "--table" in sys.argv:
        for (kernel, kind), case in sorted(first.items()):
            print("# %-26s %-36s %s" % (kernel, kind or "-", sc.case_id(case)))


if __name__ == "__main__":
    main()
