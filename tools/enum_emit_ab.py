#!/usr/bin/env python3
"""Timing of FindMatches under enumeration tolerance > 8 (pairwise.hip, the by-row odometer
emit) on the shapes of tests/compat_enum_inputs.py, for an A/B of two builds of the library:

    python tools/enum_emit_ab.py --shape J --mode memhash --repeats 7 [--lib other/libmums_hip.so]

One JSON line: per repeat the device times between the context's HIP events -- ms_total (first
key kernel to the MatchList) and ms_groups (sorted stream to the rows: tie replay, count, scan,
emit) -- after --warmup untimed calls, with median / min / max.  The emit kernel's own time comes
from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/...).
--lib loads another build (MUMS_DEV_LIB); everything read lies inside the repository."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="J")
    ap.add_argument("--mode", choices=["memhash", "parallel"], default="memhash")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        os.environ["MUMS_DEV_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    import libmems_amd as lm
    from oracle import oracle
    from tests.compat_enum_inputs import SHAPES, make_input

    spec, w, rt, et, chunk, masked, mask = SHAPES[a.shape]
    seqs = list(make_input(spec))
    mh = lm.ParallelMemHash(0, chunk) if a.mode == "parallel" else lm.MemHash(0)
    tot, grp = [], []
    with mh:
        mh.SetSeed(oracle.get_seed(w))
        mh.SetRepeatTolerance(rt)
        mh.SetEnumerationTolerance(et)
        if masked:
            mh._check(mh._lib.mums_set_mask(mh._ctx, 1, mask))
        for it in range(a.warmup + a.repeats):
            mh.Clear()
            ml = mh.FindMatches(seqs)
            st = mh.stats()
            if it >= a.warmup:
                tot.append(st["ms_total"])
                grp.append(st["ms_groups"])

    def summ(x):
        return {"median": statistics.median(x), "min": min(x), "max": max(x), "all": [round(v, 4) for v in x]}

    print(json.dumps({"lib": a.lib or "libmems_amd/libmums_hip.so", "shape": a.shape, "mode": a.mode,
                      "enum_tol": et, "rows": int(st["probes"]), "matches": len(ml), "repeats": a.repeats,
                      "warmup": a.warmup, "ms_total": summ(tot), "ms_groups": summ(grp)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
