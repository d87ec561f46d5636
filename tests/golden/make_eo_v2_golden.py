"""Writes eo_v2_cases.json: for every run of tests/test_eliminate_overlaps_v2_cpu.py (each case x
eliminate_both, the subset runs, the edge lists, and FindMatches -> EliminateOverlaps_v2 -> LengthFilter on the
repeat-rich input) the output count and the md5 of lengths (<u8) + starts (<i8), recorded from
the C++ model tests/eo2_model.cpp.  Needs g++ and the built oracle:

    python tests/golden/make_eo_v2_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_eliminate_overlaps_v2_cpu as t   # noqa: E402
from oracle import oracle   # noqa: E402


def main():
    if not os.path.exists(oracle.LIB):
        oracle.build()
    L = t.load_model()
    runs = {}
    inputs = t.all_inputs()
    for key, c, ids, both in t.fixture_runs():
        ol, os_, cnt = t.model_eo2(L, *inputs[c], ids, both)
        runs[key] = {"count": len(ol), "md5": t.digest(ol, os_)}
        print(key, runs[key]["count"], cnt)
    for G in t.CHAIN_GS:
        lengths, starts, _ = oracle.find_matches(t.repeat_rich(G), oracle.get_seed(11))
        for both in (0, 1):
            ol, os_, cnt = t.model_eo2(L, lengths, starts, None, bool(both))
            keep = ol >= t.CHAIN_MIN_LENGTH
            key = f"chain_G{G}_both{both}_min{t.CHAIN_MIN_LENGTH}"
            runs[key] = {"count": int(keep.sum()), "md5": t.digest(ol[keep], os_[keep])}
            print(key, len(lengths), len(ol), runs[key]["count"], cnt)
    with open(os.path.join(HERE, "eo_v2_cases.json"), "w") as f:
        json.dump({"source": "tests/eo2_model.cpp via tests/golden/make_eo_v2_golden.py", "runs": runs}, f, indent=1,
                  sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
