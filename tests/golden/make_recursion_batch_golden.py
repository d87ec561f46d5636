"""Writes tests/golden/recursion_batch_cases.json: for every find case of
tests/recursion_batch_cases.py, every variant (m0 / m2 / mG = the multiplicity of MultiplicityFilter)
and every problem what the CPU models give -- tests/seed_family_model.c the table over the rounds,
oracle.eliminate_overlaps the v1 EliminateOverlaps, numpy the two filters (LengthFilter(
MIN_ANCHOR_LENGTH)) -- as count and md5 of the final list (lengths <u8, then starts <i8), the
table's entries, the AddHashEntry calls over all rounds, MemCollisionCount and the MER_REPEAT_LIMIT
restarts over all rounds; under "tail" count and md5 of every tail-only list per variant and
min_length (0 and MIN_ANCHOR_LENGTH).
Run from the repository root:  python tests/golden/make_recursion_batch_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import recursion_batch_cases as rb  # noqa: E402


def main():
    find = {}
    for name in rb.FIND_CASES:
        find[name] = rb.digest_case(name)
        print(name, {v: sum(d["count"] for d in ds) for v, ds in find[name].items()})
    tail = {name: rb.digest_tail(name) for name in rb.tail_cases()}
    for name, d in tail.items():
        print(name, {v: [x["count"] for x in ds] for v, ds in d.items()})
    with open(rb.FIXTURE, "w") as f:
        json.dump(dict(find=find, tail=tail, min_length=rb.MIN_LENGTH), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
