"""Writes tests/golden/anchor_batch_cases.json: for every find case of tests/anchor_batch_cases.py,
every variant (eb0 / eb1 = eliminate_both) and every problem what the CPU models give --
tests/seed_family_model.c the table over the rounds, tests/eo2_model.cpp EliminateOverlaps_v2,
LengthFilter(MIN_ANCHOR_LENGTH + 3) -- as count and md5 of the final list (lengths <u8, then starts
<i8), the table's entries, the AddHashEntry calls over all rounds, MemCollisionCount and the
MER_REPEAT_LIMIT restarts over all rounds; under "pool" the same for the 16 classes of the full-pool
case; under "tail" count and md5 of every tail-only list.
Run from the repository root:  python tests/golden/make_anchor_batch_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import anchor_batch_cases as ab  # noqa: E402


def pool_digest():
    c = ab.pool_case()
    return [ab.digest_problem(ab.model_problem((x, x), c["patterns"][0], variants=("eb0",)), "eb0") for x in c["classes"]]


def main():
    find = {}
    for name in ab.FIND_CASES:
        find[name] = ab.digest_case(name)
        print(name, {v: sum(d["count"] for d in ds) for v, ds in find[name].items()})
    tail = {name: ab.digest_tail(name) for name in ab.tail_cases()}
    for name, d in tail.items():
        print(name, {v: [x["count"] for x in ds] for v, ds in d.items()})
    with open(ab.FIXTURE, "w") as f:
        json.dump(dict(find=find, pool=pool_digest(), tail=tail, min_length=ab.MIN_LENGTH), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
