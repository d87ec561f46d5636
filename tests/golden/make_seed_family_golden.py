"""Writes tests/golden/seed_family_cases.json: for every case of tests/seed_family_cases.py and
every round, what tests/seed_family_model.c (the oracle's MemHash looped over the seed family on
one table) gives -- count and md5 of the MatchList (lengths <u8, then starts <i8), MemCount,
MemCollisionCount, the round's AddHashEntry calls, md5 of mem_table_count (<u4) and of the
match log; and under "chain" the count and md5 of case 1's family list after
tests/eo2_model.cpp and LengthFilter(MIN_ANCHOR_LENGTH + 3), under "chain_k1" the same of
k1_spill_mid_replay's list after round 1.  Run from the repository root:  python tests/golden/make_seed_family_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import seed_family_cases as sf  # noqa: E402
import test_eliminate_overlaps_v2_cpu as eo2  # noqa: E402


def main():
    L = sf.load_model()
    out = {}
    for name in sf.CASES:
        rounds = sf.run_model(L, sf.rounds_of(name))
        out[name] = [sf.digest(r) for r in rounds]
        print(name, [(d["count"], d["collisions"]) for d in out[name]])
        if name == sf.FIRST:
            cl, cs = sf.chain_of_model(eo2, eo2.load_model(), rounds[-1])
            chain = dict(count=int(len(cl)), md5=sf.list_md5(cl, cs), min_length=sf.CHAIN_MIN_LENGTH)
            print("chain", chain)
        if name == sf.SPILL:
            cl, cs = sf.chain_of_model(eo2, eo2.load_model(), rounds[1])
            chain_k1 = dict(count=int(len(cl)), md5=sf.list_md5(cl, cs), min_length=sf.CHAIN_MIN_LENGTH)
            print("chain_k1", chain_k1)
    with open(sf.FIXTURE, "w") as f:
        json.dump(dict(cases=out, chain=chain, chain_k1=chain_k1), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
