#!/usr/bin/env python
"""Cost of a seed-family find (ClearSequences keeps the MemHash table, ProgressiveAligner.cpp:
619-653) against the same three finds run independently.

Input: G related genomes of n bases (Appendix-C generator, substitution rate p), seed weight w,
seed ranks 0-2, table size T.  Both figures are the best of --repeats runs after one warm-up, each
run the sum of the three finds' HIP-event totals (mums_get_stats ms_total):

  independent  Clear between the finds: three tables from zero (runs on any commit);
  family       Clear once, then ClearSequences + FindMatches per rank: one table (needs
               mums_clear_sequences; reported as null where the library has none).

Prints one JSON line.  Usage: python tools/bench_seed_family.py [--n 1000000] [--p 0.01] ...
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=ROOT, help="tree whose libmems_amd and oracle are used")
    ap.add_argument("--G", type=int, default=2)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--p", type=float, default=0.01)
    ap.add_argument("--w", type=int, default=15)
    ap.add_argument("--T", type=int, default=40000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    import libmems_amd as lib
    from oracle import oracle

    seqs = oracle.generate(a.G, a.n, a.p, 12345)
    seeds = [oracle.get_seed(a.w, r) for r in range(3)]
    has_family = hasattr(lib.load_library(), "mums_clear_sequences")

    def run(family: bool):
        parts, counts = [], []
        with lib.MemHash(0) as mh:
            mh.SetTableSize(a.T)
            mh.Clear()
            for seed in seeds:
                mh.ClearSequences() if family else mh.Clear()
                mh.SetSeed(seed)
                mh.FindMatches(seqs)
                st = mh.stats()
                parts.append(dict(ms_total=st["ms_total"], ms_chains=st["ms_chains"], ms_replay=st["ms_replay"],
                                  ms_output=st["ms_output"]))
                counts.append(int(st["mem_count"]))
        return sum(p["ms_total"] for p in parts), parts, counts

    def best(family: bool):
        run(family)   # warm-up
        runs = [run(family) for _ in range(a.repeats)]
        return min(runs, key=lambda r: r[0])

    ind = best(False)
    fam = best(True) if has_family else None
    out = dict(G=a.G, n=a.n, p=a.p, w=a.w, T=a.T, repeats=a.repeats,
               independent_ms=round(ind[0], 3), independent_counts=ind[2], independent_rounds=ind[1],
               family_ms=round(fam[0], 3) if fam else None, family_counts=fam[2] if fam else None,
               family_rounds=fam[1] if fam else None,
               ratio=round(fam[0] / ind[0], 3) if fam else None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
