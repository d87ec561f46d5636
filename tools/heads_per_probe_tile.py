#!/usr/bin/env python3
"""Kept group heads per probe workgroup, on the host (no GPU), for candidate sub-tile sizes.

    python3 tools/heads_per_probe_tile.py --take 2048 2016 1984

The packed-record probe stage (groups.hip, probe_tile_rec_kernel) cuts every MSD bucket of the
sorted stream into group tiles of 2 x take records; a workgroup takes `take` of them, lists the
heads of the groups of >= 2 records and probes 256 heads per round of its loop.  This computes that
list's length for every full sub-tile from the oracle's seed keys of bench.py's genome shape
(8 related genomes, 1 % substitutions, w19; 400,000 bases each by default) and prints the
distribution and the share of workgroups per round count."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

LANES = 256


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--take", type=int, nargs="+", default=[2048, 2016, 1984])
    ap.add_argument("--genomes", type=int, default=8)
    ap.add_argument("--length", type=int, default=400_000)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--weight", type=int, default=19)
    a = ap.parse_args()
    oracle.build()
    seed = oracle.get_seed(a.weight)
    seqs = oracle.generate(a.genomes, a.length, a.rate, 12345)
    keys = np.sort(np.concatenate([oracle.seed_keys(s, seed) for s in seqs])) >> np.uint64(1)
    n = len(keys)
    msd = max(0, 2 * a.weight + 1 - 32)
    # (an oracle key holds the 2w seed bits left-aligned in 64 bits and the orientation in bit 0)
    bucket = (keys >> np.uint64(63 - msd)).astype(np.int64) if msd else np.zeros(n, dtype=np.int64)
    bstart = np.searchsorted(bucket, np.arange((1 << msd) + 1))
    head = np.ones(n, dtype=bool)
    head[1:] = keys[1:] != keys[:-1]
    nxt = np.zeros(n, dtype=bool)   # the next record has the same key
    nxt[:-1] = keys[1:] == keys[:-1]
    kept = head & nxt
    ck = np.concatenate([[0], np.cumsum(kept)])
    print(f"{a.genomes} x {a.length} bases, p = {a.rate}, w{a.weight}: {n} records, {int(head.sum())} groups, "
          f"{int(kept.sum())} kept heads, {1 << msd} MSD buckets")
    for take in a.take:
        counts, nsub = [], 0
        for b in range(1 << msd):
            lo, hi = int(bstart[b]), int(bstart[b + 1])
            starts = np.arange(lo, hi, take)
            nsub += len(starts)
            full = starts[starts + take <= hi]
            counts.append(ck[full + take] - ck[full])
        c = np.concatenate(counts)
        rounds = (c + LANES - 1) // LANES
        print(f"take {take} (group tile {2 * take}): {nsub} workgroups, {len(c)} full; kept heads per full sub-tile: "
              f"mean {c.mean():.1f}, sd {c.std():.1f}, min {c.min()}, max {c.max()}")
        for r in range(1, int(rounds.max()) + 1):
            print(f"  {r} round(s) of {LANES} lanes: {100.0 * np.mean(rounds == r):.1f} % of the full sub-tiles")
        over = c[c > LANES] - LANES
        if len(over):
            print(f"  heads in the second round, where there is one: mean {over.mean():.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
