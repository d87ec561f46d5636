"""GPU: the sub-tile geometry of the packed-record probe stage (groups.hip, probe_tile_rec_kernel)
against the oracle.  The sorted stream is cut per MSD bucket into group tiles of 2 x TAKE records
and a workgroup takes TAKE of them -- fewer than the 2048 it can stage, so that at 8 genomes its
heads fit one round of 256 lanes.  G identical genomes make every group exactly G records: the
sub-tiles then hold TAKE / G heads (1, 2 and 4 rounds of the probe loop for G = 8, 4 and 2) and the
groups straddle the split, the tile end and the bucket end at every phase.  Every case compares
Probes() with oracle.seed_probes, the FindMatches MatchList and collision_count with
oracle.find_matches, and the seed-mer, group and probe counters (the groups are the distinct
oracle keys)."""
import numpy as np
import pytest

from tests.test_gpu_probe_edges import _check, _copies, _revcomp, _sorted_keys

pytestmark = pytest.mark.gpu

TAKE = 1984          # records a probe workgroup takes (kProbeTake)
LANES = 256


def _rounds(keys, msd_bits):
    """rounds of the probe loop per workgroup: ceil(heads of groups of >= 2 records / 256) for every
    sub-tile of TAKE records of every MSD bucket (keys: sorted, orientation bit dropped)"""
    n = len(keys)
    bucket = (keys >> np.uint64(63 - msd_bits)).astype(np.int64) if msd_bits else np.zeros(n, dtype=np.int64)
    bstart = np.searchsorted(bucket, np.arange((1 << msd_bits) + 1))
    kept = np.zeros(n, dtype=bool)
    kept[:-1] = keys[1:] == keys[:-1]
    kept[1:] &= keys[1:] != keys[:-1]
    ck = np.concatenate([[0], np.cumsum(kept)])
    out = set()
    for b in range(1 << msd_bits):
        lo, hi = int(bstart[b]), int(bstart[b + 1])
        for s in range(lo, hi, TAKE):
            h = int(ck[min(s + TAKE, hi)] - ck[s])
            out.add((h + LANES - 1) // LANES)
    return out


# (G, bases per genome, seed weight, rounds the full sub-tiles run)
IDENTICAL = [(2, 20_000, 15, 4), (3, 7_001, 13, 3), (4, 10_000, 14, 2), (5, 3_000, 11, 2), (7, 5_003, 12, 2),
             (8, 4_099, 15, 1), (9, 3_001, 13, 1), (8, 20_000, 19, 1), (4, 16_001, 17, 2)]


@pytest.mark.parametrize("G,n,w,rounds", IDENTICAL)
def test_identical_genomes(gpu_lib, oracle_mod, G, n, w, rounds):
    seed = oracle_mod.get_seed(w)
    seqs = _copies(oracle_mod, G, n, 0.0, 3 * G + w)   # the last one reverse-complemented
    keys = _sorted_keys(oracle_mod, seqs, seed)
    msd = max(0, 2 * w + 1 - 32)
    assert rounds in _rounds(keys, msd)
    ost = _check(gpu_lib, oracle_mod, seqs, seed)
    assert ost["probes"] > 0.9 * (n - 40)   # one probe per distinct key (palindromes and repeats aside)


def test_round_counts_covered():
    """the cases above run 1, 2 and 4 rounds of the probe loop"""
    assert {1, 2, 4} <= {r for _, _, _, r in IDENTICAL}


@pytest.mark.parametrize("phase", range(1, 9))
def test_groups_at_every_phase_of_the_split(gpu_lib, oracle_mod, phase):
    """8 identical genomes behind `phase` records of a smaller key: the groups of 8 records meet
    the split (record TAKE) and the tile end (2 x TAKE) at every phase"""
    seed = oracle_mod.get_seed(15)
    L = oracle_mod.lib().oracle_seed_length(seed)
    seqs = _copies(oracle_mod, 8, 1_100, 0.0, 70)
    seqs.append(b"A" * (L - 1 + phase))   # `phase` records of the smallest key, in one more genome
    keys = _sorted_keys(oracle_mod, seqs, seed)
    assert len(keys) > 2 * TAKE + 16 and keys[phase - 1] == 0 and keys[phase] != 0
    assert keys[TAKE - 1] == keys[TAKE] or keys[2 * TAKE - 1] == keys[2 * TAKE] or phase == 8
    _check(gpu_lib, oracle_mod, seqs, seed)


@pytest.mark.parametrize("w", [19, 15])
def test_related_genomes(gpu_lib, oracle_mod, w):
    seqs = oracle_mod.generate(8, 40_000, 0.01, 4242)
    seqs[3] = _revcomp(seqs[3])
    ost = _check(gpu_lib, oracle_mod, seqs, oracle_mod.get_seed(w))
    assert ost["probes"] > 20_000
