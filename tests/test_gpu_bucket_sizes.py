"""GPU: the hash bucket of the seed probes, ((offset % T) + T) % T (MemHash.cpp:213), for table
sizes from 1 to 2^31 against the oracle.  A reverse-complemented genome makes offsets negative.
Up to 40,000 buckets the oracle runs with the same table size.  Its hash table has one slot array
per bucket, so for 2^31 - 1 and 2^31 buckets the expected buckets come from the oracle's offsets
instead: the buckets it reports for the coprime table sizes 40,000 and 39,999 fix every offset
(|offset| < 8 * 10^8 here) by the Chinese remainder theorem."""
import random

import numpy as np
import pytest

from tests.test_gpu_probe_edges import _mutate, _revcomp

pytestmark = pytest.mark.gpu

T1, T2 = 40_000, 39_999   # coprime (consecutive); T1 = 1 (mod T2)


@pytest.fixture(scope="module")
def case(oracle_mod):
    """4 related genomes that start at different bases of one sequence (forward pairs: positive
    and negative offsets), the last reverse-complemented; the oracle's probes and their offsets"""
    rng = random.Random(17)
    base = oracle_mod.generate(1, 3_300, 1.0, 1717)[0]
    seqs = [_mutate(base[300:], 0.02, rng), _mutate(base[:3_000], 0.02, rng), _mutate(base[150:3_150], 0.02, rng),
            _mutate(base[100:3_100], 0.02, rng)]
    seqs[3] = _revcomp(seqs[3])
    seed = oracle_mod.get_seed(15)
    b1, ref1, _ = oracle_mod.seed_probes(seqs, seed, table_size=T1)
    b2, ref2, _ = oracle_mod.seed_probes(seqs, seed, table_size=T2)
    assert np.array_equal(ref1, ref2) and len(b1) > 1000
    b1, b2 = b1.astype(np.int64), b2.astype(np.int64)
    off = b1 + T1 * ((b2 - b1) % T2)            # in [0, T1 T2), = offset mod T1 T2
    off = np.where(off >= T1 * T2 // 2, off - T1 * T2, off)
    assert np.array_equal(off % T1, b1) and np.array_equal(off % T2, b2)
    assert (off < 0).sum() > 100 and (off > 0).sum() > 100 and len(np.unique(off)) >= 8
    return seqs, seed, off, ref1


def _gpu_probes(gpu_lib, seqs, seed, T):
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(seed)
        mh.SetTableSize(T)
        for s in seqs:
            mh.AddSequence(s)
        mh.FindStage(gpu_lib.STAGE_SEEDS)
        return mh.Probes()


@pytest.mark.parametrize("T", [1, 7, 40_000, 2**31 - 1, 2**31])
def test_probe_buckets(gpu_lib, oracle_mod, case, T):
    seqs, seed, off, ref = case
    b, r = _gpu_probes(gpu_lib, seqs, seed, T)
    assert np.array_equal(r, ref)
    assert np.array_equal(b.astype(np.int64), off % T)   # numpy's % is the floor remainder: in [0, T)
    if T <= 40_000:
        ob, orf, _ = oracle_mod.seed_probes(seqs, seed, table_size=T)
        assert np.array_equal(b, ob) and np.array_equal(r, orf)


@pytest.mark.parametrize("T", [1, 7, 40_000])
def test_matchlist_with_table_size(gpu_lib, oracle_mod, case, T):
    seqs, seed, _, _ = case
    ref = oracle_mod.find_matches(seqs, seed, table_size=T)
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(seed)
        mh.SetTableSize(T)
        ml = mh.FindMatches(seqs)
        st = mh.stats()
    assert len(ml) == len(ref[0]) > 0
    assert (ml.lengths == ref[0]).all() and (ml.starts == ref[1]).all()
    assert st["collision_count"] == ref[2]["collision_count"]
