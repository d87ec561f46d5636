"""GPU: tile edges of the seed stage against the oracle.  The seed kernels work on tiles of
4096 positions of one genome, the onesweep sort on tiles of 9216 records of one MSD bucket;
full tiles take paths without per-record bounds checks, the last tile of a genome / bucket is
padded.  Every case compares SeedKeys of every genome, Probes() and the FindMatches MatchList."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED_TILE = 4096
SORT_TILE = 9216


def _related(oracle_mod, lengths, rng_seed, rate=0.02):
    """genomes of the given lengths: mutated prefixes of one random sequence"""
    rng = random.Random(rng_seed)
    base = oracle_mod.generate(1, max(max(lengths), 64), 1.0, 900 + rng_seed)[0]
    out = []
    for n in lengths:
        b = bytearray(base[:n])
        for _ in range(int(n * rate)):
            b[rng.randrange(n)] = rng.choice(b"ACGT")
        out.append(bytes(b))
    return out


def _check(gpu_lib, oracle_mod, seqs, seed, dev_seqs=None):
    """keys of every genome, the probe sequence and the MatchList, all against the oracle"""
    ob, orf, ost = oracle_mod.seed_probes(seqs, seed)
    ref = oracle_mod.find_matches(seqs, seed)
    inp = dev_seqs if dev_seqs is not None else seqs
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(seed)
        for s in inp:
            mh.AddSequence(s)
        mh.FindStage(gpu_lib.STAGE_SEEDS)
        for g, s in enumerate(seqs):
            rk = oracle_mod.seed_keys(s, seed)
            if len(rk):
                assert np.array_equal(mh.SeedKeys(g, len(rk)), rk), f"keys of genome {g}"
        b, r = mh.Probes()
    assert len(b) == ost["probes"]
    assert np.array_equal(b, ob)
    assert np.array_equal(r, orf)
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(seed)
        ml = mh.FindMatches(inp)
        st = mh.stats()
    assert len(ml) == len(ref[0])
    assert (ml.lengths == ref[0]).all() and (ml.starts == ref[1]).all()
    assert st["collision_count"] == ref[2]["collision_count"]


# ---- seed tiles: 4096 positions of one genome ------------------------------------------
# w19: compiled table, 128 buckets (7-bit ranking); w17: compiled, 8 buckets; w15: compiled, one
# bucket; w20: no compiled table (run table from the kernel argument, side digits)
@pytest.mark.parametrize("w", [19, 15, 17, 20])
@pytest.mark.parametrize("counts", [(SEED_TILE + 1, 1, 2 * SEED_TILE), (SEED_TILE - 1, 2 * SEED_TILE + 1, SEED_TILE)])
def test_seed_tile_edges(gpu_lib, oracle_mod, w, counts):
    seed = oracle_mod.get_seed(w)
    L = oracle_mod.lib().oracle_seed_length(seed)
    seqs = _related(oracle_mod, [m + L - 1 for m in counts], 3 * w + counts[0] % 7)
    for s, m in zip(seqs, counts):
        assert len(oracle_mod.seed_keys(s, seed)) == m
    _check(gpu_lib, oracle_mod, seqs, seed)


# ---- sort tiles: 9216 records of one bucket ----------------------------------------------
@pytest.mark.parametrize("N", [SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 3 * SORT_TILE - 1, 3 * SORT_TILE,
                               3 * SORT_TILE + 1, 8191, 8192, 8193])
def test_sort_tile_edges_one_bucket(gpu_lib, oracle_mod, N):
    seed = oracle_mod.get_seed(15)   # 31-bit keys: one bucket
    L = oracle_mod.lib().oracle_seed_length(seed)
    m0 = N // 2
    seqs = _related(oracle_mod, [m0 + L - 1, N - m0 + L - 1], N % 97)
    assert sum(len(oracle_mod.seed_keys(s, seed)) for s in seqs) == N
    _check(gpu_lib, oracle_mod, seqs, seed)


def test_sort_tile_edges_w19_buckets(gpu_lib, oracle_mod):
    """128 MSD buckets of very different sizes (canonical keys crowd the low buckets): some
    hold several full sort tiles and a partial one, some less than one tile."""
    seed = oracle_mod.get_seed(19)
    seqs = oracle_mod.generate(3, 450_000, 0.02, 777)
    # the MSD digit = the top 7 bits of the 39-bit canonical key = of the left-aligned mer
    keys = np.concatenate([oracle_mod.seed_keys(s, seed) for s in seqs])
    hist = np.bincount((keys >> np.uint64(57)).astype(np.int64), minlength=128)
    assert hist.sum() == len(keys)
    assert any(c >= 2 * SORT_TILE and c % SORT_TILE != 0 for c in hist), hist
    assert any(0 < c < SORT_TILE for c in hist), hist
    _check(gpu_lib, oracle_mod, seqs, seed)


# ---- the same digit in every lane --------------------------------------------------------
@pytest.mark.parametrize("w", [19, 15])
def test_equal_digits_poly_a(gpu_lib, oracle_mod, w):
    _check(gpu_lib, oracle_mod, [b"A" * 20_000, b"A" * 20_000], oracle_mod.get_seed(w))


@pytest.mark.parametrize("w", [19, 15])
def test_equal_digits_half_poly_a(gpu_lib, oracle_mod, w):
    rnd = oracle_mod.generate(2, 10_000, 0.02, 31)
    _check(gpu_lib, oracle_mod, [b"A" * 10_000 + rnd[0], b"A" * 10_000 + rnd[1]], oracle_mod.get_seed(w))


# ---- the byte table ------------------------------------------------------------------------
def _all_bytes_genome():
    """every byte value 1-255 except '-', each at every position mod 16 (255 bytes per
    repetition: the phase moves by 15), twice over so that it spans seed tiles"""
    vals = bytes(v for v in range(1, 256) if v != ord("-"))
    one = b"".join(vals + b"A" for _ in range(16))
    pos = {}
    for i, c in enumerate(one):
        pos.setdefault(c, set()).add(i % 16)
    assert all(len(pos[v]) == 16 for v in vals)
    return one + one[::-1] + one[:1000]


@pytest.mark.parametrize("w", [19, 15])
def test_byte_table_every_alignment(gpu_lib, oracle_mod, w):
    import torch
    seed = oracle_mod.get_seed(w)
    genome = _all_bytes_genome()
    ref = oracle_mod.seed_keys(genome, seed)
    for off in range(16):
        buf = torch.frombuffer(bytearray(b"A" * off + genome), dtype=torch.uint8).cuda()
        view = buf[off:]
        assert view.data_ptr() % 16 == off
        with gpu_lib.MemHash(0) as mh:
            mh.SetSeed(seed)
            mh.AddSequence(view)
            mh.FindStage(gpu_lib.STAGE_SEEDS)
            assert np.array_equal(mh.SeedKeys(0, len(ref)), ref), f"offset {off}"


@pytest.mark.parametrize("off", [0, 5])
@pytest.mark.parametrize("pos", [SEED_TILE - 1, SEED_TILE, 2 * SEED_TILE - 1, 2 * SEED_TILE])
def test_gap_at_tile_edge_raises(gpu_lib, oracle_mod, pos, off):
    """'-' as the last byte of a tile and as the first byte of the next one"""
    import torch
    base = bytearray(oracle_mod.generate(1, 3 * SEED_TILE, 1.0, 3)[0])
    base[pos] = ord("-")
    buf = torch.frombuffer(bytearray(b"A" * off) + base, dtype=torch.uint8).cuda()
    with pytest.raises(gpu_lib.GapInSequence):
        with gpu_lib.MemHash(0) as mh:
            mh.SetSeed(oracle_mod.get_seed(15))
            mh.FindMatches([buf[off:], torch.frombuffer(bytearray(base[:pos]), dtype=torch.uint8).cuda()])
