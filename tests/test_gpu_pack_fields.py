"""GPU: the keys pass (seeds.hip, seed_pack_kernel) against the oracle.  For a compiled seed
pattern its MSD histogram takes the top key digit from two 32-bit fields of the packed words (a
lane handles the 16 positions of one word); other patterns build the whole key from the 64-bit
window.  A wrong histogram misplaces records in the scatter, so every case compares SeedKeys of
every genome, Probes() and the FindMatches MatchList (tests/test_gpu_tile_edges._check).  Cases:
genomes of L - 1, L and L + 1 bases and of 4095, 4096 and 4097 bases and seed-mers (the 4096-position
tile with and without its halo of L - 1 bases), device tensors at byte offsets 1-15 (the unaligned
packing path), a '-' (the gap error), one compiled pattern per weight 11-19 and a pattern
without a compiled table (w20)."""
import pytest

from tests.test_gpu_tile_edges import _check, _related

pytestmark = pytest.mark.gpu

TILE = 4096


def _lengths(L):
    return [L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, TILE + L - 2, TILE + L - 1, TILE + L]


@pytest.mark.parametrize("w", [19, 17, 20])
def test_genome_lengths(gpu_lib, oracle_mod, w):
    """w19: 7-bit digit; w17: 3-bit digit; w20: run table from the kernel argument"""
    seed = oracle_mod.get_seed(w)
    L = oracle_mod.lib().oracle_seed_length(seed)
    lengths = _lengths(L)
    seqs = _related(oracle_mod, lengths, 11 + w)
    for k in range(0, len(lengths), 3):   # three genomes per run, with a longer one so that probes exist
        part = [seqs[-1]] + seqs[k:k + 3]
        _check(gpu_lib, oracle_mod, part, seed)


@pytest.mark.parametrize("w", list(range(11, 21)))
def test_patterns(gpu_lib, oracle_mod, w):
    seed = oracle_mod.get_seed(w)
    seqs = _related(oracle_mod, [2 * TILE + 77, TILE + 5, 3 * TILE - 1], 200 + w, rate=0.01)
    _check(gpu_lib, oracle_mod, seqs, seed)


@pytest.mark.parametrize("off", list(range(1, 16)))
def test_unaligned_device_tensors(gpu_lib, oracle_mod, off):
    import torch
    seed = oracle_mod.get_seed(19)
    seqs = _related(oracle_mod, [TILE + 300, 2 * TILE + 26, TILE - 3], 300 + off, rate=0.01)
    bufs = [torch.frombuffer(bytearray(b"A" * ((off + 5 * g) % 16 or 3) + s), dtype=torch.uint8).cuda()
            for g, s in enumerate(seqs)]
    views = [b[len(b) - len(s):] for b, s in zip(bufs, seqs)]
    assert views[0].data_ptr() % 16 == off and all(v.data_ptr() % 16 for v in views)
    _check(gpu_lib, oracle_mod, seqs, seed, dev_seqs=views)


@pytest.mark.parametrize("w", [19, 15])
@pytest.mark.parametrize("pos", [0, 15, 16, TILE - 1, TILE, TILE + 20])
def test_gap_raises(gpu_lib, oracle_mod, w, pos):
    base = bytearray(oracle_mod.generate(1, TILE + 100, 1.0, 9)[0])
    base[pos] = ord("-")
    with pytest.raises(gpu_lib.GapInSequence):
        with gpu_lib.MemHash(0) as mh:
            mh.SetSeed(oracle_mod.get_seed(w))
            mh.FindMatches([bytes(base), bytes(base[:TILE // 2]).replace(b"-", b"A")])
