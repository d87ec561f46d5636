"""GPU: edges of the probe stage (groups.hip, probe_tile_rec_kernel) against the oracle.  A probe
tile is 4096 records of one MSD bucket of the sorted stream; a workgroup handles a 2048-record
half of it: it lists the heads of the groups of >= 2 records (at most 1024), builds one probe per
lane (256 per iteration) and compacts the accepted ones.  Every case compares Probes() with
oracle.seed_probes, the FindMatches MatchList and collision_count with oracle.find_matches, and
the seed-mer, group and probe counters.  The oracle reports no group count: the groups are
the distinct keys of oracle.seed_keys without the orientation bit; it reports no repeat-limit count either: that counter is
0 whenever the oracle's largest group stays at or below MER_REPEAT_LIMIT (1000)."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HALF = 2048
TILE = 4096
REPEAT_LIMIT = 1000
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(s):
    return s.translate(_RC)[::-1]


def _mutate(s, rate, rng):
    b = bytearray(s)
    for _ in range(int(len(b) * rate)):
        b[rng.randrange(len(b))] = rng.choice(b"ACGT")
    return bytes(b)


def _related(oracle_mod, lengths, rng_seed, rate=0.02):
    """genomes of the given lengths: mutated prefixes of one random sequence"""
    rng = random.Random(rng_seed)
    base = oracle_mod.generate(1, max(max(lengths), 64), 1.0, 900 + rng_seed)[0]
    return [_mutate(base[:n], rate, rng) for n in lengths]


def _copies(oracle_mod, G, n, rate, rng_seed):
    """G copies of one iid genome, each mutated at the given rate, the last reverse-complemented"""
    rng = random.Random(rng_seed)
    base = oracle_mod.generate(1, n, 1.0, 400 + rng_seed)[0]
    out = [_mutate(base, rate, rng) for _ in range(G)]
    out[-1] = _revcomp(out[-1])
    return out


def _sorted_keys(oracle_mod, seqs, seed):
    """the group keys of the merged sorted stream (bit 0 of a seed key is the orientation)"""
    return np.sort(np.concatenate([oracle_mod.seed_keys(s, seed) for s in seqs])) >> np.uint64(1)


def _check_counters(st, ost, keys):
    assert st["seedmers"] == ost["seedmers"] == len(keys)
    assert st["probes"] == ost["probes"]
    if ost["max_group"] <= REPEAT_LIMIT:   # no restart: the groups are those of the whole stream
        assert st["repeat_limit_groups"] == 0
        assert st["groups"] == len(np.unique(keys))


def _check(gpu_lib, oracle_mod, seqs, seed):
    """the probe sequence, the MatchList and the counters, all against the oracle"""
    ob, orf, ost = oracle_mod.seed_probes(seqs, seed)
    ref = oracle_mod.find_matches(seqs, seed)
    keys = _sorted_keys(oracle_mod, seqs, seed)
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(seed)
        for s in seqs:
            mh.AddSequence(s)
        mh.FindStage(gpu_lib.STAGE_SEEDS)
        b, r = mh.Probes()
        st = mh.stats()
    assert len(b) == ost["probes"]
    assert np.array_equal(b, ob)
    assert np.array_equal(r, orf)
    _check_counters(st, ost, keys)
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(seed)
        ml = mh.FindMatches(seqs)
        st = mh.stats()
    assert len(ml) == len(ref[0])
    assert (ml.lengths == ref[0]).all() and (ml.starts == ref[1]).all()
    assert st["collision_count"] == ref[2]["collision_count"]
    _check_counters(st, ref[2], keys)
    return ost


def _check_matchlist(gpu_lib, oracle_mod, seqs, seed, mask=None, repeat_tol=0, enum_tol=1):
    """the MatchList alone (the oracle's probe log knows neither masks nor tolerances)"""
    kw = dict(repeat_tol=repeat_tol, enum_tol=enum_tol)
    if mask is not None:
        kw.update(masked=True, seq_mask=mask)
    ref = oracle_mod.find_matches(seqs, seed, **kw)
    cls = gpu_lib.MaskedMemHash if mask is not None else gpu_lib.MemHash
    with cls(0) as mh:
        mh.SetSeed(seed)
        if mask is not None:
            mh.SetMask(mask)
        if repeat_tol:
            mh.SetRepeatTolerance(repeat_tol)
        if enum_tol != 1:
            mh.SetEnumerationTolerance(enum_tol)
        ml = mh.FindMatches(seqs)
        st = mh.stats()
    assert len(ml) == len(ref[0])
    assert (ml.lengths == ref[0]).all() and (ml.starts == ref[1]).all()
    assert st["collision_count"] == ref[2]["collision_count"]
    assert st["probes"] == ref[2]["probes"] and st["mem_count"] == ref[2]["mem_count"]
    return ref


# ---- 1. record-count edges: an empty second half, a one-record half, the words at a half's ends
COUNTS = [HALF - 1, HALF, HALF + 1, TILE - 1, TILE, TILE + 1, TILE + HALF - 1, TILE + HALF, TILE + HALF + 1]


@pytest.mark.parametrize("N", COUNTS)
def test_record_count_edges(gpu_lib, oracle_mod, N):
    seed = oracle_mod.get_seed(15)   # 31-bit keys: one bucket
    L = oracle_mod.lib().oracle_seed_length(seed)
    m0 = N // 2
    seqs = _related(oracle_mod, [m0 + L - 1, N - m0 + L - 1], 11 + N % 89)
    ost = _check(gpu_lib, oracle_mod, seqs, seed)
    assert ost["seedmers"] == N and ost["probes"] > 100


# ---- 2. heads per workgroup: about 1024 (the heads[] capacity), 512, 293 and 256 per half
@pytest.mark.parametrize("G,rate", [(2, 0.0), (4, 0.0), (7, 0.0), (8, 0.0), (8, 0.005), (8, 0.05)])
def test_heads_per_workgroup(gpu_lib, oracle_mod, G, rate):
    seed = oracle_mod.get_seed(15)
    seqs = _copies(oracle_mod, G, 3000, rate, 7 * G + int(rate * 1000))
    ost = _check(gpu_lib, oracle_mod, seqs, seed)
    if rate == 0.0:   # every group has all G genomes: one probe per distinct key (palindromes aside)
        assert ost["probes"] > 2900


# ---- 3. groups across a half or tile end, oversize groups -------------------------------------
def _repeat_genomes(oracle_mod, seed, G, N):
    """G related genomes with N seed-mers in all; segment A lies twice in genome 0 (groups of G + 1
    records, genome 0 twice: rejected), segment B twice in every genome (2 G records: past the
    batch of MG + 1).  The generator seed is the first one for which a group of more than G
    records straddles record 2048 of the sorted stream and another one record 4096."""
    L = oracle_mod.lib().oracle_seed_length(seed)
    assert N > TILE and N % G == 0
    n = N // G + L - 1
    for gs in range(400):
        rng = random.Random(5000 + gs)
        base = oracle_mod.generate(1, n, 1.0, 6000 + gs)[0]
        segA, segB = base[100:300], base[400:600]
        body = base[:n - 600]   # A and B lie in the body once; + (A or filler) + B + filler
        seqs = []
        for g in range(G):
            s = body + (segA if g == 0 else base[n - 600:n - 400]) + segB + base[n - 200:]
            assert len(s) == n
            seqs.append(s if g == 0 else _mutate(s, 0.01, rng))
        keys = _sorted_keys(oracle_mod, seqs, seed)
        assert len(keys) == N
        uniq, first, count = np.unique(keys, return_index=True, return_counts=True)
        big = count > G

        def straddled(edge):
            return bool(np.any(big & (first < edge) & (first + count > edge)))

        if straddled(HALF) and straddled(TILE) and np.any(count == G + 1) and np.any(count >= 2 * G):
            return seqs
    raise AssertionError("no generator seed puts oversize groups on both edges")


REPEAT_CASES = {}


def _repeat_case(oracle_mod, G, N):
    if (G, N) not in REPEAT_CASES:
        REPEAT_CASES[(G, N)] = _repeat_genomes(oracle_mod, oracle_mod.get_seed(15), G, N)
    return REPEAT_CASES[(G, N)]


@pytest.mark.parametrize("G,N", [(5, TILE + HALF + 1), (3, TILE + HALF)])
def test_groups_across_edges_and_oversize(gpu_lib, oracle_mod, G, N):
    seqs = _repeat_case(oracle_mod, G, N)
    _check(gpu_lib, oracle_mod, seqs, oracle_mod.get_seed(15))


def test_tandem_repeat_groups(gpu_lib, oracle_mod):
    """a short tandem repeat: groups far above G (and MG + 1) records next to ordinary ones"""
    unit = oracle_mod.generate(1, 37, 1.0, 77)[0]
    seqs = _related(oracle_mod, [1500, 1500, 1500], 5)
    seqs = [s[:700] + unit * (4 + g) + s[700:] for g, s in enumerate(seqs)]
    ost = _check(gpu_lib, oracle_mod, seqs, oracle_mod.get_seed(15))
    assert 8 < ost["max_group"] <= REPEAT_LIMIT


# ---- 4. G against MG: the MG 4, 8, 16 and 64 instances ----------------------------------------
@pytest.mark.parametrize("G", [3, 5, 9, 33])
def test_genome_count_instances(gpu_lib, oracle_mod, G):
    seqs = _related(oracle_mod, [2000 + 3 * g for g in range(G)], 40 + G, rate=0.01)
    ost = _check(gpu_lib, oracle_mod, seqs, oracle_mod.get_seed(15))
    assert ost["probes"] > 1000


# ---- 5. w19: 128 buckets, many shorter than one half ------------------------------------------
def test_w19_bucket_ends(gpu_lib, oracle_mod):
    seed = oracle_mod.get_seed(19)
    seqs = _related(oracle_mod, [60_000, 60_000, 60_000], 19)
    keys = _sorted_keys(oracle_mod, seqs, seed)
    hist = np.bincount((keys >> np.uint64(56)).astype(np.int64), minlength=128)   # the 7-bit MSD digit
    assert any(0 < c < HALF for c in hist) and any(c > HALF for c in hist), hist
    _check(gpu_lib, oracle_mod, seqs, seed)


# ---- 6. MaskedMemHash: no mask, all genomes, a proper subset (genome 0 = the top bit) ----------
@pytest.mark.parametrize("mask", [0, 0b1111, 0b1010])
def test_masked_memhash(gpu_lib, oracle_mod, mask):
    base = oracle_mod.generate(1, 3000, 1.0, 428)[0]
    rng = random.Random(3)
    far = [base[:1400] + _mutate(base[1400:], 0.2, rng) for _ in range(2)]   # genomes 0 and 2 alone past 1400
    seqs = [base, far[0], base, _revcomp(far[1])]
    ref = _check_matchlist(gpu_lib, oracle_mod, seqs, oracle_mod.get_seed(15), mask=mask)
    assert len(ref[0]) > 0


# ---- 7. non-default tolerances (repeat_tol 1; enum_tol 2: the general instance) ----------------
@pytest.mark.parametrize("repeat_tol,enum_tol", [(1, 1), (0, 2)])
def test_non_default_tolerances(gpu_lib, oracle_mod, repeat_tol, enum_tol):
    seqs = _repeat_case(oracle_mod, 5, TILE + HALF + 1)
    ref = _check_matchlist(gpu_lib, oracle_mod, seqs, oracle_mod.get_seed(15), repeat_tol=repeat_tol,
                           enum_tol=enum_tol)
    assert len(ref[0]) > 0


# ---- 8. without the LDS genome lookup ---------------------------------------------------------
def test_no_genome_lookup_heads(gpu_lib, oracle_mod, monkeypatch):
    monkeypatch.setenv("MUMS_DEV_NO_GL", "1")   # (read when the context adds its genomes)
    _check(gpu_lib, oracle_mod, _copies(oracle_mod, 8, 3000, 0.005, 61), oracle_mod.get_seed(15))


def test_no_genome_lookup_oversize(gpu_lib, oracle_mod, monkeypatch):
    monkeypatch.setenv("MUMS_DEV_NO_GL", "1")
    _check(gpu_lib, oracle_mod, _repeat_case(oracle_mod, 5, TILE + HALF + 1), oracle_mod.get_seed(15))
