"""Inputs of tests/test_gpu_chain_paths.py (test data only): rearranged genomes at every
genome-count class of the chain stage (MG = 8, 16, 32, 64; MG = 4 stays with
rearranged_inputs' ev_G4_w15 and ls_G3_x40k_w15).

  * evolved cases: rearranged_inputs.evolved(G, n, seed=100 + G), default rates, under four
    seeds -- w13 ranks 0 and 1 (odd weight, palindromic like every w13 pattern: the lean
    walks), w12 rank 0 (even weight, palindromic: the generic hit words, whose word-wide
    comparison is followed by the exact test of the self-reverse-complement windows) and w19
    rank 2 (non-palindromic: the generic hit words column by column, hit_word's !bitpar branch;
    a reverse homology shares no seed with the forward strand, so these runs hold next to no
    reverse component);
  * stretch cases: rearranged_inputs.long_stretch(G, 22000, seed=200 + G), w15 rank 0: walks of
    22 000 columns, past the 16 896 the short and the 16-lane tier cover, so they end in the
    whole-wave launch; with xmut=6 and w12 the same through the even-weight generic hit words,
    over columns where the genomes differ (the 6 substitutions per genome fall between hits
    less than a seed length apart, so the all-genome chains still cross the whole of X).

CASES maps a name to (generator, options); options: kind, G, w, rank, and for the stretch
cases xlen and xmut.  The genomes of a (G, n) shape are generated once and shared by its
seeds; oracle_result() computes the oracle's MatchList once per process.  Every case runs with
table size 40000 and the default tolerances.  tests/test_chain_path_cases_cpu.py holds the
conditions the GPU tests rely on.
"""
from __future__ import annotations

from tests import rearranged_inputs as ri

TABLE_SIZE = 40000
EVOLVED_SHAPES = [(6, 15000), (8, 15000), (12, 12000), (16, 10000), (20, 10000), (32, 8000), (36, 8000), (64, 6000)]
# (suffix, weight, rank)
EVOLVED_SEEDS = [("w13", 13, 0), ("w13r1", 13, 1), ("w12", 12, 0), ("w19r2", 19, 2)]
STRETCH_G = [6, 12, 20, 36, 64]
STRETCH_XMUT_G = [12, 36]
XLEN = 22000

_genomes: dict = {}


def _shared(key, make):
    if key not in _genomes:
        _genomes[key] = make()
    return _genomes[key]


def _cases():
    c = {}
    for G, n in EVOLVED_SHAPES:
        for suffix, w, rank in EVOLVED_SEEDS:
            c[f"ev_G{G}_{suffix}"] = (lambda G=G, n=n: _shared(("ev", G, n), lambda: ri.evolved(G, n, seed=100 + G)),
                                      dict(kind="evolved", G=G, w=w, rank=rank))
    for G in STRETCH_G:
        c[f"ls_G{G}_w15"] = (lambda G=G: _shared(("ls", G, 0), lambda: ri.long_stretch(G, XLEN, seed=200 + G)),
                             dict(kind="stretch", G=G, w=15, rank=0, xlen=XLEN, xmut=0))
    for G in STRETCH_XMUT_G:
        c[f"ls_G{G}_w12_xmut6"] = (lambda G=G: _shared(("ls", G, 6),
                                                       lambda: ri.long_stretch(G, XLEN, seed=200 + G, xmut=6)),
                                   dict(kind="stretch", G=G, w=12, rank=0, xlen=XLEN, xmut=6))
    return c


CASES = _cases()
EVOLVED = [k for k, v in CASES.items() if v[1]["kind"] == "evolved"]
STRETCH = [k for k, v in CASES.items() if v[1]["kind"] == "stretch" and not v[1]["xmut"]]
STRETCH_XMUT = [k for k, v in CASES.items() if v[1]["kind"] == "stretch" and v[1]["xmut"]]

_memo: dict = {}


def oracle_result(oracle, name):
    """(seqs, seed, lengths, starts, stats) of a case from the oracle, computed once per process
    and shared (read-only) by the tests that need it."""
    if name not in _memo:
        gen, opts = CASES[name]
        seqs = gen()
        seed = oracle.get_seed(opts["w"], opts["rank"])
        lengths, starts, st = oracle.find_matches(seqs, seed, table_size=TABLE_SIZE)
        for a in (lengths, starts):
            a.setflags(write=False)
        _memo[name] = (seqs, seed, lengths, starts, st)
    return _memo[name]


def genome_class(G: int) -> int:
    """MG of find_rows_dispatch: the genome-count class whose kernels a G-genome find runs."""
    return next(mg for mg in (4, 8, 16, 32, 64) if G <= mg)


def seed_is_lean(seed: int, L: int) -> bool:
    """chains.hip's seed_bitpar_odd: a palindromic care set of odd weight (every window of the
    walks is then tested by base comparison, hit_word<MG, false>)."""
    if seed == 0 or not 0 < L <= 64:
        return False
    pat = seed >> ((seed & -seed).bit_length() - 1)
    bits = [(pat >> k) & 1 for k in range(L)]
    return pat >> L == 0 and bits == bits[::-1] and bin(seed).count("1") % 2 == 1
