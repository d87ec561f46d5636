"""Rearranged genomes (test data only): many lines, long walks.

The other generators of the suite (oracle.generate, repeat_inputs, tie_inputs) give collinear
genomes: one random sequence with substitutions and at most one whole-genome reverse
complement, so nearly every chain lies on offset 0 and the MatchList has a dozen lines.  Here:

  * evolved(): genome 0 iid random; every other genome is genome 0 after substitutions, block
    inversions, translocations, segmental duplications, short tandem arrays and ~150 indels, so
    that almost every match sits on a diagonal of its own (hundreds to thousands of lines);
  * long_stretch(): a shared stretch X that occurs twice per genome (no seed inside it is
    unique, so under the default tolerances it holds no probe) next to shared unique flanks:
    the probes of a flank extend through a whole copy of X, a walk of xlen columns;
  * line_key() / count_lines(): the line of a match -- genome set, strands, diagonals.

CASES maps a name to (generator, options) in the style of tie_inputs.CASES; options are
find_matches keyword arguments plus w (seed weight), rank (seed rank), cls (MemHash /
MaskedMemHash / PairwiseMatchFinder / ParallelMemHash), kind ("evolved" / "stretch") and for
the stretch cases xlen.  numpy only, fixed seeds, ACGT only.
"""
from __future__ import annotations

import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.zeros(256, dtype=np.uint8)
for _x, _y in zip(b"ACGT", b"TGCA"):
    _COMP[_x] = _y


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, int(n))]


def revcomp(s: np.ndarray) -> np.ndarray:
    return _COMP[s[::-1]]


def _substitute(rng, s, p):
    hit = rng.random(len(s)) < p
    s = s.copy()
    s[hit] = _ACGT[rng.integers(0, 4, int(hit.sum()))]
    return s


def evolved(G, n, seed, p=0.02, inversions=3, translocations=3, duplications=2, tandems=2, indels=150,
            block=(200, 3000), dup=(100, 800), rc=True):
    """G genomes of about n bases: genome 0 iid random, every other one genome 0 changed by, in
    this order, substitutions at rate p, block inversions (reverse complement in place),
    translocations (cut and paste elsewhere), segmental duplications (copy to another place),
    tandem arrays (unit 2-11 bp, 10-60 copies) and indels of 1-29 bp; genome 2 is
    reverse-complemented whole.  `block` bounds the inverted / moved blocks (shrunk for short
    genomes), `dup` the duplicated ones."""
    rng = np.random.default_rng(seed)
    base = _rand(rng, n)
    out = [base]
    hi = max(min(block[1], n // 4), 4)
    lo = min(block[0], hi // 2)
    dhi = max(min(dup[1], n // 4), 4)
    dlo = min(dup[0], dhi // 2)
    for g in range(1, G):
        s = _substitute(rng, base, p)
        for _ in range(inversions):
            ln = int(rng.integers(lo, hi + 1))
            a = int(rng.integers(0, len(s) - ln + 1))
            s[a:a + ln] = revcomp(s[a:a + ln])
        for _ in range(translocations):
            ln = int(rng.integers(lo, hi + 1))
            a = int(rng.integers(0, len(s) - ln + 1))
            blk = s[a:a + ln].copy()
            s = np.concatenate([s[:a], s[a + ln:]])
            c = int(rng.integers(0, len(s) + 1))
            s = np.concatenate([s[:c], blk, s[c:]])
        for _ in range(duplications):
            ln = int(rng.integers(dlo, dhi + 1))
            a = int(rng.integers(0, len(s) - ln + 1))
            blk = s[a:a + ln].copy()
            c = int(rng.integers(0, len(s) + 1))
            s = np.concatenate([s[:c], blk, s[c:]])
        for _ in range(tandems):
            unit = _rand(rng, int(rng.integers(2, 12)))
            arr = np.tile(unit, int(rng.integers(10, 61)))
            c = int(rng.integers(0, len(s) + 1))
            s = np.concatenate([s[:c], arr, s[c:]])
        for _ in range(indels):
            ln = int(rng.integers(1, 30))
            c = int(rng.integers(0, len(s) - ln))
            if rng.random() < 0.5:
                s = np.concatenate([s[:c], _rand(rng, ln), s[c:]])
            else:
                s = np.concatenate([s[:c], s[c + ln:]])
        if rc and g == 2:
            s = revcomp(s)
        out.append(s)
    return [s.tobytes() for s in out]


def long_stretch(G, xlen, seed, flank=2000, own=3000, xmut=0, bridge=False):
    """Every genome is own_g + U1 + X + own_g' + X + U2 + own_g'' (bridge: own_g + U1 + X + U2 +
    own_g' + X + own_g''): U1, U2 (flank bp) and X (xlen bp) are shared by all genomes, the own
    pieces are random per genome, genome 2 is reverse-complemented.  Every seed inside X occurs
    twice per genome, so X holds no probe under the default tolerances: the probes of U1 extend
    right through the first copy of X and those of U2 left through the second (bridge: one chain
    has probes on both sides of the first copy).  xmut: that many substitutions (to another
    base) at random places of X in the genomes other than 0, the same in both copies."""
    rng = np.random.default_rng(seed)
    u1, u2, x = _rand(rng, flank), _rand(rng, flank), _rand(rng, xlen)
    out = []
    for g in range(G):
        xg = x
        if xmut and g > 0:
            xg = x.copy()
            at = rng.choice(xlen, size=xmut, replace=False)
            xg[at] = _ACGT[(np.searchsorted(_ACGT, xg[at]) + rng.integers(1, 4, xmut)) % 4]
        o = [_rand(rng, own) for _ in range(3)]
        if bridge:
            s = np.concatenate([o[0], u1, xg, u2, o[1], xg, o[2]])
        else:
            s = np.concatenate([o[0], u1, xg, o[1], xg, u2, o[2]])
        if g == 2:
            s = revcomp(s)
        out.append(s.tobytes())
    return out


def line_key(length, starts_row):
    """The line of a match: (genome set, strand per component, diagonal per component relative
    to the first defined start); for a reverse component the diagonal is start - ref - length."""
    length = int(length)
    comps = [(g, int(s)) for g, s in enumerate(starts_row) if s != 0]
    ref = comps[0][1]
    return (tuple(g for g, _ in comps), tuple(s < 0 for _, s in comps),
            tuple(s - ref - (length if s < 0 else 0) for _, s in comps))


def count_lines(lengths, starts) -> int:
    return len({line_key(ln, row) for ln, row in zip(np.asarray(lengths).tolist(), np.asarray(starts).tolist())})


def _cases():
    c = {}

    def ev(name, G, n, seed, opts, **kw):
        c[name] = (lambda: evolved(G, n, seed, **kw), dict(kind="evolved", **opts))

    ev("ev_G3_w15", 3, 30_000, 1, dict(w=15))
    ev("ev_G4_w11", 4, 40_000, 2, dict(w=11))
    ev("ev_G4_w15", 4, 40_000, 3, dict(w=15))
    ev("ev_G4_w15_t7", 4, 40_000, 3, dict(w=15, table_size=7))
    ev("ev_G4_w15_t1", 4, 40_000, 4, dict(w=15, table_size=1))
    ev("ev_G3_w25", 3, 30_000, 5, dict(w=25))
    ev("ev_G4_w31", 4, 40_000, 6, dict(w=31))
    ev("ev_G3_w27", 3, 30_000, 14, dict(w=27))
    ev("ev_G5_w13_rtol2_etol2", 5, 30_000, 7, dict(w=13, repeat_tol=2, enum_tol=2))
    ev("ev_G3_w15_rtol3_etol9", 3, 30_000, 8, dict(w=15, repeat_tol=3, enum_tol=9))
    ev("ev_G4_w15_pairwise", 4, 30_000, 9, dict(w=15, cls="PairwiseMatchFinder"))
    ev("ev_G3_w15_compat", 3, 30_000, 10, dict(w=15, cls="ParallelMemHash", chunk_size=3000))
    # (only the seeds of genomes {0, 1, 3} exactly are hashed: more indels for 300 lines)
    ev("ev_G4_w15_masked", 4, 40_000, 11, dict(w=15, cls="MaskedMemHash", seq_mask=0b1011), indels=450)
    ev("ev_G9_w13", 9, 20_000, 12, dict(w=13))
    ev("ev_G4_w19_rank2", 4, 30_000, 13, dict(w=19, rank=2))
    # (two genomes, one pair of strands: more inversions and indels for 300 lines / 100 reverse matches)
    ev("ev_G2_w15", 2, 40_000, 15, dict(w=15), inversions=30, indels=500)

    def ls(name, G, xlen, seed, w, **kw):
        c[name] = (lambda: long_stretch(G, xlen, seed, **kw),
                   dict(kind="stretch", w=w, xlen=xlen, bridge=bool(kw.get("bridge"))))

    ls("ls_G3_x40k_w15", 3, 40_000, 21, 15)
    ls("ls_G2_x40k_w19", 2, 40_000, 22, 19)
    ls("ls_G3_x40k_w15_xmut6", 3, 40_000, 23, 15, xmut=6)
    ls("ls_G4_x70k_w11", 4, 70_000, 24, 11)
    ls("ls_G3_x40k_w15_bridge", 3, 40_000, 25, 15, bridge=True)
    return c


CASES = _cases()
EVOLVED = sorted(k for k, v in CASES.items() if v[1]["kind"] == "evolved")
STRETCH = sorted(k for k, v in CASES.items() if v[1]["kind"] == "stretch")


def oracle_kwargs(opts):
    """find_matches keyword arguments of the oracle for a case's options."""
    cls = opts.get("cls", "MemHash")
    return dict(repeat_tol=opts.get("repeat_tol", 0), enum_tol=opts.get("enum_tol", 1),
                table_size=opts.get("table_size", 40000),
                masked=cls == "MaskedMemHash", seq_mask=opts.get("seq_mask", 0),
                pairwise=cls == "PairwiseMatchFinder", parallel_compat=cls == "ParallelMemHash",
                chunk_size=opts.get("chunk_size", 0))


def is_default_memhash(opts) -> bool:
    """MemHash with the default tolerances (the table size may differ)."""
    return (opts.get("cls", "MemHash") == "MemHash" and opts.get("repeat_tol", 0) == 0
            and opts.get("enum_tol", 1) == 1)


_memo: dict = {}


def oracle_result(oracle, name):
    """(seqs, seed, lengths, starts, stats) of a case from the oracle, computed once per process
    and shared (read-only) by the tests that need it."""
    if name not in _memo:
        gen, opts = CASES[name]
        seqs = gen()
        seed = oracle.get_seed(opts["w"], opts.get("rank", 0))
        lengths, starts, st = oracle.find_matches(seqs, seed, **oracle_kwargs(opts))
        for a in (lengths, starts):
            a.setflags(write=False)
        _memo[name] = (seqs, seed, lengths, starts, st)
    return _memo[name]


def batch_problems():
    """40 evolved two-genome problems of 0.5-3 kbp (the counts scaled to the length)."""
    rng = np.random.default_rng(77)
    out = []
    for k in range(40):
        n = int(rng.integers(500, 3001))
        out.append(tuple(evolved(2, n, 1000 + k, inversions=1, translocations=1, duplications=1, tandems=1,
                                 indels=max(n // 200, 2))))
    return out


FAMILY_CASE = "ev_G3_w15"
OVERLAP_CASE = "ev_G4_w11"


def family_rounds(oracle, ranks=(0, 1, 2)):
    """[(sequences, seed pattern, find_matches keywords)] of one seed family on FAMILY_CASE: the
    round format of tests/seed_family_cases.py."""
    seqs = oracle_result(oracle, FAMILY_CASE)[0]
    w = CASES[FAMILY_CASE][1]["w"]
    return [(seqs, oracle.get_seed(w, r), dict(table_size=40000)) for r in ranks]


# ---- probe-free stretches of the long-stretch cases ------------------------------------------
# chains.hip's walk tiers: chain_walk_short_kernel covers MUMS_WALK_BUDGET = 8 words of 64 columns;
# the 16-lane chain_walk_kernel then runs MUMS_WALK_HANDOFF = 16 steps of MUMS_WALK_GROUP = 16
# words before it hands the walk to the whole-wave launch: 512 + 16 * 16 * 64 = 16 896 columns.
WALK_BUDGET, WALK_GROUP, WALK_HANDOFF = 8, 16, 16
TIER_COLUMNS = WALK_BUDGET * 64 + WALK_HANDOFF * WALK_GROUP * 64
STRETCH_SLACK = 4000


def probe_positions(oracle, seqs, seed, table_size=40000):
    """Per genome g the sorted 0-based positions of the probes (of oracle.seed_probes) whose
    first start lies in g (ref = global seed-mer index, genome bases = cumulative SMLLength)."""
    _, ref, _ = oracle.seed_probes(seqs, seed, table_size=table_size)
    L = oracle.lib().oracle_seed_length(seed)
    base = np.concatenate([[0], np.cumsum([max(len(s) - L + 1, 0) for s in seqs])]).astype(np.int64)
    ref = np.sort(ref.astype(np.int64))
    return [ref[(ref >= base[g]) & (ref < base[g + 1])] - base[g] for g in range(len(seqs))]


def stretches(oracle, name):
    """Per match of length >= xlen of a long-stretch case: (match index, longest probe-free run
    of columns inside the match in its reference genome -- the first defined component, always
    forward --, probes left of it, probes right of it)."""
    seqs, seed, lengths, starts, _ = oracle_result(oracle, name)
    return stretches_of(oracle, seqs, seed, lengths, starts, CASES[name][1]["xlen"])


def stretches_of(oracle, seqs, seed, lengths, starts, min_len, table_size=40000):
    """stretches() of any MatchList: the matches of length >= min_len."""
    per_genome = probe_positions(oracle, seqs, seed, table_size)
    out = []
    for i in np.nonzero(lengths >= min_len)[0]:
        g = int(np.argmax(starts[i] != 0))
        s0 = int(starts[i, g])
        assert s0 > 0   # SetDirection: the first defined component is forward
        pos = per_genome[g]
        a, b = s0 - 1, s0 - 1 + int(lengths[i])
        inside = pos[(pos >= a) & (pos < b)]
        edges = np.concatenate([[a - 1], inside, [b]])
        gaps = np.diff(edges) - 1
        k = int(np.argmax(gaps))
        out.append((int(i), int(gaps[k]), k, len(inside) - k))
    return out
