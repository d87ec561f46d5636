"""Inputs and shared oracle answers of the ParallelMemHash compat + enumeration tolerance tests
(test_gpu_compat_enum.py, test_gpu_compat_enum_ranks.py): every oracle run happens once."""
import functools

from tests import repeat_inputs


# id: (input, w, repeat_tol, enum_tol, chunk, masked, mask); inputs: ("rep", G, n, p, gseed) =
# generate + two copies of one 4 kbp segment inside every genome (test_gpu_enumerate.py's
# with_repeats), ("hc", G, n, copies, seed) = repeat_inputs.high_copy(tandem=False)
REP_A = ("rep", 3, 200_000, 0.02, 34)
SHAPES = {
    "A": (REP_A, 15, 1, 2, 3000, False, 0),
    "B": (REP_A, 15, 2, 3, 7000, False, 0),
    "C": (("rep", 4, 150_000, 0.03, 35), 15, 1, 2, 2500, False, 0),
    "D": (("rep", 2, 300_000, 0.01, 33), 19, 3, 2, 8000, False, 0),
    "E": (("rep", 4, 120_000, 0.02, 35), 17, 2, 8, 8000, False, 0),
    "F": (REP_A, 15, 1, 2, 3000, True, 7),
    "G": (REP_A, 15, 2, 2, 3000, True, 0),
    "H": (("hc", 3, 60_000, 40, 9), 15, 8, 9, 2000, False, 0),
    "I": (("hc", 3, 60_000, 40, 12), 15, 39, 12, 2000, False, 0),
    "J": (("hc", 4, 60_000, 40, 16), 15, 15, 16, 2000, False, 0),
    "K": (("hc", 3, 60_000, 40, 10), 15, 39, 10, 2000, True, 5),
    # chunks cut at their first group above MER_REPEAT_LIMIT
    "L": (("hc", 4, 300_000, 1500, 8500), 15, 2, 3, 7000, False, 0),
    "M": (("hc", 4, 300_000, 1200, 4200), 11, 1, 2, 3000, False, 0),
}


@functools.lru_cache(maxsize=None)
def make_input(spec):
    from oracle import oracle
    if spec[0] == "rep":
        _, G, n, p, gseed = spec
        seqs = oracle.generate(G, n, p, gseed)
        rep = seqs[0][5000:9000]
        return tuple(s[: n // 3] + rep + s[n // 3 + 4000: 2 * n // 3] + rep + s[2 * n // 3 + 4000:] for s in seqs)
    _, G, n, copies, seed = spec
    return tuple(repeat_inputs.high_copy(G=G, n=n, copies=copies, tandem=False, seed=seed))


@functools.lru_cache(maxsize=None)
def oracle_answer(spec, w, rt, et, chunk, masked, mask, table_size=40000, compat=True):
    """One oracle run per (input, settings), shared by the tests (the arrays are only read)."""
    from oracle import oracle
    return oracle.find_matches(list(make_input(spec)), oracle.get_seed(w), repeat_tol=rt, enum_tol=et,
                               table_size=table_size, masked=masked, seq_mask=mask, parallel_compat=compat,
                               chunk_size=chunk if compat else 0)
