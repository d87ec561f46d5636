"""Every row form, line order and walk form of the chain stage (chains.hip launch_chains) at
every genome-count class, bit for bit against the oracle, with the path each call took read
from the library's own report.

Per case (tests/chain_path_cases.py, plus the G <= 4 cases of tests/rearranged_inputs.py): one
context, the sequences added once, then CreateMatches per variant with the development
switches set per call.  The variants are the full product of

  rows   default | WIDE_ROWS=1 | WIDE_ROWS=retry | FIND_CHUNK=c | FIND_CHUNK=c + WIDE_LINE_ROWS=1 |
         FIND_CHUNK=c + WIDE_LINE_ROWS=retry          (c = a quarter of the oracle's probe count)
  order  default (onesweep records) | LINE_RADIX (64-bit pairs) | LINE_EXACT | both
  walks  default | WALK_GEN=1 (only where the default is the lean form, rank-0 seeds); the w12
         (even weight) and w19 rank 2 (non-palindromic) cases are generic with no switch set

and each runs twice: plain, and under MUMS_DEV_CHAIN_DEBUG, whose stderr lines

  chains: probe rows <int32|int64>                          (one-pass path: each materialize pass)
  chains: path MG <m> P <p> rows <int32|int32-gathered|int64> order <records|pairs|exact> walks <lean|generic>
  chains: pass <0|1> walks <n>, long <n> (to whole waves <n>) of <p> probes; ...

say which kernels ran.  The expected lines are derived here from G, the seed and the variant,
mirroring materialize_dispatch (mums_capi.hip) and launch_chains: a variant that silently fell
back to the default path fails.  What the mirror says about the switches:

  * WIDE_ROWS=1 / retry act in materialize_dispatch (G <= 16): the probe rows come out 64-bit
    ("probe rows int64"; retry: "int32" then "int64"); launch_chains then gathers them to int32
    line rows (gather_line_rows_kernel), so its path line says int32-gathered, not int64.
  * WIDE_LINE_ROWS acts in launch_chains on 64-bit rows only, i.e. with the sliced path here:
    "1" gives int64 line rows, "retry" the int32-gathered labelling and then the int64 one.
  * At G > 16 every row is 64-bit and both retry values do nothing: those variants repeat the
    plain int64 path (asserted as such; they add no coverage above 16 genomes).
  * LINE_EXACT adds one labelling in the exact order after the others, on the last row form.

Durations on an MI355X: 0.15-2.9 s per case, except the two even-weight stretch cases
(ls_G12_w12_xmut6 8.4 s, ls_G36_w12_xmut6 25 s): with a reverse component an even-weight seed
re-tests every hit column of a walk word (hit_word's self-reverse-complement check), 132 ms per
chain labelling at G = 36, and the sliced variants label every slice.  Their X cannot be much
shorter: the walks must pass the 16 896 columns of the first two tiers.
"""
import itertools
import re

import pytest

from tests import chain_path_cases as cp
from tests import rearranged_inputs as ri
from tests.test_gpu_rearranged import assert_parity

pytestmark = pytest.mark.gpu

SMALL_G = ["ev_G4_w15", "ls_G3_x40k_w15"]   # (rearranged_inputs.CASES: MG = 4)
ALL = cp.EVOLVED + cp.STRETCH + cp.STRETCH_XMUT + SMALL_G


def load_case(oracle_mod, name):
    """(G, rank, seqs, seed, (lengths, starts, stats), is a whole-X stretch case)"""
    if name in cp.CASES:
        opts = cp.CASES[name][1]
        seqs, seed, lengths, starts, ost = cp.oracle_result(oracle_mod, name)
    else:
        opts = ri.CASES[name][1]
        assert ri.is_default_memhash(opts) and opts.get("table_size", 40000) == cp.TABLE_SIZE
        seqs, seed, lengths, starts, ost = ri.oracle_result(oracle_mod, name)
    stretch = opts["kind"] == "stretch"   # the xmut cases too: their all-genome chains cross X
    return len(seqs), opts.get("rank", 0), seqs, seed, (lengths, starts, ost), stretch


def variants(chunk, lean_seed, rank):
    c = str(chunk)
    rows = [{}, {"MUMS_DEV_WIDE_ROWS": "1"}, {"MUMS_DEV_WIDE_ROWS": "retry"}, {"MUMS_DEV_FIND_CHUNK": c},
            {"MUMS_DEV_FIND_CHUNK": c, "MUMS_DEV_WIDE_LINE_ROWS": "1"},
            {"MUMS_DEV_FIND_CHUNK": c, "MUMS_DEV_WIDE_LINE_ROWS": "retry"}]
    order = [{}, {"MUMS_DEV_LINE_RADIX": "1"}, {"MUMS_DEV_LINE_EXACT": "1"},
             {"MUMS_DEV_LINE_RADIX": "1", "MUMS_DEV_LINE_EXACT": "1"}]
    walks = [{}, {"MUMS_DEV_WALK_GEN": "1"}] if lean_seed and rank == 0 else [{}]
    return [{**r, **o, **w} for r, o, w in itertools.product(rows, order, walks)]


def expected_path(G, lean_seed, var):
    """(materialize lines, (rows, order) of the labellings of one slice or of the whole call,
    walk form, whether a retry value was set that does nothing) for a variant."""
    sliced = "MUMS_DEV_FIND_CHUNK" in var
    wide_rows, wide_line = var.get("MUMS_DEV_WIDE_ROWS"), var.get("MUMS_DEV_WIDE_LINE_ROWS")
    noop = False
    if sliced:   # 64-bit rows, materialized outside the one-pass path (no "probe rows" line)
        mat = []
        if G > 16 or wide_line == "1":
            forms = ["int64"]
            noop = G > 16 and wide_line == "retry"
        elif wide_line == "retry":
            forms = ["int32-gathered", "int64"]
        else:
            forms = ["int32-gathered"]
    elif G > 16:
        mat, forms, noop = ["int64"], ["int64"], wide_rows == "retry"
    elif wide_rows is None:
        mat, forms = ["int32"], ["int32"]
    else:
        mat = ["int64"] if wide_rows == "1" else ["int32", "int64"]
        forms = ["int32-gathered"]
    first = "pairs" if "MUMS_DEV_LINE_RADIX" in var else "records"
    calls = [(f, first) for f in forms]
    if "MUMS_DEV_LINE_EXACT" in var:
        calls.append((forms[-1], "exact"))
    walks = "lean" if lean_seed and var.get("MUMS_DEV_WALK_GEN") != "1" else "generic"
    return mat, calls, walks, noop


_PATH = re.compile(r"^chains: path MG (\d+) P (\d+) rows (\S+) order (\S+) walks (\S+)$")
_PASS = re.compile(r"^chains: pass ([01]) walks (\d+), long (\d+) \(to whole waves (\d+)\) of (\d+) probes;")
_ROWS = re.compile(r"^chains: probe rows (\S+)$")


def parse_report(err):
    """(materialize lines, labellings) of one CreateMatches; a labelling is a dict of its path
    line's fields plus `passes`, the (walks, long, whole) of its two pass lines."""
    mat, calls = [], []
    for line in err.splitlines():
        if m := _ROWS.match(line):
            mat.append(m.group(1))
        elif m := _PATH.match(line):
            calls.append(dict(MG=int(m.group(1)), P=int(m.group(2)), rows=m.group(3), order=m.group(4),
                              walks=m.group(5), passes=[]))
        elif m := _PASS.match(line):
            assert calls and int(m.group(1)) == len(calls[-1]["passes"]) and int(m.group(5)) == calls[-1]["P"], line
            calls[-1]["passes"].append(tuple(int(m.group(k)) for k in (2, 3, 4)))
        else:
            assert not line.startswith("chains: p"), line   # a report line this parser does not know
    return mat, calls


def check_report(err, G, lean_seed, var, probes, chunk, stretch):
    mat, calls = parse_report(err)
    exp_mat, exp_calls, exp_walks, _ = expected_path(G, lean_seed, var)
    assert mat == exp_mat, (var, mat)
    assert calls and all(len(c["passes"]) == 2 for c in calls), var
    assert {c["MG"] for c in calls} == {cp.genome_class(G)}, var
    assert {c["walks"] for c in calls} == {exp_walks}, var
    got = [(c["rows"], c["order"]) for c in calls]
    if "MUMS_DEV_FIND_CHUNK" in var:
        n = len(exp_calls)
        slices = [calls[i:i + n] for i in range(0, len(calls), n)]
        assert len(slices) >= 4 and got == exp_calls * len(slices), (var, got)
        assert all(c["P"] <= chunk and c["P"] == s[0]["P"] for s in slices for c in s), var
        assert sum(s[0]["P"] for s in slices) == probes, var
        assert all(r != "int32" for r, _ in got), var
        rounds = [[s[k] for s in slices] for k in range(n)]
    else:
        assert got == exp_calls, (var, got)
        assert all(c["P"] == probes for c in calls), var
        rounds = [[c] for c in calls]
    if stretch:
        # each of the two all-genome matches is walked through a whole copy of X (22 000 columns
        # and more, past the 16 896 of the first two tiers) from the one flank that holds its
        # probes: in every labelling of all probes, both passes summed, two walks at least
        # leave the short tier and two reach the whole-wave launch
        for r in rounds:
            assert sum(p[1] for c in r for p in c["passes"]) >= 2, (var, r)
            assert sum(p[2] for c in r for p in c["passes"]) >= 2, (var, r)


@pytest.mark.parametrize("name", ALL)
def test_chain_paths(gpu_lib, oracle_mod, monkeypatch, capfd, name):
    G, rank, seqs, seed, ref, stretch = load_case(oracle_mod, name)
    probes = ref[2]["probes"]
    chunk = max(probes // 4, 1)
    lean_seed = cp.seed_is_lean(seed, oracle_mod.lib().oracle_seed_length(seed))
    vs = variants(chunk, lean_seed, rank)
    assert len(vs) == (48 if lean_seed and rank == 0 else 24)
    noops = []
    with gpu_lib.MemHash(0) as mh:
        mh.SetTableSize(cp.TABLE_SIZE)
        mh.SetSeed(seed)
        for s in seqs:
            mh.AddSequence(s)
        for var in vs:
            for debug in (False, True):
                with monkeypatch.context() as m:
                    for k, v in var.items():
                        m.setenv(k, v)
                    if debug:
                        m.setenv("MUMS_DEV_CHAIN_DEBUG", "1")
                    capfd.readouterr()
                    mh.CreateMatches()
                    err = capfd.readouterr().err
                    st = mh.stats()
                    ml = mh.GetMatchList()
                assert_parity(ml, st, ref, {}, (var, debug))
                if debug:
                    check_report(err, G, lean_seed, var, probes, chunk, stretch)
                else:
                    assert "chains:" not in err, var
            if expected_path(G, lean_seed, var)[3]:
                noops.append(var)
    # the retry values above 16 genomes: run and compared, but they repeat the int64 path
    assert len(noops) == (0 if G <= 16 else len(vs) // 3)
    print(f"{name}: G {G}, {probes} probes, {len(vs)} variants x 2 runs, "
          f"{len(noops)} of them retry variants without effect at this G")
