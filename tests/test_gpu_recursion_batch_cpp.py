"""mums::MemHash::RecursionBatch / RecursionTailBatch (include/mums_memhash.hpp) through the C++
host tool, on three problems of R200 (tests/recursion_batch_cases.py): the batch's lists equal the
fixture, the loop of Aligner::Recursion's calls on one object, and the tail batch over the problems'
tables."""
import os
import subprocess

import numpy as np
import pytest

import recursion_batch_cases as rb
from conftest import ROOT

pytestmark = pytest.mark.gpu

G = 4
WEIGHTS = (9, 9, 9, 7)   # Aligner.cpp:1142-1203 on these: one round at 9, one at 7


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools")], check=True)
    return os.path.join(ROOT, "tools", "mums_find")


def parse(text):
    """[(lengths, starts)] per "# problem k" block of the tool's output."""
    out = []
    for part in text.split("# problem")[1:]:
        rows = [[int(v) for v in line.split("\t")] for line in part.strip().splitlines()[1:]]
        a = np.asarray(rows, dtype=np.int64).reshape(len(rows), G + 1)
        out.append((a[:, 0].astype(np.uint64), a[:, 1:]))
    return out


@pytest.mark.parametrize("nway,variant", [(0, "m0"), (1, "mG")])
def test_cpp_recursion_batch_on_three_r200_problems(tool, tmp_path, nway, variant):
    case, recorded = rb.find_case("r200"), rb.fixture()["find"]["r200"][variant]
    assert rb.rounds_model(WEIGHTS, bool(nway)) == ([9, 7] if not nway else [7])
    # nway_only searches these weights at 7 alone: the fixture's rounds are the C call's, so only
    # the run without nway_only is held to the fixture; with it the three outputs are held to each other
    pats = rb.patterns_of((9, 7))
    picks = [p for p in range(200) if len(case["problems"][p]) == G and case["patterns"][p] == pats
             and recorded[p]["count"] > 0][:3]
    assert len(picks) == 3
    args = []
    for p in picks:
        for g, s in enumerate(case["problems"][p]):
            path = tmp_path / f"p{p}_{g}.txt"
            path.write_bytes(s + b"\n")
            args.append(str(path))
    r = subprocess.run([tool, "recursion", "files", str(G), str(nway), ",".join(str(w) for w in WEIGHTS)] + args, check=True,
                       capture_output=True, timeout=120)
    batch, rest = r.stdout.decode().split("== loop\n")
    loop, tail = rest.split("== tail\n")
    assert batch == loop == tail
    lists = parse(batch)
    assert len(lists) == 3 and sum(len(l) for l, _ in lists) > 0
    if not nway:
        for p, (l, s) in zip(picks, lists):
            assert len(l) == recorded[p]["count"] and rb.sf.list_md5(l, s) == recorded[p]["list_md5"], p
        entries = sum(recorded[p]["table_entries"] for p in picks)
        assert r.stderr.decode().strip().endswith(f"problems 3 table entries {entries}")
    else:
        assert all((s != 0).all() for _, s in lists)
