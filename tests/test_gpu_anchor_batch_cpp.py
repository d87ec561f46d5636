"""mums::MemHash::AnchorSearchBatch / AnchorTailBatch (include/mums_memhash.hpp) through the C++
host tool, on three problems of A200 (tests/anchor_batch_cases.py): the batch's anchor lists equal
the fixture, the loop of pairwiseAnchorSearch's calls on one object, and the tail batch over the
problems' family tables."""
import os
import subprocess

import numpy as np
import pytest

import anchor_batch_cases as ab
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools")], check=True)
    return os.path.join(ROOT, "tools", "mums_find")


def parse(text):
    """[(lengths, starts)] per "# problem k" block of the tool's output."""
    out = []
    for part in text.split("# problem")[1:]:
        rows = [[int(v) for v in line.split("\t")] for line in part.strip().splitlines()[1:]]
        a = np.asarray(rows, dtype=np.int64).reshape(len(rows), 3)
        out.append((a[:, 0].astype(np.uint64), a[:, 1:]))
    return out


def test_cpp_anchor_batch_on_three_a200_problems(tool, tmp_path):
    case, recorded = ab.find_case("a200"), ab.fixture()["find"]["a200"]["eb0"]
    weights = [ab.default_weight(p) for p in case["problems"]]
    picks = [next(p for p in range(200) if weights[p] == w and recorded[p]["count"] > 0) for w in (9, 7, 5)]
    args = []
    for p in picks:
        for g, s in enumerate(case["problems"][p]):
            path = tmp_path / f"p{p}_{g}.txt"
            path.write_bytes(s + b"\n")
            args.append(str(path))
    r = subprocess.run([tool, "anchor", "files"] + args, check=True, capture_output=True, timeout=120)
    batch, rest = r.stdout.decode().split("== loop\n")
    loop, tail = rest.split("== tail\n")
    assert batch == loop == tail
    lists = parse(batch)
    assert len(lists) == 3
    for p, (l, s) in zip(picks, lists):
        assert len(l) == recorded[p]["count"] and ab.sf.list_md5(l, s) == recorded[p]["list_md5"], p
    entries = sum(recorded[p]["table_entries"] for p in picks)
    assert r.stderr.decode().strip().endswith(f"problems 3 table entries {entries}")
