"""mums::MemHash::FindMatchesBatch (include/mums_memhash.hpp) through the C++ host tool: the
batch's lists equal a loop of Clear + FindMatches with the same default seeds."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools")], check=True)
    return os.path.join(ROOT, "tools", "mums_find")


def test_cpp_batch_equals_loop(tool):
    """8 problems of 2 x (24000 / (k + 1)) bases, 4 % substitutions: default weights 11, 9 and 7."""
    r = subprocess.run([tool, "batch", "8", "24000", "0.04"], check=True, capture_output=True, timeout=120)
    batch, loop = r.stdout.decode().split("== loop\n")
    assert batch == loop
    assert batch.count("# problem") == 8
    per_problem = [len(part.strip().splitlines()) - 1 for part in batch.split("# problem")[1:]]
    assert all(n > 0 for n in per_problem), per_problem
    assert b"problems 8 probes " in r.stderr and int(r.stderr.split()[-1]) > 1000
