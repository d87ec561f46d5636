"""Writes ref_cases.json: the answers of libMems itself for every case of tests/ref_cases.py.

Each case goes through oracle/_ref/ref_driver (oracle/ref_driver.cpp linked with the reference's
own translation units; `make -C oracle` builds it where the libMems tree is present) twice; the
file is written only if both runs agree on every case.  Per case: the sha256 of the driver's case
file, and per section of the output (lists in GetMatchList order, counters, logs) its line count,
a digest (of the text or, for lists, seed_family_cases.list_md5); the text itself up to 200 lines,
else the first and last three.  The whole list of one case is also written to ref_enum3_list.txt:
it is the input of the enum3 overlap cases.

    python tests/golden/make_ref_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ref_cases as rc   # noqa: E402


def main():
    if not rc.have_driver():
        sys.exit(f"{rc.DRIVER} is missing: run `make -C oracle` with the libMems tree present")
    cases = {}
    for name in rc.CASES:
        first, second = rc.run_driver(name), rc.run_driver(name)
        if name == rc.ENUM3_SOURCE:   # the input of the enum3 overlap cases, which come later in the list
            with open(rc.ENUM3_ROWS, "w") as f:
                f.write("".join(ln + "\n" for ln in first["list"]))
            rc.enum3_list.cache_clear()
        if first != second:
            sys.exit(f"{name}: two runs of the reference differ; nothing written")
        cases[name] = rc.record(name, first)
        print(name, {sec: r["count"] for sec, r in cases[name]["sections"].items()})
    with open(rc.FIXTURE, "w") as f:
        # one case per line
        f.write('{"source": "libMems through oracle/ref_driver.cpp via tests/golden/make_ref_golden.py",\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True, separators=(',', ':'))}" for k, v in cases.items()))
        f.write("\n}}\n")
    print(os.path.getsize(rc.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
