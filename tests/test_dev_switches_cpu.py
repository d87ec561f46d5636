"""The development switches of the product library, kept in step with DESIGN.md.

Every `MUMS_DEV_*` environment variable the library reads is listed in the "Development
switches" table of DESIGN.md (§5n), and the table lists nothing else: a switch added without a
row, or a row left behind by a removed switch, fails here.  The A/B variants pruned in §5n --
their switches and the build macros that selected them -- stay out of the library, the tests
and the tools; git history has them."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# whole names: MUMS_DEV_SEGFIX lost two values only and stays a switch
REMOVED_SWITCHES = [
    "OS_VARIANT", "OS_XD", "OS_XCD", "LINE_GHIST", "LINE_ORD", "LINE_NORUNS", "LINE_GATHER", "WALK_REFILL",
    "WALK_SORT", "WALK_SHIFT", "PACK_LINEAR", "PROBE_GENERAL", "KEEP_BUCKET_ORDER", "BUCKET_ONESWEEP", "MSD_BITS",
    "RS_NOAGG",
]
REMOVED_MACROS = [
    "MUMS_OS_LATEPUB", "MUMS_OS_NEXTHIST", "MUMS_OS_FUSED", "MUMS_OS_CTILES", "MUMS_OS_STATS", "MUMS_SORT_NT",
    "MUMS_SORT_PERSIST", "MUMS_SORT_BLOCK", "MUMS_SORT_TILE", "MUMS_WALK_SWZ", "MUMS_WALK_REFILL_MIN",
    "MUMS_WALK_SORT_SHIFT",
]


def _files(*patterns):
    out = []
    for p in patterns:
        out += [f for f in glob.glob(os.path.join(ROOT, p), recursive=True) if os.path.isfile(f)]
    return sorted(set(out))


def _library_sources():
    return _files("libmems_amd/csrc/*", "include/*")


def _table_names():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^\*\*Development switches\.\*\*[^|]*\n((?:\|[^\n]*\n)+)", text, re.M)
    assert m, "DESIGN.md has no 'Development switches' table"
    rows = m.group(1).splitlines()[2:]   # header, rule
    names = [re.match(r"\|\s*`(MUMS_DEV_[A-Z0-9_]+)`\s*\|", r) for r in rows]
    assert all(names), [r for r, n in zip(rows, names) if not n]
    cells = [[c.strip() for c in r.strip().strip("|").split("|")] for r in rows]
    kinds = {"forces a product path", "alternative implementation", "diagnostics"}
    assert all(len(c) == 4 and c[1] in kinds and c[2] and c[3] for c in cells), cells
    return [n.group(1) for n in names]


def test_switch_table_lists_what_the_library_reads():
    read = set()
    for f in _library_sources():
        read |= set(re.findall(r"MUMS_DEV_[A-Z0-9_]+", open(f, errors="replace").read()))
    listed = _table_names()
    assert len(listed) == len(set(listed)), "a switch is listed twice"
    assert set(listed) == read, {"not in DESIGN.md": sorted(read - set(listed)),
                                 "not in the library": sorted(set(listed) - read)}


def test_tests_named_in_the_table_set_the_switch():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, test in re.findall(r"^\|\s*`(MUMS_DEV_[A-Z0-9_]+)`\s*\|[^|]*\|[^|]*\|\s*([^|]*?)\s*\|$", text, re.M):
        if test == "no test":
            continue
        for t in re.findall(r"`([^`]+)`", test):
            assert re.search(name + r"\b", open(os.path.join(ROOT, "tests", t)).read()), (name, t)


def test_product_paths_and_alternatives_have_a_test():
    """A switch that forces a product path or selects an alternative implementation exists to be
    set by a test: only a diagnostics row may say "no test"."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    rows = re.findall(r"^\|\s*`(MUMS_DEV_[A-Z0-9_]+)`\s*\|\s*([^|]*?)\s*\|[^|]*\|\s*([^|]*?)\s*\|$", text, re.M)
    assert len(rows) == len(_table_names())
    untested = [name for name, kind, test in rows if kind != "diagnostics" and not re.findall(r"`[^`]+\.py`", test)]
    assert not untested, untested
    assert not [name for name, kind, test in rows if "no test" in test and kind != "diagnostics"]


def test_pruned_variants_stay_out():
    where = _files("libmems_amd/**", "include/**", "tests/*.py", "tools/*.py", "tools/*.sh", "tools/*.cpp",
                   "tools/dev/**")
    where = [f for f in where if os.path.abspath(f) != os.path.abspath(__file__) and
             not f.endswith((".so", ".o", ".pyc"))]
    assert len(where) > 50
    gone = ["MUMS_DEV_" + s for s in REMOVED_SWITCHES] + REMOVED_MACROS
    pat = re.compile(r"(?<![A-Za-z0-9_])(" + "|".join(gone) + r")(?![A-Za-z0-9_])")
    hits = {}
    for f in where:
        found = set(pat.findall(open(f, errors="replace").read()))
        if found:
            hits[os.path.relpath(f, ROOT)] = sorted(found)
    assert not hits, hits
    # the two wrong-result timing modes of the segment fix-up are gone, modes 1 and 2 stay
    seg = open(os.path.join(ROOT, "libmems_amd", "csrc", "radix_seg.hip")).read()
    assert "MUMS_DEV_SEGFIX" in seg and "results wrong" not in seg
    assert not re.search(r"e\[0\] == '[34]'", seg)
