"""The cases whose answers are recorded from libMems itself (tests/golden/ref_cases.json).

One list for oracle/ref_driver.cpp (through golden/make_ref_golden.py), test_ref_pinning_cpu.py
and test_gpu_ref_pinning.py.  A case is a dict: mode (a mode of the driver), the driver's keys
(weight, rank, finder, repeat_tol, enum_tol, table_size, mask, start_points, match_log, offset_log,
filters, rounds, eliminate_both, seq_ids, nway_only; whole: a recursion case without rounds, which
the driver runs through the reference's own weight loop and tail), and its input: `seqs` (a function that returns the
genomes as bytes, built by the existing seeded generators) or `rows` (a function that returns the
MatchList (lengths, starts) of an overlap case).  Nothing here reads the reference or the driver;
run_driver() is the only function that needs oracle/_ref/ref_driver.

Where a case gives no sequences of its own: G = 3, n = 40 000, 2 % substitutions, genome 2
reverse-complemented (oracle.generate, the SURVEY Appendix C generator)."""
from __future__ import annotations

import functools
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

import anchor_batch_cases as ab
import recursion_batch_cases as rb
import rearranged_inputs
import repeat_inputs
import seed_family_cases as sf
import test_eliminate_overlaps_v2_cpu as eo2
import tie_inputs
from oracle import oracle
from test_eliminate_overlaps_cpu import random_matchlist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_cases.json")
FULL_TEXT_MAX = 200   # longer sections are recorded by count, md5 and their first and last three lines
N, P = 40_000, 0.02
# the sections that hold matches (`len s0 .. sG-1`): they also get the list digest of
# seed_family_cases.list_md5 (lengths <u8, then starts <i8)
MATCH_SECTIONS = ("list", "table", "overlaps", "match_log", "final")


def is_match_section(name):
    return name in MATCH_SECTIONS or name.startswith("round") or name.startswith("filter_")


# ---- inputs -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def related(G=3, n=N, p=P, seed=12345):
    return tuple(oracle.generate(G, n, p, seed))


def diverged(G, swap=False):
    """5 % substitutions, so that many seeds are missing from one genome; swap: genomes 0 and 1
    change places (every other genome descends from genome 0, so a seed shared by all but the
    ancestor needs the ancestor elsewhere)."""
    s = list(related(G, N, 0.05))
    if swap:
        s[0], s[1] = s[1], s[0]
    return tuple(s)


@functools.lru_cache(maxsize=None)
def evolved():
    """Inversions, translocations, duplications and indels: matches on many diagonals, so the
    bucket of a match, and with it the order of the list, depends on the table size."""
    return tuple(rearranged_inputs.evolved(3, 30_000, 5))


def uneven():
    """Genome lengths 60 000 / 20 000 / 45 000."""
    a, b, c = related(3, 60_000)
    return (a, b[:20_000], c[:45_000])


def sml_input():
    """3 000 bases: poly-A, a tandem repeat, an N run, lower-case and IUPAC letters."""
    rng = np.random.default_rng(8100)
    s = bytearray(ab.rand_seq(rng, 3000))
    s[200:300] = b"A" * 100
    s[600:900] = (bytes(s[600:623]) * 14)[:300]
    s[1200:1260] = b"N" * 60
    s[1500:1700] = bytes(s[1500:1700]).lower()
    for i in rng.integers(1800, 2400, size=80):
        s[i] = b"RYKMSWBDHVNrykmswbdhvn"[int(rng.integers(0, 22))]
    s[2600:2700] = s[100:200]
    return (bytes(s),)


def alphabet():
    """Related genomes with N, lower-case and IUPAC letters sprinkled in (the same rule in every
    genome, own positions per genome) and one lower-case stretch."""
    rng = np.random.default_rng(8200)
    out = []
    for g, seq in enumerate(related(3, 20_000)):
        s = bytearray(seq)
        for i in rng.integers(0, len(s), size=150):
            s[i] = b"NNNRYKMSWBDHVacgtnry"[int(rng.integers(0, 20))]
        s[3000 + 500 * g:5000 + 500 * g] = bytes(s[3000 + 500 * g:5000 + 500 * g]).lower()
        out.append(bytes(s))
    return tuple(out)


def occurrence_input():
    """5 000 bases with a dispersed repeat, a tandem repeat and a poly-A run."""
    rng = np.random.default_rng(8300)
    s = bytearray(ab.rand_seq(rng, 5000))
    for at in (700, 1900, 3300, 4400):
        s[at:at + 150] = s[100:250]
    s[2500:2800] = (bytes(s[2500:2531]) * 10)[:300]
    s[4000:4060] = b"A" * 60
    return (bytes(s),)


def copies(G, k):
    return tuple(repeat_inputs.high_copy(G=G, n=N, copies=k))


def family_problems():
    """Three gap pairs of anchor_batch_cases.a200: with a planted repeat, at least 1 000 bases,
    the first that has its partner reverse-complemented among them."""
    probs = ab.a200_problems()
    picked = [p for p in range(1, 200, 2) if len(probs[p][0]) >= 1000]
    flipped = [p for p in picked if (p // 2) % 2 == 1]
    plain = [p for p in picked if (p // 2) % 2 == 0]
    return [probs[plain[0]], probs[flipped[0]], probs[plain[1]]]


def recursion_problems():
    """Three G = 3 problems of recursion_batch_cases.r200 (built so that the v1 tail cuts a copy
    of multiplicity G - 1 off): the first two with one round of default weights, and the first
    with two."""
    probs = [p for p in rb.r200()["problems"] if len(p) == 3]
    one = [p for p in probs if len(rb.rounds_model(rb.default_weights(p), False)) == 1]
    two = [p for p in probs if len(rb.rounds_model(rb.default_weights(p), False)) == 2]
    return [one[0], two[0], one[1]]


# Under nway_only the reference searches with nway_mh (Aligner.cpp:1190-1195, 1205), a MaskedMemHash
# (Aligner.h:199) whose mask selects every genome (Aligner.cpp:2208-2212); gap_mh, a MemHash, otherwise.
NWAY_FINDER = dict(finder="masked", mask=0b111)


def recursion_rounds(problem, nway_only):
    return tuple((w, 0) for w in rb.rounds_model(rb.default_weights(problem), nway_only))


ENUM3_SOURCE = "find_tol_G4_rt2_et3"
ENUM3_ROWS = os.path.join(ROOT, "tests", "golden", "ref_enum3_list.txt")


@functools.lru_cache(maxsize=None)
def enum3_list():
    """The list of an enum_tol 3 find on four three-copy genomes, many overlapping matches: the
    reference's own list for the case ENUM3_SOURCE, written by golden/make_ref_golden.py."""
    with open(ENUM3_ROWS) as f:
        return rows_of(f.read().splitlines(), 4)


def tied_list():
    """G = 3, 60 rows: 20 share one LeftEnd in sequence 0 and 18 another in sequence 1 (more than
    introsort's 16-element insertion threshold of equal sort keys)."""
    rng = np.random.default_rng(8400)
    l, s = random_matchlist(rng, 60, 3, max_len=80, start_span=600)
    s = s.reshape(60, 3)
    s[5:25, 0] = 300 * np.where(s[5:25, 0] < 0, -1, 1)
    s[30:48, 1] = 170 * np.where(rng.random(18) < 0.5, -1, 1)
    return l, s


def sawtooth_list():
    """adversarial_keys("sawtooth16") as sequence-0 LeftEnds: 500 rows on 16 keys."""
    return ab.adversarial_list("sawtooth16", 500)


def eo2_input(case):
    l, s = eo2.build_input(case)
    return np.asarray(l, dtype=np.uint64), np.asarray(s, dtype=np.int64).reshape(len(l), -1)


# ---- the cases ----------------------------------------------------------------------------------
def _find(seqs, weight=15, rank=0, **kw):
    return dict(mode="find", seqs=seqs, weight=weight, rank=rank, **kw)


def _cases():
    c = {}
    c["seeds"] = dict(mode="seeds")
    for w in (11, 15, 21, 31):
        c[f"sml_w{w}"] = dict(mode="sml", seqs=sml_input, weight=w, rank=0)
    for w in (11, 12, 13, 15, 17, 19, 21, 23):
        c[f"find_w{w}"] = _find(related, weight=w)
    for w in (15, 19):
        for r in (1, 2):
            c[f"find_w{w}_rank{r}"] = _find(related, weight=w, rank=r)
    for G in (2, 4, 6, 9):
        c[f"find_G{G}"] = _find(functools.partial(related, G))
    c["find_uneven"] = _find(uneven)
    for G, k in ((3, 2), (4, 3)):
        for rt, et in ((0, 1), (1, 1), (1, 2), (2, 3)):
            c[f"find_tol_G{G}_rt{rt}_et{et}"] = _find(functools.partial(copies, G, k), repeat_tol=rt, enum_tol=et)
    for G, mask in ((3, 0b101), (4, 0b1010), (4, 0b0111)):
        c[f"find_G{G}_mask{mask:0{G}b}"] = _find(functools.partial(diverged, G, swap=mask == 0b0111), finder="masked", mask=mask)
    for G in (2, 3, 4):
        c[f"find_pairwise_G{G}"] = _find(functools.partial(related, G), finder="pairwise")
    gapped = lambda: tuple(repeat_inputs.n_gapped(G=3, n=60_000, gaps=((20_000, 3000),)))   # noqa: E731
    c["restart_n_gapped"] = _find(gapped, offset_log=1)
    c["restart_high_copy"] = _find(lambda: tuple(repeat_inputs.high_copy(copies=2000)), offset_log=1)
    c["restart_high_copy_tandem"] = _find(lambda: tuple(repeat_inputs.high_copy(copies=2000, tandem=True)), offset_log=1)
    for s in range(6):
        c[f"restart_mixed_{s}"] = _find(functools.partial(lambda s: tuple(repeat_inputs.mixed_repeats(s)), s), offset_log=1)
    c["restart_from_position"] = _find(gapped, offset_log=1, start_points=(1500, 30_000, 700))
    for T in (7, 1009):
        c[f"table_T{T}"] = _find(evolved, table_size=T, match_log=1)
    c["alphabet"] = _find(alphabet)
    # inversions, translocations, duplications and indels; tandem arrays under both tolerances
    c["rearranged"] = _find(evolved)
    c["tandem_rt1_et2"] = _find(lambda: tuple(tie_inputs.tandem_blocks()), repeat_tol=1, enum_tol=2)
    c["filter_G3_mult2_len"] = _find(related, filters=(("mult", 2), ("len", 5000)))
    c["filter_G3_mult3_len"] = _find(related, filters=(("mult", 3), ("len", 1000)))
    c["filter_G4_mult2"] = _find(functools.partial(related, 4), filters=(("mult", 2), ("len", 5000)))
    c["filter_G4_mult3"] = _find(functools.partial(related, 4), filters=(("mult", 3),))
    for i in range(3):
        c[f"family_{i}"] = dict(mode="family", seqs=functools.partial(lambda i: family_problems()[i], i),
                                filters=(("len", ab.MIN_LENGTH),))
        for v, nway in (("m0", False), ("mG", True)):
            c[f"recursion_{i}_{v}"] = dict(
                mode="recursion", seqs=functools.partial(lambda i: recursion_problems()[i], i), nway_only=nway,
                rounds=functools.partial(lambda i, nway: recursion_rounds(recursion_problems()[i], nway), i, nway),
                filters=((("mult", 3),) if nway else ()) + (("len", rb.MIN_LENGTH),),
                **NWAY_FINDER if nway else {})
            # the same search as the reference wrote it, weight loop (Aligner.cpp:1142-1177) and tail included
            c[f"recursion_whole_{i}_{v}"] = dict(mode="recursion", whole=True, nway_only=nway,
                                                 seqs=functools.partial(lambda i: recursion_problems()[i], i),
                                                 **NWAY_FINDER if nway else {})
    c["eo1_enum3"] = dict(mode="eo1", rows=enum3_list)
    c["eo2_enum3"] = dict(mode="eo2", rows=enum3_list)
    c["eo1_tied"] = dict(mode="eo1", rows=tied_list)
    c["eo1_sawtooth"] = dict(mode="eo1", rows=sawtooth_list)
    for both in (0, 1):
        c[f"eo2_tied_both{both}"] = dict(mode="eo2", rows=tied_list, eliminate_both=both)
        for case in ((10, 2, 100, 2), (200, 3, 2000, 3), (3000, 4, 30000, 4)):
            c[f"eo2_M{case[0]}_G{case[1]}_both{both}"] = dict(mode="eo2", rows=functools.partial(eo2_input, case),
                                                              eliminate_both=both)
        c[f"eo2_subset_both{both}"] = dict(mode="eo2", rows=functools.partial(eo2_input, eo2.SUBSET_CASE),
                                           eliminate_both=both, seq_ids=(3, 0))
    c["eo1_M3000_G4"] = dict(mode="eo1", rows=functools.partial(eo2_input, (3000, 4, 30000, 4)))
    for w in (11, 15):
        c[f"occurrence_w{w}"] = dict(mode="occurrence", seqs=occurrence_input, weight=w, rank=0)
    c["compat"] = dict(mode="compat", seqs=functools.partial(related, 3, 450_000), weight=15, rank=0, finder="parallel",
                       md5_only=True)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case_seqs(name):
    f = CASES[name].get("seqs")
    return tuple(f()) if f else ()


@functools.lru_cache(maxsize=None)
def case_rows(name):
    f = CASES[name].get("rows")
    if f is None:
        return None
    l, s = f()
    l = np.asarray(l, dtype=np.uint64)
    return l, np.asarray(s, dtype=np.int64).reshape(len(l), -1)


def case_rounds(name):
    r = CASES[name].get("rounds")
    return tuple(r()) if callable(r) else r


def case_header(name):
    """The text part of the driver's case file."""
    c = CASES[name]
    lines = [f"mode {c['mode']}"]
    for k in ("finder", "weight", "rank", "repeat_tol", "enum_tol", "table_size", "mask", "match_log", "offset_log",
              "eliminate_both", "nway_only"):
        if k in c and not (c.get("whole") and k in ("finder", "mask")):   # the whole recursion picks its own finder
            lines.append(f"{k} {int(c[k]) if isinstance(c[k], bool) else c[k]}")
    for k in ("start_points", "seq_ids"):
        if k in c:
            lines.append(f"{k} " + " ".join(str(int(x)) for x in c[k]))
    if case_rounds(name) is not None:
        lines.append("rounds " + " ".join(f"{w}:{r}" for w, r in case_rounds(name)))
    for kind, v in c.get("filters", ()):
        lines.append(f"filter {kind} {v}")
    rows = case_rows(name)
    if rows is not None:
        lines.append(f"G {rows[1].shape[1]}")
        lines.append("lengths " + " ".join("0" for _ in range(rows[1].shape[1])))
        for ln, row in zip(rows[0].tolist(), rows[1].tolist()):
            lines.append("row " + " ".join(str(x) for x in [ln] + row))
    else:
        seqs = case_seqs(name)
        lines.append(f"G {len(seqs)}")
        lines.append("lengths " + " ".join(str(len(s)) for s in seqs))
    return "\n".join(lines) + "\ndata\n"


def case_bytes(name):
    """The whole case file: what `sha256` of the fixture is taken over."""
    rows = case_rows(name)
    body = b"" if rows is not None else b"".join(case_seqs(name))
    return case_header(name).encode() + body


def input_sha256(name):
    return hashlib.sha256(case_bytes(name)).hexdigest()


# ---- the driver's output ------------------------------------------------------------------------
def parse_output(text):
    """`@name count` sections -> {name: [lines]} in order."""
    out, lines, i = {}, text.split("\n"), 0
    while i < len(lines):
        if not lines[i]:
            i += 1
            continue
        assert lines[i][0] == "@", lines[i]
        name, n = lines[i][1:].split(" ")
        out[name] = lines[i + 1:i + 1 + int(n)]
        i += 1 + int(n)
    return out


def rows_of(lines, G):
    a = np.array([[int(x) for x in ln.split("\t")] for ln in lines], dtype=np.int64).reshape(len(lines), G + 1)
    return a[:, 0].astype(np.uint64), np.ascontiguousarray(a[:, 1:])


def lines_of(lengths, starts):
    starts = np.asarray(starts, dtype=np.int64).reshape(len(lengths), -1)
    return ["\t".join(str(x) for x in [int(ln)] + row) for ln, row in zip(np.asarray(lengths).tolist(), starts.tolist())]


def case_G(name):
    rows = case_rows(name)
    return rows[1].shape[1] if rows is not None else len(case_seqs(name))


def record_section(name, sec, lines, md5_only=False):
    """What the fixture keeps of one section."""
    text = "".join(ln + "\n" for ln in lines)
    rec = dict(count=len(lines))
    if is_match_section(sec):
        rec["list_md5"] = sf.list_md5(*rows_of(lines, case_G(name))) if lines else sf.list_md5(
            np.zeros(0, np.uint64), np.zeros((0, case_G(name)), np.int64))
    else:
        rec["md5"] = hashlib.md5(text.encode()).hexdigest()
    if md5_only:
        return rec
    if len(lines) <= FULL_TEXT_MAX:
        rec["text"] = text
    else:
        rec["head"], rec["tail"] = list(lines[:3]), list(lines[-3:])
    return rec


def digest_only(name, sec):
    """Sections recorded without their text: everything of an md5_only case; a round's list (the
    last round's is the `table` section, and every round adds to the one before); the unfiltered
    list of a filter case (the find case on the same input has its text); the table of a whole
    recursion case (the case with the same rounds given has its text)."""
    c = CASES[name]
    return (bool(c.get("md5_only")) or sec.startswith("round") or (sec == "list" and bool(c.get("filters")))
            or (sec == "table" and bool(c.get("whole"))))


def record(name, sections):
    """What the fixture keeps of a case; the counters as a dict."""
    c = CASES[name]
    keep = sections if not c.get("md5_only") else {k: v for k, v in sections.items() if k == "list"}
    rec = dict(sha256=input_sha256(name),
               sections={sec: record_section(name, sec, lines, digest_only(name, sec)) for sec, lines in keep.items()
                         if sec != "counters"})
    if "counters" in keep:
        rec["counters"] = {k: int(v) for k, v in (ln.split(" ") for ln in keep["counters"])}
    return rec


def check_section(name, sec, rec, lines):
    """Asserts that `lines` is the section the fixture recorded."""
    got = record_section(name, sec, lines, "text" not in rec and "head" not in rec)
    if got != rec:
        old = rec.get("text", "").splitlines()
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(old, lines)) if a != b][:5]
        raise AssertionError(f"{name}/{sec}: recorded count {rec['count']}, got count {got['count']}; "
                             f"digests {rec.get('list_md5', rec.get('md5'))} and {got.get('list_md5', got.get('md5'))}; first differing lines (index, recorded, got): {diff}; "
                             f"recorded head {rec.get('head', old[:3])}, got head {lines[:3]}")


def check_case(name, sections):
    rec = fixture()[name]
    want = dict(rec["sections"])
    if "counters" in rec:
        got = {k: int(v) for k, v in (ln.split(" ") for ln in sections["counters"])}
        assert got == rec["counters"], (name, got, rec["counters"])
    got_names = {k for k in sections if k != "counters"}
    if CASES[name].get("md5_only"):
        got_names &= set(want)
    assert got_names == set(want), (name, sorted(got_names), sorted(want))
    for sec in want:
        check_section(name, sec, want[sec], sections[sec])


def have_driver():
    return os.path.exists(DRIVER)


def run_driver(name):
    """The case through oracle/_ref/ref_driver: its sections."""
    with tempfile.TemporaryDirectory() as d:
        path, outp = os.path.join(d, "case"), os.path.join(d, "out")
        with open(path, "wb") as f:
            f.write(case_bytes(name))
        subprocess.run([DRIVER, path, outp], check=True, stdout=subprocess.DEVNULL)
        with open(outp) as f:
            return parse_output(f.read())


def counters_section(mem_count, collisions):
    return [f"mem_count {int(mem_count)}", f"collision_count {int(collisions)}"]


def filter_sections(c, out, l, s):
    """MultiplicityFilter / LengthFilter (MatchList.h:636-664) of a case on a host list, into out."""
    for kind, v in c.get("filters", ()):
        keep = (s != 0).sum(axis=1) == v if kind == "mult" else l >= v
        l, s = l[keep], s[keep]
        out[f"filter_{kind}_{v}"] = lines_of(l, s)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]
