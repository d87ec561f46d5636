#!/usr/bin/env python3
"""Static instruction counts of the HIP kernels, from the gfx950 assembly (no GPU needed).

    python3 tools/inst_count.py libmems_amd/csrc/seeds.hip libmems_amd/csrc/radix_seg.hip \
        --filter 'seed_pack_kernel<1.*132741359|seg_onesweep_kernel<768, 12, true, false, false>'

Compiles every named .hip file to device assembly (hipcc -O3 --offload-arch=gfx950
--cuda-device-only -S) and prints, per kernel symbol, the VGPR count, the static LDS bytes and
the instruction counts by mnemonic prefix: v_ (vector ALU), ds_ (LDS), global_/buffer_/flat_
(vector memory) and everything else as one figure.  The counts are static: a fully unrolled
kernel executes about that many per wave, a kernel with loops or divergent roles does not.
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLASSES = (("valu", ("v_",)), ("lds", ("ds_",)), ("vmem", ("global_", "buffer_", "flat_")))


def compile_asm(src: str, arch: str, extra: list[str]) -> str:
    cmd = [HIPCC, "-O3", "-std=c++17", f"--offload-arch={arch}", "--cuda-device-only", "-S", "-w",
           "-I", os.path.join(ROOT, "include"), *extra, src, "-o", "-"]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def demangle(names: list[str]) -> dict[str, str]:
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names) + "\n", check=True, capture_output=True, text=True).stdout
    return dict(zip(names, out.splitlines()))


def parse(asm: str) -> dict[str, dict]:
    """kernel symbol -> counts; a kernel's body runs from its label to its .Lfunc_end label"""
    kernels: dict[str, dict] = {}
    cur = None
    desc = None
    label = re.compile(r"^([A-Za-z_$.][\w$.]*):")
    for line in asm.splitlines():
        s = line.strip()
        if not s or s.startswith(";") or s.startswith("//"):
            continue
        m = label.match(s)
        if m:
            name = m.group(1)
            if name.startswith(".Lfunc_end"):
                cur = None
            elif not name.startswith(".") and cur is None:
                cur = kernels.setdefault(name, {"valu": 0, "lds": 0, "vmem": 0, "other": 0})
            continue
        if s.startswith(".amdhsa_kernel "):
            desc = kernels.get(s.split()[1])
            continue
        if s.startswith(".end_amdhsa_kernel"):
            desc = None
            continue
        if desc is not None:
            f = s.split()
            if f[0] == ".amdhsa_next_free_vgpr":   # arch + accumulation registers of the unified file
                desc["vgpr"] = int(f[1], 0)
            elif f[0] == ".amdhsa_group_segment_fixed_size":
                desc["lds_bytes"] = int(f[1], 0)
            continue
        if cur is None or s.startswith("."):
            continue
        mn = s.split()[0]
        for cls, prefixes in CLASSES:
            if mn.startswith(prefixes):
                cur[cls] += 1
                break
        else:
            cur["other"] += 1
    return {k: v for k, v in kernels.items() if "lds_bytes" in v}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--filter", default="", help="regex on the demangled kernel name")
    ap.add_argument("--extra", default="", help="extra compiler flags (e.g. -DX=1)")
    a = ap.parse_args()
    rx = re.compile(a.filter) if a.filter else None
    print("| file | kernel | VGPRs | LDS bytes | v_ | ds_ | global_/buffer_/flat_ | other |")
    print("|---|---|---|---|---|---|---|---|")
    for src in a.sources:
        ks = parse(compile_asm(src, a.arch, a.extra.split()))
        names = demangle(list(ks))
        for sym in sorted(ks, key=lambda s: names[s]):
            nm = re.sub(r"^void ", "", names[sym]).replace("mums::(anonymous namespace)::", "")
            nm = re.sub(r"\(.*$", "", nm)
            if rx and not rx.search(nm):
                continue
            k = ks[sym]
            print(f"| {os.path.basename(src)} | `{nm}` | {k.get('vgpr', '?')} | "
                  f"{k['lds_bytes']} | {k['valu']} | {k['lds']} | {k['vmem']} | {k['other']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
