#!/usr/bin/env python3
"""Do the kernels of the working tree compile to the machine code of another commit?

    python tools/isa_diff.py [--base REV] [--show N] [--mix] [--map OLD=NEW ...] [[base:]file.hip[:-DFLAG] ...] > profiles/<name>_isa_diff.txt

For a change that only moves source around (a shared header, a renamed helper) the proof that nothing happened to a
kernel is that its instructions did not change.  The tool exports nerf-simple_amd/csrc and include/ of REV (default
HEAD) with `git archive` into a temporary directory, assembles each listed .hip file for gfx950 from that export and
from the working tree (tools/check_vmcnt.py assemble / kernels_of; 9-15 s per file and tree, run in parallel), and
compares the instruction text kernel by kernel after normalisation:
  * comments and assembler directives are stripped;
  * local labels (.LBB<f>_<n>, ...) are renumbered in order of first appearance;
  * kernel symbol names are NOT normalised: a kernel must keep its name, unless --map OLD=NEW (regular expression and
    replacement, applied to the base's symbols; repeatable) says how it was renamed.  A mapped kernel is looked up in
    every listed file of the working tree, so it may have moved to another source.  A file or flag set that the working
    tree no longer has is listed as base:file.hip[:-DFLAG]: it is assembled from the base alone, and every kernel of it has
    to be mapped into a listed file of the working tree.
One line per kernel: instruction count, MFMA count, identical yes / no; --show N prints the first N differing lines of a
kernel that is not identical; --mix prints, for such a kernel, the counts of the chain's instruction classes (MIX) on both
sides and how many differing lines are anything but `s_setprio` / `s_nop`, and whether those are the same opcodes on
both sides (register allocation, a wait moved by a slot) -- for a change that is meant to add only those.
Exit status 1 when any kernel differs, is missing or is new.  Needs hipcc and git; no GPU.
"""
import argparse
import collections
import concurrent.futures
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_vmcnt  # noqa: E402

CSRC = os.path.join("nerf-simple_amd", "csrc")
DEFAULT = ["mlp_bf16_16.hip", "mlp_bf16_16.hip:-DNERF_HALF", "density.hip", "density.hip:-DNERF_HALF", "mlp_bwd_16.hip",
           "mlp_f32.hip", "dw_gemm.hip", "dw_gemm_f8.hip"]
LABEL = re.compile(r"\.L\w+")
MIX = (("v_mfma", r"v_mfma"), ("ds_read_b128", r"ds_read_b128"), ("v_cvt_pk_*", r"v_cvt_pk_"), ("v_pk_max_i16", r"v_pk_max_i16"),
       ("buffer_load ... lds", r"buffer_load\S* .* lds$"), ("s_barrier", r"s_barrier"), ("s_setprio", r"s_setprio"), ("s_nop", r"s_nop"))


def normalise(lines):
    """Instruction text of one kernel body: no comments, no directives, local labels renumbered."""
    out, names = [], {}
    for line in lines:
        text = line.split(";")[0].split("//")[0].strip()
        if not text or (text.startswith(".") and not text.endswith(":")):
            continue
        out.append(" ".join(LABEL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), text).split()))
    return out


def count(lines):
    """(instructions, MFMAs) of a normalised kernel body (labels are not instructions)"""
    return sum(not ln.endswith(":") for ln in lines), sum(ln.startswith("v_mfma") for ln in lines)


def kernels(tree, src, flags):
    if src.startswith("base:"):
        if tree == ROOT:
            return {}
        src = src[len("base:"):]
    asm = check_vmcnt.assemble(os.path.join(tree, CSRC, src), flags)
    return {k: normalise(v) for k, v in check_vmcnt.kernels_of(asm).items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", default="HEAD", help="the commit to compare the working tree against")
    ap.add_argument("--show", type=int, default=0, help="print this many differing lines of a kernel that differs")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW",
                    help="a renamed kernel: re.sub(OLD, NEW) on the symbols of the base")
    ap.add_argument("--mix", action="store_true", help="instruction-class counts of a kernel that differs, both sides")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("files", nargs="*", default=DEFAULT)
    args = ap.parse_args()
    jobs = [(f.split(":-")[0], tuple("-" + x for x in f.split(":-")[1:])) for f in args.files]
    rc = 0
    with tempfile.TemporaryDirectory() as base:
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.base, CSRC, "include"], check=True, stdout=subprocess.PIPE).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(base)
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            fut = {(tree, j): pool.submit(kernels, tree, *j) for j in jobs for tree in (base, ROOT)}
            moved = {}                          # mapped kernels of the working tree, from whichever listed file holds them
            for src, flags in jobs:
                old, new = fut[base, (src, flags)].result(), fut[ROOT, (src, flags)].result()
                for name in list(old):
                    to = name
                    for rule in args.map:
                        to = re.sub(*rule.split("=", 1), to)
                    if to != name or src.startswith("base:"):
                        old[to] = old.pop(name)
                        moved[to] = None
            for key in moved:
                moved[key] = next((fut[ROOT, j].result().pop(key) for j in jobs if key in fut[ROOT, j].result()), None)
            for src, flags in jobs:
                old, new = fut[base, (src, flags)].result(), fut[ROOT, (src, flags)].result()
                new.update({k: v for k, v in moved.items() if k in old and v is not None})
                print(f"== {src} {' '.join(flags)}".rstrip())
                for name in sorted(set(old) | set(new)):
                    if name not in old or name not in new:
                        print(f"  {name}: only in the {'working tree' if name in new else 'base'}")
                        rc = 1
                        continue
                    a, b = old[name], new[name]
                    same = a == b
                    rc |= not same
                    print(f"  {name}: {count(b)[0]} instructions, {count(b)[1]} MFMAs, identical {'yes' if same else 'no'}"
                          + ("" if same else " (base: %d instructions, %d MFMAs)" % count(a)))
                    if not same and args.mix:
                        for label, pat in MIX:
                            na, nb = (sum(re.match(pat, ln) is not None for ln in side) for side in (a, b))
                            print(f"      {label:20s} base {na:5d}   working tree {nb:5d}" + ("" if na == nb else "   <-- differs"))
                        other = [d for d in difflib.unified_diff(a, b, lineterm="", n=0)
                                 if d[:1] in "+-" and not d.startswith(("+++", "---")) and not d[1:].startswith(("s_setprio", "s_nop"))]
                        ops = [collections.Counter(d[1:].split()[0] for d in other if d[0] == sign) for sign in "-+"]
                        print(f"      differing lines other than s_setprio / s_nop: {len(other)}"
                              + ("" if not other else " (the same opcodes on both sides: other registers or another slot)"
                                 if ops[0] == ops[1] else " (OTHER OPCODES)"))
                    if not same and args.show:
                        diff = [d for d in difflib.unified_diff(a, b, "base", "working tree", lineterm="", n=0)]
                        print("\n".join("      " + d for d in diff[:args.show]))
    sys.exit(rc)


if __name__ == "__main__":
    main()
