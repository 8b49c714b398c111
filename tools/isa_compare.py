#!/usr/bin/env python3
"""Compare the gfx950 code of one translation unit (--unit, default cfz_engine.hip) between two source trees, function by function
(no GPU needed).

    python tools/isa_compare.py                      # the checked-in HEAD (a temporary git worktree) against the working tree
    python tools/isa_compare.py --base-ref HEAD~1    # ... the parent of a commit already made
    python tools/isa_compare.py OLD NEW [-k NAME ...]  # two trees (conflict_rez_amd/csrc with include/ beside it), or two .s listings
    python tools/isa_compare.py --unit cfz_planning.hip --base-ref HEAD~1   # the planning kernels

Each tree's unit is compiled with the flags of __graft_entry__.build plus `-S --cuda-device-only` (about a minute on one
core; the two run side by side).  The listing is split at the function labels, comments are dropped and the `.L...` labels are
renumbered by first appearance inside each function, so that a function whose code did not change compares equal even when
functions were added or removed around it.  Per function: the instruction count on either side, `same` or `different`, and the
figures DESIGN.md tabulates for the kernels (.vgpr_count, .vgpr_spill_count, .sgpr_spill_count, .private_segment_fixed_size).
The exit status is 1 when a function named with -k differs, is missing, or changed its figures (default: the twelve solver kernels
of cfz_engine.hip; EVERY function of cfz_planning.hip -- both state_ws_kernel instantiations, colloc_kernel and the out-of-line device
functions -- in either listing).
It compares text and searches for no particular instruction.  `--markdown` prints the kernels' rows as a table for DESIGN.md."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# __graft_entry__.build's flags for this unit; the source hash is host code and fixed here so that it cannot differ
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wno-unused-value", '-DCFZ_SRC_HASH="isa_compare"', "-O3"]
SOLVER_KERNELS = ("solve_kernel", "solve_kernel_pool", "loop_kernel", "loop_kernel_seq", "loop_kernel_dist", "loop_kernel_seq_dist",
                  "loop_kernel_comm", "loop_kernel_seq_comm", "loop_kernel_pool", "loop_kernel_seq_pool", "loop_kernel_pool_comm",
                  "loop_kernel_seq_pool_comm")
META = (".vgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size")


UNITS = ("cfz_engine.hip", "cfz_planning.hip")


def start_compile(tree, out, unit):
    src = os.path.join(tree, "conflict_rez_amd", "csrc", unit)
    if not os.path.exists(src):
        sys.exit(f"{src}: no such file")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return subprocess.Popen([hipcc, *FLAGS, "-S", "--cuda-device-only", "-o", out, src], cwd=tree)


def short_name(sym):
    """The last identifier of an Itanium nested name (_ZN12_GLOBAL__N_112solve_kernelE... -> solve_kernel); else the symbol."""
    m = re.match(r"_ZN?", sym)
    if not m:
        return sym
    i, last = m.end(), None
    while i < len(sym):
        if sym[i] == "L":  # internal linkage
            i += 1
        n = re.match(r"\d+", sym[i:])
        if not n:
            break
        i += n.end()
        last = sym[i:i + int(n.group())]
        i += int(n.group())
    b = re.match(r"ILb([01])E", sym[i:])  # a kernel instantiated on one bool: state_ws_kernel<true>
    return (last + ("<true>" if b.group(1) == "1" else "<false>") if b else last) if last else sym


def parse(listing):
    """{symbol: [normalised instruction lines]}, {symbol: {figure: value}} of one listing."""
    funcs, meta, cur, labels = {}, {}, None, None
    entry = []

    def close_entry():
        text = "\n".join(entry)
        name = re.search(r"^\s+(?:- )?\.name:\s+(\S+)$", text, re.M)
        if name:
            meta[name.group(1)] = {k: int(re.search(rf"^\s+(?:- )?\{k}:\s+(\d+)$", text, re.M).group(1)) for k in META}

    in_kernels = False
    with open(listing) as f:
        for raw in f:
            line = raw.split(";", 1)[0].rstrip()
            if in_kernels:
                if raw.startswith("  - "):
                    if entry:
                        close_entry()
                    entry = [raw.rstrip()]
                elif raw.startswith("    "):
                    if not raw.startswith("      "):  # the entry's own keys, not those of its arguments
                        entry.append(raw.rstrip())
                else:
                    if entry:
                        close_entry()
                    entry, in_kernels = [], False
                continue
            if raw.startswith("amdhsa.kernels:"):
                in_kernels = True
                continue
            if cur is None:
                m = re.match(r"\s+\.type\s+(\S+),@function", line)
                if m:
                    cur, labels = m.group(1), {}
                    funcs[cur] = []
                continue
            if re.match(r"\.Lfunc_end\d+:", line):
                cur = None
                continue
            s = line.strip()
            if not s or s == cur + ":":
                continue
            s = re.sub(r"\.L[A-Za-z0-9_$]+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), s)
            funcs[cur].append(re.sub(r"\s+", " ", s))
    return funcs, meta


def count(lines):
    return sum(1 for s in lines if not s.startswith(".") and not s.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trees", nargs="*", help="OLD NEW: source trees or .s listings (default: --base-ref and the working tree)")
    ap.add_argument("--base-ref", default="HEAD", help="the commit the working tree is compared with when no trees are given")
    ap.add_argument("--unit", choices=UNITS, default=UNITS[0], help="the translation unit to compile in either tree")
    ap.add_argument("-k", "--kernel", action="append", help="a function that must be the same (default: see above)")
    ap.add_argument("--keep", metavar="DIR", help="keep the two listings as DIR/old.s and DIR/new.s")
    ap.add_argument("--markdown", action="store_true", help="print the named functions as a markdown table")
    a = ap.parse_args()
    if len(a.trees) not in (0, 2):
        ap.error("give two trees or none")
    must = tuple(a.kernel) if a.kernel else SOLVER_KERNELS if a.unit == UNITS[0] else None  # None: every function
    with tempfile.TemporaryDirectory() as tmp:
        out = a.keep or tmp
        os.makedirs(out, exist_ok=True)
        trees, worktree = list(a.trees), None
        try:
            if not trees:
                worktree = os.path.join(tmp, "base")
                subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", "--quiet", worktree, a.base_ref])
                trees = [worktree, ROOT]
            listings, procs = [], []
            for tree, name in zip(trees, ("old.s", "new.s")):
                if os.path.isfile(tree):
                    listings.append(tree)
                else:
                    listings.append(os.path.join(out, name))
                    procs.append(start_compile(os.path.abspath(tree), listings[-1], a.unit))
            if any([p.wait() != 0 for p in procs]):
                sys.exit("hipcc failed")
        finally:
            if worktree:
                subprocess.call(["git", "-C", ROOT, "worktree", "remove", "--force", worktree])
        (fa, ma), (fb, mb) = parse(listings[0]), parse(listings[1])
    bad, rows = [], []
    if must is None:
        must = tuple(dict.fromkeys(short_name(s) for s in list(fa) + list(fb)))
    for sym in list(fa) + [s for s in fb if s not in fa]:
        name = short_name(sym)
        if sym not in fa or sym not in fb:
            verdict = "only in " + ("old" if sym in fa else "new")
        else:
            verdict = "same" if fa[sym] == fb[sym] and ma.get(sym) == mb.get(sym) else "different"
        na, nb = (count(f[sym]) if sym in f else "-" for f in (fa, fb))
        figs = [f"{ma[sym][k] if sym in ma else '-'} / {mb[sym][k] if sym in mb else '-'}" for k in META] if sym in ma or sym in mb else []
        rows.append((name, na, nb, verdict, figs))
        if name in must and verdict != "same":
            bad.append(name)
    seen = {r[0] for r in rows}
    bad += [k for k in must if k not in seen]
    if a.markdown:
        print("| kernel | instructions | VGPRs | spilled VGPRs | spilled SGPRs | scratch (B) | code |")
        print("|---|---|---|---|---|---|---|")
        for name, na, nb, verdict, figs in rows:
            if name in must:
                print(f"| `{name}` | {na} / {nb} | " + " | ".join(figs or ["-"] * len(META)) + f" | {verdict} |")
    else:
        print(f"{'function':34s} {'instructions':>17s}  {'':10s} " + " ".join(f"{k:>15s}" for k in ("vgpr", "vgpr_spill", "sgpr_spill", "scratch")) + "   (old / new)")
        for name, na, nb, verdict, figs in rows:
            print(f"{name:34s} {str(na):>8s} {str(nb):>8s}  {verdict:10s} " + " ".join(f"{x:>15s}" for x in figs))
        print(f"{len(rows)} functions, {sum(r[3] == 'same' for r in rows)} same")
    if bad:
        print("NOT THE SAME: " + ", ".join(dict.fromkeys(bad)), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
