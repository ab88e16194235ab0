"""Kernel-by-kernel comparison of the device assembly of two source trees.
usage: python tools/isa_diff.py [--map FILE] [--work DIR] [-v] A B UNIT...
A and B are each a directory holding a tree (its dlrm.jl_amd/csrc and include) or a git revision, taken as
tools/ab_build.sh takes one ("." is the working tree); UNIT is a file of csrc (interact.hip).  Each unit is compiled
with its own tree's Makefile flags plus --cuda-device-only -S -Rpass-analysis=kernel-resource-usage, and split per
kernel.  Comment, .loc / .file / .ident lines are dropped, block labels and the kernel's own symbol normalised: what
is left is compared as text, and the resource remarks as numbers.  --map FILE: lines "REGEX<tab>REPLACEMENT" applied
(re.sub, in order) to A's demangled kernel names, for kernels renamed in B.  --work DIR keeps the assembly there and
reuses a tree's when no file of its csrc is newer.  -v lists the identical kernels and every kernel's figures too.
Exit status 1 when a kernel differs or exists on one side only."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

FIGURES = ["VGPRs", "AGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]",
           "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def tree_of(arg, work, side):
    """The root directory of tree `arg`: itself, or a revision's csrc and include extracted below work."""
    if os.path.isdir(os.path.join(arg, "dlrm.jl_amd", "csrc")):
        return arg
    root = os.path.join(work, side, "tree")
    os.makedirs(root, exist_ok=True)
    top = subprocess.check_output(["git", "rev-parse", "--show-toplevel"], text=True).strip()
    tar = subprocess.run(["git", "archive", arg, "--", "dlrm.jl_amd/csrc", "include"], cwd=top, check=True,
                         stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", root], input=tar, check=True)
    return root


def compile_unit(root, unit, out):
    """unit -> out (.s) and out + '.remarks', with the flags of the tree's own Makefile."""
    csrc = os.path.join(root, "dlrm.jl_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc))
    if os.path.exists(out + ".remarks") and os.path.getmtime(out) > newest:
        return
    cmd = subprocess.check_output(["make", "-s", "-C", csrc, "--eval", "isa-flags: ; @echo $(HIPCC) $(HIPFLAGS)",
                                   "isa-flags"], text=True).split()
    cmd += ["-x", "hip", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", unit, "-o", out]
    with open(out + ".remarks", "w") as err:
        subprocess.run(cmd, cwd=csrc, stderr=err, check=True)


def kernels(path, renames):
    """{demangled name: (normalised text, figures)} of an assembly file, in the file's order."""
    s = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", s, flags=re.M)
    plain = subprocess.run(["c++filt"], input="\n".join(names), text=True, check=True,
                           stdout=subprocess.PIPE).stdout.split("\n")
    figs, cur = {}, None
    for line in open(path + ".remarks"):
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|([A-Za-z][^:]*): (\S+)) \[-Rpass", line)
        if m and m.group(1):
            cur = figs.setdefault(m.group(1), {})
        elif m and cur is not None and m.group(2) in FIGURES:
            cur[m.group(2)] = m.group(3)
    out = {}
    for sym, name in zip(names, plain):
        body = s[s.index("\n" + sym + ":"):]
        body = body[:body.index(".Lfunc_end")]
        lines = []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].rstrip()
            if ln and not re.match(r"\s*\.(loc|file|ident)\b", ln):
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln).replace(sym, "KERNEL").replace(sym[2:], "KERNEL"))
        for rx, to in renames:
            name = re.sub(rx, to, name)
        out[name] = ("\n".join(lines), tuple(figs.get(sym, {}).get(k, "?") for k in FIGURES))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--map")
    ap.add_argument("--work")
    ap.add_argument("-v", action="store_true")
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("units", nargs="+")
    o = ap.parse_args()
    work = o.work or tempfile.mkdtemp(prefix="isa_diff_")
    renames = [ln.rstrip("\n").split("\t") for ln in open(o.map) if "\t" in ln] if o.map else []
    bad = 0
    for unit in o.units:
        side = []
        for tag, arg, ren in (("a", o.a, renames), ("b", o.b, [])):
            os.makedirs(os.path.join(work, tag), exist_ok=True)
            out = os.path.join(work, tag, unit + ".s")
            compile_unit(tree_of(arg, work, tag), unit, out)
            side.append(kernels(out, ren))
        ka, kb = side
        both = [k for k in ka if k in kb]
        same = [k for k in both if ka[k][0] == kb[k][0]]
        moved = [i for i, (x, y) in enumerate(zip(both, [k for k in kb if k in ka])) if x != y]
        print(f"{unit}: {len(ka)} kernels in A, {len(kb)} in B: {len(same)} identical, {len(both) - len(same)} "
              f"differing, {len(ka) - len(both)} only in A, {len(kb) - len(both)} only in B; emitted in "
              + (f"another order from common kernel {moved[0] + 1} on" if moved else "the same order")
              + "; figures: " + " / ".join(FIGURES))
        for k in both:
            fa, fb = ka[k][1], kb[k][1]
            if ka[k][0] != kb[k][0] or fa != fb or o.v:
                la, lb = ka[k][0].split("\n"), kb[k][0].split("\n")
                n = sum(1 for d in difflib.ndiff(la, lb) if d[0] in "+-") if la != lb else 0
                print(f"  {f'DIFFERS ({len(la)} / {len(lb)} lines, {n} of them)' if n else 'identical'}  {k}\n"
                      f"      {' / '.join(fa)}" + ("" if fa == fb else f"  ->  {' / '.join(fb)}  FIGURES DIFFER"))
        for tag, x, y in (("A", ka, kb), ("B", kb, ka)):
            for k in x:
                if k not in y:
                    print(f"  only in {tag}  {k}\n      {' / '.join(x[k][1])}")
        bad += len(ka) + len(kb) - 2 * len(same)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
