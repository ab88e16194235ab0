"""One row of a case module (tests/build_cases.py, tests/interact_cases.py) through its entry point, once -- for a
kernel trace; and the comparison of two sets of such traces.

  rocprofv3 --kernel-trace --output-format csv -d DIR/CASE -- python tools/launch_trace.py [--cases MODULE] CASE
      (DLRM_HIP_LIB selects the library: the parent's, built by tools/ab_build.sh, or this tree's)
  python tools/launch_trace.py [--cases MODULE] --compare PARENT_DIR THIS_DIR
      per case of the module's GPU_CASES: the ordered kernels of this library (name with template arguments, grid,
      workgroup, dynamic LDS bytes) in both traces must be equal, and must hold the kernels the row expects
      (build_cases: FORM_KERNELS of its form; interact_cases: the kernel its plan spells, or none of the site's
      family where the plan refuses).  Prints one line per case and a verdict; exit status 1 on any difference.
MODULE: build_cases (the default) or interact_cases.
"""
import csv
import glob
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(cases, name):
    import torch

    import dlrm_pkg
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    case = cases.BY_NAME[name]
    if cases.__name__ == "build_cases":
        rc, ix, _, _, ts = cases.drive(pkg, dev, case)
        torch.cuda.synchronize()
        ts.ctx.check_bounds()
        print(f"{name}: rc {rc} state {ix.state():#x} lib {pkg._lib.LIB_PATH}")
        return 0 if rc == case.expected[7] else 1
    rc = cases.drive(pkg, dev, case)
    torch.cuda.synchronize()
    print(f"{name}: rc {rc} lib {pkg._lib.LIB_PATH}")
    return 0 if rc == 0 else 1  # (a shape without the site's kernel: the ABI's other route, still DLRM_OK)


def kernels(d):
    """The library's kernels of one trace directory, in launch order."""
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        return None
    rows = []
    with open(paths[0], newline="") as f:
        for r in csv.DictReader(f):
            if "dlrm::" not in r["Kernel_Name"]:
                continue
            # (dispatch order, not start time: a side-stream build starts beside the forward)
            # (the demangler closes nested template arguments as "> >": spelled ">>" here, as the case modules do)
            rows.append((int(r["Dispatch_Id"]), r["Kernel_Name"].replace("> >", ">>"),
                         tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"),
                         int(r["LDS_Block_Size"])))
    rows.sort()
    return [r[1:] for r in rows]


def expected_kernels(cases, case):
    """(substrings the trace's kernel names must hold, in order; substrings none may hold)"""
    if cases.__name__ == "interact_cases":
        name = case.expected[0]
        if name == cases.UNSUPPORTED:  # (the traced rows that refuse are the step forward's)
            return [], ["interact_fwd_index_kernel"]
        return ["dlrm::" + name + "("], []
    form, kind = case.expected[0], case.expected[1]
    if case.site == "in_apply":  # the apply launch carries it: sgd_apply_kernel<TT, GT, VPR, MODE, ...>
        return [f", {cases.APPLY_MODE[kind.rstrip('0123456789')]}, dlrm::Descent>"], []
    return cases.FORM_KERNELS[(form, kind)], []


def compare(cases, pdir, tdir):
    bad = 0
    for name in cases.GPU_CASES:
        case = cases.BY_NAME[name]
        a, b = kernels(os.path.join(pdir, name)), kernels(os.path.join(tdir, name))
        if a is None or b is None:
            print(f"{name}: MISSING trace ({'parent' if a is None else 'this tree'})")
            bad += 1
            continue
        same = a == b
        want, never = expected_kernels(cases, case)
        names = [k[0] for k in a]
        pos, held = 0, not any(w in n for w in never for n in names)
        for w in want:  # in order
            hit = next((i for i in range(pos, len(names)) if w in names[i]), None)
            held, pos = held and hit is not None, (hit + 1 if hit is not None else pos)
        short = [n.split("dlrm::", 1)[1].split("(")[0][:110] + f" grid{g} wg{w} lds{l}" for n, g, w, l in a]
        print(f"{name}: {len(a)} kernels, {'identical' if same else 'DIFFERENT'}, expected {' / '.join(map(str, case.expected[:2]))} "
              f"{'held' if held else 'NOT HELD'} by the parent's launches: " + "; ".join(short))
        if not same:
            print("   this tree: " + "; ".join(f"{n.split('dlrm::', 1)[1][:110]} grid{g} wg{w} lds{l}" for n, g, w, l in b))
        bad += (not same) + (not held)
    print("launch_trace: " + ("every list equal, every expected kernel held" if not bad else f"{bad} FAILURES"))
    return 1 if bad else 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    module = "build_cases"
    if argv[:1] == ["--cases"]:
        module, argv = argv[1], argv[2:]
    cases = importlib.import_module(module)
    if len(argv) == 3 and argv[0] == "--compare":
        sys.exit(compare(cases, argv[1], argv[2]))
    sys.exit(run(cases, argv[0]))
