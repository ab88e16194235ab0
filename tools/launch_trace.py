"""One row of tests/build_cases.py through its entry point, once -- for a kernel trace; and the comparison of two
sets of such traces.

  rocprofv3 --kernel-trace --output-format csv -d DIR/CASE -- python tools/launch_trace.py CASE
      (DLRM_HIP_LIB selects the library: the parent's, built by tools/ab_build.sh, or this tree's)
  python tools/launch_trace.py --compare PARENT_DIR THIS_DIR
      per case of build_cases.GPU_CASES: the ordered kernels of this library (name, grid, workgroup, dynamic LDS
      bytes) in both traces must be equal, and must hold the kernels of the row's expected form
      (build_cases.FORM_KERNELS).  Prints one line per case and a verdict; exit status 1 on any difference.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_cases  # noqa: E402


def run(name):
    import torch

    import dlrm_pkg
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    rc, ix, _, _, ts = build_cases.drive(pkg, dev, build_cases.BY_NAME[name])
    torch.cuda.synchronize()
    ts.ctx.check_bounds()
    print(f"{name}: rc {rc} state {ix.state():#x} lib {pkg._lib.LIB_PATH}")
    return 0 if rc == build_cases.BY_NAME[name].expected[7] else 1


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
            rows.append((int(r["Dispatch_Id"]), r["Kernel_Name"],
                         tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"),
                         int(r["LDS_Block_Size"])))
    rows.sort()
    return [r[1:] for r in rows]


def expected_kernels(case):
    form, kind = case.expected[0], case.expected[1]
    if case.site == "in_apply":  # the apply launch carries it: sgd_apply_kernel<TT, GT, VPR, MODE, ...>
        return [f", {build_cases.APPLY_MODE[kind.rstrip('0123456789')]}, dlrm::Descent>"]
    return build_cases.FORM_KERNELS[(form, kind)]


def compare(pdir, tdir):
    bad = 0
    for name in build_cases.GPU_CASES:
        case = build_cases.BY_NAME[name]
        a, b = kernels(os.path.join(pdir, name)), kernels(os.path.join(tdir, name))
        if a is None or b is None:
            print(f"{name}: MISSING trace ({'parent' if a is None else 'this tree'})")
            bad += 1
            continue
        same = a == b
        want = expected_kernels(case)
        names = [k[0] for k in a]
        pos, held = 0, True
        for w in want:  # in order
            hit = next((i for i in range(pos, len(names)) if w in names[i]), None)
            held, pos = held and hit is not None, (hit + 1 if hit is not None else pos)
        short = [n.split("dlrm::", 1)[1].split("(")[0][:60] + f" grid{g} wg{w} lds{l}" for n, g, w, l in a]
        print(f"{name}: {len(a)} kernels, {'identical' if same else 'DIFFERENT'}, form {case.expected[0]}/{case.expected[1]} "
              f"{'held' if held else 'NOT HELD'} by the parent's launches: " + "; ".join(short))
        if not same:
            print("   this tree: " + "; ".join(f"{n.split('dlrm::', 1)[1][:60]} grid{g} wg{w} lds{l}" for n, g, w, l in b))
        bad += (not same) + (not held)
    print("launch_trace: " + ("every list equal, every expected form held" if not bad else f"{bad} FAILURES"))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(run(sys.argv[1]))
