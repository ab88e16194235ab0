"""Writes tests/golden/fwd_window.npz: the one-hot forward's output bits, case by case, as the
commit named in the file computed them (tests/test_fwd_window.py compares the working tree's
against them with np.array_equal).

The fused and the two-operator forwards share one body, so comparing them with each other cannot
see a changed summation order; random floats are not exactly summable, so any reordering of the
Gram sums flips bits.  The reference is therefore the output of the commit before the forward's
row loads were rolled into a window, recorded once on an MI355X:

    python tests/golden/make_fwd_window.py        (on the GPU, at the commit to record)

The file holds outputs only (fp32 as float32, bf16 as their uint16 bits) and the commit's hash;
inputs are regenerated from fixed numpy seeds by `inputs` below, which the test imports too.
"""
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "fwd_window.npz")

# name -> (dtype, d, tables, B, pad_to, form).  F = tables + 1; W = d + F (F - 1) / 2 (+ padding).
# form: "fwd" the fused forward without ys, "ys" with ys kept, "step" dlrm_step_fwd with the
# indexer built in its launch, "oob" the fused forward with one out-of-range index.
CASES = {
    # the metric instantiation (fp32, d = 128, NB = 2): a partial last workgroup, W = 479 (unaligned rows)
    "f32_d128_t26_b6": ("f32", 128, 26, 6, 1, "fwd"),
    "f32_d128_t26_b6_pad8": ("f32", 128, 26, 6, 8, "fwd"),    # W = 480: aligned rows (16-B row stores)
    "f32_d128_t26_b6_pad64": ("f32", 128, 26, 6, 64, "fwd"),  # W = 512: 33 padding columns
    "f32_d128_t16_b5": ("f32", 128, 16, 5, 1, "fwd"),         # F = 17: second 16-row block nearly empty
    "f32_d128_t8_b4": ("f32", 128, 8, 4, 1, "fwd"),           # F = 9: NB = 1
    "bf16_d128_t26_b6": ("bf16", 128, 26, 6, 1, "fwd"),       # four column steps per block: the window clamps
    "f32_d48_t26_b5": ("f32", 48, 26, 5, 1, "fwd"),           # generic kernel: column steps past d
    "f32_d256_t26_b5": ("f32", 256, 26, 5, 1, "fwd"),         # generic kernel: four column blocks
    "f32_d128_t26_b1": ("f32", 128, 26, 1, 1, "fwd"),
    "f32_d128_t26_b6_ys": ("f32", 128, 26, 6, 1, "ys"),
    "f32_d128_t26_b6_step": ("f32", 128, 26, 6, 1, "step"),
    "f32_d128_t26_b6_oob": ("f32", 128, 26, 6, 1, "oob"),
}
OOB_TABLE, OOB_SAMPLE = 5, 2  # the out-of-range index of the "oob" case: one past table 5's last row


def rows_of(tables):
    """Row counts: a few thousand at most, a one-row table among them."""
    return [1 + (t * 389) % 2900 for t in range(tables)]


def inputs(name):
    """(tables [n_t][d] float32, idx [T][B] int32, x [B][d] float32) of a case, from its seed.  The
    three d = 128, 26-table, B = 6 forms share their inputs with f32_d128_t26_b6 (one seed)."""
    dtype, d, T, B, pad_to, form = CASES[name]
    rng = np.random.default_rng(zlib.crc32(repr((dtype, d, T, B)).encode()))
    rows = rows_of(T)
    tables = [rng.standard_normal((n, d)).astype(np.float32) for n in rows]
    idx = np.stack([rng.integers(0, n, B) for n in rows]).astype(np.int32)
    x = rng.standard_normal((B, d)).astype(np.float32)
    if form == "oob":
        idx[OOB_TABLE, OOB_SAMPLE] = rows[OOB_TABLE]
    return tables, idx, x


def run_case(pkg, dev, name):
    """Runs a case on the GPU.  Returns (out as float32 or uint16 bits, ys or None, raised: whether
    the bounds check after the launch raised)."""
    import torch
    dtype, d, T, B, pad_to, form = CASES[name]
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    tables, idx, x = inputs(name)
    ts = pkg.EmbeddingTableSet([torch.from_numpy(t).to(dev).to(tdt) for t in tables])
    pk = pkg.PackedIndices(torch.from_numpy(idx).to(dev).reshape(T, B, 1))
    hp = pkg.HotPath(ts, B, 1, lr=0.01, index_base=0, pad_to=pad_to, materialize_ys=(form == "ys"))
    hp.out.fill_(float("nan"))
    xd = torch.from_numpy(x).to(dev).to(tdt)
    if form == "step":
        hp.step_fwd(xd, pk)
    else:
        hp.lookup_interact_fwd(xd, pk)
    torch.cuda.synchronize()
    raised = False
    try:
        hp.check_bounds()
    except pkg.BoundsError:
        raised = True
    out = hp.out if dtype == "f32" else hp.out.view(torch.int16)
    out = out.cpu().numpy()
    return (out if dtype == "f32" else out.view(np.uint16)), (hp.ys.cpu().numpy() if form == "ys" else None), raised


def main():
    import torch
    sys.path.insert(0, ROOT)
    import dlrm_pkg
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    head = os.environ.get("DLRM_HEAD") or subprocess.run(
        ["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    if not head:
        raise SystemExit("name the recorded commit in DLRM_HEAD (no git checkout here)")
    blobs = {"commit": np.array(head)}
    for name in CASES:
        out, _, raised = run_case(pkg, dev, name)
        assert raised == (CASES[name][5] == "oob"), name
        assert CASES[name][0] == "bf16" or not np.isnan(out).any(), name  # every element written
        blobs[name] = out
    np.savez_compressed(PATH, **blobs)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes, commit {head}")


if __name__ == "__main__":
    main()
