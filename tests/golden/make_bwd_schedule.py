"""Writes tests/golden/bwd_schedule.npz: the step backward's output bits (dx, dt, the touched table rows), case by
case, as the commit named in the file computed them (tests/test_bwd_schedule.py compares the working tree's against
them with np.array_equal).

The step backward's forms share one kernel text and the operator routes run the same MFMA sequence, so comparing them
with each other cannot see a changed summation order; random floats are not exactly summable, so any reordering of
an accumulator's steps flips bits.  The reference is therefore the output of the commit before the backward's
schedule was changed (row loads issued off the index load, MFMAs tracking the arrivals), recorded once on an MI355X:

    python tests/golden/make_bwd_schedule.py        (on the GPU, at the commit to record)

Each case runs dlrm_step_fwd (the indexer built in its launch), then dlrm_step_bwd with DLRM_STEP_BWD_ONLY on dx and
dt filled with a sentinel.  The file holds outputs only (fp32 as float32, bf16 as their uint16 bits) and the commit's
hash; inputs are regenerated from fixed numpy seeds by `inputs` below, which the test imports too.
"""
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "bwd_schedule.npz")
SENTINEL = -777.25  # dx and dt before the launch: what it does not write keeps this
LR = 0.01

# name -> (dtype, d, tables, B, form).  F = tables + 1.
# form: "plain"; "ld" dout with a padded leading dimension; "base1" indices + 1 with index base 1 (both compute what
# SAME_AS names, bit for bit, and are compared with its record); "oob" one out-of-range index.
CASES = {
    # the metric instantiation (fp32, d = 128, NB = 2, 4 samples per block): a partial last block
    "f32_d128_t26_b6": ("f32", 128, 26, 6, "plain"),
    "f32_d128_t26_b1": ("f32", 128, 26, 1, "plain"),       # a single sample: every row once-hit
    "f32_d128_t16_b5": ("f32", 128, 16, 5, "plain"),       # F = 17: tile row 1 holds one feature
    "f32_d128_t8_b4": ("f32", 128, 8, 4, "plain"),         # F = 9: NB = 1
    "f32_d128_t26_b6_ld": ("f32", 128, 26, 6, "ld"),       # dout_ld = W + 5
    "f32_d128_t26_b3_oob": ("f32", 128, 26, 3, "oob"),     # error raised, no table row written
    "f32_d128_t26_b6_base1": ("f32", 128, 26, 6, "base1"),
    # forms that keep the kernel's text
    "f32_d16_t26_b6": ("f32", 16, 26, 6, "plain"),         # one wave per sample
    "bf16_d128_t26_b4": ("bf16", 128, 26, 4, "plain"),     # bf16 rows, two waves per sample
}
SAME_AS = {"f32_d128_t26_b6_ld": "f32_d128_t26_b6", "f32_d128_t26_b6_base1": "f32_d128_t26_b6"}
OOB_TABLE, OOB_SAMPLE = 5, 1  # the out-of-range index of the "oob" case: one past table 5's last row


def rows_of(tables):
    """Row counts: even tables 1..3 rows (repeated rows in any batch of more than 3), odd tables above a thousand
    (once-hit rows) -- so each group of four features, in either tile row, holds both kinds."""
    return [1 + t % 3 if t % 2 == 0 else 1000 + 37 * t for t in range(tables)]


def inputs(name):
    """(tables [n_t][d] float32, idx [T][B] int32 (base 0), x [B][d], dout [B][W]) of a case, from its seed; the
    forms of one shape share their inputs.  A large table's indices are distinct."""
    dtype, d, T, B, form = CASES[name]
    rng = np.random.default_rng(zlib.crc32(repr((dtype, d, T, B)).encode()))
    rows = rows_of(T)
    tables = [rng.standard_normal((n, d)).astype(np.float32) for n in rows]
    idx = np.stack([rng.integers(0, n, B) if n < 1000 else rng.choice(n, B, replace=False)
                    for n in rows]).astype(np.int32)
    x = rng.standard_normal((B, d)).astype(np.float32)
    F = T + 1
    dout = (rng.standard_normal((B, d + F * (F - 1) // 2)) * 1e-3).astype(np.float32)
    if form == "oob":
        idx[OOB_TABLE, OOB_SAMPLE] = rows[OOB_TABLE]
    return tables, idx, x, dout


def once_hit(idx):
    """[T][B] bool: the position's row is hit once in the batch."""
    return np.stack([np.array([(row == r).sum() == 1 for r in row]) for row in idx])


def run_case(pkg, dev, name):
    """Runs a case on the GPU.  Returns (dx [B][d] float32, dt [B][F d] float32, rows [T][B][d]: the table rows of
    the batch's positions after the launch (float32, or bf16 bits as uint16; the out-of-range position: zeros),
    tables: every table after the launch, raised: whether the bounds check after the launch raised)."""
    import torch
    dtype, d, T, B, form = CASES[name]
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    tables, idx, x, dout = inputs(name)
    base = 1 if form == "base1" else 0
    ts = pkg.EmbeddingTableSet([torch.from_numpy(t).to(dev).to(tdt) for t in tables])
    pk = pkg.PackedIndices(torch.from_numpy(idx + base).to(dev).reshape(T, B, 1))
    hp = pkg.HotPath(ts, B, 1, lr=LR, index_base=base)
    xd = torch.from_numpy(x).to(dev).to(tdt)
    W = dout.shape[1]
    dd = torch.zeros((B, W + (5 if form == "ld" else 0)), dtype=tdt, device=dev)[:, :W]
    dd.copy_(torch.from_numpy(dout).to(dev).to(tdt))
    hp.dx.fill_(SENTINEL)
    hp.dt.fill_(SENTINEL)
    hp.step_fwd(xd, pk)
    hp.step_bwd(dd, flags=pkg._lib.STEP_BWD_ONLY)
    torch.cuda.synchronize()
    raised = False
    try:
        hp.check_bounds()
    except pkg.BoundsError:
        raised = True

    def host(t):
        return t.cpu().numpy() if t.dtype == torch.float32 else t.view(torch.int16).cpu().numpy().view(np.uint16)

    after = [host(t.data) for t in ts]
    rows = np.zeros((T, B, d), dtype=after[0].dtype)
    for t in range(T):
        for b in range(B):
            if idx[t, b] < after[t].shape[0]:
                rows[t, b] = after[t][idx[t, b]]
    return hp.dx.cpu().numpy(), hp.dt.cpu().numpy(), rows, after, raised


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
    got = {}
    for name in CASES:
        dx, dt, rows, _, raised = run_case(pkg, dev, name)
        assert raised == (CASES[name][4] == "oob"), name
        assert not (dx == SENTINEL).any(), name  # every dx element written
        got[name] = (dx, dt, rows)
        if name in SAME_AS:
            for a, b in zip(got[name], got[SAME_AS[name]]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
            continue
        blobs[name + "/dx"], blobs[name + "/dt"], blobs[name + "/rows"] = dx, dt, rows
    np.savez_compressed(PATH, **blobs)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes, commit {head}")


if __name__ == "__main__":
    main()
