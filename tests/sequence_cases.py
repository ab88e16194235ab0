"""One indexer across builds of different forms, sizes and tables: the scripts as literal rows, and their inputs.

Shared by tests/test_indexer_sequences.py (GPU: every step through the real entry points on ONE indexer, each followed
by check_build) and tests/test_sequence_cases_host.py (CPU: the forms through tests/build_plan_print.cpp, the
exactness of the gradients and the segment classes of the hot steps, all on the inputs alone).

A script: Script(name, cap, rows, steps); the indexer is dlrm_indexer_create(len(rows), cap).
A step:   S(site, N, form, kind, L=1, i64=False, hot=False, chunk=32, parts=0, rc=0, absent=())
  site         the entry point (build_cases.SITES)
  N, L         positions per table (batch * lookups) and lookups per bag
  form, kind   the form plan_build picks, as build_cases.CASES names it -- read off the rows of CASES by hand
               (the host test holds them against plan_build: a changed plan fails the step's row)
  i64          int64 indices (else int32)
  hot          the step is run on two fresh draws of indices, and every segment class the apply distinguishes must
               occur in each (CLASSES; `absent`: the classes the step's settings make impossible, with the reason
               beside the row)
  chunk, parts dlrm_indexer_set_chunk / dlrm_indexer_set_parts in force at the step (set before it where it changes)
  rc           the entry point's return code (DLRM_E_UNSUPPORTED = -4: refused, the previous build stands)

The scan build with 8 waves per workgroup is reached by no script: its T * 2^vshift / 4 workgroups must exceed the
compute units, which needs 17 tables of 64 parts.
"""
import zlib
from collections import namedtuple

import numpy as np

import build_cases

M = 1 << 20
ROWS, ROWS_2, DIM = [3, 64, 300, 5000], [3, 5000], 16
E_UNSUPPORTED = -4
# constants of csrc/indexer.hpp the classes rest on (kChunkInline, kMinChunk, kChunk, kHotSlice)
INLINE, MIN_CHUNK, CHUNK, HOT_SLICE = 5, 16, 32, 256
# the segment classes of the apply, by positions per row: once-hit; a chunk whose positions all travel with its
# descriptor; longer chunks on both sides of set_chunk(16); a hot segment of one slice; one of several slices,
# combined through partial rows and hot_cnt
CLASSES = [("once", 1, 1), ("inline", 2, INLINE), ("chunk16", INLINE + 1, MIN_CHUNK), ("chunk32", MIN_CHUNK + 1, CHUNK),
           ("slice", CHUNK + 1, HOT_SLICE), ("slices", HOT_SLICE + 1, 1 << 31)]

Step = namedtuple("Step", "site N form kind L i64 hot chunk parts rc absent")
Script = namedtuple("Script", "name cap rows steps")


def S(site, N, form, kind="-", L=1, i64=False, hot=False, chunk=32, parts=0, rc=0, absent=()):
    return Step(site, N, form, kind, L, i64, hot, chunk, parts, rc, tuple(absent))


SCRIPTS = [
    # capacity 4096: one virtual table per table, no hash arrays
    Script("A", 4096, ROWS, [
        S("build", 4096, "lds4", L=4, hot=True),
        S("build", 300, "lds2"),
        S("build_split", 2049, "lds4"),
        S("prepare", 2048, "wave", "one", hot=True),
        S("step_fwd", 2048, "in_forward", "one", hot=True),
        S("build", 17, "lds2"),
        S("build_split", 4096, "lds4"),
        S("prepare", 2049, "wave", "rounds"),
        S("in_apply", 2048, "wave", "one", hot=True),
        S("build", 1, "lds2"),
        S("build", 4096, "lds4"),
    ]),
    # capacity 8192: 8 virtual tables per table (the in-LDS parts build's layout), hash arrays
    Script("B", 8192, ROWS, [
        S("build", 8192, "lds_parts", L=4, hot=True),
        S("build", 3000, "lds4"),
        S("build_split", 6000, "bag", hot=True),
        S("build", 6000, "lds_parts"),
        S("prepare", 8192, "wave", "scan16", hot=True),
        S("build", 2048, "lds2", hot=True),
        S("prepare", 2052, "wave", "rounds", i64=True),
        S("build_split", 3000, "lds4"),
        S("step_fwd", 6000, "lds_parts"),  # (no forward-launch build above 2048 positions: on the side stream)
        S("build", 8192, "lds_parts"),
    ]),
    Script("C", 32768, ROWS, [
        S("build", 32768, "bag", L=4, hot=True),
        S("build", 100, "lds2"),
        S("build", 6000, "hash", hot=True),
        S("build_split", 6000, "bag"),
        # (256 parts per table.  No row of 17 to 32 positions at this N: the tables' rows average 5463, 256, 55 and
        # 3.3 positions, and neither 55 - 3 sigma nor 3.3 + 7 sigma reaches the range)
        S("prepare", 16388, "wave", "scan16", hot=True, absent=["chunk32"]),
        S("build", 9000, "bag"),
        S("prepare", 2048, "wave", "one"),
        S("prepare", 2048, "wave", "one", parts=64, hot=True),
        S("prepare", 2048, "wave", "one", parts=64, chunk=16, hot=True),
        S("build", 20000, "bag", L=4, parts=64),
        S("step_fwd", 2048, "in_forward", parts=64, hot=True),  # (capacity above 16384: in LDS per table)
        S("build_split", 32768, "bag", parts=64),
        S("prepare", 32768, "wave", "scan16", parts=64, hot=True),
    ]),
    Script("D", 40000, ROWS, [
        S("build", 40000, "hash", hot=True),
        S("build", 8193, "bag"),
        S("build", 33000, "hash"),
        S("build_split", 40000, "hash", hot=True),
        S("build", 5000, "hash"),
        S("build", 2000, "lds2"),
        S("build", 40000, "hash"),
    ]),
    # capacity 2^20 + 1, two tables: the sorted unsplit build, and the two refusals after it
    Script("E", M + 1, ROWS_2, [
        S("build", M + 1, "sorted"),
        S("build", 2048, "lds2"),
        S("build_split", 20000, "bag"),
        S("build", M + 1, "sorted"),
        S("build_split", M + 1, "none", rc=E_UNSUPPORTED),
        S("prepare", 40000, "none", rc=E_UNSUPPORTED),
    ]),
]
BY_NAME = {s.name: s for s in SCRIPTS}

# The interrupted histories, each on capacities 8192 and 32768 with the multi-slice hot table present (the 3-row
# table: three or more slices per row from 2048 positions): per capacity (the interrupted step, the clean step of
# ANOTHER form that follows it).  What interrupts the first step is the test's (tests/test_indexer_sequences.py).
HISTORIES = {
    "bounds_build": {8192: (S("build", 6000, "lds_parts"), S("build_split", 6000, "bag")),
                     32768: (S("build", 9000, "bag"), S("build", 6000, "hash"))},
    "bounds_prepare": {8192: (S("prepare", 8192, "wave", "scan16"), S("build", 3000, "lds4")),
                       32768: (S("prepare", 16388, "wave", "scan16"), S("build", 9000, "bag"))},
    "never_applied": {8192: (S("build_split", 6000, "bag"), S("build", 8192, "lds_parts")),
                      32768: (S("build", 6000, "hash"), S("build_split", 6000, "bag"))},
    "never_consumed": {8192: (S("prepare", 2052, "wave", "scan16"), S("build", 6000, "lds_parts")),
                       32768: (S("prepare", 2048, "wave", "one"), S("build", 6000, "hash"))},
    "bwd_without_apply": {8192: (S("step_fwd", 2048, "in_forward", "one"), S("prepare", 2048, "wave", "one")),
                          32768: (S("step_fwd", 2048, "in_forward"), S("build", 9000, "bag"))},
    "next_build_never_used": {8192: (S("in_apply", 2048, "wave", "one"), S("build", 6000, "lds_parts")),
                              32768: (S("in_apply", 2052, "wave", "scan"), S("build", 6000, "hash"))},
}
# Another table set on the same indexer: capacity 8192, 4096 positions per table, hot
TABLE_SET_CAP, TABLE_SET_STEP = 8192, S("build", 4096, "lds4", hot=True)
TABLE_SETS = [("float32", 16), ("float32", 512), ("float32", 512), ("float32", 16), ("bfloat16", 128), ("float32", 512)]


def as_case(cap, rows, st, name="step"):
    """The step as a row of build_cases (expected: the eight columns are not the script's to state; form, kind and the
    return code are)."""
    caps = {}
    if st.site == "step_fwd" and st.N > 2048:
        caps["step_fwd"] = 0  # (what step_fwd_supported answers for the size: no forward-launch build)
    if st.i64 or st.N % 4:
        caps["idx_vec32"] = 0  # (int64, or a table's int32 indices not 16-B aligned)
    return build_cases.C(name, st.site, cap, st.N, (st.form, st.kind, st.rc), T=len(rows), L=st.L,
                         set_parts={0: 0, 16: 4, 32: 5, 64: 6}[st.parts], caps=caps)


def form_class(st):
    """The class of a step's form for the transition counts: the wave build by its kernel."""
    return "wave_" + st.kind if st.form == "wave" else st.form


# ---- inputs: a function of (script or test name, step number, draw) alone
def _rng(name, k, draw, what):
    return np.random.default_rng([zlib.crc32(name.encode()), k, draw, what])


def draw_indices(name, k, draw, rows, N):
    """[T][N] int64, uniform per table."""
    rng = _rng(name, k, draw, 0)
    return np.stack([rng.integers(0, n, size=N) for n in rows])


def exact_k(N):
    """The largest power of two K <= 256 with N * K < 2^24: sums of N terms k / 64, |k| <= K, are exact in fp32 in
    any order (every partial sum is an integer below 2^24 over 64)."""
    K = 256
    while N * K >= 1 << 24:
        K //= 2
    assert K >= 1
    return K


def draw_exact(name, k, draw, B, width, N):
    """[B][width] integers k, |k| <= exact_k(N): the gradient is k / 64."""
    K = exact_k(N)
    return _rng(name, k, draw, 1).integers(-K, K + 1, size=(B, width)).astype(np.int32)


def draw_normal(name, k, draw, B, width):
    return _rng(name, k, draw, 2).standard_normal((B, width), dtype=np.float32)


def scatter_sums(idx_t, kt, n, L):
    """float64 [n][D]: per row of the table the sum of the integer gradients kt [B][D] of its positions (position p
    belongs to bag p // L).  np.bincount sums in float64: exact for integers of this size."""
    bag = np.arange(idx_t.shape[0]) // L
    return np.stack([np.bincount(idx_t, weights=kt[bag, c].astype(np.float64), minlength=n) for c in range(kt.shape[1])],
                    axis=1)


def classes_present(idx, chunk=CHUNK):
    """The names of CLASSES that occur in idx [T][N]."""
    seen = set()
    for row in idx:
        c = np.bincount(row)
        for name, lo, hi in CLASSES:
            if ((c >= lo) & (c <= hi)).any():
                seen.add(name)
    return seen
