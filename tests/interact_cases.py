"""Which interaction kernel a call launches: the table of DESIGN.md section 22 as literal rows.

Shared by tests/test_interact_plan_host.py (every row, through csrc/interact_plan.hpp's interact_align and
plan_interact in a stand-alone host program) and tools/launch_trace.py (the rows of GPU_CASES through the real entry
points, one per process, for a kernel trace).

A row: C(name, site, expected, dtype=F32, d=16, F=3, B=8, L=1, ys=0, rule="descent", knobs={...}, ptr={...},
         tabs16=1, max_rows=5000).
  site      the launcher that asks (SITES)
  d, F, B   feature size, features (tables + 1) and batch; L lookups per bag; ys: lookup_fwd keeps the gathered rows
  rule      step_bwd: the optimizer rule (RULES)
  knobs     the environment knobs that differ from 0 (csrc/build_plan.hpp Knobs: bwd_ys_body is DLRM_BWD_YS=0,
            bwd_nosplit DLRM_BWD_SPLIT=0, the other three their variables' values)
  ptr       {"x" | "t" | "dx" | "dt": (address, leading dimension)} where they differ from the site's defaults
            (pointers(): address 4096, packed rows; "t" is ys or the backward's materialized ys, "dt" the blocked
            backward's dst with leading dimension 0)
  tabs16    every table row 16-B aligned; max_rows: the largest table's rows (-1: no host descriptors)
  expected  (kernel, extras): the kernel as a trace spells it, template arguments included, or UNSUPPORTED / NOTHING
            (no launch, DLRM_E_UNSUPPORTED / DLRM_OK); extras: "tp" the table pointers travel by value, "ix" the
            index build rides in the launch, "first" the indexer's own launch goes first
Every row was read against the parent's launchers in interact.hip by hand (a row is no copy of what plan_interact
says today: changing plan_interact must fail the row); tools/launch_trace.py's comparison
(profiles/interact_plan/launch_diff.txt) holds the kernels of GPU_CASES against what the parent's library launched.
"""
from collections import namedtuple

SITES = ["fwd", "lookup_fwd", "bwd", "bwd_gather", "bwd_gather_ix", "bwd_blocked", "step_fwd", "step_bwd"]
RULES = ["descent", "split", "adagrad", "rowwise", "stochastic"]
KNOBS = ["bwd_ys_body", "bwd_nosplit", "bwd_spb", "bwd_cpl", "upd_sbu"]
F32, BF16 = 0, 1  # DLRM_F32, DLRM_BF16
E_UNSUPPORTED = -4

Case = namedtuple("Case", "name site expected dtype d F B L ys rule knobs ptr tabs16 max_rows")


def C(name, site, expected, dtype=F32, d=16, F=3, B=8, L=1, ys=0, rule="descent", knobs=None, ptr=None, tabs16=1,
      max_rows=5000):
    if isinstance(expected, str):
        expected = (expected, "")
    return Case(name, site, expected, dtype, d, F, B, L, ys, rule, knobs or {}, ptr or {}, tabs16, max_rows)


A0 = 4096  # a 16-B aligned address


def pointers(c):
    """{"x", "t", "dx", "dt"} -> (address, leading dimension) of the case: what its site passes, then c.ptr."""
    row, rows = (A0, c.d), (A0, c.F * c.d)
    p = {"fwd": dict(x=row, t=rows), "lookup_fwd": dict(x=row, t=rows if c.ys else (0, 0)),
         "bwd": dict(t=rows, dx=row, dt=rows), "bwd_gather": dict(x=row, dx=row, dt=rows),
         "bwd_gather_ix": dict(x=row, dx=row, dt=rows), "bwd_blocked": dict(x=row, dx=row, dt=(A0, 0)),
         "step_fwd": dict(x=row), "step_bwd": dict(x=row)}[c.site]
    assert set(c.ptr) <= set(p), c.name
    return {k: c.ptr.get(k, p.get(k, (0, 0))) for k in ("x", "t", "dx", "dt")}


def encode(c):
    """The case as interact_plan_print's input line."""
    p = pointers(c)
    return " ".join(str(v) for v in [SITES.index(c.site), c.dtype, c.d, c.F, c.B, c.L, c.ys, *p["x"], *p["t"], *p["dx"],
                                     *p["dt"], c.tabs16, c.max_rows] + [c.knobs.get(k, 0) for k in KNOBS] +
                    [RULES.index(c.rule)])


# ---- the kernels as a trace spells them
FL, BF = "float", "unsigned short"
SU = {"descent": "dlrm::StepUpdate", "split": "dlrm::SplitStepUpdate", "adagrad": "dlrm::AdagradStepUpdate<false>",
      "rowwise": "dlrm::AdagradStepUpdate<true>", "stochastic": "dlrm::StochasticStepUpdate"}
UNSUPPORTED, NOTHING = "unsupported", "nothing"


def b(v):
    return "true" if v else "false"


def fwd_scalar(T):
    return f"interact_fwd_scalar<{T}>"


def fwd(T, NB, fused, pooled=0, DC=0):  # (4: its waves per workgroup, the template's default)
    return f"interact_fwd_kernel<{T}, {NB}, {b(fused)}, {b(pooled)}, {DC}, 4>"


def fwd_index(T, NB, DC=0):
    return f"interact_fwd_index_kernel<{T}, {NB}, {DC}>"


def bwd_scalar(T, gather):
    return f"interact_bwd_scalar<{T}, {b(gather)}>"


def bwd(T, NB, gather):
    return f"interact_bwd_kernel<{T}, {NB}, {b(gather)}>"


def bwd_index(T, NB):
    return f"interact_bwd_index_kernel<{T}, {NB}>"


def split(T, NB, DC, SPB, WPS, mapped=0, CPL=4, ys=0, rule="descent"):
    return f"interact_bwd_split_kernel<{T}, {NB}, {DC}, {SPB}, {WPS}, {b(mapped)}, {CPL}, {b(ys)}, {SU[rule]}>"


def update(T, NB, SBU, DC, rule="descent"):
    return f"interact_bwd_update_kernel<{T}, {NB}, {SBU}, {DC}, {SU[rule]}>"


def spelled(f, rule):
    """An answer line of interact_plan_print (split into words) for a case of `rule` as an `expected`."""
    kernel, (rc, f32, NB, DC, WPS, CPL, SPB, SBU, fused, pooled, gather, mapped, ys, tp, ix, first) = f[0], map(int, f[1:])
    T = FL if f32 else BF
    extras = ",".join(n for n, v in (("tp", tp), ("ix", ix), ("first", first)) if v)
    name = {"none": lambda: UNSUPPORTED if rc == E_UNSUPPORTED else NOTHING if rc == 0 else f"rc {rc}",
            "fwd_scalar": lambda: fwd_scalar(T), "fwd": lambda: fwd(T, NB, fused, pooled, DC),
            "fwd_index": lambda: fwd_index(T, NB, DC), "bwd_scalar": lambda: bwd_scalar(T, gather),
            "bwd": lambda: bwd(T, NB, gather), "bwd_index": lambda: bwd_index(T, NB),
            "bwd_split": lambda: split(T, NB, DC, SPB, WPS, mapped, CPL, ys, rule),
            "bwd_update": lambda: update(T, NB, SBU, DC, rule)}[kernel]()
    return name, extras


X8, X4 = {"x": (A0 + 8, 16)}, {"x": (A0 + 4, 16)}
CASES = [
    # ---- F = 16 | 17, 32 | 33, 96 | 97, 112 | 113 (NB 1 | 2, 2 | 3, 6 | 7, 7 | 8), site by site
    C("fwd-F16", "fwd", fwd(FL, 1, 0), F=16),
    C("fwd-F17", "fwd", fwd(FL, 2, 0), F=17),
    C("fwd-F32", "fwd", fwd(FL, 2, 0), F=32),
    C("fwd-F33", "fwd", fwd(FL, 3, 0), F=33),
    C("fwd-F96", "fwd", fwd(FL, 6, 0), F=96),
    C("fwd-F97", "fwd", fwd_scalar(FL), F=97),
    C("fwd-F112", "fwd", fwd_scalar(FL), F=112),
    C("fwd-F113", "fwd", fwd_scalar(FL), F=113),
    C("lookup_fwd-F16", "lookup_fwd", (fwd(FL, 1, 1), "tp"), F=16),
    C("lookup_fwd-F17", "lookup_fwd", (fwd(FL, 2, 1), "tp"), F=17),
    C("lookup_fwd-F32", "lookup_fwd", (fwd(FL, 2, 1), "tp"), F=32),
    C("lookup_fwd-F33", "lookup_fwd", fwd(FL, 3, 1), F=33),
    C("lookup_fwd-F96", "lookup_fwd", fwd(FL, 6, 1), F=96),
    C("lookup_fwd-F97", "lookup_fwd", UNSUPPORTED, F=97),
    C("lookup_fwd-F112", "lookup_fwd", UNSUPPORTED, F=112),
    C("lookup_fwd-F113", "lookup_fwd", UNSUPPORTED, F=113),
    C("bwd-F16", "bwd", bwd(FL, 1, 0), F=16),
    C("bwd-F17", "bwd", bwd(FL, 2, 0), F=17),
    C("bwd-F32", "bwd", bwd(FL, 2, 0), F=32),
    C("bwd-F33", "bwd", bwd(FL, 3, 0), F=33),
    C("bwd-F96", "bwd", bwd(FL, 6, 0), F=96),
    C("bwd-F97", "bwd", bwd(FL, 7, 0), F=97),
    C("bwd-F112", "bwd", bwd(FL, 7, 0), F=112),
    C("bwd-F113", "bwd", bwd_scalar(FL, 0), F=113),
    # (a materialized ys of d = 64: the split kernel's load plan for 33..96 features)
    C("bwd-d64-F32", "bwd", bwd(FL, 2, 0), d=64, F=32),
    C("bwd-d64-F33", "bwd", split(FL, 3, 0, 1, 1, ys=1), d=64, F=33),
    C("bwd-d64-F96", "bwd", split(FL, 6, 0, 1, 1, ys=1), d=64, F=96),
    C("bwd-d64-F97", "bwd", bwd(FL, 7, 0), d=64, F=97),
    C("bwd_gather-F16", "bwd_gather", bwd(FL, 1, 1), F=16),
    C("bwd_gather-F17", "bwd_gather", bwd(FL, 2, 1), F=17),
    C("bwd_gather-F32", "bwd_gather", bwd(FL, 2, 1), F=32),
    C("bwd_gather-F33", "bwd_gather", bwd(FL, 3, 1), F=33),
    C("bwd_gather-F96", "bwd_gather", bwd(FL, 6, 1), F=96),
    C("bwd_gather-F97", "bwd_gather", bwd(FL, 7, 1), F=97),
    C("bwd_gather-F112", "bwd_gather", bwd(FL, 7, 1), F=112),
    C("bwd_gather-F113", "bwd_gather", bwd_scalar(FL, 1), F=113),
    C("bwd_gather_ix-F16", "bwd_gather_ix", (bwd_index(FL, 1), "ix"), F=16),
    C("bwd_gather_ix-F17", "bwd_gather_ix", (bwd_index(FL, 2), "ix"), F=17),
    C("bwd_gather_ix-F32", "bwd_gather_ix", (bwd_index(FL, 2), "ix"), F=32),
    C("bwd_gather_ix-F33", "bwd_gather_ix", (bwd(FL, 3, 1), "first"), F=33),
    C("bwd_gather_ix-F96", "bwd_gather_ix", (bwd(FL, 6, 1), "first"), F=96),
    C("bwd_gather_ix-F97", "bwd_gather_ix", (bwd(FL, 7, 1), "first"), F=97),
    C("bwd_gather_ix-F112", "bwd_gather_ix", (bwd(FL, 7, 1), "first"), F=112),
    C("bwd_gather_ix-F113", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), F=113),
    C("bwd_blocked-F16", "bwd_blocked", split(FL, 1, 0, 2, 1, mapped=1), F=16),
    C("bwd_blocked-F17", "bwd_blocked", split(FL, 2, 0, 2, 1, mapped=1), F=17),
    C("bwd_blocked-F32", "bwd_blocked", split(FL, 2, 0, 2, 1, mapped=1), F=32),
    C("bwd_blocked-F33", "bwd_blocked", bwd(FL, 3, 1), F=33),
    C("bwd_blocked-F96", "bwd_blocked", bwd(FL, 6, 1), F=96),
    C("bwd_blocked-F97", "bwd_blocked", bwd(FL, 7, 1), F=97),
    C("bwd_blocked-F112", "bwd_blocked", bwd(FL, 7, 1), F=112),
    C("bwd_blocked-F113", "bwd_blocked", UNSUPPORTED, F=113),
    C("step_fwd-F16", "step_fwd", (fwd_index(FL, 1), "tp,ix"), F=16),
    C("step_fwd-F17", "step_fwd", (fwd_index(FL, 2), "tp,ix"), F=17),
    C("step_fwd-F32", "step_fwd", (fwd_index(FL, 2), "tp,ix"), F=32),
    C("step_fwd-F33", "step_fwd", UNSUPPORTED, F=33),
    C("step_fwd-F96", "step_fwd", UNSUPPORTED, F=96),
    C("step_fwd-F97", "step_fwd", UNSUPPORTED, F=97),
    C("step_fwd-F112", "step_fwd", UNSUPPORTED, F=112),
    C("step_fwd-F113", "step_fwd", UNSUPPORTED, F=113),
    C("step_bwd-F16", "step_bwd", split(FL, 1, 0, 8, 1), F=16),
    C("step_bwd-F17", "step_bwd", split(FL, 2, 0, 8, 1), F=17),
    C("step_bwd-F32", "step_bwd", split(FL, 2, 0, 8, 1), F=32),
    C("step_bwd-F33", "step_bwd", UNSUPPORTED, F=33),
    C("step_bwd-F96", "step_bwd", UNSUPPORTED, F=96),
    C("step_bwd-F97", "step_bwd", UNSUPPORTED, F=97),
    C("step_bwd-F112", "step_bwd", UNSUPPORTED, F=112),
    C("step_bwd-F113", "step_bwd", UNSUPPORTED, F=113),
    # ---- d = 64 | 68, 128, 132, 256
    C("fwd-d64", "fwd", fwd(FL, 1, 0), d=64),
    C("fwd-d68", "fwd", fwd(FL, 1, 0), d=68),
    C("fwd-d128", "fwd", fwd(FL, 1, 0, DC=128), d=128),
    C("fwd-d132", "fwd", fwd(FL, 1, 0), d=132),
    C("fwd-d256", "fwd", fwd(FL, 1, 0), d=256),
    C("lookup_fwd-d64", "lookup_fwd", (fwd(FL, 1, 1), "tp"), d=64),
    C("lookup_fwd-d68", "lookup_fwd", (fwd(FL, 1, 1), "tp"), d=68),
    C("lookup_fwd-d128", "lookup_fwd", (fwd(FL, 1, 1, DC=128), "tp"), d=128),
    C("lookup_fwd-d132", "lookup_fwd", (fwd(FL, 1, 1), "tp"), d=132),
    C("lookup_fwd-d256", "lookup_fwd", (fwd(FL, 1, 1), "tp"), d=256),
    # (pooled bags have no d = 128 form)
    C("lookup_fwd-d128-L2", "lookup_fwd", fwd(FL, 1, 1, pooled=1), d=128, L=2),
    C("bwd-F40-d64", "bwd", split(FL, 3, 0, 1, 1, ys=1), d=64, F=40),
    C("bwd-F40-d68", "bwd", bwd(FL, 3, 0), d=68, F=40),
    C("bwd-F40-d128", "bwd", split(FL, 3, 0, 1, 2, ys=1), d=128, F=40),
    C("bwd-F40-d132", "bwd", bwd(FL, 3, 0), d=132, F=40),
    C("bwd-F40-d256", "bwd", split(FL, 3, 0, 1, 4, ys=1), d=256, F=40),
    C("bwd-F40-d512", "bwd", bwd(FL, 3, 0), d=512, F=40),
    C("bwd-F40-d64-bf16", "bwd", split(BF, 3, 0, 1, 1, ys=1), BF16, d=64, F=40),
    C("bwd_gather-d128", "bwd_gather", bwd(FL, 1, 1), d=128),
    C("bwd_blocked-d64", "bwd_blocked", split(FL, 1, 0, 2, 1, mapped=1), d=64),
    C("bwd_blocked-d68", "bwd_blocked", bwd(FL, 1, 1), d=68),
    C("bwd_blocked-d128", "bwd_blocked", split(FL, 1, 128, 4, 2, mapped=1), d=128),
    C("bwd_blocked-d132", "bwd_blocked", bwd(FL, 1, 1), d=132),
    C("bwd_blocked-d256", "bwd_blocked", bwd(FL, 1, 1), d=256),
    C("bwd_blocked-d128-bf16", "bwd_blocked", split(BF, 1, 128, 4, 2, mapped=1), BF16, d=128),
    # (pooled bags: the one-wave kernel)
    C("bwd_blocked-d64-L2", "bwd_blocked", bwd(FL, 1, 1), d=64, L=2),
    C("step_fwd-d64", "step_fwd", (fwd_index(FL, 1), "tp,ix"), d=64),
    C("step_fwd-d68", "step_fwd", (fwd_index(FL, 1), "tp,ix"), d=68),
    C("step_fwd-d128", "step_fwd", (fwd_index(FL, 1, 128), "tp,ix"), d=128),
    C("step_fwd-d132", "step_fwd", (fwd_index(FL, 1), "tp,ix"), d=132),
    C("step_fwd-d256", "step_fwd", (fwd_index(FL, 1), "tp,ix"), d=256),
    C("step_fwd-d128-bf16-F17", "step_fwd", (fwd_index(BF, 2, 128), "tp,ix"), BF16, d=128, F=17),
    C("step_bwd-d64", "step_bwd", split(FL, 1, 0, 8, 1), d=64),
    C("step_bwd-d68", "step_bwd", update(FL, 1, 1, 0), d=68),
    C("step_bwd-d128", "step_bwd", split(FL, 1, 128, 4, 2), d=128),
    C("step_bwd-d132", "step_bwd", update(FL, 1, 1, 0), d=132),
    C("step_bwd-d256", "step_bwd", update(FL, 1, 1, 0), d=256),
    # ---- d not a multiple of the forward's vector (fp32 6, bf16 12: the backward's 4 elements divide 12)
    C("fwd-d6", "fwd", fwd_scalar(FL), d=6),
    C("fwd-d12-bf16", "fwd", fwd_scalar(BF), BF16, d=12),
    C("fwd-d16-bf16", "fwd", fwd(BF, 1, 0), BF16),
    C("lookup_fwd-d6", "lookup_fwd", UNSUPPORTED, d=6),
    C("lookup_fwd-d12-bf16", "lookup_fwd", UNSUPPORTED, BF16, d=12),
    C("bwd-d6", "bwd", bwd_scalar(FL, 0), d=6),
    C("bwd-d12-bf16", "bwd", bwd(BF, 1, 0), BF16, d=12),
    C("bwd-d10-bf16", "bwd", bwd_scalar(BF, 0), BF16, d=10),
    C("bwd_gather-d6", "bwd_gather", bwd_scalar(FL, 1), d=6),
    C("bwd_gather-d12-bf16", "bwd_gather", bwd(BF, 1, 1), BF16, d=12),
    C("bwd_gather_ix-d6", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), d=6),
    C("bwd_gather_ix-d12-bf16", "bwd_gather_ix", (bwd_index(BF, 1), "ix"), BF16, d=12),
    C("bwd_blocked-d6", "bwd_blocked", UNSUPPORTED, d=6),
    C("bwd_blocked-d12-bf16", "bwd_blocked", bwd(BF, 1, 1), BF16, d=12),
    C("step_fwd-d6", "step_fwd", UNSUPPORTED, d=6),
    C("step_fwd-d12-bf16", "step_fwd", UNSUPPORTED, BF16, d=12),
    C("step_bwd-d6", "step_bwd", UNSUPPORTED, d=6),
    C("step_bwd-d12-bf16", "step_bwd", UNSUPPORTED, BF16, d=12),
    # ---- the row-wise rule: d a power of two of at least 8 (17..32 features: its only forms)
    C("step_bwd-rowwise-d4", "step_bwd", UNSUPPORTED, d=4, F=17, rule="rowwise"),
    C("step_bwd-rowwise-d8", "step_bwd", split(FL, 2, 0, 8, 1, rule="rowwise"), d=8, F=17, rule="rowwise"),
    C("step_bwd-rowwise-d16", "step_bwd", split(FL, 2, 0, 8, 1, rule="rowwise"), d=16, F=17, rule="rowwise"),
    C("step_bwd-rowwise-d24", "step_bwd", UNSUPPORTED, d=24, F=17, rule="rowwise"),
    C("step_bwd-rowwise-d48", "step_bwd", UNSUPPORTED, d=48, F=17, rule="rowwise"),
    C("step_bwd-adagrad-d24", "step_bwd", split(FL, 2, 0, 8, 1, rule="adagrad"), d=24, F=17, rule="adagrad"),
    # ---- B = 2048 | 2049: launch_step_fwd's indexer, and 8 columns per lane for bf16 rows of d = 128
    C("step_fwd-B2048", "step_fwd", (fwd_index(FL, 1), "tp,ix"), B=2048),
    C("step_fwd-B2049", "step_fwd", UNSUPPORTED, B=2049),
    C("step_bwd-bf16-d128-B2048", "step_bwd", split(BF, 1, 128, 4, 2), BF16, d=128, B=2048),
    C("step_bwd-bf16-d128-B2049", "step_bwd", split(BF, 1, 128, 2, 1, CPL=8), BF16, d=128, B=2049),
    C("step_bwd-bf16-d128-F17-B2048", "step_bwd", split(BF, 2, 128, 4, 2), BF16, d=128, F=17, B=2048),
    C("step_bwd-bf16-d128-F17-B2049", "step_bwd", split(BF, 2, 128, 2, 1, CPL=8), BF16, d=128, F=17, B=2049),
    C("step_bwd-f32-d128-B2049", "step_bwd", split(FL, 1, 128, 4, 2), d=128, B=2049),
    C("step_bwd-bf16-d64-B2049", "step_bwd", split(BF, 1, 0, 8, 1), BF16, d=64, B=2049),
    # (the other rules: 8 columns per lane with 17..32 features only)
    C("step_bwd-split-B2049", "step_bwd", split(BF, 1, 128, 4, 2, rule="split"), BF16, d=128, B=2049, rule="split"),
    C("step_bwd-split-F17-B2049", "step_bwd", split(BF, 2, 128, 2, 1, CPL=8, rule="split"), BF16, d=128, F=17, B=2049,
      rule="split"),
    C("step_bwd-adagrad-B2049", "step_bwd", split(BF, 1, 128, 4, 2, rule="adagrad"), BF16, d=128, B=2049, rule="adagrad"),
    C("step_bwd-adagrad-F17-B2049", "step_bwd", split(BF, 2, 128, 2, 1, CPL=8, rule="adagrad"), BF16, d=128, F=17,
      B=2049, rule="adagrad"),
    C("step_bwd-adagrad-F17-B2048", "step_bwd", split(BF, 2, 128, 4, 2, rule="adagrad"), BF16, d=128, F=17, B=2048,
      rule="adagrad"),
    C("step_bwd-adagrad-f32-F17-B2049", "step_bwd", split(FL, 2, 128, 4, 2, rule="adagrad"), d=128, F=17, B=2049,
      rule="adagrad"),
    C("step_bwd-rowwise-F17-B2049", "step_bwd", split(BF, 2, 128, 2, 1, CPL=8, rule="rowwise"), BF16, d=128, F=17,
      B=2049, rule="rowwise"),
    C("step_bwd-stochastic-B2049", "step_bwd", split(BF, 1, 128, 4, 2, rule="stochastic"), BF16, d=128, B=2049,
      rule="stochastic"),
    C("step_bwd-stochastic-F17-B2049", "step_bwd", split(BF, 2, 128, 2, 1, CPL=8, rule="stochastic"), BF16, d=128, F=17,
      B=2049, rule="stochastic"),
    # ---- B L = 2048 | 2049: the backward that carries the indexer
    C("bwd_gather_ix-BL2048", "bwd_gather_ix", (bwd_index(FL, 1), "ix"), B=2048),
    C("bwd_gather_ix-BL2049", "bwd_gather_ix", (bwd(FL, 1, 1), "first"), B=2049),
    C("bwd_gather_ix-B1024-L2", "bwd_gather_ix", (bwd_index(FL, 1), "ix"), B=1024, L=2),
    C("bwd_gather_ix-B1025-L2", "bwd_gather_ix", (bwd(FL, 1, 1), "first"), B=1025, L=2),
    # ---- L = 1 | 9 | 10 with and without ys: T L > 64 with ys kept has no fused forward (7 tables: 63 | 70)
    C("lookup_fwd-L1-ys", "lookup_fwd", (fwd(FL, 1, 1), "tp"), F=8, L=1, ys=1),
    C("lookup_fwd-L9-ys", "lookup_fwd", fwd(FL, 1, 1, pooled=1), F=8, L=9, ys=1),
    C("lookup_fwd-L10-ys", "lookup_fwd", UNSUPPORTED, F=8, L=10, ys=1),
    C("lookup_fwd-L1", "lookup_fwd", (fwd(FL, 1, 1), "tp"), F=8, L=1),
    C("lookup_fwd-L9", "lookup_fwd", fwd(FL, 1, 1, pooled=1), F=8, L=9),
    C("lookup_fwd-L10", "lookup_fwd", fwd(FL, 1, 1, pooled=1), F=8, L=10),
    # ---- T = 32 | 33: 32 table pointers go by value -- which only forms of up to 32 features take
    C("lookup_fwd-T31", "lookup_fwd", (fwd(FL, 2, 1), "tp"), F=32),
    C("lookup_fwd-T32", "lookup_fwd", fwd(FL, 3, 1), F=33, max_rows=1 << 32),
    C("lookup_fwd-T33", "lookup_fwd", fwd(FL, 3, 1), F=34, max_rows=-1),
    # ---- a table of 2^32 rows (TabPtrs holds rows in 32 bits, all ones left out), no host descriptors
    C("lookup_fwd-rows-2^32-2", "lookup_fwd", (fwd(FL, 1, 1), "tp"), max_rows=(1 << 32) - 2),
    C("lookup_fwd-rows-2^32-1", "lookup_fwd", UNSUPPORTED, max_rows=(1 << 32) - 1),
    C("lookup_fwd-rows-2^32", "lookup_fwd", UNSUPPORTED, max_rows=1 << 32),
    C("lookup_fwd-rows-2^32-L2", "lookup_fwd", fwd(FL, 1, 1, pooled=1), L=2, max_rows=1 << 32),
    C("lookup_fwd-no-host-tabs", "lookup_fwd", UNSUPPORTED, max_rows=-1),
    C("step_fwd-rows-2^32-2", "step_fwd", (fwd_index(FL, 1), "tp,ix"), max_rows=(1 << 32) - 2),
    C("step_fwd-rows-2^32", "step_fwd", UNSUPPORTED, max_rows=1 << 32),
    C("step_fwd-no-host-tabs", "step_fwd", UNSUPPORTED, max_rows=-1),
    C("step_bwd-rows-2^32", "step_bwd", split(FL, 1, 0, 8, 1), max_rows=1 << 32),
    C("bwd_gather-rows-2^32", "bwd_gather", bwd(FL, 1, 1), max_rows=1 << 32),
    # ---- each alignment fact false, one at a time.  The forward asks x, ys for 16 B and the leading dimensions for
    # a whole vector (4 fp32, 8 bf16); the backward asks x, ys for 4 elements (16 B fp32, 8 B bf16), dx, dt for 16 B
    # and every leading dimension for 4 elements
    C("fwd-x+8", "fwd", fwd_scalar(FL), ptr=X8),
    C("fwd-x_ld18", "fwd", fwd_scalar(FL), ptr={"x": (A0, 18)}),
    C("fwd-ys+8", "fwd", fwd_scalar(FL), ptr={"t": (A0 + 8, 48)}),
    C("fwd-ys_ld50", "fwd", fwd_scalar(FL), ptr={"t": (A0, 50)}),
    C("fwd-bf16-x+8", "fwd", fwd_scalar(BF), BF16, ptr=X8),
    C("fwd-bf16-x_ld20", "fwd", fwd_scalar(BF), BF16, ptr={"x": (A0, 20)}),
    C("fwd-bf16-ys_ld52", "fwd", fwd_scalar(BF), BF16, ptr={"t": (A0, 52)}),
    C("fwd-bf16-x_ld24", "fwd", fwd(BF, 1, 0), BF16, ptr={"x": (A0, 24)}),
    C("lookup_fwd-x+8", "lookup_fwd", UNSUPPORTED, ptr=X8),
    C("lookup_fwd-x_ld18", "lookup_fwd", UNSUPPORTED, ptr={"x": (A0, 18)}),
    C("lookup_fwd-ys+8", "lookup_fwd", UNSUPPORTED, ys=1, ptr={"t": (A0 + 8, 48)}),
    C("lookup_fwd-ys_ld50", "lookup_fwd", UNSUPPORTED, ys=1, ptr={"t": (A0, 50)}),
    C("lookup_fwd-tabs-unaligned", "lookup_fwd", UNSUPPORTED, tabs16=0),
    C("bwd-t+8", "bwd", bwd_scalar(FL, 0), ptr={"t": (A0 + 8, 48)}),
    C("bwd-t_ld50", "bwd", bwd_scalar(FL, 0), ptr={"t": (A0, 50)}),
    C("bwd-dx+8", "bwd", bwd_scalar(FL, 0), ptr={"dx": (A0 + 8, 16)}),
    C("bwd-dx_ld18", "bwd", bwd_scalar(FL, 0), ptr={"dx": (A0, 18)}),
    C("bwd-dt+8", "bwd", bwd_scalar(FL, 0), ptr={"dt": (A0 + 8, 48)}),
    C("bwd-dt_ld50", "bwd", bwd_scalar(FL, 0), ptr={"dt": (A0, 50)}),
    C("bwd-bf16-t+8", "bwd", bwd(BF, 1, 0), BF16, ptr={"t": (A0 + 8, 48)}),
    C("bwd-bf16-t+4", "bwd", bwd_scalar(BF, 0), BF16, ptr={"t": (A0 + 4, 48)}),
    C("bwd-bf16-t_ld52", "bwd", bwd(BF, 1, 0), BF16, ptr={"t": (A0, 52)}),
    C("bwd-bf16-dx+8", "bwd", bwd_scalar(BF, 0), BF16, ptr={"dx": (A0 + 8, 16)}),
    C("bwd-F40-d64-t+8", "bwd", bwd_scalar(FL, 0), d=64, F=40, ptr={"t": (A0 + 8, 40 * 64)}),
    C("bwd_gather-x+8", "bwd_gather", bwd_scalar(FL, 1), ptr=X8),
    C("bwd_gather-x_ld18", "bwd_gather", bwd_scalar(FL, 1), ptr={"x": (A0, 18)}),
    C("bwd_gather-dx+8", "bwd_gather", bwd_scalar(FL, 1), ptr={"dx": (A0 + 8, 16)}),
    C("bwd_gather-dx_ld18", "bwd_gather", bwd_scalar(FL, 1), ptr={"dx": (A0, 18)}),
    C("bwd_gather-dt+8", "bwd_gather", bwd_scalar(FL, 1), ptr={"dt": (A0 + 8, 48)}),
    C("bwd_gather-dt_ld50", "bwd_gather", bwd_scalar(FL, 1), ptr={"dt": (A0, 50)}),
    C("bwd_gather-tabs-unaligned", "bwd_gather", bwd_scalar(FL, 1), tabs16=0),
    C("bwd_gather-bf16-x+8", "bwd_gather", bwd(BF, 1, 1), BF16, ptr=X8),
    C("bwd_gather-bf16-x+4", "bwd_gather", bwd_scalar(BF, 1), BF16, ptr=X4),
    C("bwd_gather-bf16-x_ld20", "bwd_gather", bwd(BF, 1, 1), BF16, ptr={"x": (A0, 20)}),
    C("bwd_gather_ix-x+8", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), ptr=X8),
    C("bwd_gather_ix-x_ld18", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), ptr={"x": (A0, 18)}),
    C("bwd_gather_ix-dx+8", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), ptr={"dx": (A0 + 8, 16)}),
    C("bwd_gather_ix-dx_ld18", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), ptr={"dx": (A0, 18)}),
    C("bwd_gather_ix-dt+8", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), ptr={"dt": (A0 + 8, 48)}),
    C("bwd_gather_ix-dt_ld50", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), ptr={"dt": (A0, 50)}),
    C("bwd_gather_ix-tabs-unaligned", "bwd_gather_ix", (bwd_scalar(FL, 1), "first"), tabs16=0),
    C("bwd_gather_ix-bf16-x+8", "bwd_gather_ix", (bwd_index(BF, 1), "ix"), BF16, ptr=X8),
    C("bwd_blocked-x+8", "bwd_blocked", UNSUPPORTED, ptr=X8),
    C("bwd_blocked-x_ld18", "bwd_blocked", UNSUPPORTED, ptr={"x": (A0, 18)}),
    C("bwd_blocked-dx+8", "bwd_blocked", UNSUPPORTED, ptr={"dx": (A0 + 8, 16)}),
    C("bwd_blocked-dx_ld18", "bwd_blocked", UNSUPPORTED, ptr={"dx": (A0, 18)}),
    C("bwd_blocked-dst+8", "bwd_blocked", UNSUPPORTED, ptr={"dt": (A0 + 8, 0)}),
    C("bwd_blocked-tabs-unaligned", "bwd_blocked", UNSUPPORTED, tabs16=0),
    # (bf16: x that suits the backward's 8-B loads and not the split kernel's 16-B ones takes the one-wave kernel)
    C("bwd_blocked-bf16", "bwd_blocked", split(BF, 1, 0, 2, 1, mapped=1), BF16),
    C("bwd_blocked-bf16-x+8", "bwd_blocked", bwd(BF, 1, 1), BF16, ptr=X8),
    C("bwd_blocked-bf16-x+4", "bwd_blocked", UNSUPPORTED, BF16, ptr=X4),
    C("bwd_blocked-bf16-x_ld20", "bwd_blocked", bwd(BF, 1, 1), BF16, ptr={"x": (A0, 20)}),
    C("step_fwd-x+8", "step_fwd", UNSUPPORTED, ptr=X8),
    C("step_fwd-x_ld18", "step_fwd", UNSUPPORTED, ptr={"x": (A0, 18)}),
    C("step_fwd-bf16-x_ld20", "step_fwd", UNSUPPORTED, BF16, ptr={"x": (A0, 20)}),
    C("step_fwd-tabs-unaligned", "step_fwd", UNSUPPORTED, tabs16=0),
    C("step_bwd-x+8", "step_bwd", UNSUPPORTED, ptr=X8),
    C("step_bwd-x_ld18", "step_bwd", UNSUPPORTED, ptr={"x": (A0, 18)}),
    C("step_bwd-bf16-x_ld20", "step_bwd", UNSUPPORTED, BF16, ptr={"x": (A0, 20)}),
    C("step_bwd-tabs-unaligned", "step_bwd", UNSUPPORTED, tabs16=0),
    # ---- nothing to do: an empty batch, no tables
    C("fwd-B0", "fwd", NOTHING, B=0),
    C("lookup_fwd-B0", "lookup_fwd", NOTHING, B=0),
    C("lookup_fwd-B0-unaligned", "lookup_fwd", NOTHING, B=0, ptr=X8),
    C("bwd-B0", "bwd", NOTHING, B=0),
    C("bwd_gather-B0", "bwd_gather", NOTHING, B=0),
    C("bwd_gather_ix-B0", "bwd_gather_ix", NOTHING, B=0),
    C("bwd_blocked-B0", "bwd_blocked", NOTHING, B=0),
    C("bwd_blocked-B0-unaligned", "bwd_blocked", NOTHING, B=0, ptr=X8),
    C("step_fwd-B0", "step_fwd", UNSUPPORTED, B=0),
    C("step_bwd-B0", "step_bwd", NOTHING, B=0),
    C("step_bwd-B0-unaligned", "step_bwd", NOTHING, B=0, ptr=X8),
    C("lookup_fwd-T0", "lookup_fwd", UNSUPPORTED, F=1),
    C("bwd_gather-T0", "bwd_gather", bwd(FL, 1, 1), F=1),
    C("bwd_gather_ix-T0", "bwd_gather_ix", bwd(FL, 1, 1), F=1),
    C("bwd_blocked-T0", "bwd_blocked", NOTHING, F=1),
    C("step_fwd-T0", "step_fwd", UNSUPPORTED, F=1),
    C("step_bwd-T0", "step_bwd", NOTHING, F=1),
]

# ---- every rule x {fp32, bf16} x NB {1, 2} x d {16, 64, 128, 256}, B = 8: per (rule, element type, NB) the kernels at
# d = 16 and 64 (one wave per sample, 8 samples per block), 128 (two waves per sample, 4 samples per block) and 256
# (the one-wave update kernel: Descent and the split rule alone), "-": none.  The split rule's rows are bf16
# whatever the tables' dtype says (launch_step_bwd takes no dtype for it); the stochastic rule has no fp32 form.
_ONE, _TWO, _UPD = "one", "two", "upd"
RULE_FORMS = {
    ("descent", F32, 1): (_ONE, _ONE, _TWO, _UPD), ("descent", F32, 2): (_ONE, _ONE, _TWO, _UPD),
    ("descent", BF16, 1): (_ONE, _ONE, _TWO, _UPD), ("descent", BF16, 2): (_ONE, _ONE, _TWO, _UPD),
    ("split", F32, 1): (_ONE, _ONE, _TWO, _UPD), ("split", F32, 2): (_ONE, _ONE, _TWO, _UPD),
    ("split", BF16, 1): (_ONE, _ONE, _TWO, _UPD), ("split", BF16, 2): (_ONE, _ONE, _TWO, _UPD),
    ("adagrad", F32, 1): ("-", "-", _TWO, "-"), ("adagrad", F32, 2): (_ONE, _ONE, _TWO, "-"),
    ("adagrad", BF16, 1): (_ONE, _ONE, _TWO, "-"), ("adagrad", BF16, 2): (_ONE, _ONE, _TWO, "-"),
    ("rowwise", F32, 1): ("-", "-", "-", "-"), ("rowwise", F32, 2): (_ONE, _ONE, _TWO, "-"),
    ("rowwise", BF16, 1): ("-", "-", "-", "-"), ("rowwise", BF16, 2): (_ONE, _ONE, _TWO, "-"),
    ("stochastic", F32, 1): ("-", "-", "-", "-"), ("stochastic", F32, 2): ("-", "-", "-", "-"),
    ("stochastic", BF16, 1): (_ONE, _ONE, _TWO, "-"), ("stochastic", BF16, 2): (_ONE, _ONE, _TWO, "-"),
}
for (_rule, _dt, _nb), _forms in RULE_FORMS.items():
    _T = FL if _dt == F32 and _rule != "split" else BF
    for _d, _f in zip((16, 64, 128, 256), _forms):
        _k = {"-": UNSUPPORTED, _ONE: split(_T, _nb, 0, 8, 1, rule=_rule), _TWO: split(_T, _nb, 128, 4, 2, rule=_rule),
              _UPD: update(_T, _nb, 1, 0, _rule)}[_f]
        CASES.append(C(f"rule-{_rule}-{'f32' if _dt == F32 else 'bf16'}-NB{_nb}-d{_d}", "step_bwd", _k, _dt, d=_d,
                       F=16 * _nb, rule=_rule))

CASES += [
    # ---- DLRM_BWD_YS=0
    C("bwd-ys_body-F40-d64", "bwd", bwd(FL, 3, 0), d=64, F=40, knobs={"bwd_ys_body": 1}),
    C("bwd-ys_body-F16", "bwd", bwd(FL, 1, 0), F=16, knobs={"bwd_ys_body": 1}),
    # ---- DLRM_BWD_SPLIT=0: the one-wave update kernel, which an Adagrad or the stochastic rule does not have
    C("step_bwd-nosplit-d128", "step_bwd", update(FL, 1, 1, 128), d=128, knobs={"bwd_nosplit": 1}),
    C("step_bwd-nosplit-d128-F17", "step_bwd", update(FL, 2, 1, 128), d=128, F=17, knobs={"bwd_nosplit": 1}),
    C("step_bwd-nosplit-d64", "step_bwd", update(FL, 1, 1, 0), d=64, knobs={"bwd_nosplit": 1}),
    C("step_bwd-nosplit-bf16-d128", "step_bwd", update(BF, 1, 1, 128), BF16, d=128, knobs={"bwd_nosplit": 1}),
    C("step_bwd-nosplit-split-d128", "step_bwd", update(BF, 1, 1, 0, "split"), BF16, d=128, rule="split",
      knobs={"bwd_nosplit": 1}),
    C("step_bwd-nosplit-adagrad-d128", "step_bwd", UNSUPPORTED, d=128, rule="adagrad", knobs={"bwd_nosplit": 1}),
    C("step_bwd-nosplit-rowwise-d128", "step_bwd", UNSUPPORTED, d=128, F=17, rule="rowwise", knobs={"bwd_nosplit": 1}),
    C("step_bwd-nosplit-stochastic-d128", "step_bwd", UNSUPPORTED, BF16, d=128, rule="stochastic",
      knobs={"bwd_nosplit": 1}),
    # ---- DLRM_UPD_SBU: Descent's update kernel at d = 128
    C("step_bwd-sbu1", "step_bwd", update(FL, 1, 1, 128), d=128, knobs={"bwd_nosplit": 1, "upd_sbu": 1}),
    C("step_bwd-sbu2", "step_bwd", update(FL, 1, 2, 128), d=128, knobs={"bwd_nosplit": 1, "upd_sbu": 2}),
    C("step_bwd-sbu2-F17", "step_bwd", update(FL, 2, 2, 128), d=128, F=17, knobs={"bwd_nosplit": 1, "upd_sbu": 2}),
    C("step_bwd-sbu3", "step_bwd", update(FL, 1, 1, 128), d=128, knobs={"bwd_nosplit": 1, "upd_sbu": 3}),
    C("step_bwd-sbu2-d256", "step_bwd", update(FL, 1, 1, 0), d=256, knobs={"upd_sbu": 2}),
    C("step_bwd-sbu2-split", "step_bwd", update(BF, 1, 1, 0, "split"), BF16, d=128, rule="split",
      knobs={"bwd_nosplit": 1, "upd_sbu": 2}),
    C("step_bwd-sbu2-unused", "step_bwd", split(FL, 1, 128, 4, 2), d=128, knobs={"upd_sbu": 2}),
    # ---- DLRM_BWD_SPB: Descent's samples per block at d = 128, rounded down to 2, 4 or 8
    C("step_bwd-spb1", "step_bwd", split(FL, 1, 128, 2, 2), d=128, knobs={"bwd_spb": 1}),
    C("step_bwd-spb2", "step_bwd", split(FL, 1, 128, 2, 2), d=128, knobs={"bwd_spb": 2}),
    C("step_bwd-spb3", "step_bwd", split(FL, 1, 128, 2, 2), d=128, knobs={"bwd_spb": 3}),
    C("step_bwd-spb4", "step_bwd", split(FL, 1, 128, 4, 2), d=128, knobs={"bwd_spb": 4}),
    C("step_bwd-spb5", "step_bwd", split(FL, 1, 128, 4, 2), d=128, knobs={"bwd_spb": 5}),
    C("step_bwd-spb8", "step_bwd", split(FL, 1, 128, 8, 2), d=128, knobs={"bwd_spb": 8}),
    C("step_bwd-spb9", "step_bwd", split(FL, 1, 128, 8, 2), d=128, knobs={"bwd_spb": 9}),
    C("step_bwd-spb8-F17", "step_bwd", split(FL, 2, 128, 8, 2), d=128, F=17, knobs={"bwd_spb": 8}),
    C("step_bwd-spb2-d64", "step_bwd", split(FL, 1, 0, 8, 1), d=64, knobs={"bwd_spb": 2}),
    C("step_bwd-spb2-adagrad", "step_bwd", split(FL, 1, 128, 4, 2, rule="adagrad"), d=128, rule="adagrad",
      knobs={"bwd_spb": 2}),
    C("step_bwd-spb4-cpl8", "step_bwd", split(BF, 1, 128, 4, 1, CPL=8), BF16, d=128, B=2049, knobs={"bwd_spb": 4}),
    C("step_bwd-spb8-cpl8", "step_bwd", split(BF, 1, 128, 8, 1, CPL=8), BF16, d=128, B=2049, knobs={"bwd_spb": 8}),
    # ---- DLRM_BWD_CPL: Descent's bf16 form at d = 128 whatever the batch; ignored under any other rule
    C("step_bwd-cpl4-B2049", "step_bwd", split(BF, 1, 128, 4, 2), BF16, d=128, B=2049, knobs={"bwd_cpl": 4}),
    C("step_bwd-cpl8-B8", "step_bwd", split(BF, 1, 128, 2, 1, CPL=8), BF16, d=128, knobs={"bwd_cpl": 8}),
    C("step_bwd-cpl8-f32", "step_bwd", split(FL, 1, 128, 4, 2), d=128, knobs={"bwd_cpl": 8}),
    C("step_bwd-cpl8-d64", "step_bwd", split(BF, 1, 0, 8, 1), BF16, d=64, knobs={"bwd_cpl": 8}),
    C("step_bwd-cpl8-adagrad-B8", "step_bwd", split(BF, 2, 128, 4, 2, rule="adagrad"), BF16, d=128, F=17, rule="adagrad",
      knobs={"bwd_cpl": 8}),
    C("step_bwd-cpl4-adagrad-B2049", "step_bwd", split(BF, 2, 128, 2, 1, CPL=8, rule="adagrad"), BF16, d=128, F=17,
      B=2049, rule="adagrad", knobs={"bwd_cpl": 4}),
    C("step_bwd-cpl4-split-B2049", "step_bwd", split(BF, 2, 128, 2, 1, CPL=8, rule="split"), BF16, d=128, F=17, B=2049,
      rule="split", knobs={"bwd_cpl": 4}),
]
CASES += [
    # ---- the block counts between the thresholds (NB 4 and 5), for the traced rows
    C("fwd-F64", "fwd", fwd(FL, 4, 0), F=64),
    C("lookup_fwd-F80", "lookup_fwd", fwd(FL, 5, 1), F=80),
    C("bwd-F80", "bwd", bwd(FL, 5, 0), F=80),
    C("bwd-d64-F64", "bwd", split(FL, 4, 0, 1, 1, ys=1), d=64, F=64),
    C("bwd-d64-F80", "bwd", split(FL, 5, 0, 1, 1, ys=1), d=64, F=80),
    C("bwd_gather-F64", "bwd_gather", bwd(FL, 4, 1), F=64),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ---- the rows tools/launch_trace.py runs through the real entry points, one call each (a step backward: after its
# step forward): every kernel family at every site that reaches it, each NB a family has, both sides of B = 2048 | 2049
# for the step forward and for 8 columns per lane, one row per rule.  Batches of 8 but for those four rows.
GPU_ROWS = 3000  # rows per table
GPU_CASES = (["fwd-F16", "fwd-F17", "fwd-F64", "fwd-F96", "fwd-F97", "fwd-d128"] +
             ["lookup_fwd-F16", "lookup_fwd-F32", "lookup_fwd-F33", "lookup_fwd-F80", "lookup_fwd-d128", "lookup_fwd-L9-ys"] +
             ["bwd-F16", "bwd-F33", "bwd-F80", "bwd-F112", "bwd-F113", "bwd-d64-F33", "bwd-d64-F64", "bwd-d64-F80",
              "bwd-d64-F96", "bwd-F40-d128", "bwd-F40-d256"] +
             ["bwd_gather-F32", "bwd_gather-F64", "bwd_gather-F96", "bwd_gather-F113"] +
             ["bwd_gather_ix-F16", "bwd_gather_ix-F17", "bwd_gather_ix-F33"] +
             ["bwd_blocked-F16", "bwd_blocked-F17", "bwd_blocked-d128", "bwd_blocked-F33"] +
             ["step_fwd-F16", "step_fwd-F17", "step_fwd-d128", "step_fwd-B2048", "step_fwd-B2049"] +
             ["step_bwd-F16", "step_bwd-F17", "step_bwd-d128", "step_bwd-d68", "rule-descent-f32-NB2-d256",
              "step_bwd-bf16-d128-B2048", "step_bwd-bf16-d128-B2049", "rule-split-bf16-NB1-d128",
              "rule-adagrad-f32-NB2-d64", "rule-rowwise-f32-NB2-d128", "rule-stochastic-bf16-NB1-d64"])


def drive(pkg, dev, case, seed=0):
    """Runs the case's entry point once on its shape (default pointers and knobs only).  Returns the library's return
    code."""
    import numpy as np
    import torch
    lib, ptr = pkg._lib, pkg.runtime.ptr
    assert not case.ptr and not case.knobs and case.tabs16 and case.max_rows == 5000, case.name
    d, F, B, L, T = case.d, case.F, case.B, case.L, case.F - 1
    dtype = torch.float32 if case.dtype == F32 else torch.bfloat16
    rng = np.random.default_rng(seed + F)
    ts = pkg.EmbeddingTableSet([torch.zeros((GPU_ROWS, d), dtype=dtype, device=dev) for _ in range(T)])
    idx = torch.from_numpy(rng.integers(0, GPU_ROWS, size=(T, B, L) if L > 1 else (T, B))).to(torch.int32).to(dev)
    p = pkg.PackedIndices(idx)
    width = d + F * (F - 1) // 2
    x = torch.zeros((B, d), dtype=dtype, device=dev)
    ys = torch.zeros((B, F * d), dtype=dtype, device=dev)
    out = torch.zeros((B, width), dtype=dtype, device=dev)
    dout = torch.zeros((B, width), dtype=dtype, device=dev)
    dx = torch.zeros((B, d), device=dev)
    dt = torch.zeros((B, F * d), device=dev)
    ctx = ts.ctx
    h, code = ctx.bind(), pkg.runtime.dtype_code(dtype)
    if case.site == "fwd":
        return ctx.lib.dlrm_interact_fwd(h, code, d, F, B, ptr(x), d, ptr(ys), F * d, ptr(out), width, 0)
    if case.site == "lookup_fwd":
        return ctx.lib.dlrm_lookup_interact_fwd(h, ts.handle, ptr(p.data), p.itype, p.stride, 0, B, L, ptr(x), d,
                                                ptr(ys) if case.ys else None, F * d if case.ys else 0, ptr(out), width, 0)
    if case.site == "bwd":
        return ctx.lib.dlrm_interact_bwd(h, code, d, F, B, ptr(dout), width, 0, ptr(ys), F * d, ptr(dx), d, ptr(dt), F * d)
    if case.site in ("bwd_gather", "bwd_gather_ix"):
        ix = pkg.SparseIndexer(T, B * L, dev) if case.site == "bwd_gather_ix" else None
        return ctx.lib.dlrm_interact_bwd_gather(h, ts.handle, ix.handle if ix else None, ptr(p.data), p.itype, p.stride, 0,
                                                B, L, ptr(x), d, ptr(dout), width, 0, ptr(dx), d, ptr(dt), F * d)
    if case.site == "bwd_blocked":  # table t's rows at dst + t * d + b * T * d
        dbase = torch.arange(T, dtype=torch.int64, device=dev) * d
        dld = torch.full((T,), T * d, dtype=torch.int64, device=dev)
        dst = torch.zeros((B, T * d), device=dev)
        return ctx.lib.dlrm_interact_bwd_blocked(h, ts.handle, ptr(p.data), p.itype, p.stride, 0, B, ptr(x), d, ptr(dout),
                                                 width, 0, ptr(dx), d, ptr(dst), ptr(dbase), ptr(dld))
    opt, kw = {"descent": (None, {}), "split": (pkg.SplitDescent(0.5), dict(fused_step=True)),
               "adagrad": (pkg.ADAGrad(0.5, 1e-8), dict(adagrad_step=True)),
               "rowwise": (pkg.RowwiseADAGrad(0.5, 1e-8), dict(adagrad_step=True)),
               "stochastic": (pkg.StochasticDescent(0.5, seed=1), dict(stochastic_step=True))}[case.rule]
    hp = pkg.HotPath(ts, B, 1, lr=0.5, index_base=0, opt=opt, **kw)
    assert hp.step_api
    try:
        hp.step_fwd(x, p)
        if case.site == "step_bwd":
            hp.step_bwd(dout, flags=lib.STEP_BWD_ONLY)
        return lib.OK
    except lib.DLRMError as e:
        return e.code
