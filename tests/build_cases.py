"""Which index build a batch takes: the table of DESIGN.md section 20 as literal rows.

Shared by tests/test_build_plan_host.py (every row, through csrc/build_plan.hpp's plan_build in a stand-alone host
program), tests/test_build_forms.py (the rows of GPU_CASES, through the real entry points on a small shape) and
tools/launch_trace.py (one row of GPU_CASES per process, for a kernel trace).

A row: C(name, site, cap, N, expected, T=2, L=1, set_parts=0, knobs={...}, caps={...}).
  site       the entry point that asks (SITES)
  cap, T     the indexer as dlrm_indexer_create(T, cap) carves it (TV and hsize follow: carved())
  N, L       positions per table (batch * lookups) and lookups per bag
  set_parts  dlrm_indexer_set_parts as log2 (0: not set)
  knobs      the environment knobs that differ from KNOB_DEFAULTS (csrc/build_plan.hpp Knobs)
  caps       the shape facts that differ from CAP_DEFAULTS (BuildCaps)
  expected   (form, kind, vshift, split, has_map, bounds word, side stream, return code); kind: the wave build's
             kernel -- one round / rounds / scan with its waves per workgroup where the host decides them
Every row was read against the parent's abi.cpp / update.hip by hand (a row is no copy of what plan_build says
today: changing plan_build must fail the row); tools/launch_trace.py's comparison
(profiles/build_plan/launch_diff.txt) holds the forms of GPU_CASES against the kernels the parent's library launched.
"""
from collections import namedtuple

SITES = ["build", "build_split", "prepare", "step_fwd", "in_apply", "bwd_gather"]
KNOBS = ["step_parts", "build_parts", "bag_hash", "bag_vs", "bag_split", "wave_rounds"]
KNOB_DEFAULTS = dict(step_parts=0, build_parts=0, bag_hash=0, bag_vs=0, bag_split=1, wave_rounds=0)
CAPS = ["prepared", "step_fwd", "step_split", "split_bwd", "bwd_only", "idx_vec32", "cus"]
CAP_DEFAULTS = dict(prepared=0, step_fwd=1, step_split=1, split_bwd=1, bwd_only=0, idx_vec32=1, cus=256)
# (bag_hash = 1 is DLRM_BAG_WAVE=0; bag_split is DLRM_BAG_SPLIT itself; the others are their variables' values)

Case = namedtuple("Case", "name site cap N expected T L set_parts knobs caps")


def C(name, site, cap, N, expected, T=2, L=1, set_parts=0, knobs=None, caps=None):
    return Case(name, site, cap, N, expected, T, L, set_parts, knobs or {}, caps or {})


def carved(cap, T):
    """(TV, hsize) of dlrm_indexer_create(T, cap): 8 virtual tables per table for a capacity of 4097..8192, hash
    arrays (a power of two of at least 2 cap slots) above 4096."""
    tv = T * (8 if 4096 < cap <= 8192 else 1)
    hs = 0
    if cap > 4096:
        hs = 1024
        while hs < 2 * cap:
            hs *= 2
    return tv, hs


def encode(c):
    """The case as build_plan_print's input line."""
    tv, hs = carved(c.cap, c.T)
    k = dict(KNOB_DEFAULTS, **c.knobs)
    p = dict(CAP_DEFAULTS, **c.caps)
    return " ".join(str(v) for v in [SITES.index(c.site), c.cap, c.T, tv, hs, c.set_parts, c.N] + [k[n] for n in KNOBS] +
                    [p[n] for n in CAPS])


M = 1 << 20
CASES = [
    # ---- both sides of every threshold, capacity = N
    C("build-2048", "build", 2048, 2048, ('lds2', '-', 0, 1, 0, 'ctx', 0, 0), L=4),
    C("build-2049", "build", 2049, 2049, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("build-4096", "build", 4096, 4096, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0), L=4),
    C("build-4097", "build", 4097, 4097, ('lds_parts', '-', 2, 1, 0, 'ctx', 0, 0)),
    C("build-8192", "build", 8192, 8192, ('lds_parts', '-', 2, 1, 0, 'ctx', 0, 0), L=4),
    C("build-8193", "build", 8193, 8193, ('bag', '-', 6, 1, 1, 'ctx', 0, 0)),
    C("build-16384", "build", 16384, 16384, ('bag', '-', 6, 1, 1, 'ctx', 0, 0), L=4),
    C("build-16385", "build", 16385, 16385, ('bag', '-', 7, 1, 1, 'ctx', 0, 0)),
    C("build-32768", "build", 32768, 32768, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), L=4),
    C("build-32769", "build", 32769, 32769, ('hash', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("build-1048576", "build", M, M, ('hash', '-', 0, 1, 0, 'ctx', 0, 0), L=4),
    C("build-1048577", "build", M + 1, M + 1, ('sorted', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("split-2048", "build_split", 2048, 2048, ('lds2', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("split-2049", "build_split", 2049, 2049, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("split-4096", "build_split", 4096, 4096, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("split-4097", "build_split", 4097, 4097, ('bag', '-', 5, 1, 1, 'ctx', 0, 0)),
    C("split-8192", "build_split", 8192, 8192, ('bag', '-', 5, 1, 1, 'ctx', 0, 0)),
    C("split-8193", "build_split", 8193, 8193, ('bag', '-', 6, 1, 1, 'ctx', 0, 0)),
    C("split-16384", "build_split", 16384, 16384, ('bag', '-', 6, 1, 1, 'ctx', 0, 0)),
    C("split-16385", "build_split", 16385, 16385, ('bag', '-', 7, 1, 1, 'ctx', 0, 0)),
    C("split-32768", "build_split", 32768, 32768, ('bag', '-', 7, 1, 1, 'ctx', 0, 0)),
    C("split-32769", "build_split", 32769, 32769, ('hash', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("split-1048576", "build_split", M, M, ('hash', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("split-1048577", "build_split", M + 1, M + 1, ('none', '-', 0, 1, 0, 'ctx', 0, -4)),
    C("prepare-2048", "prepare", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep0', 0, 0)),
    C("prepare-2049", "prepare", 2049, 2049, ('wave', 'rounds', 5, 1, 1, 'prep0', 0, 0)),
    C("prepare-4096", "prepare", 4096, 4096, ('wave', 'scan16', 5, 1, 1, 'prep0', 0, 0)),
    C("prepare-4097", "prepare", 4097, 4097, ('wave', 'rounds', 6, 1, 1, 'prep0', 0, 0)),
    C("prepare-8192", "prepare", 8192, 8192, ('wave', 'scan16', 6, 1, 1, 'prep0', 0, 0)),
    C("prepare-8193", "prepare", 8193, 8193, ('wave', 'rounds', 7, 1, 1, 'prep0', 0, 0)),
    C("prepare-16384", "prepare", 16384, 16384, ('wave', 'scan16', 7, 1, 1, 'prep0', 0, 0)),
    C("prepare-16385", "prepare", 16385, 16385, ('wave', 'rounds', 8, 1, 1, 'prep0', 0, 0)),
    C("prepare-32768", "prepare", 32768, 32768, ('wave', 'scan16', 8, 1, 1, 'prep0', 0, 0)),
    C("prepare-32769", "prepare", 32769, 32769, ('none', '-', 0, 0, 0, 'ctx', 0, -4)),
    C("prepare-1048576", "prepare", M, M, ('none', '-', 0, 0, 0, 'ctx', 0, -4)),
    C("prepare-1048577", "prepare", M + 1, M + 1, ('none', '-', 0, 0, 0, 'ctx', 0, -4)),
    # (step_fwd: what step_fwd_supported answers for the size is part of the row)
    C("fwd-2048", "step_fwd", 2048, 2048, ('in_forward', 'one', 4, 1, 1, 'ctx', 0, 0)),
    C("fwd-2049", "step_fwd", 2049, 2049, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0), caps={'step_fwd': 0}),
    C("fwd-4096", "step_fwd", 4096, 4096, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0), caps={'step_fwd': 0}),
    C("fwd-4097", "step_fwd", 4097, 4097, ('lds_parts', '-', 2, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-8192", "step_fwd", 8192, 8192, ('lds_parts', '-', 2, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-8193", "step_fwd", 8193, 8193, ('hash', '-', 0, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-16384", "step_fwd", 16384, 16384, ('hash', '-', 0, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-16385", "step_fwd", 16385, 16385, ('hash', '-', 0, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-32768", "step_fwd", 32768, 32768, ('hash', '-', 0, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-32769", "step_fwd", 32769, 32769, ('hash', '-', 0, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-1048576", "step_fwd", M, M, ('hash', '-', 0, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-1048577", "step_fwd", M + 1, M + 1, ('sorted', '-', 0, 0, 0, 'ctx', 0, 0), caps={'step_fwd': 0}),
    C("apply-2048", "in_apply", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep1', 0, 0)),
    C("apply-2049", "in_apply", 2049, 2049, ('wave', 'rounds', 5, 1, 1, 'prep1', 0, 0)),
    C("apply-4096", "in_apply", 4096, 4096, ('wave', 'scan', 5, 1, 1, 'prep1', 0, 0)),
    C("apply-4097", "in_apply", 4097, 4097, ('wave', 'rounds', 6, 1, 1, 'prep1', 0, 0)),
    C("apply-8192", "in_apply", 8192, 8192, ('wave', 'scan', 6, 1, 1, 'prep1', 0, 0)),
    C("apply-8193", "in_apply", 8193, 8193, ('wave', 'rounds', 7, 1, 1, 'prep1', 0, 0)),
    C("apply-16384", "in_apply", 16384, 16384, ('wave', 'scan', 7, 1, 1, 'prep1', 0, 0)),
    C("apply-16385", "in_apply", 16385, 16385, ('none', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("apply-32768", "in_apply", 32768, 32768, ('none', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("apply-32769", "in_apply", 32769, 32769, ('none', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("apply-1048576", "in_apply", M, M, ('none', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("apply-1048577", "in_apply", M + 1, M + 1, ('none', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("gather-2048", "bwd_gather", 2048, 2048, ('in_backward', '-', 0, 0, 0, 'ctx', 0, 0)),
    # ---- the capacity's carving class against an N of another class
    C("build-cap8192-3000", "build", 8192, 3000, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("build-cap8192-6000", "build", 8192, 6000, ('lds_parts', '-', 2, 1, 0, 'ctx', 0, 0)),
    C("build-cap32768-6000", "build", 32768, 6000, ('hash', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("build-cap32768-3000", "build", 32768, 3000, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("build-cap20000-9000", "build", 20000, 9000, ('bag', '-', 6, 1, 1, 'ctx', 0, 0)),
    C("split-cap8192-3000", "build_split", 8192, 3000, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("split-cap8192-6000", "build_split", 8192, 6000, ('bag', '-', 5, 1, 1, 'ctx', 0, 0)),
    C("split-cap32768-6000", "build_split", 32768, 6000, ('bag', '-', 5, 1, 1, 'ctx', 0, 0)),
    C("split-cap32768-3000", "build_split", 32768, 3000, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("split-cap20000-9000", "build_split", 20000, 9000, ('bag', '-', 6, 1, 1, 'ctx', 0, 0)),
    C("fwd-cap8192-3000", "step_fwd", 8192, 3000, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0), caps={'step_fwd': 0}),
    C("fwd-cap8192-6000", "step_fwd", 8192, 6000, ('lds_parts', '-', 2, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    C("fwd-cap32768-6000", "step_fwd", 32768, 6000, ('hash', '-', 0, 1, 0, 'ctx', 1, 0), caps={'step_fwd': 0}),
    # (a capacity above 16384: the forward's launch builds in LDS per table, not by waves)
    C("fwd-cap20000-2048", "step_fwd", 20000, 2048, ('in_forward', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("fwd-cap16384-2048", "step_fwd", 16384, 2048, ('in_forward', 'one', 4, 1, 1, 'ctx', 0, 0)),
    C("prepare-cap32768-2052", "prepare", 32768, 2052, ('wave', 'scan16', 5, 1, 1, 'prep0', 0, 0)),
    C("prepare-2052", "prepare", 2052, 2052, ('wave', 'scan16', 5, 1, 1, 'prep0', 0, 0)),
    C("prepare-2052-i64", "prepare", 2052, 2052, ('wave', 'rounds', 5, 1, 1, 'prep0', 0, 0), caps={'idx_vec32': 0}),
    C("prepare-16388", "prepare", 16388, 16388, ('wave', 'scan16', 8, 1, 1, 'prep0', 0, 0)),
    C("apply-2052", "in_apply", 2052, 2052, ('wave', 'scan', 5, 1, 1, 'prep1', 0, 0)),
    # ---- tables x capacity at 2^31 - 1 (a prime: one table) and at 2^31
    C("build-tcap-2^31-1", "build", (1 << 31) - 1, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), T=1),
    C("build-tcap-2^31", "build", 1 << 30, 20000, ('hash', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("split-tcap-2^31-1", "build_split", (1 << 31) - 1, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), T=1),
    C("split-tcap-2^31", "build_split", 1 << 30, 20000, ('hash', '-', 0, 1, 0, 'ctx', 0, 0)),
    C("prepare-tcap-2^31-1", "prepare", (1 << 31) - 1, 20000, ('wave', 'scan16', 8, 1, 1, 'prep0', 0, 0), T=1),
    C("prepare-tcap-2^31", "prepare", 1 << 30, 20000, ('none', '-', 0, 0, 0, 'ctx', 0, -4)),
    C("apply-tcap-2^31-1", "in_apply", (1 << 31) - 1, 2048, ('wave', 'one', 4, 1, 1, 'prep1', 0, 0), T=1),
    C("apply-tcap-2^31", "in_apply", 1 << 30, 2048, ('none', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("fwd-tcap-2^31-1", "step_fwd", (1 << 31) - 1, 2048, ('in_forward', '-', 0, 1, 0, 'ctx', 0, 0), T=1),
    C("fwd-tcap-2^31", "step_fwd", 1 << 30, 2048, ('in_forward', '-', 0, 1, 0, 'ctx', 0, 0)),
    # ---- DLRM_STEP_PARTS: the wave builds of <= 2048 positions (never fewer than 4 parts)
    C("prepare-step_parts1", "prepare", 2048, 2048, ('wave', 'one', 2, 1, 1, 'prep0', 0, 0), knobs={'step_parts': 1}),
    C("fwd-step_parts1", "step_fwd", 2048, 2048, ('in_forward', 'one', 2, 1, 1, 'ctx', 0, 0), knobs={'step_parts': 1}),
    C("apply-step_parts1", "in_apply", 2048, 2048, ('wave', 'one', 2, 1, 1, 'prep1', 0, 0), knobs={'step_parts': 1}),
    C("prepare-step_parts2", "prepare", 2048, 2048, ('wave', 'one', 2, 1, 1, 'prep0', 0, 0), knobs={'step_parts': 2}),
    C("fwd-step_parts2", "step_fwd", 2048, 2048, ('in_forward', 'one', 2, 1, 1, 'ctx', 0, 0), knobs={'step_parts': 2}),
    C("apply-step_parts2", "in_apply", 2048, 2048, ('wave', 'one', 2, 1, 1, 'prep1', 0, 0), knobs={'step_parts': 2}),
    C("prepare-step_parts4", "prepare", 2048, 2048, ('wave', 'one', 2, 1, 1, 'prep0', 0, 0), knobs={'step_parts': 4}),
    C("fwd-step_parts4", "step_fwd", 2048, 2048, ('in_forward', 'one', 2, 1, 1, 'ctx', 0, 0), knobs={'step_parts': 4}),
    C("apply-step_parts4", "in_apply", 2048, 2048, ('wave', 'one', 2, 1, 1, 'prep1', 0, 0), knobs={'step_parts': 4}),
    C("prepare-step_parts8", "prepare", 2048, 2048, ('wave', 'one', 3, 1, 1, 'prep0', 0, 0), knobs={'step_parts': 8}),
    C("fwd-step_parts8", "step_fwd", 2048, 2048, ('in_forward', 'one', 3, 1, 1, 'ctx', 0, 0), knobs={'step_parts': 8}),
    C("apply-step_parts8", "in_apply", 2048, 2048, ('wave', 'one', 3, 1, 1, 'prep1', 0, 0), knobs={'step_parts': 8}),
    C("prepare-step_parts16", "prepare", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep0', 0, 0), knobs={'step_parts': 16}),
    C("fwd-step_parts16", "step_fwd", 2048, 2048, ('in_forward', 'one', 4, 1, 1, 'ctx', 0, 0), knobs={'step_parts': 16}),
    C("apply-step_parts16", "in_apply", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep1', 0, 0), knobs={'step_parts': 16}),
    C("prepare-step_parts32", "prepare", 2048, 2048, ('wave', 'one', 5, 1, 1, 'prep0', 0, 0), knobs={'step_parts': 32}),
    C("fwd-step_parts32", "step_fwd", 2048, 2048, ('in_forward', 'one', 5, 1, 1, 'ctx', 0, 0), knobs={'step_parts': 32}),
    C("apply-step_parts32", "in_apply", 2048, 2048, ('wave', 'one', 5, 1, 1, 'prep1', 0, 0), knobs={'step_parts': 32}),
    # (above 2048 positions the knob is not read)
    C("prepare-step_parts8-4100", "prepare", 4100, 4100, ('wave', 'scan16', 6, 1, 1, 'prep0', 0, 0), knobs={'step_parts': 8}),
    # ---- DLRM_BUILD_PARTS: the in-LDS parts build
    C("split-build_parts2", "build_split", 8192, 6000, ('lds_parts', '-', 1, 1, 0, 'ctx', 0, 0),
      knobs={'build_parts': 2, 'bag_split': 0}),
    C("fwd-build_parts2", "step_fwd", 8192, 6000, ('lds_parts', '-', 1, 1, 0, 'ctx', 1, 0), knobs={'build_parts': 2},
      caps={'step_fwd': 0}),
    C("split-build_parts4", "build_split", 8192, 6000, ('lds_parts', '-', 2, 1, 0, 'ctx', 0, 0),
      knobs={'build_parts': 4, 'bag_split': 0}),
    C("fwd-build_parts4", "step_fwd", 8192, 6000, ('lds_parts', '-', 2, 1, 0, 'ctx', 1, 0), knobs={'build_parts': 4},
      caps={'step_fwd': 0}),
    C("split-build_parts8", "build_split", 8192, 6000, ('lds_parts', '-', 3, 1, 0, 'ctx', 0, 0),
      knobs={'build_parts': 8, 'bag_split': 0}),
    C("fwd-build_parts8", "step_fwd", 8192, 6000, ('lds_parts', '-', 3, 1, 0, 'ctx', 1, 0), knobs={'build_parts': 8},
      caps={'step_fwd': 0}),
    # ---- DLRM_BAG_WAVE=0, DLRM_BAG_VS (dlrm_indexer_build's bag build alone reads it), DLRM_BAG_SPLIT=0
    C("build-bag_wave0-20000", "build", 20000, 20000, ('hash', '-', 0, 1, 0, 'ctx', 0, 0), knobs={'bag_hash': 1}),
    C("build-bag_wave0-8193", "build", 8193, 8193, ('hash', '-', 0, 1, 0, 'ctx', 0, 0), knobs={'bag_hash': 1}),
    C("build-bag_vs1", "build", 20000, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 1}),
    C("split-bag_vs1", "build_split", 20000, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 1}),
    C("build-bag_vs2", "build", 20000, 20000, ('bag', '-', 2, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 2}),
    C("split-bag_vs2", "build_split", 20000, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 2}),
    C("build-bag_vs8", "build", 20000, 20000, ('bag', '-', 8, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 8}),
    C("split-bag_vs8", "build_split", 20000, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 8}),
    C("build-bag_vs9", "build", 20000, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 9}),
    C("split-bag_vs9", "build_split", 20000, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 9}),
    # (the knob's upper end is the capacity's wave_vshift: 7 at 8193)
    C("build-bag_vs8-cap8193", "build", 8193, 8193, ('bag', '-', 6, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 8}),
    C("build-bag_vs7-cap8193", "build", 8193, 8193, ('bag', '-', 7, 1, 1, 'ctx', 0, 0), knobs={'bag_vs': 7}),
    C("split-bag_split0-cap8192-6000", "build_split", 8192, 6000, ('lds_parts', '-', 2, 1, 0, 'ctx', 0, 0),
      knobs={'bag_split': 0}),
    C("split-bag_split0-cap32768-6000", "build_split", 32768, 6000, ('hash', '-', 0, 1, 0, 'ctx', 0, 0),
      knobs={'bag_split': 0}),
    C("split-bag_split0-cap20000-20000", "build_split", 20000, 20000, ('hash', '-', 0, 1, 0, 'ctx', 0, 0),
      knobs={'bag_split': 0}),
    C("split-bag_split0-cap4097-4097", "build_split", 4097, 4097, ('lds_parts', '-', 2, 1, 0, 'ctx', 0, 0),
      knobs={'bag_split': 0}),
    # ---- DLRM_WAVE_ROUNDS
    C("prepare-rounds-16388", "prepare", 16388, 16388, ('wave', 'rounds', 8, 1, 1, 'prep0', 0, 0), knobs={'wave_rounds': 1}),
    C("prepare-rounds-2048", "prepare", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep0', 0, 0), knobs={'wave_rounds': 1}),
    C("apply-rounds-2052", "in_apply", 2052, 2052, ('wave', 'rounds', 5, 1, 1, 'prep1', 0, 0), knobs={'wave_rounds': 1}),
    # ---- dlrm_indexer_set_parts 0 / 16 / 32 / 64
    C("prepare-set_parts0", "prepare", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep0', 0, 0)),
    C("fwd-set_parts0", "step_fwd", 2048, 2048, ('in_forward', 'one', 4, 1, 1, 'ctx', 0, 0)),
    C("apply-set_parts0", "in_apply", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep1', 0, 0)),
    C("prepare-set_parts16", "prepare", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep0', 0, 0), set_parts=4),
    C("fwd-set_parts16", "step_fwd", 2048, 2048, ('in_forward', 'one', 4, 1, 1, 'ctx', 0, 0), set_parts=4),
    C("apply-set_parts16", "in_apply", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep1', 0, 0), set_parts=4),
    C("prepare-set_parts32", "prepare", 2048, 2048, ('wave', 'one', 5, 1, 1, 'prep0', 0, 0), set_parts=5),
    C("fwd-set_parts32", "step_fwd", 2048, 2048, ('in_forward', 'one', 5, 1, 1, 'ctx', 0, 0), set_parts=5),
    C("apply-set_parts32", "in_apply", 2048, 2048, ('wave', 'one', 5, 1, 1, 'prep1', 0, 0), set_parts=5),
    C("prepare-set_parts64", "prepare", 2048, 2048, ('wave', 'one', 6, 1, 1, 'prep0', 0, 0), set_parts=6),
    C("fwd-set_parts64", "step_fwd", 2048, 2048, ('in_forward', 'one', 6, 1, 1, 'ctx', 0, 0), set_parts=6),
    C("apply-set_parts64", "in_apply", 2048, 2048, ('wave', 'one', 6, 1, 1, 'prep1', 0, 0), set_parts=6),
    C("prepare-set_parts64-2049", "prepare", 2049, 2049, ('wave', 'rounds', 5, 1, 1, 'prep0', 0, 0), set_parts=6),
    # (DLRM_STEP_PARTS, where set, wins over set_parts)
    C("prepare-set_parts32-step_parts8", "prepare", 2048, 2048, ('wave', 'one', 3, 1, 1, 'prep0', 0, 0), set_parts=5,
      knobs={'step_parts': 8}),
    C("apply-set_parts32-step_parts8", "in_apply", 2048, 2048, ('wave', 'one', 3, 1, 1, 'prep1', 0, 0), set_parts=5,
      knobs={'step_parts': 8}),
    # ---- each caps bit off (the two flags: on)
    C("fwd-prepared", "step_fwd", 2048, 2048, ('kept', '-', 0, 0, 0, 'ctx', 0, 0), caps={'prepared': 1}),
    C("fwd-prepared-4097", "step_fwd", 4097, 4097, ('kept', '-', 0, 0, 0, 'ctx', 0, 0), caps={'prepared': 1, 'step_fwd': 0}),
    C("fwd-no_step_fwd-2048", "step_fwd", 2048, 2048, ('lds2', '-', 0, 1, 0, 'ctx', 0, 0), caps={'step_fwd': 0}),
    C("fwd-no_step_fwd-2049", "step_fwd", 2049, 2049, ('lds4', '-', 0, 1, 0, 'ctx', 0, 0), caps={'step_fwd': 0}),
    # (no split backward for the shape: the fused forward, then dlrm_indexer_build's row, on the ctx's stream)
    C("fwd-no_split-2048", "step_fwd", 2048, 2048, ('lds2', '-', 0, 1, 0, 'ctx', 0, 0), caps={'step_fwd': 0, 'step_split': 0}),
    C("fwd-no_split-4097", "step_fwd", 4097, 4097, ('lds_parts', '-', 2, 1, 0, 'ctx', 0, 0),
      caps={'step_fwd': 0, 'step_split': 0}),
    C("fwd-no_split-8193", "step_fwd", 8193, 8193, ('bag', '-', 6, 1, 1, 'ctx', 0, 0), caps={'step_fwd': 0, 'step_split': 0}),
    C("fwd-no_split-20000", "step_fwd", 20000, 20000, ('bag', '-', 7, 1, 1, 'ctx', 0, 0),
      caps={'step_fwd': 0, 'step_split': 0}),
    C("apply-no_split_bwd", "in_apply", 2048, 2048, ('none', '-', 0, 0, 0, 'ctx', 0, 0), caps={'split_bwd': 0}),
    C("apply-bwd_only", "in_apply", 2048, 2048, ('none', '-', 0, 0, 0, 'ctx', 0, 0), caps={'bwd_only': 1}),
    C("apply-33-features", "in_apply", 2048, 2048, ('none', '-', 0, 0, 0, 'ctx', 0, 0), T=32),
    C("apply-32-features", "in_apply", 2048, 2048, ('wave', 'one', 4, 1, 1, 'prep1', 0, 0), T=31),
    C("apply-empty", "in_apply", 2048, 0, ('none', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("apply-cap-short", "in_apply", 2048, 2049, ('none', '-', 0, 0, 0, 'ctx', 0, 0)),
    C("prepare-16388-unaligned", "prepare", 16388, 16388, ('wave', 'rounds', 8, 1, 1, 'prep0', 0, 0), caps={'idx_vec32': 0}),
    C("apply-2052-unaligned", "in_apply", 2052, 2052, ('wave', 'rounds', 5, 1, 1, 'prep1', 0, 0), caps={'idx_vec32': 0}),
    # (the scan build's workgroups, T * 2^vshift / 4, against the compute units: 272 and 256 against 256; above
    # 16384 positions always 16 waves)
    C("prepare-4100-over-cus", "prepare", 4100, 4100, ('wave', 'scan8', 6, 1, 1, 'prep0', 0, 0), T=17),
    C("prepare-4100-within-cus", "prepare", 4100, 4100, ('wave', 'scan16', 6, 1, 1, 'prep0', 0, 0), T=16),
    C("prepare-20000-over-cus", "prepare", 20000, 20000, ('wave', 'scan16', 8, 1, 1, 'prep0', 0, 0), T=40),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ---- the rows a small shape reaches through the real entry points: two fp32 tables of 3 and 5000 rows, dim 16,
# uniform indices, capacity = N unless the row says otherwise
GPU_ROWS, GPU_DIM = [3, 5000], 16
# (2^20 + 1: the sorted unsplit kernel, and dlrm_indexer_build_split's refusal -- the parent's library builds and
# passes the row in 0.6 s)
GPU_CASES = (["build-%d" % n for n in (2048, 2049, 4096, 4097, 8192, 8193, 32768, 32769, M + 1)] +
             ["split-%d" % n for n in (2048, 2049, 4096, 4097, 8192, 8193, 32768, 32769, M + 1)] +
             ["prepare-2048", "prepare-2049", "prepare-2052", "prepare-2052-i64", "prepare-16388"] +
             ["fwd-2048", "fwd-2049", "fwd-4097", "fwd-cap20000-2048"] + ["apply-2048", "apply-2052"])
# The kernels of this library a form launches, in order, as substrings of their names (a wave build inside an apply
# launch: that launch's MODE, the kernel's fourth template argument)
FORM_KERNELS = {
    ("none", "-"): [],
    ("lds2", "-"): ["indexer_fast_kernel<1024, 2, true>"],
    ("lds4", "-"): ["indexer_fast_kernel<1024, 4, true>"],
    ("lds_parts", "-"): ["indexer_fast_kernel<1024, 8, true>"],
    ("hash", "-"): ["hix_insert_kernel", "hix_alloc_kernel", "hix_place_kernel", "hix_order_kernel"],
    ("sorted", "-"): ["indexer_build_kernel<false>"],
    ("bag", "-"): ["bag_count_kernel", "bag_place_kernel", "bag_sort_kernel"],
    ("wave", "one"): ["step_index_kernel<0>"],
    ("wave", "rounds"): ["step_index_kernel<1>"],
    ("wave", "scan16"): ["step_index_scan_kernel<16, "],
    ("wave", "scan8"): ["step_index_scan_kernel<8, "],
    ("in_forward", "one"): ["interact_fwd_index_kernel"],
    ("in_forward", "-"): ["interact_fwd_index_kernel"],
}
APPLY_MODE = {"one": 2, "rounds": 3, "scan": 5}


def drive(pkg, dev, case, seed=0):
    """Runs the case's entry point once on the small shape.  Returns (rc, indexer, idx, p, ts): the library's return
    code, the indexer that holds the build, its indices as numpy [T][N], the PackedIndices they were passed in, and
    the (all-zero) tables."""
    import ctypes

    import numpy as np
    import torch
    lib, ptr = pkg._lib, pkg.runtime.ptr
    assert case.T == len(GPU_ROWS) and not case.knobs and not case.set_parts, case.name
    N, L = case.N, case.L
    B = N // L
    rng = np.random.default_rng(seed + N)
    ity = torch.int32 if case.caps.get("idx_vec32", 1) else torch.int64

    def indices():
        idx = np.stack([rng.integers(0, n, size=N) for n in GPU_ROWS])
        t = torch.from_numpy(idx).to(ity).to(dev)
        return idx, pkg.PackedIndices(t.reshape(len(GPU_ROWS), B, L) if L > 1 else t)

    ts = pkg.EmbeddingTableSet([torch.zeros((n, GPU_DIM), device=dev) for n in GPU_ROWS])
    idx, p = indices()
    h = ts.ctx.bind()
    if case.site in ("build", "build_split", "prepare"):
        ix = pkg.SparseIndexer(len(GPU_ROWS), case.cap, dev)
        args = (h, ix.handle, ts.handle, ptr(p.data), p.itype, p.stride, 0, B)
        if case.site == "build":
            rc = ts.ctx.lib.dlrm_indexer_build(*args, L)
        elif case.site == "build_split":
            rc = ts.ctx.lib.dlrm_indexer_build_split(*args)
        else:
            rc = ts.ctx.lib.dlrm_indexer_prepare(*args)
        return rc, ix, idx, p, ts
    hp = pkg.HotPath(ts, B, 1, lr=1.0, index_base=0, pipeline="apply" if case.site == "in_apply" else None)
    assert hp.step_api
    x = torch.zeros((B, GPU_DIM), device=dev)
    if case.cap != B:
        hp.indexer = pkg.SparseIndexer(len(GPU_ROWS), case.cap, dev)
    try:
        hp.step_fwd(x, p)
        if case.site == "step_fwd":
            return lib.OK, hp.indexer, idx, p, ts
        assert case.site == "in_apply"
        nidx, np_ = indices()
        nix = hp._ixs[1]
        hp.step_bwd(torch.zeros((B, hp.width), device=dev), x=x, idx=p, prepare=(nix, np_))
        return lib.OK, nix, nidx, np_, ts
    except lib.DLRMError as e:
        return e.code, hp.indexer, idx, p, ts
