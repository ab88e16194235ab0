"""csrc/interact_plan.hpp alone, on the host: interact_align and plan_interact against the literal rows of
tests/interact_cases.py.

tests/interact_plan_print.cpp (its own main, includes only interact_plan.hpp) is compiled with the host C++ compiler
-- which is also the proof that the header needs no HIP -- fed every case on stdin and must print each row's expected
kernel, spelled with its template arguments as a kernel trace spells it, and what rides with the launch.  A second
build with -fsanitize=address,undefined runs the same input.
"""
import os
import shutil
import subprocess

import pytest

import interact_cases as ic

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def _build(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe,
                    os.path.join(HERE, "interact_plan_print.cpp")], check=True)
    return exe


def _run(exe):
    text = "".join(ic.encode(c) + "\n" for c in ic.CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ic.CASES)
    return [ln.split() for ln in out]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    return _run(_build(tmp_path_factory.mktemp("interact_plan"), "plan", ["-O1"]))


@pytest.mark.parametrize("k", range(len(ic.CASES)), ids=[c.name for c in ic.CASES])
def test_plan_row(answers, k):
    c = ic.CASES[k]
    got = ic.spelled(answers[k], c.rule)
    assert got == c.expected, (c.name, got, c.expected)


def test_cases_cover_what_the_table_needs():
    """Both sides of every threshold the launchers have, each alignment fact off, every rule's forms, every value of
    every knob."""
    names = {c.name for c in ic.CASES}
    for site in ic.SITES:
        assert {f"{site}-F{f}" for f in (16, 17, 32, 33, 96, 97, 112, 113)} <= names
        assert f"{site}-B0" in names
    for site in ("fwd", "lookup_fwd", "bwd_blocked", "step_fwd", "step_bwd"):
        assert {f"{site}-d{d}" for d in (64, 68, 128, 132, 256)} <= names
    assert {f"bwd-F40-d{d}" for d in (64, 68, 128, 132, 256)} <= names
    for site in ic.SITES:
        assert {f"{site}-d6", f"{site}-d12-bf16"} <= names
    assert {f"step_bwd-rowwise-d{d}" for d in (8, 16, 24)} <= names
    assert {"step_fwd-B2048", "step_fwd-B2049", "step_bwd-bf16-d128-B2048", "step_bwd-bf16-d128-B2049",
            "bwd_gather_ix-BL2048", "bwd_gather_ix-BL2049"} <= names
    assert {f"lookup_fwd-L{n}{ys}" for n in (1, 9, 10) for ys in ("", "-ys")} <= names
    assert {"lookup_fwd-T32", "lookup_fwd-T33", "lookup_fwd-rows-2^32", "step_fwd-rows-2^32"} <= names
    # each alignment fact, off alone, at each site that reads it: the address and the leading dimension of x, of
    # ys / t, of dx and of dt / dst, and the tables' rows
    off = {(c.site, k, "addr" if v[0] % 16 else "ld") for c in ic.CASES for k, v in c.ptr.items() if len(c.ptr) == 1}
    off |= {(c.site, "tabs", "addr") for c in ic.CASES if not c.tabs16}
    want = {("fwd", "x"), ("fwd", "t"), ("lookup_fwd", "x"), ("lookup_fwd", "t"), ("bwd", "t"), ("bwd", "dx"), ("bwd", "dt"),
            ("bwd_gather", "x"), ("bwd_gather", "dx"), ("bwd_gather", "dt"), ("bwd_gather_ix", "x"), ("bwd_gather_ix", "dx"),
            ("bwd_gather_ix", "dt"), ("bwd_blocked", "x"), ("bwd_blocked", "dx"), ("step_fwd", "x"), ("step_bwd", "x")}
    assert {(s, k, w) for s, k in want for w in ("addr", "ld")} | {("bwd_blocked", "dt", "addr")} <= off
    assert {(s, "tabs", "addr") for s in ic.SITES if s not in ("fwd", "bwd")} <= off
    for rule in ic.RULES:
        for dt in ("f32", "bf16"):
            assert {f"rule-{rule}-{dt}-NB{nb}-d{d}" for nb in (1, 2) for d in (16, 64, 128, 256)} <= names
    seen = {(k, v) for c in ic.CASES for k, v in c.knobs.items()}
    want = ({("bwd_ys_body", 1), ("bwd_nosplit", 1), ("bwd_cpl", 4), ("bwd_cpl", 8), ("upd_sbu", 1), ("upd_sbu", 2)} |
            {("bwd_spb", v) for v in (1, 2, 3, 4, 5, 8, 9)})
    assert want <= seen
    # (DLRM_BWD_CPL and DLRM_BWD_SPB under a rule that does not read them)
    assert any(c.rule != "descent" and "bwd_cpl" in c.knobs for c in ic.CASES)
    assert any(c.rule != "descent" and "bwd_spb" in c.knobs for c in ic.CASES)
    assert all(n in ic.BY_NAME for n in ic.GPU_CASES)


def test_plan_under_sanitizers(tmp_path, answers):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer (stand-alone host code): no report, the
    same answers."""
    exe = _build(tmp_path, "plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert _run(exe) == answers
