"""tests/sequence_cases.py on the host: what the scripts of tests/test_indexer_sequences.py claim about themselves.

  - Forms: through tests/build_plan_print.cpp (as tests/test_build_plan_host.py drives it) every step's planned form,
    wave kernel and return code are the ones its row names; across scripts A to E each form class is followed at least
    once by a form of another class on the same indexer, and wave -> non-wave, non-wave -> wave and larger N ->
    smaller N each occur at least three times.
  - Exactness: for every step's indices and integer gradient k (the update's gradient is k / 64),
    64 * max |row sum| < 2^24 on the float64 reference: a condition on the inputs, checked on the reference alone.
  - Segment classes: every draw of a hot step holds every class of sequence_cases.CLASSES but those its row lists as
    absent.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import build_cases
import sequence_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def _all_steps():
    """(label, cap, rows, step) of every step of every script, history and of the table-set test."""
    out = [(f"{s.name}{k}", s.cap, s.rows, st) for s in sc.SCRIPTS for k, st in enumerate(s.steps)]
    for name, by_cap in sc.HISTORIES.items():
        for cap, pair in by_cap.items():
            out += [(f"{name}-{cap}-{k}", cap, sc.ROWS, st) for k, st in enumerate(pair)]
    out.append(("tables", sc.TABLE_SET_CAP, sc.ROWS, sc.TABLE_SET_STEP))
    return out


STEPS = _all_steps()


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("sequence_plan")), "plan")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(HERE, "build_plan_print.cpp")], check=True)
    text = "".join(build_cases.encode(sc.as_case(cap, rows, st, label)) + "\n" for label, cap, rows, st in STEPS)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(STEPS)
    return {label: ln.split() for (label, _, _, _), ln in zip(STEPS, out)}


@pytest.mark.parametrize("k", range(len(STEPS)), ids=[s[0] for s in STEPS])
def test_step_takes_the_form_its_row_names(plans, k):
    label, _cap, _rows, st = STEPS[k]
    f = plans[label]
    assert (f[0], f[1], int(f[7])) == (st.form, st.kind, st.rc), (label, f)
    assert st.N % st.L == 0 and (st.L == 1 or st.site == "build")


def test_histories_are_followed_by_another_form():
    for name, by_cap in sc.HISTORIES.items():
        assert set(by_cap) == {8192, 32768}, name
        for first, then in by_cap.values():
            assert sc.form_class(first) != sc.form_class(then), name
            assert first.N >= 2048 and then.N >= 2048  # (the 3-row table's rows: several slices each)


def test_scripts_cover_the_transitions():
    followed, wave_out, wave_in, shrink = set(), 0, 0, 0
    for s in sc.SCRIPTS:
        done = [st for st in s.steps if st.rc == 0]
        for a, b in zip(done, done[1:]):
            if sc.form_class(a) != sc.form_class(b):
                followed.add(sc.form_class(a))
            wave_out += a.form == "wave" and b.form != "wave"
            wave_in += a.form != "wave" and b.form == "wave"
            shrink += b.N < a.N
    assert followed >= {"lds2", "lds4", "lds_parts", "bag", "hash", "sorted", "wave_one", "wave_rounds", "wave_scan16",
                        "in_forward"}
    assert wave_out >= 3 and wave_in >= 3 and shrink >= 3, (wave_out, wave_in, shrink)
    assert {st.site for s in sc.SCRIPTS for st in s.steps} == {"build", "build_split", "prepare", "step_fwd", "in_apply"}


def _draws(label, k, st, rows):
    for draw in range(2 if st.hot else 1):
        yield draw, sc.draw_indices(label, k, draw, rows, st.N)


def _built():
    """(name, step number, step, rows) of every build check_build follows: the scripts' steps, the histories' clean
    steps (their step 1) and the table-set test's."""
    out = [(s.name, k, st, s.rows) for s in sc.SCRIPTS for k, st in enumerate(s.steps) if st.rc == 0]
    out += [(f"{h}-{cap}", 1, pair[1], sc.ROWS) for h, by_cap in sc.HISTORIES.items() for cap, pair in by_cap.items()]
    out += [("tables", k, sc.TABLE_SET_STEP, sc.ROWS) for k in range(len(sc.TABLE_SETS))]
    return out


@pytest.mark.parametrize("group", [s.name for s in sc.SCRIPTS] + ["histories", "tables"])
def test_gradients_sum_exactly(group):
    """64 * max |row sum| < 2^24 for every step's indices and gradient (N * K < 2^24 bounds every partial sum too)."""
    mine = [b for b in _built() if b[0] == group or (group == "histories" and "-" in b[0])]
    assert mine
    for name, k, st, rows in mine:
        dim = sc.TABLE_SETS[k][1] if name == "tables" else sc.DIM
        assert st.N * sc.exact_k(st.N) < 1 << 24
        for draw, idx in _draws(name, k, st, rows):
            if name == "tables" and draw:
                continue  # (one draw per table set)
            kk = sc.draw_exact(name, k, draw, st.N // st.L, len(rows) * dim, st.N)
            assert np.abs(kk).max() <= sc.exact_k(st.N)
            for t, n in enumerate(rows):
                sums = sc.scatter_sums(idx[t], kk[:, t * dim:(t + 1) * dim], n, st.L)
                assert np.abs(sums).max() < 1 << 24, (name, k, t)  # (sums of k: 64 times the gradient's)


def test_hot_steps_hold_every_segment_class():
    want = {c[0] for c in sc.CLASSES}
    hot = 0
    for s in sc.SCRIPTS:
        for k, st in enumerate(s.steps):
            if not st.hot:
                assert not st.absent
                continue
            hot += 1
            for draw, idx in _draws(s.name, k, st, s.rows):
                assert sc.classes_present(idx) == want - set(st.absent), (s.name, k, draw)
    assert hot >= 12
    for k in range(len(sc.TABLE_SETS)):
        idx = sc.draw_indices("tables", k, 0, sc.ROWS, sc.TABLE_SET_STEP.N)
        assert sc.classes_present(idx) == want - set(sc.TABLE_SET_STEP.absent), k
    # the multi-slice hot table of the histories
    for by_cap in sc.HISTORIES.values():
        for pair in by_cap.values():
            for st in pair:
                assert st.N // 3 > 2 * sc.HOT_SLICE
