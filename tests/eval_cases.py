"""Inputs shared by tests/test_eval_host.py (CPU) and tests/test_eval.py (GPU)."""
import numpy as np

SOFT, NAN = 7, 11  # positions of the one soft label and the one NaN score


def crafted(n=500, seed=5):
    """n probabilities and labels that hit every edge of the evaluation rules: 0, 1, 0.5 (a rounding tie),
    the float after 0.5, 0.25 and the float before it (neighbouring bins), each under both labels; duplicates
    (the rest is drawn from 40 values, a few pairs of them closer than one bin); one soft label; one NaN."""
    rng = np.random.default_rng(seed)
    f = np.float32
    edges = np.array([0.0, 1.0, 0.5, np.nextafter(f(0.5), f(1.0)), 0.25, np.nextafter(f(0.25), f(0.0))], dtype=f)
    pool = rng.random(40).astype(f)
    pool[1] = np.nextafter(pool[0], f(1.0))  # same bin unless pool[0] ends one
    pool[3] = pool[2] * f(1.0 + 2.0 ** -9)   # a neighbouring bin or the one after
    p = pool[rng.integers(0, 40, n)]
    y = (rng.random(n) < 0.4).astype(f)
    k = 20
    for e in edges:  # each edge value as a negative and as a positive
        p[k], y[k], p[k + 1], y[k + 1] = e, 0.0, e, 1.0
        k += 2
    y[SOFT] = 0.3
    p[NAN] = np.nan
    y[NAN] = 1.0
    return p, y
