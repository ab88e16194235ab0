"""Row families shared by tests/test_q8_host.py (CPU) and tests/test_q8.py (GPU): seeded float32 rows [N][D]."""
import numpy as np

F = np.float32


def extremes(n, d, seed=7):
    """Rows whose extremes sit in the first and the last column (min first, max last; then the other way)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, size=(n, d)).astype(F)
    w[:, 0], w[:, -1] = -3.0, 5.0
    w[1::2, 0], w[1::2, -1] = 5.0, -3.0
    return w


def families(d, n=12, seed=0):
    """name -> [n][d] float32 rows: standard normal, uniform +-0.05, 1000 + 1e-3 normal, constant, two-valued,
    rows scaled by 1e-30 and by 1e30, extremes in the first and the last column."""
    rng = np.random.default_rng(1000 * d + seed)
    normal = rng.standard_normal((n, d)).astype(F)
    out = {
        "normal": normal,
        "uniform": rng.uniform(-0.05, 0.05, size=(n, d)).astype(F),
        "offset": (F(1000.0) + F(1e-3) * rng.standard_normal((n, d)).astype(F)).astype(F),
        "constant": np.repeat(rng.standard_normal((n, 1)).astype(F), d, axis=1),
        "two-valued": np.where(rng.random((n, d)) < 0.5, F(-0.75), F(1.5)).astype(F),
        "tiny": (normal * F(1e-30)).astype(F),
        "huge": (normal * F(1e30)).astype(F),
        "extremes": extremes(n, d, seed),
    }
    if d > 1:  # both values present in every two-valued row
        out["two-valued"][:, 0], out["two-valued"][:, -1] = F(-0.75), F(1.5)
    return out


def bf16_values(w):
    """float32 rows truncated to values a bf16 holds exactly."""
    return (np.ascontiguousarray(w, dtype=F).view(np.uint32) & np.uint32(0xFFFF0000)).view(F)


def mixed(d, rows, seed=0):
    """Tables of the given row counts, rows drawn from every family in turn."""
    fam = list(families(d, n=max(rows), seed=seed).values())
    out = []
    for t, n in enumerate(rows):
        w = np.empty((n, d), dtype=F)
        for r in range(n):
            w[r] = fam[(r + t) % len(fam)][r]
        out.append(w)
    return out
