"""Shared input builders for the tests (same generators tests/golden/make_golden.py used)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def synth(m, n, seed, noise=0.1, density=0.05, dtype=np.float64):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    xt = np.zeros(n)
    nz = max(1, int(round(density * n)))
    idx = rng.choice(n, size=nz, replace=False)
    xt[idx] = rng.standard_normal(nz)
    b = A @ xt + noise * rng.standard_normal(m)
    return A.astype(dtype), b.astype(dtype), xt


def load(tag):
    return np.load(os.path.join(GOLDEN, f"{tag}.npz"))


def cases(tag):
    with open(os.path.join(GOLDEN, "cases.json")) as fh:
        return json.load(fh)["cases"][tag]


def problem(tag):
    """(A, b, fixture) for a golden tag; the 'aligned' A is regenerated from its seed and checked."""
    fx = load(tag)
    if tag == "aligned":
        meta = cases(tag)
        A, b, _ = synth(meta["m"], meta["n"], meta["seed"])
        assert np.array_equal(A[:2, :8], fx["aligned/A_head"]) and np.isclose(A.sum(), fx["aligned/A_sum"], rtol=1e-13), \
            "NumPy Generator stream changed: regenerate goldens"
        assert np.array_equal(b, fx["aligned/b"])
        return A, b, fx
    return fx[f"{tag}/A"], fx[f"{tag}/b"], fx


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))


def fp32_pass_tolerances(A, y, b, g_ref, rr_ref):
    """(gradient, ||r||^2) bounds of one fp32 pass over A against the fp64 oracle on the stored A.  r_i = A_i.y - b_i is
    formed with an absolute error of a few eps32 * (|A_i|.|y| + |b_i|) however small r_i itself is (m = 1, 2 rows with a
    nearly exact fit: seeds 438, 1409, 1444 of a 2000-case soak), grad = A^T r inherits it times |A|, ||r||^2 inherits
    2|r| times it.  b may be None."""
    A = np.asarray(A, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    m, n = A.shape
    eps32 = float(np.finfo(np.float32).eps)
    ab = np.abs(A) @ np.abs(y)
    if b is not None:
        ab = ab + np.abs(np.asarray(b, dtype=np.float64))
    dr = 4.0 * eps32 * float(np.linalg.norm(ab))
    r_norm = float(np.sqrt(rr_ref))
    g_tol = 2e-6 * float(np.linalg.norm(g_ref)) + float(np.linalg.norm(A, 2) if m * n <= 1 << 16 else np.linalg.norm(A)) * dr
    rr_tol = 5e-6 * rr_ref + 2.0 * r_norm * dr + dr * dr
    return g_tol, rr_tol


def fp32_pass_tolerances_cols(A, Y, B, G_ref, rr_ref):
    """fp32_pass_tolerances for every column of Y (n x k) at once: the same two bounds, as arrays of k entries (|A| is formed
    once for the block).  B: None, one b (m) for all columns or a block (m x k); G_ref (n x k), rr_ref (k)."""
    A = np.asarray(A, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    m, n = A.shape
    eps32 = float(np.finfo(np.float32).eps)
    ab = np.abs(A) @ np.abs(Y)
    if B is not None:
        B = np.abs(np.asarray(B, dtype=np.float64))
        ab = ab + (B if B.ndim == 2 else B[:, None])
    dr = 4.0 * eps32 * np.linalg.norm(ab, axis=0)
    rr_ref = np.asarray(rr_ref, dtype=np.float64)
    g_tol = 2e-6 * np.linalg.norm(np.asarray(G_ref, dtype=np.float64), axis=0) + \
        float(np.linalg.norm(A, 2) if m * n <= 1 << 16 else np.linalg.norm(A)) * dr
    rr_tol = 5e-6 * rr_ref + 2.0 * np.sqrt(rr_ref) * dr + dr * dr
    return g_tol, rr_tol
