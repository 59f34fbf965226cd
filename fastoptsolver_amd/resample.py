"""Resampled fits in the matrix-core lockstep: bootstrap paths, bagging, out-of-bag error and stability selection (extension).

Every lockstep column fits a resample of the rows of its own - row i enters the data term of column j with the multiplicity
c_ij in 0..15:

    minimise   sum_i c_ij w_i f(a_i.x, b_i)  +  alpha1 ||x||_1  +  0.5 alpha2 ||x||^2

with f the loss of the handle (squared with its 1/2, logistic, Huber, squared hinge) and w its sample weights (or 1): the problem
of a ``prepare_weighted`` handle with the weights w * c_j, but 16 resamples share one read of A per iteration instead of taking one
each, and nothing is bound to the handle.  The multiplicities travel as one 8-byte word per row, a nibble per column
(``pack_counts``; include/fos_resample.h); per row panel the launches are product 1 in its plain storing form, one link kernel
that forms the residual and multiplies it by the count (csrc/resample_link.hpp), and product 2.  Updates, restarts and stops are
the lockstep's own, so penalty factors, box bounds and feature groups compose.

``bootstrap_counts`` and ``subsample_counts`` draw the resamples, ``resampled_path`` solves a regularisation path on every one of
them (with the out-of-bag loss from one more pass), ``stability_selection`` (Meinshausen & Buehlmann 2010; complementary pairs:
Shah & Samworth 2013) counts how often a coordinate is selected.  A bootstrap column's Lipschitz constant lambda_max(A^T diag(w *
c_j) A) can exceed that of the whole A - a row drawn three times weighs three times -, so ``resampled_lipschitz`` runs the power
iteration per resample, 16 resamples per pass; for 0/1 counts the constant of the whole A is valid and is what is used.

Not served: the multinomial loss, the group penalty across columns, sharded problems, ``tol`` (the gradient-norm rule), ``comm=``
and ``cols=``.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _core, _lib
from . import iterative_solvers as _its

MAX_COUNT = 15                            # a nibble per (row, column)
COLUMNS = _its.LOCKSTEP_COLUMNS

ResampleResult = collections.namedtuple("ResampleResult", "alphas coefs oob_loss oob_size L info")
ResampleResult.__doc__ = """``coefs``: n x B x L, the fit of resample r at ``alphas[a]`` in ``coefs[:, r, a]``, of the kind that went
in; ``oob_loss``: B x L float64, the loss SUM over the rows resample r left out (None unless asked for); ``oob_size``: B float64, the
number of such rows - on a weighted handle their weight sum -; ``L``: B float64, lambda_max(A^T diag(w * c_r) A) as used for the
steps (before the logistic quarter); ``info[r][a] = (iterations, stop_code)``."""

StabilityResult = collections.namedtuple("StabilityResult", "alphas frequency max_frequency selected")
StabilityResult.__doc__ = """``frequency``: L x n float64, the share of the subsamples whose coefficient is non-zero at
``alphas[a]``; ``max_frequency``: n, its maximum over the path; ``selected``: the indices with ``max_frequency >= threshold``, in
increasing order."""


def _checked_counts(counts, m=None):
    """counts as a 2-D integer ndarray or tensor (left where it lives) with entries in 0..15; ValueError otherwise."""
    c = counts.detach() if _core.is_tensor(counts) else np.asarray(counts)
    if c.ndim != 2 or (m is not None and int(c.shape[0]) != int(m)):
        raise ValueError(f"counts: an m x nv integer array expected{'' if m is None else f' (m = {m})'}, got shape {tuple(c.shape)}")
    integral = (not c.dtype.is_floating_point and not c.dtype.is_complex) if _core.is_tensor(c) else c.dtype.kind in "iub"
    if not integral:
        raise ValueError(f"counts: integers expected, got {c.dtype}")
    if c.shape[0] and c.shape[1] and (int(c.min()) < 0 or int(c.max()) > MAX_COUNT):
        raise ValueError(f"counts: every multiplicity lies in 0..{MAX_COUNT} (a nibble per row and column; larger counts are not clipped)")
    return c


def pack_counts(counts, device=None):
    """The words the resample link kernel reads, from an m x nv (nv <= 16) integer array or tensor of multiplicities in 0..15: m
    int64 values (the bit pattern of the little-endian uint64 words), bits 4 j .. 4 j + 3 of word i holding counts[i, j]; columns
    from nv on are 0.  Packed where ``counts`` lives - a device tensor never leaves the device -, then moved to ``device`` if
    given.  ValueError for a count outside 0..15 (not clipped), nv > 16 or a shape that is not m x nv."""
    c = _checked_counts(counts)
    m, nv = int(c.shape[0]), int(c.shape[1])
    if nv < 1 or nv > COLUMNS:
        raise ValueError(f"counts: 1..{COLUMNS} columns expected (the lockstep's width), got {nv}")
    t = c if _core.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c).astype(np.int64))
    wide = torch.zeros(m, COLUMNS, dtype=torch.uint8, device=t.device)
    wide[:, :nv] = t.to(torch.uint8)
    words = (wide[:, 0::2] | (wide[:, 1::2] << 4)).contiguous().view(torch.int64).reshape(m)    # byte k: columns 2 k and 2 k + 1
    return words if device is None else words.to(device)


def bootstrap_counts(m, n_boot, seed=0):
    """m x n_boot int64 ndarray: column r counts how often each row is drawn when m of the m rows are drawn with replacement
    (``np.random.default_rng(seed)``, column after column).  Every column sums to m.  ValueError if a row is drawn more than 15
    times (about 2e-14 per row)."""
    m, n_boot = int(m), int(n_boot)
    if m < 1 or n_boot < 1:
        raise ValueError("bootstrap_counts: m >= 1 and n_boot >= 1 expected")
    rng = np.random.default_rng(seed)
    out = np.stack([np.bincount(rng.integers(0, m, size=m), minlength=m) for _ in range(n_boot)], axis=1).astype(np.int64)
    if out.max() > MAX_COUNT:
        raise ValueError(f"bootstrap_counts: a row was drawn {int(out.max())} times; the lockstep holds multiplicities up to {MAX_COUNT}")
    return out


def subsample_counts(m, n_sub, fraction=0.5, seed=0, complementary=True):
    """m x n_sub int64 ndarray of 0/1 columns with floor(fraction * m) ones each (``np.random.default_rng(seed)``).
    ``complementary``: columns 2 p and 2 p + 1 are the first and the second floor(fraction * m) rows of ONE permutation - disjoint
    halves at fraction 0.5 - (needs fraction <= 0.5; an odd n_sub leaves the last column without its partner); otherwise every
    column has a permutation of its own."""
    m, n_sub = int(m), int(n_sub)
    k = int(np.floor(float(fraction) * m))
    if m < 1 or n_sub < 1 or not 0.0 < float(fraction) < 1.0 or k < 1:
        raise ValueError("subsample_counts: m >= 1, n_sub >= 1 and a fraction in (0, 1) that keeps a row expected")
    if complementary and 2 * k > m:
        raise ValueError("subsample_counts: complementary pairs need fraction <= 0.5")
    rng = np.random.default_rng(seed)
    out = np.zeros((m, n_sub), dtype=np.int64)
    for col in range(0, n_sub, 2 if complementary else 1):
        perm = rng.permutation(m)
        out[perm[:k], col] = 1
        if complementary and col + 1 < n_sub:
            out[perm[k:2 * k], col + 1] = 1
    return out


def selection_frequencies(coefs):
    """L x n float64: the share of the B fits of an n x B x L block (ndarray or tensor) whose coefficient is non-zero."""
    c = coefs.detach().cpu().numpy() if _core.is_tensor(coefs) else np.asarray(coefs)
    if c.ndim != 3 or c.shape[1] < 1:
        raise ValueError(f"coefs: an n x B x L block expected, got shape {tuple(c.shape)}")
    return (c != 0).mean(axis=1).T.astype(np.float64)


def _handle(handle, who):
    if not isinstance(handle, _core.Problem):
        raise ValueError(f"{who}: a handle is expected (prepare, prepare_weighted, prepare_penalized, prepare_grouped, prepare_huber, prepare_hinge)")
    return handle


def _counts_on(prob, counts):
    """The checked m x B counts as an int64 tensor on the handle's device."""
    c = _checked_counts(counts, prob.m)
    if int(c.shape[1]) < 1:
        raise ValueError("counts: at least one resample is needed")
    t = c if _core.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c).astype(np.int64))
    return t.to(device=prob.device, dtype=torch.int64)


def _gram_apply(prob, X, words):
    """A^T diag(w * c_j) A X_j for the nv <= 16 columns of X (fos_gram_apply_resampled): n x nv float32 device tensor."""
    Xf, nv = prob._block16(X)
    G = torch.empty(nv, prob.n_dev, dtype=torch.float32, device=prob.device)
    with prob.ctx():
        _lib.check(prob.lib.fos_gram_apply_resampled(_core.ptr(Xf), nv, _core.ptr(words), prob.h, _core.ptr(G)), "fos_gram_apply_resampled")
    return prob.vec_out(G).t()


def resampled_lipschitz(handle, counts, n_iter=100, tol=1e-6):
    """lambda_max(A^T diag(w * c_r) A) per resample (the columns of ``counts``, m x B): float64 ndarray of length B.

    The power iteration of ``estimate_lipschitz`` on a weighted handle, 16 resamples per pass over A (fos_gram_apply_resampled;
    v is rounded to fp32 for the pass, the norms and v itself stay in fp64 on the host): one ``np.random.randn(n)`` per resample
    from the global legacy stream, in resample order, and the rule ``|L_k - L_{k-1}| < tol`` per resample - a resample that has
    stopped keeps its value while the others of its group go on."""
    prob = _handle(handle, "resampled_lipschitz")
    cdev = _counts_on(prob, counts)
    B = int(cdev.shape[1])
    V0 = np.stack([np.random.randn(prob.n) for _ in range(B)], axis=1)
    out = np.zeros(B)
    for first, number in _its._groups(B, COLUMNS):
        words = pack_counts(cdev[:, first:first + number])
        V = V0[:, first:first + number] / np.linalg.norm(V0[:, first:first + number], axis=0)
        prev, L, live = np.zeros(number), np.zeros(number), np.ones(number, dtype=bool)
        for _ in range(int(n_iter)):
            W = _gram_apply(prob, torch.from_numpy(V), words).to("cpu", torch.float64).numpy()
            nrm = np.linalg.norm(W, axis=0)
            L[live] = nrm[live]
            V[:, live] = W[:, live] / nrm[live]
            live = live & ~(np.abs(L - prev) < tol)
            if not live.any():
                break
            prev = L.copy()
        out[first:first + number] = L
    return out


def _run(handles, words, iters):
    arr = (C.c_void_p * len(handles))(*[h.h for h in handles])
    prob = handles[0].prob
    with prob.ctx():
        _lib.check(prob.lib.fos_fista_run_multi_resampled(arr, len(handles), int(iters), _core.ptr(words)), "fos_fista_run_multi_resampled")


def _oob_sums(prob, X, words):
    """The out-of-bag loss sums of the nv <= 16 columns of X (fos_gradient_batch_resampled, oob = 1): host list.  Synchronises."""
    Xf, nv = prob._block16(X)
    with prob.ctx():
        _lib.check(prob.lib.fos_gradient_batch_resampled(_core.ptr(Xf), nv, _core.ptr(words), 1, prob.h, None, _core.ptr(prob.scratch)),
                   "fos_gradient_batch_resampled")
    return prob.scratch[:nv].cpu().tolist()


def resampled_path(handle, alphas, counts, max_iter=500, *, L=None, t_init_factor=1.0, delta=None, tol_ratio=0.0,
                   adaptive_restart=False, restart_threshold=1.0, oob=False, **not_served):
    """The regularisation path ``alphas`` (``(alpha1, alpha2)`` pairs) on every resample of ``counts`` (m x B multiplicities in
    0..15: ``bootstrap_counts``, ``subsample_counts`` or the caller's) of the handle's problem.

    Every (resample, weight) pair is a lockstep column; the pairs run resample-major in groups of 16, each group one
    fos_fista_run_multi_resampled call on its own packed words (built on the device).  The step of resample r is ``t_init_factor /
    (L_r / divisor + alpha2 max_j p_j)``, divisor 4 for the logistic loss and 1 otherwise.  ``L``: None - for 0/1 counts the
    constant of the whole A (``estimate_lipschitz(handle)``: valid for every subsample), else ``resampled_lipschitz`` -, a number,
    or one number per resample; what the caller gives is used as it is.  ``delta``, ``tol_ratio``, ``adaptive_restart`` and
    ``restart_threshold`` as in ``fista_path``; there is no ``tol`` (the gradient-norm rule), ``comm=`` or ``cols=`` (ValueError).
    ``oob=True``: one more pass per group for the loss sums over the rows each resample left out.

    Contract: ``coefs[:, r, a]`` is what the path function of the handle's loss returns at ``alphas[a]`` on a handle with the
    sample weights ``w * counts[:, r]`` and that L.  Returns ``ResampleResult(alphas, coefs, oob_loss, oob_size, L, info)``.  What
    the library does not serve (the multinomial loss, a handle without b, ...) raises FosError with its refusal."""
    if not_served:
        for name in not_served:
            if name not in ("tol", "comm", "cols"):
                raise TypeError(f"resampled_path() got an unexpected keyword argument {name!r}")
        raise ValueError("resampled_path: a resampled lockstep cannot be combined with tol (the gradient-norm rule), comm= or cols=")
    prob = _handle(handle, "resampled_path")
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    cdev = _counts_on(prob, counts)
    B, La = int(cdev.shape[1]), len(alphas)
    mode = _lib.MODE_FISTA if delta is None else _lib.MODE_DELTA
    control = dict(mode=mode, delta=delta, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
    # the library's refusals come first, in its words: a call of no iterations decides the route and launches nothing
    _run([_its._new_state(prob, _its._params(1.0, alphas[0][0], alphas[0][1], **control))], pack_counts(cdev[:, :1]), 0)
    if L is None:
        Ls = np.full(B, _its.estimate_lipschitz(prob)) if int(cdev.max()) <= 1 else resampled_lipschitz(prob, cdev)
    else:
        Ls = np.broadcast_to(np.asarray(L, dtype=np.float64), (B,)).copy()
    divisor = 4.0 if prob.loss == "logistic" else 1.0
    pairs = [(r, a) for r in range(B) for a in range(La)]
    X = torch.zeros(prob.n, B, La, dtype=torch.float64, device=prob.device)
    oob_loss = np.zeros((B, La)) if oob else None
    info = [[None] * La for _ in range(B)]
    gtimer = _its._EventTimer(_its.grad_call_times)
    for first, number in _its._groups(len(pairs), COLUMNS):
        grp = pairs[first:first + number]
        words = pack_counts(cdev[:, [r for r, _ in grp]])
        handles = [_its._new_state(prob, _its._params(_its._tau(Ls[r] / divisor, alphas[a][1], t_init_factor, prob.penalty_max),
                                                      alphas[a][0], alphas[a][1], **control)) for r, a in grp]
        ev = gtimer.start()
        _run(handles, words, max_iter)
        gtimer.stop(ev, max_iter)
        xg = torch.stack([st.x_tensor() for st in handles], dim=1)
        q = _oob_sums(prob, xg, words) if oob else None
        stats = [st.status() for st in handles]
        gtimer.recount(max(int(s.k) for s in stats))
        for i, (r, a) in enumerate(grp):
            X[:, r, a] = xg[:, i]
            info[r][a] = (int(stats[i].k), int(stats[i].stopped))
            if oob:
                oob_loss[r, a] = q[i]
    gtimer.flush()
    out = (cdev == 0).to(torch.float64)
    size = (out.sum(dim=0) if prob.sample_weight is None else prob.sample_weight.to(torch.float64) @ out).cpu().numpy()
    return ResampleResult(alphas, _core.from_device_vec(X, prob.like), oob_loss, size, Ls, info)


def stability_selection(handle, alphas, n_pairs=50, fraction=0.5, threshold=0.6, seed=0, **path_args):
    """Stability selection with complementary pairs: ``2 * n_pairs`` subsamples of floor(fraction * m) rows
    (``subsample_counts(m, 2 * n_pairs, fraction, seed)``), the path ``alphas`` on every one through ``resampled_path``
    (``path_args``: its keyword arguments), and how often every coordinate is selected.  Returns ``StabilityResult(alphas,
    frequency, max_frequency, selected)``; ``threshold`` in (0, 1]."""
    prob = _handle(handle, "stability_selection")
    if int(n_pairs) < 1 or not 0.0 < float(threshold) <= 1.0:
        raise ValueError("stability_selection: n_pairs >= 1 and a threshold in (0, 1] expected")
    counts = subsample_counts(prob.m, 2 * int(n_pairs), fraction, seed, complementary=True)
    res = resampled_path(prob, alphas, counts, **path_args)
    freq = selection_frequencies(res.coefs)
    top = freq.max(axis=0)
    return StabilityResult(res.alphas, freq, top, np.flatnonzero(top >= float(threshold)))
