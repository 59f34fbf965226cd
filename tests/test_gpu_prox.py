"""GPU: the stand-alone prox kernels (fos_prox_l1, fos_prox_l1_vec, fos_prox_elastic_net, fos_prox_elastic_net_vec) through the
C entry points, at the sizes where the grid-stride loop changes shape and on the values where a soft threshold goes wrong.

Sizes: 1, 255, 256, 257 (around one 256-thread block) and 2048 * 256 + 1, the first n at which grid_1d(n, 256, 2048) is capped
and the stride loop takes a second trip (of one element).  Inputs: +-0, subnormals, +-inf, values exactly at +-thr, thr = 0, a
per-element threshold vector with zeros in it.  The output sits inside a NaN-filled buffer that has to stay NaN around it.

prox_l1 / prox_l1_vec equal the fp32 evaluation of sign(v) * max(|v| - thr, 0) bit for bit (one correctly rounded subtraction),
the sign of zero included.  The elastic-net kernels are within 4 eps32 (relative) of the fp64 oracle on the fp32 inputs: alpha1
is a power of two here, so thr = tau * alpha1 is exact and what is left are the roundings of the subtraction, of tau * alpha2,
of 1 + that (or its fused form) and of the division - half an eps32 each.  (With an inexact thr the rounding of the product is
amplified without limit by the cancellation in |v| - thr: no relative bound holds for any fp32 evaluation.)  A result in the
subnormal range is allowed one quantum (2^-149), which no relative bound can express."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
TINY = float(np.finfo(np.float32).smallest_subnormal)
SIZES = (1, 255, 256, 257, 2048 * 256 + 1)
THR = np.float32(0.7)
GUARD = 4
ALPHA1, ALPHA2 = 2.0, 0.5                      # alpha1 a power of two: tau * alpha1 is exact in fp32


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return _lib.load()


def _specials(thr):
    sub = np.float32(1e-40)
    return np.array([-0.0, 0.0, sub, -sub, TINY, -TINY, np.inf, -np.inf, thr, -thr, np.nextafter(thr, np.float32(2)),
                     -np.nextafter(thr, np.float32(2)), np.nextafter(thr, np.float32(0)), 1.5, -1.5, 3e38, -3e38, 1e-38, -1e-38],
                    dtype=np.float32)


def _inputs(n, thr):
    """(v, per-element thresholds, where v = +-thr[i]): the special values first and again at the very end (the element of the
    second trip), seeded normals between; the threshold vector has zeros in it, and v sits exactly at +-thr[i] on some elements."""
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n).astype(np.float32)
    sp = _specials(np.float32(thr))
    k = min(n, sp.size)
    v[:k] = sp[:k]
    if n > 2 * sp.size:
        v[-sp.size:] = sp[::-1]
    tv = np.abs(rng.standard_normal(n)).astype(np.float32)
    tv[::3] = 0.0
    at = np.arange(sp.size + 1, n - sp.size, 7)                 # between the special values
    v[at] = np.where(at % 2 == 0, tv[at], -tv[at])
    return v, tv, at


def _run(fn, n, *args):
    """Call a prox entry point with its output inside a NaN-filled buffer: (out, the guards stayed NaN).  args: device tensors
    (passed as pointers) and ctypes scalars, in the C order with `out` and n appended by position."""
    from fastoptsolver_amd import _core
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + n]
    cargs = [_core.ptr(a) if torch.is_tensor(a) else a for a in args]
    assert fn(*cargs, _core.ptr(out), n, _core.stream_ptr()) == 0
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return h[GUARD:GUARD + n], bool(np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + n:]).all())


def _soft32(v, thr):
    """sign(v) * max(|v| - thr, 0) evaluated in fp32 (prox_operators.py:8)."""
    v, thr = np.asarray(v, dtype=np.float32), np.asarray(thr, dtype=np.float32)
    return (np.sign(v) * np.maximum(np.abs(v) - thr, np.float32(0))).astype(np.float32)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_prox_l1_is_the_fp32_expression_bit_for_bit(lib, n):
    for thr in (THR, np.float32(0.0)):
        v, tv, at = _inputs(n, thr)
        vd = torch.as_tensor(v).cuda()
        got, clean = _run(lib.fos_prox_l1, n, vd, C.c_float(float(thr)))
        want = _soft32(v, thr)
        assert clean and _same_bits(got, want), (n, thr, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
        if thr == 0:
            nz = v != 0
            assert _same_bits(got[nz], v[nz]) and not np.signbit(got[~nz]).any()      # the identity, and +0 for +-0
    v, tv, at = _inputs(n, THR)
    got, clean = _run(lib.fos_prox_l1_vec, n, torch.as_tensor(v).cuda(), torch.as_tensor(tv).cuda())
    want = _soft32(v, tv)
    assert clean and _same_bits(got, want), (n, "vec", np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    assert not got[at].any() and np.array_equal(np.signbit(got[at]), np.signbit(v[at]) & (v[at] != 0))    # exactly at +-thr[i]


def _within(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    inf = np.isinf(ref)
    assert np.array_equal(got[inf].astype(np.float64), ref[inf]), what
    err = np.abs(got[~inf].astype(np.float64) - ref[~inf])
    bound = 4.0 * EPS32 * np.abs(ref[~inf]) + TINY
    worst = int(np.argmax(err - bound)) if err.size else 0
    assert (err <= bound).all(), (what, worst, err[worst], bound[worst])
    z = ref == 0
    assert not got[z].any() and np.array_equal(np.signbit(got[z]), np.signbit(ref[z])), what       # zeros and their sign


@pytest.mark.parametrize("n", SIZES)
def test_prox_elastic_net_within_four_eps_of_the_oracle(lib, n):
    for tau in (np.float32(0.35), np.float32(0.0)):
        thr = np.float32(tau * np.float32(ALPHA1))
        assert float(thr) == float(tau) * ALPHA1                                       # exact
        v, tv, at = _inputs(n, thr)
        got, clean = _run(lib.fos_prox_elastic_net, n, torch.as_tensor(v).cuda(), C.c_float(float(tau)), C.c_float(ALPHA1),
                          C.c_float(ALPHA2))
        with np.errstate(invalid="ignore"):
            ref = orc.prox_elastic_net(v.astype(np.float64), float(tau), ALPHA1, ALPHA2)
        assert clean, (n, tau)
        _within(got, ref, (n, float(tau)))
    # per-element tau with zeros in it; v exactly at +-tau[i] * alpha1 on some elements
    v, tv, at = _inputs(n, THR)
    tauv = (tv / np.float32(ALPHA1)).astype(np.float32)
    assert np.array_equal(tauv * np.float32(ALPHA1), tv)
    got, clean = _run(lib.fos_prox_elastic_net_vec, n, torch.as_tensor(v).cuda(), torch.as_tensor(tauv).cuda(),
                      C.c_float(ALPHA1), C.c_float(ALPHA2))
    with np.errstate(invalid="ignore"):
        ref = orc.prox_elastic_net(v.astype(np.float64), tauv.astype(np.float64), ALPHA1, ALPHA2)
    assert clean, (n, "vec")
    _within(got, ref, (n, "vec"))
