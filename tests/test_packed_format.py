"""The 28-bit packed format of fp32 A (csrc/gemv_packed.hpp), mirrored in NumPy: pack arithmetic, row layout, decode and the
refusals.  With P the decoded packed matrix and D the exception list (+true, -placeholder), P + D == A bit for bit."""
import numpy as np
import pytest

CPT, BPT = 16, 56                 # columns and packed bytes per thread and row
E0_MAX = 238
MAX_EXCEPTIONS = 1e-3


def window(bits):
    """pack_window: the even first exponent of the 16-binade window that holds most elements (ties: the lowest)."""
    hist = np.bincount((bits.ravel() >> 23) & 0xFF, minlength=256).astype(np.int64)
    counts = [(int(hist[e0:e0 + 16].sum()), -e0) for e0 in range(2, E0_MAX + 1, 2)]
    return -max(counts)[1]


def pack(A, threads):
    """-> (P uint8 [m, threads * 56], rows, cols, true bits, placeholder bits, e0), or None where the packer refuses."""
    m, n = A.shape
    assert n % CPT == 0 and n <= threads * CPT
    bits = np.ascontiguousarray(A, dtype=np.float32).view(np.uint32)
    ex = (bits >> 23) & 0xFF
    if (ex == 0xFF).any():
        return None                                        # inf / NaN
    e0 = window(bits)
    out = (ex < e0) | (ex > e0 + 15)
    if out.sum() > MAX_EXCEPTIONS * m * n:
        return None
    rows, cols = np.nonzero(out)
    ph = (bits & np.uint32(0x807FFFFF)) | (np.where(ex < e0, e0, e0 + 15).astype(np.uint32) << 23)      # pk::placeholder
    stored = np.where(out, ph, bits)
    full = np.zeros((m, threads * CPT), dtype=np.uint32)
    live = np.zeros((m, threads * CPT), dtype=bool)
    full[:, :n], live[:, :n] = stored, True
    g = full.reshape(m, threads, 4, 4)                     # [row][thread][group][element a b c d]
    lv = live.reshape(m, threads, 4, 4)
    d = g[..., 3]
    planes = np.stack([(g[..., 0] & 0xFFFFFF) | ((d & 0xFF) << 24), (g[..., 1] & 0xFFFFFF) | (((d >> 8) & 0xFF) << 24),
                       (g[..., 2] & 0xFFFFFF) | (((d >> 16) & 0xFF) << 24)], axis=1)        # [row][plane][thread][group]
    planes = np.where(lv[..., 0][:, None], planes, 0)
    nib = ((g >> 31) << 3) | ((((g >> 23) & 0xFF) - e0) >> 1)                               # pk::nibble_of
    nib = np.where(lv, nib, 0).astype(np.uint32)
    shift = (8 * np.arange(4)[None, :] + 4 * (np.arange(4)[:, None] & 1)).astype(np.uint32)  # [group][element]
    nb = np.zeros((m, threads, 2), dtype=np.uint32)
    for grp in range(4):
        nb[..., grp >> 1] |= (nib[:, :, grp, :] << shift[grp]).sum(axis=-1, dtype=np.uint32)
    P = np.concatenate([planes.reshape(m, -1), nb.reshape(m, -1)], axis=1).astype("<u4").view(np.uint8)
    assert P.shape == (m, threads * BPT)
    return P, rows, cols, bits[rows, cols], ph[rows, cols], e0


def decode(P, threads, n, e0):
    """The kernel's decode (top_bytes + the byte permutes of decode_group), vectorised."""
    m = P.shape[0]
    w = np.ascontiguousarray(P).view("<u4").reshape(m, -1)
    planes = w[:, :3 * threads * 4].reshape(m, 3, threads, 4)
    nb = w[:, 3 * threads * 4:].reshape(m, threads, 2)
    out = np.zeros((m, threads, 4, 4), dtype=np.uint32)
    e0h4 = np.uint32((e0 >> 1) * 0x01010101)
    for grp in range(4):
        word = nb[..., grp >> 1] >> np.uint32(4 * (grp & 1))
        top = ((((word & 0x0F0F0F0F) + 0x78787878) & 0x87878787) + e0h4).astype(np.uint32)
        p0, p1, p2 = planes[:, 0, :, grp], planes[:, 1, :, grp], planes[:, 2, :, grp]
        out[:, :, grp, 0] = (p0 & 0xFFFFFF) | ((top & 0xFF) << 24)
        out[:, :, grp, 1] = (p1 & 0xFFFFFF) | (((top >> 8) & 0xFF) << 24)
        out[:, :, grp, 2] = (p2 & 0xFFFFFF) | (((top >> 16) & 0xFF) << 24)
        out[:, :, grp, 3] = (p0 >> 24) | ((p1 >> 24) << 8) | ((p2 >> 24) << 16) | ((top >> 24) << 24)
    return out.reshape(m, -1)[:, :n]


def roundtrip(A, threads):
    res = pack(A, threads)
    assert res is not None
    P, rows, cols, tv, pv, e0 = res
    dec = decode(P, threads, A.shape[1], e0)
    bits = np.ascontiguousarray(A, dtype=np.float32).view(np.uint32)
    # P holds the placeholders exactly where D lists them, and A everywhere else: P + D == A bit for bit
    assert (dec[rows, cols] == pv).all() and (bits[rows, cols] == tv).all()
    dec[rows, cols] = tv
    assert (dec == bits).all()
    ex = (pv >> 23) & 0xFF
    assert ((ex >= e0) & (ex <= e0 + 15)).all() and e0 % 2 == 0
    return len(rows), e0


@pytest.mark.parametrize("m,n,threads", [(67, 16384, 1024), (131, 8192, 512), (37, 16368, 1024), (29, 4112, 512)])
def test_normal_data_roundtrips_bit_for_bit(m, n, threads):
    A = np.random.default_rng(n + m).standard_normal((m, n)).astype(np.float32)
    nex, e0 = roundtrip(A, threads)
    assert e0 in (112, 114, 116) and nex <= 3e-4 * m * n      # ~1e-4 of standard normal draws leave a 16-binade window


def test_zeros_denormals_tiny_and_huge_values_become_exceptions():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((64, 4096)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30, 1e30, -1e30, np.finfo(np.float32).max, np.finfo(np.float32).tiny],
                       dtype=np.float32)
    r, c = rng.integers(0, 64, 40), rng.integers(0, 4096, 40)
    A[r, c] = np.resize(special, 40)
    A[0, 0], A[0, -1], A[-1, 0], A[-1, -1] = 0.0, 1e30, -1e-40, -1e30
    nex, _ = roundtrip(A, 512)
    assert nex >= 30


def test_refuses_above_the_exception_cap_and_on_inf_nan():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((32, 1024)).astype(np.float32)
    sparse01 = (rng.random((32, 1024)) < 0.05).astype(np.float32)          # a 0/1 design: 95 % zeros
    assert pack(sparse01, 512) is None
    few = A.copy()
    few.ravel()[rng.choice(few.size, int(2e-3 * few.size), replace=False)] = 0.0
    assert pack(few, 512) is None
    for bad in (np.inf, -np.inf, np.nan):
        B = A.copy()
        B[5, 7] = bad
        assert pack(B, 512) is None
    assert pack(A, 512) is not None
