"""Device-side plumbing: tensors in, C-ABI handles out.  torch is used for device memory, streams and
events only; every arithmetic operation on the hot path is a HIP kernel behind include/fos.h."""
import ctypes as C
import collections
import math

import numpy as np
import torch

from . import _lib


def require_gpu():
    if not torch.cuda.is_available():
        raise _lib.FosError("fastoptsolver_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                            "there is no CPU fallback by design")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def is_tensor(x):
    return isinstance(x, torch.Tensor)


def to_device(x, device=None, dtype=torch.float32):
    """Contiguous CUDA tensor (float32 unless told otherwise) of the same shape from an ndarray / tensor of any rank."""
    if is_tensor(x):
        t = x.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return t.to(device=dev, dtype=dtype).contiguous()


to_device_vec = to_device       # the name for a vector


def stores_bf16(A, dtype=None):
    """Whether the device copy of A is kept in bf16: asked for by `dtype`, or A arrives as a bf16 tensor and nothing else was
    asked for."""
    return (dtype in ("bf16", torch.bfloat16)) or (dtype is None and is_tensor(A) and A.dtype == torch.bfloat16)


UPLOAD_CHUNK_BYTES = 256 << 20
LOSSES = {"squared": _lib.LOSS_SQUARED, "logistic": _lib.LOSS_LOGISTIC, "multinomial": _lib.LOSS_MULTINOMIAL}
# the losses behind the pointwise link kernel (fos_problem_set_link_loss): they take a parameter, so `prepare_huber` /
# `prepare_hinge` build their handles, not `prepare(loss=...)`
LINK_LOSSES = {"huber": _lib.LOSS_HUBER, "squared_hinge": _lib.LOSS_SQUARED_HINGE}
MAX_CLASSES = 16                         # a class group of the multinomial lockstep is C of its 16 columns
LOGIT_MAX_N = 16384                      # device columns the matrix-core pair serves (csrc/fos_plan.hip pair_dd_multi_supported)
GROUPED_BOUNDS = "the group penalty does not compose with box bounds (lower / upper); penalty factors do"
LOGIT_MIN_N = {"f32": 68, "bf16": 72}    # the narrowest streaming width: 64 columns plus one 16-byte chunk


def upload_matrix(src, out):
    """Host matrix -> the device view `out` (same shape; any float dtype, row- or column-major source).  The reference's
    callers hand float64 ndarrays: converting on the host first cost 0.44 s for 65536 x 8192 (the 500-iteration solve behind
    it takes 0.19 s).  Here the bytes cross in the SOURCE dtype and layout, 256 MiB at a time, and the conversion / transposition
    is the device copy into place - the rounding (to nearest even, via float32 for bf16) is the one the host cast performs."""
    m, n = src.shape
    if m == 0 or n == 0:
        return out
    esz = src.element_size()
    if src.dtype == out.dtype and src.is_contiguous() and out.is_contiguous():
        out.copy_(src)
    elif src.stride(1) == 1 and src.stride(0) == n:                      # row-major: row blocks
        step = max(1, UPLOAD_CHUNK_BYTES // (n * esz))
        for r0 in range(0, m, step):
            out[r0:r0 + step].copy_(src[r0:r0 + step].to(out.device))
    elif src.stride(0) == 1 and src.stride(1) == m:                      # column-major (Fortran order): column blocks, whose
        step = max(1, UPLOAD_CHUNK_BYTES // (m * esz))                   # transposes are contiguous on the host
        for c0 in range(0, n, step):
            out[:, c0:c0 + step].copy_(src[:, c0:c0 + step].t().to(out.device).t())
    else:
        out.copy_(src.to(out.dtype))
    return out


def checked_weights(w, m):
    """Sample weights as a float64 tensor where they live: m entries, finite, >= 0 and not all zero - ValueError otherwise.
    Checked once, before any device work of the problem."""
    t = (w.detach() if is_tensor(w) else torch.from_numpy(np.array(w, dtype=np.float64))).to(torch.float64)
    if t.dim() != 1 or t.numel() != m:
        raise ValueError(f"sample_weight must have m = {m} entries, got shape {tuple(t.shape)}")
    if not bool((torch.isfinite(t) & (t >= 0)).all()):
        raise ValueError("sample_weight must be finite and >= 0")
    if not bool((t > 0).any()):
        raise ValueError("sample_weight must not be all zero")
    return t


def checked_labels(y, classes=None):
    """The labels of a multinomial problem as a float64 ndarray and the number of classes C: one integral class index 0 .. C-1
    per row, C given or (None) max(y) + 1, 2 <= C <= 16 - ValueError otherwise.  Checked on the host, before any device work."""
    if y is None:
        raise ValueError("a multinomial problem needs its labels")
    a = np.asarray(y.detach().cpu().numpy() if is_tensor(y) else y)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iufb":
        raise ValueError(f"multinomial labels: one class index per row expected, got shape {a.shape} and dtype {a.dtype}")
    a = a.astype(np.float64)
    if not np.isfinite(a).all() or (a != np.floor(a)).any() or a.min() < 0:
        raise ValueError("multinomial labels must be integral class indices >= 0")
    if classes is None:
        classes = int(a.max()) + 1
    elif isinstance(classes, (bool, np.bool_)) or not isinstance(classes, (int, np.integer)):
        raise ValueError(f"classes: an int expected, got {classes!r}")
    classes = int(classes)
    if not 2 <= classes <= MAX_CLASSES:
        raise ValueError(f"classes: 2 <= C <= {MAX_CLASSES} expected, got {classes}")
    if a.max() > classes - 1:
        raise ValueError(f"multinomial labels must lie in 0 .. {classes - 1}, got {int(a.max())}")
    return a, classes


def checked_threshold(threshold):
    """The Huber threshold as a float: finite and > 0 - ValueError otherwise, before any device work."""
    if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"threshold: a number expected, got {threshold!r}")
    threshold = float(threshold)
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError(f"threshold: finite and > 0 expected, got {threshold}")
    return threshold


def checked_signs(y):
    """The labels of a squared-hinge problem as a float64 ndarray: one value per row, each exactly -1 or +1 - ValueError
    otherwise.  Checked on the host, before any device work."""
    if y is None:
        raise ValueError("a squared-hinge problem needs its labels")
    a = np.asarray(y.detach().cpu().numpy() if is_tensor(y) else y)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iuf":
        raise ValueError(f"squared-hinge labels: one value -1 / +1 per row expected, got shape {a.shape} and dtype {a.dtype}")
    a = a.astype(np.float64)
    if not (np.abs(a) == 1.0).all():
        raise ValueError("squared-hinge labels must be exactly -1 or +1")
    return a


def checked_class_groups(ncols, classes):
    """The number of class groups that `ncols` lockstep columns of a C-class multinomial problem hold: ncols is a multiple of C
    and at most 16 - ValueError otherwise, before any device work."""
    if ncols < 1 or ncols > 16 or ncols % classes:
        raise ValueError(f"a multinomial problem with {classes} classes takes a multiple of {classes} columns (at most 16), got {ncols}")
    return ncols // classes


def checked_coord(penalty_factor, lower, upper, n):
    """Per-coordinate penalty factors and box bounds as float64 ndarrays of length n (None stays None; scalars broadcast):
    factors finite and >= 0, bounds not NaN with lower <= 0 <= upper (x0 = 0 stays feasible; -inf / +inf mean "no bound") -
    ValueError otherwise.  Checked on the host, before any device work."""
    def vec(v, name):
        if v is None:
            return None
        a = np.asarray(v.detach().cpu().numpy() if is_tensor(v) else v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(n, float(a))
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"{name} must be a scalar or have n = {n} entries, got shape {a.shape}")
        if np.isnan(a).any():
            raise ValueError(f"{name} must not hold NaN")
        return a
    pf, lo, hi = vec(penalty_factor, "penalty_factor"), vec(lower, "lower"), vec(upper, "upper")
    if pf is not None and not (np.isfinite(pf) & (pf >= 0)).all():
        raise ValueError("penalty_factor must be finite and >= 0")
    if lo is not None and (lo > 0).any():
        raise ValueError("lower must be <= 0 (the start x0 = 0 has to be feasible)")
    if hi is not None and (hi < 0).any():
        raise ValueError("upper must be >= 0 (the start x0 = 0 has to be feasible)")
    return pf, lo, hi


FeatureGroups = collections.namedtuple("FeatureGroups", "start weight l1_ratio")


def checked_feature_groups(groups, group_weight, l1_ratio, n):
    """The feature groups of `Problem.set_feature_groups` as (start, weight, l1_ratio): start the ngroups + 1 boundaries (int32
    ndarray, start[0] = 0, start[-1] = n), weight ngroups float64 values (sqrt(size) where none are given), l1_ratio a float in
    [0, 1].  groups: n labels whose equal labels are contiguous, or positive sizes summing to n (a sequence of n entries is read
    as labels).  ValueError otherwise.  Checked on the host, before any device work."""
    g = np.asarray(groups.detach().cpu().numpy() if is_tensor(groups) else groups)
    if g.ndim != 1 or g.shape[0] < 1:
        raise ValueError(f"groups: n = {n} labels or a sequence of group sizes expected, got shape {g.shape}")
    if g.shape[0] == n:                                  # labels
        change = np.flatnonzero(g[1:] != g[:-1]) + 1
        start = np.concatenate(([0], change, [n]))
        first = g[start[:-1]]
        if len(set(first.tolist())) != len(first):
            raise ValueError("groups: a label reappears after a gap - the columns of a group must be contiguous: permute the "
                             "columns of A so that every group is one block")
    else:                                                # sizes
        if g.dtype.kind not in "iu" and not (g.dtype.kind == "f" and np.all(np.isfinite(g)) and np.all(g == np.floor(g))):
            raise ValueError("groups: integer group sizes expected")
        sizes = g.astype(np.int64)
        if (sizes < 1).any() or int(sizes.sum()) != n:
            raise ValueError(f"groups: {g.shape[0]} entries are neither n = {n} labels nor positive sizes summing to n "
                             f"(sum {int(sizes.sum())})")
        start = np.concatenate(([0], np.cumsum(sizes)))
    start = start.astype(np.int32)
    ngroups = len(start) - 1
    if group_weight is None:
        w = np.sqrt(np.diff(start).astype(np.float64))
    else:
        w = np.asarray(group_weight.detach().cpu().numpy() if is_tensor(group_weight) else group_weight, dtype=np.float64)
        if w.ndim == 0:
            w = np.full(ngroups, float(w))
        if w.ndim != 1 or w.shape[0] != ngroups:
            raise ValueError(f"group_weight must be a scalar or have one entry per group ({ngroups}), got shape {w.shape}")
        if not (np.isfinite(w) & (w >= 0)).all():
            raise ValueError("group_weight must be finite and >= 0")
    r = float(l1_ratio)
    if not (0.0 <= r <= 1.0):                            # NaN fails too
        raise ValueError(f"l1_ratio must lie in [0, 1], got {l1_ratio!r}")
    return start, w, r


class Like:
    """What the caller handed in (so results come back as the same kind) without keeping the object alive."""

    def __init__(self, obj):
        self.tensor = is_tensor(obj)
        if self.tensor:
            self.dtype = obj.dtype if obj.dtype in (torch.float32, torch.float64) else torch.float32
            self.device = obj.device


def from_device_vec(t, like):
    """Return `t` as the same kind of object the caller handed in: ndarray float64, or a tensor on the caller's
    device in the caller's floating dtype (bf16 inputs get float32 back)."""
    if isinstance(like, Like):
        if like.tensor:
            return t.to(device=like.device, dtype=like.dtype, copy=True)
        return t.detach().to("cpu", torch.float64).numpy()
    if is_tensor(like):
        return from_device_vec(t, Like(like))
    return t.detach().to("cpu", torch.float64).numpy()


class Problem:
    """A (m x n, fp32 or bf16, row-major) and b bound to a fos_problem handle.

    Accepts ndarrays or tensors; a contiguous CUDA tensor of the right dtype is borrowed without a copy.
    Build it once with ``prepare(A, b)`` and pass it wherever the solvers take ``A`` to avoid re-uploading A.
    """

    def __init__(self, A, b=None, dtype=None, pad=None, loss="squared", sample_weight=None):
        """loss: "squared" (b is the target of 0.5 ||Ax - b||^2), "logistic" (b holds labels in [0, 1]; the data term is the
        log-loss, served by `logistic_path` / `logistic_cv` / `logistic_objective` only: fos_problem_set_loss) or "multinomial"
        (b holds class indices 0 .. C-1, C = max(b) + 1 - `Problem.multinomial` takes C; the data term is the softmax
        cross-entropy, served by `multinomial_path` / `multinomial_cv` / `multinomial_objective` only: fos_problem_set_multinomial;
        `.classes` is C, None on any other handle).
        pad: zero-pad the columns of the device copy of A to the fused kernel's granularity (4 fp32 / 8 bf16
        elements, 16-byte aligned rows) so that a ragged n or a misaligned view still gets the single-pass kernel
        (4x faster than the two-pass path at 65536 x 8190).  Zero columns stay exactly zero through gradient and
        prox, and every vector is padded / trimmed here, so callers never see them.  None = only for problems large
        enough for it to matter (m*n >= 2^20: the padded single pass is 3-14x faster from there on); small ragged problems
        keep the fp64-accumulating two-pass path.  A logistic problem runs on the matrix-core pair alone, so for it None means
        always: rows are padded to the granularity, and to 68 fp32 / 72 bf16 columns when n <= 64 - every shape up to 16384
        device columns is served; more raise ValueError.
        sample_weight: m per-row weights w_i >= 0 of the data term (`prepare_weighted`; fos_row_weights_bind).  A weighted problem
        runs on the matrix-core pair alone as a logistic one does and is padded by the same rules."""
        self._setup(A, b, dtype, pad, loss, sample_weight)

    @classmethod
    def penalized(cls, A, b, penalty_factor=None, lower=None, upper=None, dtype=None, loss="squared", sample_weight=None):
        """The handle of a problem with per-coordinate penalty factors and box bounds (`prepare_penalized`): __init__'s
        parameter list is part of the interface and stays as it is, so this is the constructor that takes them."""
        prob = cls.__new__(cls)
        prob._setup(A, b, dtype, None, loss, sample_weight, penalty_factor, lower, upper)
        return prob

    @classmethod
    def multinomial(cls, A, y, classes=None, dtype=None, sample_weight=None, penalty_factor=None, lower=None, upper=None):
        """The handle of a multinomial (softmax) problem with C = `classes` classes (None: max(y) + 1), with or without row
        weights, penalty factors and bounds: the constructor that takes the number of classes (`prepare_multinomial`)."""
        prob = cls.__new__(cls)
        prob._setup(A, y, dtype, None, "multinomial", sample_weight, penalty_factor, lower, upper, classes)
        return prob

    @classmethod
    def link(cls, A, b, loss, threshold=None, dtype=None, sample_weight=None):
        """The handle of a Huber (`prepare_huber`; `threshold` is c) or squared-hinge (`prepare_hinge`; b holds the labels -1 /
        +1) problem, with or without row weights: the constructor that takes the loss's parameter."""
        if loss not in LINK_LOSSES:
            raise ValueError(f"loss: one of {sorted(LINK_LOSSES)} expected, got {loss!r}")
        prob = cls.__new__(cls)
        prob._setup(A, b, dtype, None, loss, sample_weight, threshold=threshold)
        return prob

    @classmethod
    def grouped_features(cls, A, b, groups, group_weight=None, l1_ratio=0.0, dtype=None, loss="squared", sample_weight=None):
        """The handle of a problem with feature groups (`prepare_grouped`): the constructor that takes them."""
        prob = cls.__new__(cls)
        prob._setup(A, b, dtype, None, loss, sample_weight, feature_groups=(groups, group_weight, l1_ratio))
        return prob

    def _setup(self, A, b, dtype, pad, loss, sample_weight, penalty_factor=None, lower=None, upper=None, classes=None,
               feature_groups=None, threshold=None):
        """__init__, and with penalty_factor / lower / upper (`prepare_penalized`; `set_penalty`, fos_coord_bind) the handle of a
        problem with per-coordinate penalty factors and box bounds: it runs on the matrix-core pair alone too and is padded by
        the rules of a logistic problem."""
        if loss not in LOSSES and loss not in LINK_LOSSES:
            raise ValueError(f"loss: one of {sorted(LOSSES)} expected, got {loss!r}")
        self.threshold = None
        if loss in LINK_LOSSES:                                          # before any device work
            if isinstance(b, Problem) or isinstance(A, Problem):
                raise ValueError("a Huber or squared-hinge problem binds an array or tensor")
            if b is None:
                raise ValueError("a Huber or squared-hinge problem needs b")
            if loss == "huber":
                if threshold is None:
                    raise ValueError("a Huber problem takes its threshold: prepare_huber(A, b, threshold)")
                self.threshold = checked_threshold(threshold)
            else:
                if threshold is not None:
                    raise ValueError("threshold belongs to the Huber loss")
                b = checked_signs(b)
        elif threshold is not None:
            raise ValueError("threshold belongs to the Huber loss")
        coord = any(v is not None for v in (penalty_factor, lower, upper))
        pair_only = loss != "squared" or sample_weight is not None or coord or feature_groups is not None   # served by the matrix-core pair alone
        self.classes = None
        if loss == "multinomial":                                        # before any device work
            if isinstance(b, Problem) or isinstance(A, Problem):
                raise ValueError("a multinomial problem binds an array or tensor")
            b, self.classes = checked_labels(b, classes)
        elif classes is not None:
            raise ValueError('classes belongs to loss="multinomial"')
        if coord:                                                        # before any device work
            coord = checked_coord(penalty_factor, lower, upper, int(A.shape[1] if hasattr(A, "shape") else np.shape(A)[1]))
        if feature_groups is not None:                                   # before any device work
            if coord or loss == "multinomial":
                raise ValueError("feature groups compose with neither penalty factors / bounds nor the multinomial loss")
            feature_groups = checked_feature_groups(*feature_groups, int(A.shape[1] if hasattr(A, "shape") else np.shape(A)[1]))
        if sample_weight is not None:                                    # before any device work
            sample_weight = checked_weights(sample_weight, int(A.shape[0] if hasattr(A, "shape") else np.shape(A)[0]))
        require_gpu()
        lib = _lib.load()
        self.like = Like(A)
        want_bf16 = stores_bf16(A, dtype)
        tdtype = torch.bfloat16 if want_bf16 else torch.float32
        gran = 8 if want_bf16 else 4
        dev = A.device if is_tensor(A) and A.is_cuda else torch.device("cuda", torch.cuda.current_device())
        if is_tensor(A):
            At = A.detach()
        else:
            At = torch.from_numpy(np.asarray(A))
        if At.dim() != 2:
            raise ValueError("A must be 2-D")
        m, n = int(At.shape[0]), int(At.shape[1])
        borrowable = At.is_cuda and At.dtype == tdtype and At.stride(1) == 1 and At.stride(0) >= n
        esz = 2 if want_bf16 else 4
        fused_ok = borrowable and n % gran == 0 and (At.stride(0) % gran == 0 or m == 1) and At.data_ptr() % 16 == 0
        if pad is None:
            # n <= 64 runs the row-per-thread kernel, which takes ragged / misaligned rows as they are
            pad = pair_only or ((not fused_ok) and m * n >= (1 << 20) and n > 64)
        n_dev = n
        n_min = LOGIT_MIN_N["bf16" if want_bf16 else "f32"] if pair_only and n <= 64 else 0
        if pad and (not fused_ok or n < n_min):
            n_dev = max((n + gran - 1) // gran * gran, n_min)
            Ap = torch.zeros(m, n_dev, dtype=tdtype, device=dev)
            if At.is_cuda:
                Ap[:, :n].copy_(At)                  # one strided device copy
            else:
                upload_matrix(At, Ap[:, :n])
            At = Ap
        elif not borrowable:
            if At.is_cuda:
                At = At.to(device=dev, dtype=tdtype).contiguous()
            else:
                At = upload_matrix(At, torch.empty(m, n, dtype=tdtype, device=dev))
        self.A = At
        self.m, self.n, self.n_dev = m, n, n_dev
        self.lda = int(At.stride(0)) if self.m > 1 else self.n_dev
        self.device = At.device
        self.dtype = "bf16" if want_bf16 else "f32"
        self.loss = loss
        if pair_only and n_dev > LOGIT_MAX_N:
            raise ValueError(f"a logistic, multinomial or weighted problem, or one with penalty factors or bounds, is limited to {LOGIT_MAX_N} device columns, "
                             f"got {n_dev}")
        self.sample_weight = None
        self._coord = (None, None, None)
        self.penalty_max = 1.0
        self.grouped = False
        self._fgroups = None
        self._bind(b, lib)
        if coord:
            self._set_checked(*coord)
        if feature_groups is not None:
            self._bind_feature_groups(*feature_groups)
        if sample_weight is not None:
            # zero-padded to a multiple of 4 entries: product 1 fetches the weights of 4 rows with one 16-byte load
            buf = torch.zeros((m + 3) // 4 * 4, dtype=torch.float32, device=self.device)
            buf[:m] = sample_weight.to(device=self.device, dtype=torch.float32)
            self.set_sample_weight(buf[:m])

    def sibling(self, b):
        """Another handle on the SAME device A (borrowed as it is: no upload, no padding) with its own b - the column-by-column
        runs of a multi-target solve."""
        sib = Problem.__new__(Problem)
        sib.like = self.like
        sib.A, sib.m, sib.n, sib.n_dev, sib.lda = self.A, self.m, self.n, self.n_dev, self.lda
        sib.device, sib.dtype, sib.loss, sib.sample_weight = self.device, self.dtype, self.loss, None
        sib.classes = self.classes
        sib.threshold = self.threshold
        if self.loss == "squared_hinge":            # the sibling's own labels, checked on the host
            b = checked_signs(b)
        sib.grouped = self.grouped
        if self.loss == "multinomial":              # the sibling's own labels, checked against the same C on the host
            b = checked_labels(b, self.classes)[0]
        sib._coord, sib.penalty_max = (None, None, None), 1.0
        sib._fgroups = None
        sib._bind(b, self.lib)
        if self._fgroups is not None:               # the columns are the same columns: the library copies the table again
            sib._bind_feature_groups(*self._fgroups)
        if self.has_coord:                          # the columns are the same columns: the device vectors are shared
            sib._bind_coord(self._coord, self.penalty_max)
        if self.sample_weight is not None:          # the rows are the same rows: a sibling of a weighted handle is weighted
            sib.set_sample_weight(self.sample_weight)
        return sib

    def _bind(self, b, lib):
        """Create the fos_problem handle on self.A and b."""
        want_bf16 = self.dtype == "bf16"
        self.b = None if b is None else to_device_vec(b, self.device)
        if self.b is not None and self.b.numel() != self.m:
            raise ValueError("b must have m entries")
        if self.loss == "logistic":
            if self.b is None:
                raise ValueError("a logistic problem needs its labels")
            if not bool((torch.isfinite(self.b) & (self.b >= 0) & (self.b <= 1)).all()):     # once, on the device
                raise ValueError("logistic labels must be finite and lie in [0, 1]")
        self.gbuf = torch.zeros(self.n_dev + 4, dtype=torch.float32, device=self.device)
        self.scratch = torch.zeros(32, dtype=torch.float64, device=self.device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.fos_problem_create(C.byref(h), ptr(self.A), self.m, self.n_dev, self.lda,
                                              _lib.FOS_BF16 if want_bf16 else _lib.FOS_F32, ptr(self.b), stream_ptr()),
                       "fos_problem_create")
            self.h = h
            self._stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(lib.fos_problem_set_gbuf(self.h, ptr(self.gbuf)), "fos_problem_set_gbuf")
            if self.loss == "multinomial":
                _lib.check(lib.fos_problem_set_multinomial(int(self.classes), self.h), "fos_problem_set_multinomial")
            elif self.loss in LINK_LOSSES:
                _lib.check(lib.fos_problem_set_link_loss(LINK_LOSSES[self.loss], float(self.threshold or 0.0), self.h),
                           "fos_problem_set_link_loss")
            elif self.loss != "squared":
                _lib.check(lib.fos_problem_set_loss(self.h, LOSSES[self.loss]), "fos_problem_set_loss")
        self.lib = lib

    def set_sample_weight(self, w):
        """Bind the fp32 device vector `w` (m checked weights, 16-byte aligned, readable up to m rounded up to 4) or, with None,
        detach the weights (fos_row_weights_bind): the handle is an unweighted one again."""
        with self.ctx():
            _lib.check(self.lib.fos_row_weights_bind(ptr(w), self.h), "fos_row_weights_bind")
        self.sample_weight = w

    def set_grouped(self, on=True):
        """The penalty of a multinomial handle becomes (on) or stops being the group penalty over the classes, alpha1 sum_j p_j
        ||X[j, :]||_2 + 0.5 alpha2 sum_j p_j ||X[j, :]||_2^2 (`.grouped`; `multinomial_path` / `multinomial_cv` /
        `multinomial_objective` read it and set fos_fista_params.group = C on every class handle).  Host state only.  ValueError on
        a handle of another loss and on one with box bounds, with which the group penalty has no composed closed-form prox."""
        if on and self.loss != "multinomial":
            raise ValueError(f"the grouped penalty belongs to a multinomial handle; this one has the {self.loss} loss")
        if on and (self.lower is not None or self.upper is not None):
            raise ValueError(GROUPED_BOUNDS)
        self.grouped = bool(on)

    def set_penalty(self, penalty_factor=None, lower=None, upper=None):
        """Per-coordinate penalty factors p_j >= 0 and box bounds lower_j <= 0 <= upper_j (fos_coord_bind): the penalties become
        alpha1 sum_j p_j |x_j| + 0.5 alpha2 sum_j p_j x_j^2 and the solution is held to lower_j <= x_j <= upper_j.  Each is None
        (factor 1, -inf, +inf), a scalar (``lower=0.0``: the non-negative lasso) or n values; factors are used as given, p_j = 0
        is an unpenalised coordinate (an intercept column).  All None detaches.  Checked on the host before any device work
        (ValueError: a wrong length, a non-finite or negative factor, NaN, lower > 0 or upper < 0).  The handle then runs on the
        matrix-core lockstep alone (``fista_path`` / ``fista_cv`` / ``logistic_path`` / ``logistic_cv``) with the step
        t_init_factor / (L + alpha2 * penalty_max); every other solver refuses it."""
        self._set_checked(*checked_coord(penalty_factor, lower, upper, self.n))

    def _set_checked(self, pf, lo, hi):
        """set_penalty with what checked_coord returned."""
        n4 = (self.n_dev + 3) // 4 * 4              # the update fetches the values of 4 coordinates with one 16-byte load

        def dev(v, fill):
            if v is None:
                return None
            buf = torch.full((n4,), fill, dtype=torch.float32, device=self.device)
            buf[: self.n] = torch.from_numpy(v).to(device=self.device, dtype=torch.float32)
            return buf
        self._bind_coord((dev(pf, 1.0), dev(lo, -math.inf), dev(hi, math.inf)), 1.0 if pf is None else float(pf.max()))

    def _bind_coord(self, bufs, penalty_max):
        with self.ctx():
            _lib.check(self.lib.fos_coord_bind(ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), self.h), "fos_coord_bind")
        self._coord = tuple(bufs)                   # the device vectors live as long as the handle borrows them
        self.penalty_max = float(penalty_max) if bufs[0] is not None else 1.0

    def set_feature_groups(self, groups, group_weight=None, l1_ratio=0.0):
        """Feature groups of the fit (fos_feature_groups_bind): the penalty becomes alpha1 [(1 - l1_ratio) sum_g w_g ||x_g||_2 +
        l1_ratio ||x||_1] + 0.5 alpha2 ||x||_2^2 - the group lasso (l1_ratio = 0), the sparse-group lasso, the plain lasso
        (l1_ratio = 1).  groups: n labels whose equal labels are contiguous (a label that reappears after a gap is a ValueError:
        permute the columns), or positive sizes summing to n; None detaches.  group_weight: one w_g >= 0 per group (a scalar
        broadcasts), None for sqrt(size); w_g = 0 keeps a group - an intercept column - out of the group term.  Checked on the
        host before any device work.  The handle then runs on the matrix-core lockstep alone (``fista_path`` / ``fista_cv`` /
        ``logistic_path`` / ``logistic_cv``) with the step of the separable penalty; every other solver refuses it, and so does
        the library where the handle carries penalty factors or bounds, is multinomial, sharded or of a shape without the
        matrix-core pair (FosError)."""
        if groups is None:
            with self.ctx():
                _lib.check(self.lib.fos_feature_groups_bind(None, None, 0, 0.0, self.h), "fos_feature_groups_bind")
            self._fgroups = None
            return
        self._bind_feature_groups(*checked_feature_groups(groups, group_weight, l1_ratio, self.n))

    def _bind_feature_groups(self, start, weight, l1_ratio):
        """set_feature_groups with what checked_feature_groups returned.  The zero columns the device copy of A is padded with
        form one more group of weight 0: they stay exactly zero."""
        s, w = start, weight
        if self.n_dev > self.n:
            s, w = np.concatenate((start, [self.n_dev])).astype(np.int32), np.concatenate((weight, [0.0]))
        s = np.ascontiguousarray(s, dtype=np.int32)
        w32 = np.ascontiguousarray(w, dtype=np.float32)
        with self.ctx():
            _lib.check(self.lib.fos_feature_groups_bind(s.ctypes.data_as(C.POINTER(C.c_int32)), w32.ctypes.data_as(C.POINTER(C.c_float)),
                                                        len(s) - 1, float(l1_ratio), self.h), "fos_feature_groups_bind")
        self._fgroups = (np.array(start, dtype=np.int32), np.array(weight, dtype=np.float64), float(l1_ratio))

    @property
    def has_feature_groups(self):
        return getattr(self, "_fgroups", None) is not None

    @property
    def feature_groups(self):
        """The bound feature groups as FeatureGroups(start, weight, l1_ratio) - ngroups + 1 boundaries, the weights as given (fp64;
        the device holds them in fp32) - or None."""
        if not self.has_feature_groups:
            return None
        start, weight, ratio = self._fgroups
        return FeatureGroups(start.copy(), weight.copy(), ratio)

    @property
    def has_coord(self):
        return any(v is not None for v in self._coord)

    def _coord_view(self, i):
        return None if self._coord[i] is None else self._coord[i][: self.n]

    penalty_factor = property(lambda self: self._coord_view(0), doc="the bound fp32 device factors (n), or None")
    lower = property(lambda self: self._coord_view(1), doc="the bound fp32 device lower bounds (n), or None")
    upper = property(lambda self: self._coord_view(2), doc="the bound fp32 device upper bounds (n), or None")

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                self.lib.fos_problem_destroy(h)
            except Exception:
                pass
            self.h = None

    def ctx(self):
        """Device guard for a call into the library; the handle follows torch's CURRENT stream (fos_problem_set_stream
        orders the new stream behind work still enqueued on the old one), so temporaries allocated by the caching
        allocator and the kernels that read them always share a stream."""
        cur = torch.cuda.current_stream(self.device).cuda_stream
        if cur != self._stream:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.fos_problem_set_stream(self.h, C.c_void_p(cur)), "fos_problem_set_stream")
            self._stream = cur
        return torch.cuda.device(self.device)

    # ---- user-length <-> device-length vectors ------------------------------------------------------------
    def vec_in(self, x, dtype=torch.float32):
        """1-D device tensor of the kernel's length n_dev (zero beyond n) from a user vector of length n or n_dev."""
        t = to_device(x, self.device, dtype)
        if t.numel() == self.n_dev:
            return t
        if t.numel() != self.n:
            raise ValueError(f"expected a vector of length {self.n}")
        out = torch.zeros(self.n_dev, dtype=dtype, device=self.device)
        out[: self.n] = t
        return out

    def vec_out(self, t):
        """Trim a device-length vector (or [k, n_dev] history block) to the user's n."""
        return t if self.n_dev == self.n else t[..., : self.n]

    # ---- plan / tuning -------------------------------------------------------------------------------
    def plan(self):
        arr = (C.c_int32 * 8)()
        _lib.check(self.lib.fos_problem_plan(self.h, arr), "fos_problem_plan")
        keys = ("path", "threads", "chunks", "rows", "workgroups", "slabs", "nontemporal", "cus")
        plan = dict(zip(keys, list(arr)))
        flags = plan["nontemporal"]
        plan["nontemporal"] = flags & 1
        plan["resident"] = (flags >> 1) & 1       # small problem: whole runs execute in one LDS-resident launch
        plan["tall"] = (flags >> 2) & 1           # n <= 64: row-per-thread single pass (any alignment)
        plan["colblock"] = (flags >> 3) & 1       # rows wider than any single-pass kernel: column blocks, two phases
        plan["cluster"] = (flags >> 4) & 1        # multi-lambda pass: one-read cluster form planned (after its first run)
        plan["interleave"] = (flags >> 5) & 1     # streaming pass: rows dealt round-robin to the workgroups
        plan["fused_mfma"] = (flags >> 6) & 1     # opt-in: plain runs take the one-launch persistent step
        plan["chip_resident"] = (flags >> 7) & 1  # tall-skinny plain runs keep A in the LDS of up to all CUs: forced on
        plan["packed"] = (flags >> 8) & 1         # the gradient pass streams the 28-bit copy of A (after the first run packed it)
        plan["pack_rows"] = (flags >> 9) & 7      # rows per burst of that pass on this plan: replan(pack_rows=) or the planner's (0: not served)
        return plan

    def replan(self, no_resident=False, no_tall=False, no_wide=False, no_colblock=False, cluster=None, interleave=None,
               fused_mfma=False, chip_resident=None, pack=None, pack_rows=None):
        """Re-run the planner with kernel families switched off; ``cluster`` / ``interleave``: True / False force the
        one-read cluster form of the multi-weight pass / the round-robin row order on or off, None leaves the planner's
        choice; ``fused_mfma=True`` opts plain runs in to the one-launch persistent step (fos_fista_run_fused),
        ``chip_resident=True`` / ``False`` takes the chip-resident loop for tall-skinny plain runs (fos_fista_run_chip)
        wherever it is served / never, None leaves the planner's region (n <= 8, up to 131072 rows);
        ``pack=True`` / ``False`` streams the gradient pass of FISTA runs from a lossless 28-bit copy of an fp32 A at any
        size it is served for / never, None leaves the planner's size threshold (the copy costs 87.5 % of A in device
        memory and assumes A does not change while bound; any replan drops it and the next run packs again);
        ``pack_rows=1 .. 4`` (1 .. 3 above 8192 columns) makes that pass drain its loads every so many rows instead of the
        planner's number for the geometry (same bits, another speed) until the next replan / tune
        (fos_problem_replan): tests and A/B measurements.
        Call before creating Fista handles on this problem."""
        flags = ((_lib.PLAN_NO_RESIDENT if no_resident else 0) | (_lib.PLAN_NO_TALL if no_tall else 0) |
                 (_lib.PLAN_NO_WIDE if no_wide else 0) | (_lib.PLAN_NO_COLBLOCK if no_colblock else 0) |
                 (0 if cluster is None else (_lib.PLAN_CLUSTER if cluster else _lib.PLAN_NO_CLUSTER)) |
                 (0 if interleave is None else (_lib.PLAN_INTERLEAVE if interleave else _lib.PLAN_NO_INTERLEAVE)) |
                 (_lib.PLAN_FUSED_MFMA if fused_mfma else 0) |
                 (0 if chip_resident is None else (_lib.PLAN_CHIP_RESIDENT if chip_resident else _lib.PLAN_NO_CHIP_RESIDENT)) |
                 (0 if pack is None else (_lib.PLAN_PACK if pack else _lib.PLAN_NO_PACK)))
        if pack_rows is not None:
            if int(pack_rows) not in (1, 2, 3, 4):
                raise ValueError("pack_rows: 1 .. 4 rows per burst")
            flags |= int(pack_rows) * _lib.PLAN_PACK_ROWS
        with self.ctx():
            _lib.check(self.lib.fos_problem_replan(self.h, flags), "fos_problem_replan")

    def set_comm(self, comm):
        """Attach a `distributed.Comm` (or None): this problem's rows are one shard of a row-sharded problem and every
        row-sum is all-reduced on the stream (fos_problem_set_comm)."""
        _lib.check(self.lib.fos_problem_set_comm(self.h, comm.h if comm is not None else None), "fos_problem_set_comm")
        self.comm = comm               # keeps the communicator alive as long as the problem

    def set_comm_cols(self, comm):
        """COLUMN sharding: this problem holds A[:, this rank's columns] (all rows) and the whole b; the iterate is
        partitioned over the ranks (fos_problem_set_comm_cols)."""
        with self.ctx():
            _lib.check(self.lib.fos_problem_set_comm_cols(self.h, comm.h), "fos_problem_set_comm_cols")
        self.comm = comm
        self.col_sharded = True

    def tune(self, threads, chunks, rows, workgroups=0):
        _lib.check(self.lib.fos_problem_tune(self.h, threads, chunks, rows, workgroups), "fos_problem_tune")

    def profile(self, every=1):
        """Bracket every `every`-th A-pass launch with HIP events (0 / False = off)."""
        _lib.check(self.lib.fos_problem_profile(self.h, int(every)), "fos_problem_profile")

    def profile_read(self):
        """(device milliseconds, launches) of the A-pass kernel since the last read; synchronises."""
        ms, cnt = C.c_double(), C.c_int64()
        with self.ctx():
            _lib.check(self.lib.fos_problem_profile_read(self.h, C.byref(ms), C.byref(cnt)), "fos_problem_profile_read")
        return ms.value, cnt.value

    # ---- kernels -------------------------------------------------------------------------------------
    def gemv_pair(self, y, alpha2=0.0, out=None, rr_out=None):
        """grad = A^T (A y - b) + alpha2 y (device tensor); rr_out: optional 1-element float64 device tensor."""
        user_out = out
        if out is None or out.numel() != self.n_dev:
            out = torch.empty(self.n_dev, dtype=torch.float32, device=self.device)
        y = self.vec_in(y)
        with self.ctx():
            _lib.check(self.lib.fos_gemv_pair(self.h, ptr(y), float(alpha2), ptr(out), ptr(rr_out)), "fos_gemv_pair")
        if user_out is not None and user_out is not out:
            user_out.copy_(self.vec_out(out))
            return user_out
        return self.vec_out(out)

    def residual_objective(self, x):
        """Host tuple (||Ax-b||^2, ||x||^2, ||x||_1); synchronises.  x is rounded to fp32 for the pass over A."""
        x = self.vec_in(x)
        with self.ctx():
            _lib.check(self.lib.fos_residual_objective(self.h, ptr(x), ptr(self.scratch)), "fos_residual_objective")
        v = self.scratch[:3].cpu()
        return float(v[0]), float(v[1]), float(v[2])

    def _block16(self, X):
        """(X (n x nv, nv <= 16) zero-padded to the n_dev x 16 fp32 device block the MFMA passes read, nv)."""
        X = torch.as_tensor(X, device=self.device, dtype=torch.float32)
        nv = X.shape[1]
        Xf = torch.zeros(self.n_dev, 16, dtype=torch.float32, device=self.device)
        Xf[: X.shape[0], :nv] = X
        return Xf, nv

    def residual_batch(self, X, use_b=True):
        """||A X_j - b||^2 for the <= 16 columns of X (n x nv) in one MFMA pass; host list.  Synchronises.  On a multinomial
        handle (use_b) the columns are whole class groups and entry s * C is the loss sum of group s, the others 0."""
        if self.classes and use_b:
            checked_class_groups(int(X.shape[1]), self.classes)
        Xf, nv = self._block16(X)
        with self.ctx():
            _lib.check(self.lib.fos_residual_batch(self.h, ptr(Xf), nv, int(bool(use_b)), ptr(self.scratch)),
                       "fos_residual_batch")
        return self.scratch[:nv].cpu().tolist()

    def residual_batch_rhs(self, X, B):
        """||A X_j - B_j||^2 for the nv <= 16 columns of X (n x nv) against the columns of B (m x nv fp32 device tensor with
        unit column stride, any row stride) in one MFMA pass; host list, or None where the shape has no such pass.
        Synchronises."""
        Xf, nv = self._block16(X)
        with self.ctx():
            rc = self.lib.fos_residual_batch_rhs(self.h, ptr(Xf), nv, ptr(B), int(B.stride(0)), ptr(self.scratch))
        if not _lib.served(rc, "fos_residual_batch_rhs"):
            return None
        return self.scratch[:nv].cpu().tolist()

    def residual_batch_folds(self, X, fold_ids, held):
        """Held-out squared errors: sum over the rows i with fold_ids[i] == held[j] of (A_i . X_j - b_i)^2 for the nv <= 16
        columns of X (n x nv) in one MFMA pass (fos_residual_batch_folds); fold_ids: `fold_ids_tensor`, held: nv ints
        (-1: no row).  Host list, or None where the shape has no such pass.  Synchronises."""
        Xf, nv = self._block16(X)
        with self.ctx():
            rc = self.lib.fos_residual_batch_folds(self.h, ptr(Xf), nv, ptr(fold_ids), (C.c_int32 * nv)(*held), ptr(self.scratch))
        if not _lib.served(rc, "fos_residual_batch_folds"):
            return None
        return self.scratch[:nv].cpu().tolist()

    def gram_apply(self, X):
        """A^T W A X_j for the nv <= 16 columns of X (n x nv), W the bound weights or the identity (fos_gram_apply): an n x nv
        float32 device tensor.  Enqueues only."""
        Xf, nv = self._block16(X)
        G = torch.empty(nv, self.n_dev, dtype=torch.float32, device=self.device)
        with self.ctx():
            _lib.check(self.lib.fos_gram_apply(ptr(Xf), nv, self.h, ptr(G)), "fos_gram_apply")
        return self.vec_out(G).t()

    # ---- working-set solve (include/fos_working_set.h; working_set.py drives these) ----------------------------------
    def gradient_block(self, X, want_loss=False):
        """The gradient of the data term at the nv <= 16 columns of X (n x nv): A^T W (A X_j - b), or A^T W (sigma(A X_j) - b) on
        a logistic handle (fos_gradient_batch), as the nv x n_dev float32 device block fos_kkt_scan reads (row j: column j).
        want_loss: also the data-term sums of `residual_batch` from the same pass, as a host list (synchronises)."""
        return self._gradient_block("fos_gradient_batch", X, want_loss, 1)

    def _gradient_block(self, entry, X, want_loss, stride):
        """`gradient_block` / `multinomial_gradient_block`: the loss sums of the fits are every stride-th of the 16."""
        Xf, nv = self._block16(X)
        G = torch.empty(nv, self.n_dev, dtype=torch.float32, device=self.device)
        with self.ctx():
            _lib.check(getattr(self.lib, entry)(ptr(Xf), nv, self.h, ptr(G), ptr(self.scratch) if want_loss else None), entry)
        return (G, self.scratch[:nv:stride].cpu().tolist()) if want_loss else G

    def gradient_batch(self, X):
        """`gradient_block` in the layout of `gram_apply`: an n x nv float32 device tensor.  Enqueues only."""
        return self.vec_out(self.gradient_block(X)).t()

    def gather_columns(self, idx, n_ws_pad=None, out=None):
        """The device columns idx of A as an m x n_ws_pad tensor of A's element type, zero from column len(idx) on
        (fos_gather_columns).  idx: strictly increasing device column numbers in 0 .. n_dev - 1 (checked here: ValueError);
        n_ws_pad: a multiple of 8, default len(idx) rounded up to 8; out: a tensor to write into (row stride a multiple of 8
        elements, at least n_ws_pad)."""
        idx = torch.as_tensor(idx, device=self.device).to(torch.int64).reshape(-1)
        n_ws = int(idx.numel())
        if n_ws < 1 or n_ws > self.n_dev:
            raise ValueError(f"gather_columns: 1 .. {self.n_dev} columns expected, got {n_ws}")
        if int(idx[0]) < 0 or int(idx[-1]) >= self.n_dev or (n_ws > 1 and not bool((idx[1:] > idx[:-1]).all())):
            raise ValueError(f"gather_columns: idx must be strictly increasing within 0 .. {self.n_dev - 1}")
        n_ws_pad = (n_ws + 7) // 8 * 8 if n_ws_pad is None else int(n_ws_pad)
        if out is None:
            out = torch.empty(self.m, n_ws_pad, dtype=self.A.dtype, device=self.device)
        idx32 = idx.to(torch.int32)
        lda_ws = int(out.stride(0)) if self.m > 1 else n_ws_pad
        with self.ctx():
            _lib.check(self.lib.fos_gather_columns(ptr(idx32), n_ws, ptr(out), lda_ws, n_ws_pad, self.h), "fos_gather_columns")
        return out

    def kkt_scan(self, G, alpha1, slack, in_ws):
        """The optimality check of the coordinates outside a working set (fos_kkt_scan) on the nv x n_dev block G of
        `gradient_block`: (excess - n_dev floats on the device -, the violators in increasing order as an int32 device tensor).
        alpha1: nv host weights; in_ws: n_dev device bytes, non-zero inside the set.  Synchronises (the count is read)."""
        nv = int(G.shape[0])
        return self._scan("fos_kkt_scan", G, (nv,), (C.c_double * nv)(*[float(a) for a in alpha1]), slack, in_ws)

    def _scan(self, entry, G, head, a1, slack, in_ws):
        """`kkt_scan` / `multinomial_kkt_scan`; head: the arguments between G and the weights."""
        excess = torch.empty(self.n_dev, dtype=torch.float32, device=self.device)
        viol = torch.empty(self.n_dev, dtype=torch.int32, device=self.device)
        count = torch.zeros(1, dtype=torch.int32, device=self.device)
        with self.ctx():
            _lib.check(getattr(self.lib, entry)(ptr(G), *head, a1, float(slack), ptr(in_ws), self.h, ptr(excess), ptr(viol), ptr(count)), entry)
        return excess, viol[: int(count.item())]

    # ---- duality-gap certificate (include/fos_duality.h; duality.py drives this) ---------------------------------------
    def duality_gap_block(self, X, alpha1, alpha2):
        """The duality-gap certificate of the nv <= 16 columns of X (n x nv) under the host weights alpha1, alpha2 (nv each;
        fos_duality_gap): (out64 - 64 device doubles: primal[16], dual[16], gap[16], scale[16] -, G - the nv x n_dev float32
        gradient block of `gradient_block` at X, from the same pass).  Enqueues only."""
        Xf, nv = self._block16(X)
        return self._gap_block("fos_duality_gap", Xf, (nv,), (C.c_double * nv)(*[float(a) for a in alpha1]),
                               (C.c_double * nv)(*[float(a) for a in alpha2]))

    def _gap_block(self, entry, Xf, head, a1, a2):
        """`duality_gap_block` / `multinomial_duality_gap_block`; head: the arguments between X and the weights, nv first."""
        G = torch.empty(head[0], self.n_dev, dtype=torch.float32, device=self.device)
        out64 = torch.empty(64, dtype=torch.float64, device=self.device)
        with self.ctx():
            _lib.check(getattr(self.lib, entry)(ptr(Xf), *head, a1, a2, self.h, ptr(G), ptr(out64)), entry)
        return out64, G

    # ---- working set and duality gap of the multinomial lockstep (include/fos_multinomial_ws.h; multinomial_ws.py drives these)
    def multinomial_gradient_block(self, X, want_loss=False):
        """The class gradients at the columns of X (n x nv, nv a multiple of C: column s * C + c is class c of fit s) on a
        multinomial handle: A^T (w (softmax(A X_s)_c - [y = c])) as the nv x n_dev float32 device block `multinomial_kkt_scan`
        reads (fos_multinomial_gradient_batch).  want_loss: also the cross-entropy sums of `residual_batch` from the same pass,
        one per fit, as a host list (synchronises)."""
        return self._gradient_block("fos_multinomial_gradient_batch", X, want_loss, self.classes)

    def multinomial_kkt_scan(self, G, alpha1, slack, in_ws, grouped=None):
        """The optimality check of the coordinates (rows of X) outside a working set on the nv x n_dev block G of
        `multinomial_gradient_block` (fos_multinomial_kkt_scan): (excess - n_dev floats on the device -, the violators in
        increasing order as an int32 device tensor).  alpha1: one host weight per fit (nv / C); grouped: the group penalty over
        the classes (None: as `.grouped` says).  Synchronises (the count is read)."""
        nv = int(G.shape[0])
        a1 = (C.c_double * len(alpha1))(*[float(a) for a in alpha1])
        if self.classes and len(alpha1) * self.classes != nv:
            raise ValueError(f"alpha1: one weight per fit expected ({nv} columns, {self.classes} classes), got {len(alpha1)}")
        grouped = self.grouped if grouped is None else grouped
        return self._scan("fos_multinomial_kkt_scan", G, (nv, int(bool(grouped))), a1, slack, in_ws)

    def multinomial_duality_gap_block(self, X, alpha1, alpha2, grouped=None):
        """The duality-gap certificate of the fits in the columns of X (n x nv, nv a multiple of C) under the host weights alpha1,
        alpha2 (one per fit; fos_multinomial_duality_gap): (out64 - 64 device doubles: primal[16], dual[16], gap[16], scale[16],
        the values of fit s at entry s * C -, G - the block of `multinomial_gradient_block` at X, from the same pass).  grouped:
        None takes `.grouped`.  Enqueues only."""
        Xf, nv = self._block16(X)
        if self.classes and (len(alpha1) * self.classes != nv or len(alpha2) != len(alpha1)):
            raise ValueError(f"alpha1, alpha2: one weight per fit expected ({nv} columns, {self.classes} classes)")
        grouped = self.grouped if grouped is None else grouped
        return self._gap_block("fos_multinomial_duality_gap", Xf, (nv, int(bool(grouped))), (C.c_double * len(alpha1))(*[float(a) for a in alpha1]),
                               (C.c_double * len(alpha2))(*[float(a) for a in alpha2]))

    def power_iter(self, v0, n_iter=100, tol=1e-6):
        """The reference's power iteration (ref:45-60) from v0 (n values, need not be normalised): ``(L, it, v)``.  On every
        plan ``it`` is the step at which ``|L_k - L_{k-1}| < tol`` fired (``n_iter`` when it never did), ``L`` the norm of that
        step and ``v`` (n floats on the device) the normalised iterate after exactly ``it`` steps (fos_power_iter).
        Synchronises."""
        v = self.vec_in(v0).clone()
        L = C.c_double()
        it = C.c_int()
        with self.ctx():
            _lib.check(self.lib.fos_power_iter(self.h, ptr(v), int(n_iter), float(tol), C.byref(L), C.byref(it)),
                       "fos_power_iter")
        return L.value, it.value, self.vec_out(v)


def prepare(A, b=None, dtype=None, pad=None, *, loss="squared"):
    """Upload/bind A (and b) once; the result can be passed as ``A`` to every solver (``b`` may then be None).
    ``loss="logistic"``: b holds labels in [0, 1] and the handle is one for ``logistic_path`` / ``logistic_cv`` /
    ``logistic_objective`` (see ``Problem``); a handle that is passed in keeps the loss it was prepared with.
    ``loss="multinomial"``: b holds one integral class index 0 .. C-1 per row with C = max(b) + 1 (2 <= C <= 16; checked on the
    host before any device work) and the handle is one for ``multinomial_path`` / ``multinomial_cv`` / ``multinomial_objective``;
    ``prepare_multinomial`` takes C explicitly (a class that no row carries).  ``prepare_weighted`` and ``prepare_penalized``
    take the loss likewise."""
    if isinstance(A, Problem):
        if loss != "squared" and A.loss != loss:
            raise ValueError(f"this Problem was prepared for the {A.loss} loss")
        return A
    return Problem(A, b, dtype, pad, loss)


def prepare_weighted(A, b, sample_weight, dtype=None, *, loss="squared"):
    """``prepare`` with per-row sample weights w_i >= 0: the data term is sum_i w_i 0.5 (a_i.x - b_i)^2, or with
    ``loss="logistic"`` sum_i w_i (log(1 + e^{a_i.x}) - b_i a_i.x).  The weights belong to the handle (``.sample_weight``, the
    fp32 device vector): pass it as ``A`` (``b`` None) to ``fista_path`` / ``fista_cv`` (squared loss) or ``logistic_path`` /
    ``logistic_cv`` / ``logistic_objective``, which then run on the matrix-core lockstep alone; ``estimate_lipschitz(handle)``
    is lambda_max(A^T W A).  Padded as a logistic problem is; every solver that would answer with an unweighted quantity
    refuses the handle.  ValueError for weights that are not m finite values >= 0 or are all zero."""
    if isinstance(A, Problem):
        raise ValueError("prepare_weighted binds an array or tensor; this is already a Problem")
    if sample_weight is None:
        raise ValueError("sample_weight is needed")
    if b is None:
        raise ValueError("a weighted problem needs b")
    return Problem(A, b, dtype, None, loss, sample_weight=sample_weight)


def prepare_huber(A, b, threshold, dtype=None, *, sample_weight=None):
    """The handle of a Huber regression: data term sum_i w_i rho_c(a_i.x - b_i) with c = ``threshold`` > 0, rho_c(r) = r^2 / 2
    for |r| <= c and c |r| - c^2 / 2 otherwise, w the ``sample_weight`` (None: 1).  Pass it as ``A`` (``b`` None) to
    ``huber_path`` / ``huber_cv`` / ``huber_objective`` / ``working_set_path``; `.threshold` is c.  ``Problem.set_penalty`` and
    ``Problem.set_feature_groups`` compose.  Runs on the matrix-core lockstep alone and is padded by the rules of a logistic
    problem; every squared-loss entry point refuses the handle."""
    if isinstance(A, Problem):
        raise ValueError("prepare_huber binds an array or tensor")
    return Problem.link(A, b, "huber", threshold, dtype, sample_weight)


def prepare_hinge(A, y, dtype=None, *, sample_weight=None):
    """The handle of a squared-hinge classifier (the L2-loss linear SVM): data term sum_i w_i max(0, 1 - y_i a_i.x)^2 / 2 with
    labels ``y`` exactly -1 or +1 (checked on the host; ValueError before any device work), w the ``sample_weight`` (None: 1).
    Pass it as ``A`` (``y`` None) to ``hinge_path`` / ``hinge_cv`` / ``hinge_objective`` / ``working_set_path``.
    ``Problem.set_penalty`` and ``Problem.set_feature_groups`` compose.  Runs on the matrix-core lockstep alone and is padded by
    the rules of a logistic problem; every squared-loss entry point refuses the handle."""
    if isinstance(A, Problem):
        raise ValueError("prepare_hinge binds an array or tensor")
    return Problem.link(A, y, "squared_hinge", None, dtype, sample_weight)


def prepare_penalized(A, b, penalty_factor=None, lower=None, upper=None, dtype=None, *, loss="squared", sample_weight=None):
    """``prepare`` with per-coordinate penalty factors p_j >= 0 and box bounds lower_j <= 0 <= upper_j (glmnet's penalty.factor
    and lower.limits / upper.limits, sklearn's positive=True): the objective is

        data term + alpha1 sum_j p_j |x_j| + 0.5 alpha2 sum_j p_j x_j^2    subject to    lower_j <= x_j <= upper_j

    with the squared or (``loss="logistic"``) the logistic data term, weighted per row with ``sample_weight``.  Each of the
    three is None (factor 1, -inf, +inf), a scalar (``lower=0.0``: the non-negative lasso) or n values; the factor scales both
    penalties and is used as given (no rescaling), p_j = 0 is an unpenalised coordinate - an intercept is a constant column
    with factor 0.  The data belongs to the handle (``.penalty_factor`` / ``.lower`` / ``.upper``, fp32 device vectors;
    ``.penalty_max``; ``Problem.set_penalty`` rebinds or detaches): pass it as ``A`` (``b`` None) to ``fista_path`` /
    ``fista_cv`` (squared loss) or ``logistic_path`` / ``logistic_cv`` / ``logistic_objective``, which then run on the
    matrix-core lockstep alone with the step t_init_factor / (L + alpha2 max_j p_j); every other solver refuses the handle.
    Padded as a logistic problem is (at most 16384 device columns).  ValueError, before any device work, for a wrong length,
    a non-finite or negative factor, NaN, lower > 0 or upper < 0."""
    if isinstance(A, Problem):
        raise ValueError("prepare_penalized binds an array or tensor; on a Problem use its set_penalty")
    if b is None:
        raise ValueError("a problem with penalty factors or bounds needs b")
    if penalty_factor is None and lower is None and upper is None:
        raise ValueError("penalty_factor, lower or upper is needed")
    return Problem.penalized(A, b, penalty_factor, lower, upper, dtype, loss, sample_weight)


def prepare_grouped(A, b, groups, group_weight=None, l1_ratio=0.0, dtype=None, *, loss="squared", sample_weight=None):
    """``prepare`` with feature groups: the group lasso of Yuan & Lin over groups of coordinates of one fit (the dummy columns of a
    categorical variable, a spline basis, a gene set) and, with ``l1_ratio`` > 0, the sparse-group lasso of Simon et al.:

        data term + alpha1 [ (1 - l1_ratio) sum_g w_g ||x_g||_2 + l1_ratio ||x||_1 ] + 0.5 alpha2 ||x||_2^2

    with the squared or (``loss="logistic"``) the logistic data term, weighted per row with ``sample_weight``.  ``groups``: n
    labels whose equal labels are contiguous, or positive group sizes summing to n; ``group_weight``: one w_g >= 0 per group,
    None for sqrt(size), 0 for a group outside the group term (an intercept).  The groups belong to the handle
    (``.feature_groups``; ``Problem.set_feature_groups`` rebinds or detaches): pass it as ``A`` (``b`` None) to ``fista_path`` /
    ``fista_cv`` (squared loss) or ``logistic_path`` / ``logistic_cv``, which then run on the matrix-core lockstep alone with the
    step t_init_factor / (L + alpha2); every other solver refuses the handle.  Padded as a logistic problem is (at most 16384
    device columns).  ValueError, before any device work, for labels that are not contiguous, sizes that do not sum to n, a wrong
    number of weights, a weight that is not finite and >= 0 or an l1_ratio outside [0, 1]."""
    if isinstance(A, Problem):
        raise ValueError("prepare_grouped binds an array or tensor; on a Problem use its set_feature_groups")
    if b is None:
        raise ValueError("a problem with feature groups needs b")
    if groups is None:
        raise ValueError("groups is needed")
    return Problem.grouped_features(A, b, groups, group_weight, l1_ratio, dtype, loss, sample_weight)


def refuse_link(A, who):
    """A Huber or squared-hinge handle (`prepare_huber` / `prepare_hinge`) belongs to the functions of `robust` and to
    `working_set_path`: no other front end may answer for it with another loss's quantity.  ValueError before any device work."""
    if isinstance(A, Problem) and A.loss in LINK_LOSSES:
        own = "huber_path / huber_cv / huber_objective" if A.loss == "huber" else "hinge_path / hinge_cv / hinge_objective"
        raise ValueError(f"{who}: A was prepared for the {A.loss} loss: use {own} (or working_set_path)")


def as_problem(A, b, dtype=None):
    if isinstance(A, Problem):
        refuse_link(A, "a squared-loss solver")
        if b is not None and A.b is None:
            raise ValueError("Problem was prepared without b")
        return A
    return Problem(A, b, dtype)


class Fista:
    """fos_fista handle: x_k, x_{k-1} and the momentum scalars live on the device."""

    def __init__(self, prob):
        self.prob = prob
        self.lib = prob.lib
        h = C.c_void_p()
        with prob.ctx():
            _lib.check(self.lib.fos_fista_create(prob.h, C.byref(h)), "fos_fista_create")
        self.h = h
        self.prm = _lib.FistaParams()

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                self.lib.fos_fista_destroy(h)
            except Exception:
                pass
            self.h = None

    def reset(self, tau, alpha1, alpha2, mode=_lib.MODE_FISTA, prox_kind=_lib.PROX_L1, delta=0.0,
              adaptive_restart=False, restart_threshold=1.0, tol_step=0.0, tol_ratio=0.0, tol_grad=0.0, x0=None, group=0):
        """group: 0 (or 1) the separable penalty; G in 2..16 makes this handle one of G consecutive lockstep columns under the
        row-group penalty alpha1 p_j ||X[j,:]||_2 + 0.5 alpha2 p_j ||X[j,:]||_2^2 (fos_fista_params.group), served by
        `run_multi` / `run_multi_rhs` / `run_multi_folds` alone."""
        p = self.prm
        p.tau, p.alpha1, p.alpha2, p.delta = float(tau), float(alpha1), float(alpha2), float(delta)
        p.restart_threshold, p.tol_step, p.tol_ratio = float(restart_threshold), float(tol_step), float(tol_ratio)
        p.tol_grad = float(tol_grad)
        p.mode, p.prox_kind, p.adaptive_restart, p.group = int(mode), int(prox_kind), int(bool(adaptive_restart)), int(group)
        if x0 is not None:
            x0 = self.prob.vec_in(x0, torch.float64)
        with self.prob.ctx():
            _lib.check(self.lib.fos_fista_reset(self.h, C.byref(p), ptr(x0)), "fos_fista_reset")

    def set_precise(self, on=True, own_buffer=False):
        """Split-form gradient from the fp64-accumulating pass at the unrounded y_k (fos_fista_set_precise).
        own_buffer: keep [gradient ; ||r||^2] in a torch tensor of this object (`gbuf64`, n_dev + 4 doubles) so that a
        split-form reducer can sum it over the ranks between grad() and its consumers (fos_fista_set_gbuf64)."""
        with self.prob.ctx():
            if on and own_buffer and getattr(self, "gbuf64", None) is None:
                self.gbuf64 = torch.zeros(self.prob.n_dev + 4, dtype=torch.float64, device=self.prob.device)
                _lib.check(self.lib.fos_fista_set_gbuf64(self.h, ptr(self.gbuf64)), "fos_fista_set_gbuf64")
            _lib.check(self.lib.fos_fista_set_precise(self.h, int(bool(on))), "fos_fista_set_precise")
        self.precise = bool(on)

    def set_tau(self, tau):
        _lib.check(self.lib.fos_fista_set_tau(self.h, float(tau)), "fos_fista_set_tau")

    def run(self, iters):
        with self.prob.ctx():
            _lib.check(self.lib.fos_fista_run(self.h, int(iters)), "fos_fista_run")

    def run_fused(self, iters):
        """`iters` plain iterations in ONE persistent launch (fos_fista_run_fused: LDS-staged panels, row dots on the matrix
        cores, the owned slice of the iterate resident in LDS).  False when this problem / configuration is not served."""
        with self.prob.ctx():
            rc = self.lib.fos_fista_run_fused(self.h, int(iters))
        return _lib.served(rc, "fos_fista_run_fused")

    def run_chip(self, iters):
        """`iters` plain iterations in ONE launch with A resident in the LDS of up to all CUs and one grid-wide barrier per
        iteration (fos_fista_run_chip: tall-skinny fp32 problems, n <= 16).  False when not served."""
        with self.prob.ctx():
            rc = self.lib.fos_fista_run_chip(self.h, int(iters))
        return _lib.served(rc, "fos_fista_run_chip")

    def run_history(self, iters):
        """Device-resident history run: (x_hist [iters, n] float64, hist [iters, 4] float64 =
        {||Ax-b||^2, ||x||_1, ||x||_2^2, ||dx||^2}) as device tensors, or None when this solver configuration /
        problem shape needs the host-driven loop."""
        dev = self.prob.device
        xh = torch.empty(iters, self.prob.n_dev, dtype=torch.float64, device=dev)
        hist = torch.empty(iters, 4, dtype=torch.float64, device=dev)
        nbytes = self.lib.fos_fista_history_workspace(self.h, int(iters))
        work = torch.empty(max(1, (nbytes + 7) // 8), dtype=torch.float64, device=dev)
        with self.prob.ctx():
            rc = self.lib.fos_fista_run_history(self.h, int(iters), ptr(xh), ptr(hist), ptr(work))
        if not _lib.served(rc, "fos_fista_run_history"):
            return None
        self._keep = work            # stays alive until the stream has consumed it (next sync)
        return self.prob.vec_out(xh), hist

    def run_resident(self, iters, *, backtracking=False, eta=0.5, armijo_c=1e-2, grad_tol=0.0, record=False):
        """Small problems: the whole run - backtracking, restart, stops, history included - in one launch of the
        LDS-resident loop (fos_fista_run_resident).  Returns dict(done, tau, ls, taus[, x, hist]) with host lists for
        the per-iteration integers / steps and device tensors for the history, or None when the problem does not fit.
        Synchronises."""
        if not self.prob.plan().get("resident"):
            return None
        dev = self.prob.device
        iters = int(iters)
        xh = torch.empty(max(iters, 1), self.prob.n_dev, dtype=torch.float64, device=dev) if record else None
        hist = torch.empty(max(iters, 1), 4, dtype=torch.float64, device=dev) if record else None
        ls = torch.zeros(max(iters, 1), dtype=torch.int32, device=dev)
        taus = torch.zeros(max(iters, 1), dtype=torch.float64, device=dev)
        done, tau = C.c_int32(0), C.c_double(0.0)
        with self.prob.ctx():
            rc = self.lib.fos_fista_run_resident(self.h, iters, 1 if backtracking else 0, float(eta), float(armijo_c),
                                                 float(grad_tol), ptr(xh), ptr(hist), ptr(ls), ptr(taus),
                                                 C.byref(done), C.byref(tau))
        if not _lib.served(rc, "fos_fista_run_resident"):
            return None
        k = int(done.value)
        out = dict(done=k, tau=float(tau.value), ls=ls[:k].cpu().tolist(), taus=taus[:k].cpu().tolist())
        if record:
            out["x"] = self.prob.vec_out(xh[:k])
            out["hist"] = hist[:k]
        return out

    def run_backtracking(self, iters, eta, armijo_c, grad_eps):
        """Enqueue `iters` backtracking iterations decided on the device (fos_fista_run_backtracking).  Returns
        (ls_iters int32 tensor, tau_hist float64 tensor) - device tensors, valid for the completed iterations - or
        None when this plan has no candidate pass (callers then drive the search from the host)."""
        dev = self.prob.device
        ls = torch.zeros(max(int(iters), 1), dtype=torch.int32, device=dev)
        taus = torch.zeros(max(int(iters), 1), dtype=torch.float64, device=dev)
        with self.prob.ctx():
            rc = self.lib.fos_fista_run_backtracking(self.h, int(iters), float(eta), float(armijo_c), float(grad_eps),
                                                     ptr(ls), ptr(taus))
        if not _lib.served(rc, "fos_fista_run_backtracking"):
            return None
        return ls, taus

    def run_recorded(self, iters, backtracking, eta, armijo_c, grad_eps, want_rr=True):
        """Device-driven iterations with the history recorded on the device (fos_fista_run_recorded).  Returns dict of
        device tensors x [iters, n], hist [iters, 4], rr_seen [iters], ls [iters], taus [iters] - or None when
        unsupported for this plan."""
        dev, iters = self.prob.device, int(iters)
        rec = dict(x=torch.empty(max(iters, 1), self.prob.n_dev, dtype=torch.float64, device=dev),
                   hist=torch.zeros(max(iters, 1), 4, dtype=torch.float64, device=dev),
                   rr_seen=torch.full((max(iters, 1),), float("nan"), dtype=torch.float64, device=dev),
                   ls=torch.zeros(max(iters, 1), dtype=torch.int32, device=dev),
                   taus=torch.zeros(max(iters, 1), dtype=torch.float64, device=dev))
        with self.prob.ctx():
            rc = self.lib.fos_fista_run_recorded(self.h, iters, int(bool(backtracking)), float(eta), float(armijo_c),
                                                 float(grad_eps), ptr(rec["x"]), ptr(rec["hist"]),
                                                 ptr(rec["rr_seen"] if want_rr else None),
                                                 ptr(rec["ls"]), ptr(rec["taus"]))
        if not _lib.served(rc, "fos_fista_run_recorded"):
            return None
        return rec

    def resume_after_stall(self):
        """The device parked a search whose 16 candidates were all rejected: take the current step back to the host."""
        tau = C.c_double()
        with self.prob.ctx():
            _lib.check(self.lib.fos_fista_resume_after_stall(self.h, C.byref(tau)), "fos_fista_resume_after_stall")
        return float(tau.value)

    def grad(self, dual=False):
        """Gradient pass at y_k; dual=True also leaves ||A x_k - b||^2 in status().rr_x (same pass over A)."""
        with self.prob.ctx():
            if dual:
                _lib.check(self.lib.fos_fista_grad_dual(self.h), "fos_fista_grad_dual")
            else:
                _lib.check(self.lib.fos_fista_grad(self.h), "fos_fista_grad")

    def update(self):
        with self.prob.ctx():
            _lib.check(self.lib.fos_fista_update(self.h), "fos_fista_update")

    def trial(self, t, with_residual=True):
        out = (C.c_double * 8)()
        with self.prob.ctx():
            _lib.check(self.lib.fos_fista_trial(self.h, float(t), int(bool(with_residual)), out), "fos_fista_trial")
        keys = ("gd", "dd", "nnz", "gnorm2", "y2", "q", "rr_y")
        return dict(zip(keys, list(out)))

    def trial_batch(self, t, eta, nv=16):
        """Candidates t*eta^j, j < nv, decided by one MFMA pass over A; list of dicts like trial().  None when the
        problem runs the two-pass fallback."""
        out = (C.c_double * (8 * nv))()
        with self.prob.ctx():
            rc = self.lib.fos_fista_trial_batch(self.h, float(t), float(eta), int(nv), out)
        if not _lib.served(rc, "fos_fista_trial_batch"):
            return None
        keys = ("gd", "dd", "nnz", "gnorm2", "y2", "q", "rr_y")
        return [dict(zip(keys, out[8 * j: 8 * j + 7])) for j in range(nv)]

    def status(self):
        st = _lib.FistaStatus()
        with self.prob.ctx():
            _lib.check(self.lib.fos_fista_status_get(self.h, C.byref(st)), "fos_fista_status_get")
        return st

    def x_tensor(self):
        """Copy of x_k as a float64 device tensor."""
        out = torch.empty(self.prob.n_dev, dtype=torch.float64, device=self.prob.device)
        with self.prob.ctx():
            _lib.check(self.lib.fos_fista_get_x(self.h, ptr(out)), "fos_fista_get_x")
        return self.prob.vec_out(out)


def stream_read_probe(t, launches=20):
    """(GB/s, microseconds per pass) of a read-only pass over the contiguous CUDA tensor `t` (fos_stream_read_probe): the
    box's own streaming-read figure that bench.py reports beside the nominal peak.  Synchronises."""
    if not (t.is_cuda and t.is_contiguous()):
        raise ValueError("stream_read_probe: contiguous device tensor expected")
    nbytes = t.numel() * t.element_size() // 16 * 16
    gbps, us = C.c_double(), C.c_double()
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().fos_stream_read_probe(ptr(t), nbytes, int(launches), torch.cuda.current_stream().cuda_stream,
                                                    C.byref(gbps), C.byref(us)), "fos_stream_read_probe")
    return gbps.value, us.value


def _check_class_groups(handles):
    """On a multinomial problem the handles are whole class groups (ValueError before any device work)."""
    classes = getattr(handles[0].prob, "classes", None)
    if classes:
        checked_class_groups(len(handles), classes)


def run_multi(handles, iters):
    """Advance up to 16 Fista handles of one Problem in lockstep (fos_fista_run_multi).
    Returns False when this shape / configuration has no multi-vector kernel (callers then run them one by one)."""
    lib = handles[0].lib
    _check_class_groups(handles)
    arr = (C.c_void_p * len(handles))(*[h.h for h in handles])
    with handles[0].prob.ctx():
        rc = lib.fos_fista_run_multi(arr, len(handles), int(iters))
    return _lib.served(rc, "fos_fista_run_multi")


def run_multi_rhs(handles, B, iters):
    """Advance up to 16 Fista handles of one Problem in lockstep, handle v solving for column v of B (an m x nv fp32 device
    tensor with unit column stride, any row stride; the problem's own b is not used) (fos_fista_run_multi_rhs).
    Returns False when this shape / configuration has no multi-vector kernel (callers then run the columns one by one)."""
    lib = handles[0].lib
    arr = (C.c_void_p * len(handles))(*[h.h for h in handles])
    with handles[0].prob.ctx():
        rc = lib.fos_fista_run_multi_rhs(arr, len(handles), ptr(B), int(B.stride(0)), int(iters))
    return _lib.served(rc, "fos_fista_run_multi_rhs")


def fold_ids_tensor(ids, device):
    """The fold id of every row (0..254) as the uint8 device tensor the fold kernels read: padded with zeros to a multiple of
    4 entries (they fetch the ids of 4 rows with one 32-bit load; the allocation is aligned far beyond 4 bytes)."""
    ids = np.ascontiguousarray(np.asarray(ids), dtype=np.uint8)
    out = torch.zeros((ids.shape[0] + 3) // 4 * 4, dtype=torch.uint8, device=device)
    out[: ids.shape[0]] = torch.from_numpy(ids).to(device)
    return out


def run_multi_folds(handles, fold_ids, held, iters):
    """Advance up to 16 Fista handles of one Problem in lockstep, handle v fitting the rows whose fold id differs from held[v]
    (-1: all rows) (fos_fista_run_multi_folds); fold_ids: `fold_ids_tensor`.  Returns False when this shape / configuration
    is not served (callers then gather the rows fold by fold)."""
    lib = handles[0].lib
    nv = len(handles)
    _check_class_groups(handles)
    arr = (C.c_void_p * nv)(*[h.h for h in handles])
    with handles[0].prob.ctx():
        rc = lib.fos_fista_run_multi_folds(arr, nv, int(iters), ptr(fold_ids), (C.c_int32 * nv)(*held))
    return _lib.served(rc, "fos_fista_run_multi_folds")


# ---- batches of small problems (fos_fista_run_batch / fos_power_iter_batch) -------------------------------------------
RS_MAX_N, RS_MAX_M, RS_MAX_A = 64, 4096, 10240        # csrc/resident.hpp


def resident_fits(m, n):
    """The LDS-resident limits of csrc/resident.hpp (resident_fits): n <= 64, m <= 4096, m * (n | 1) <= 10240."""
    return 1 <= n <= RS_MAX_N and 1 <= m <= RS_MAX_M and m * (n | 1) <= RS_MAX_A


def batch_items(shapes):
    """ctypes array of fos_batch_item from (a_offset, lda, b_offset, m, n) tuples."""
    arr = (_lib.BatchItem * max(len(shapes), 1))()
    for i, (ao, lda, bo, m, n) in enumerate(shapes):
        arr[i].a_offset, arr[i].lda, arr[i].b_offset, arr[i].m, arr[i].n = int(ao), int(lda), int(bo), int(m), int(n)
    return arr


def power_iter_batch(A, dtype, shapes, V, n_iter=100, tol=1e-6):
    """fos_power_iter of every problem in one launch: A a device buffer of the problems' elements (dtype "f32" / "bf16"),
    shapes (a_offset, lda, b_offset, m, n) per problem, V (P x ldv float32 device) the start vectors (overwritten).
    Returns (L, iterations) as host lists.  Synchronises."""
    lib = _lib.load()
    P = len(shapes)
    if P == 0:
        return [], []
    dev = A.device
    L = torch.empty(P, dtype=torch.float64, device=dev)
    used = torch.empty(P, dtype=torch.int32, device=dev)
    work = torch.empty((P * C.sizeof(_lib.BatchItem) + 7) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fos_power_iter_batch(ptr(A), _lib.FOS_BF16 if dtype == "bf16" else _lib.FOS_F32, batch_items(shapes),
                                            P, ptr(V), int(V.stride(0)), int(n_iter), float(tol), ptr(L), ptr(used),
                                            ptr(work), stream_ptr()), "fos_power_iter_batch")
        return L.cpu().tolist(), used.cpu().tolist()


def run_batch(A, dtype, B, shapes, params, iters, *, backtracking=False, eta=0.5, armijo_c=1e-2, ldx, record=False):
    """fos_fista_run_batch: every problem from x = 0 for up to `iters` iterations, one workgroup each.  A / B: device
    buffers of the problems' elements / right-hand sides; shapes (a_offset, lda, b_offset, m, n) and params (FistaParams)
    per problem.  Returns dict of device tensors x [P, ldx], done [P], stopped [P], tau [P], ls [P, iters], taus [P, iters]
    (and with record: x_hist [P, iters, ldx], hist [P, iters, 4]).  Enqueues only."""
    lib = _lib.load()
    P, dev, it1 = len(shapes), A.device, max(int(iters), 1)
    out = dict(x=torch.zeros(P, ldx, dtype=torch.float64, device=dev),
               done=torch.zeros(P, dtype=torch.int32, device=dev), stopped=torch.zeros(P, dtype=torch.int32, device=dev),
               tau=torch.zeros(P, dtype=torch.float64, device=dev),
               ls=torch.zeros(P, it1, dtype=torch.int32, device=dev), taus=torch.zeros(P, it1, dtype=torch.float64, device=dev))
    if record:
        out["x_hist"] = torch.zeros(P, it1, ldx, dtype=torch.float64, device=dev)
        out["hist"] = torch.zeros(P, it1, 4, dtype=torch.float64, device=dev)
    if P == 0:
        return out
    prm = (_lib.FistaParams * P)(*params)
    work = torch.empty((lib.fos_fista_batch_workspace(P, int(ldx)) + 7) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fos_fista_run_batch(ptr(A), _lib.FOS_BF16 if dtype == "bf16" else _lib.FOS_F32, ptr(B),
                                           batch_items(shapes), prm, P, int(iters), int(bool(backtracking)), float(eta),
                                           float(armijo_c), int(ldx), ptr(out["x"]), ptr(out["done"]), ptr(out["stopped"]),
                                           ptr(out["tau"]), ptr(out["ls"]), ptr(out["taus"]), ptr(out.get("hist")),
                                           ptr(out.get("x_hist")), ptr(work), stream_ptr()), "fos_fista_run_batch")
    out["_work"] = work              # alive until the caller has synchronised
    return out
