"""GPU: the FISTA run forms on a packed plan (tests/_forms.py names the forms; tests/test_gpu_fista_forms.py supplies the
calls).  Only fos.fista - fos_fista_run - had run on one: grad + update, the device search and the host search reach
launch_pass_packed through the hook in launch_pass, with YSource in its momentum form and the stopped flag, and
pk_bprime_kernel forms y from x_cur, x_prev and beta itself.

The matrix is family S-f32 of tests/_forms.py made heavy-tailed (tests/_packed_probes.forms_data: 9e-4 exceptions, planted
entries of 16 .. 256), so that the exception lists matter: tests/test_packed_probes.py shows that a pass without D ends the
window 0.9 from the oracle.  Two Problems share the device matrix, replan(pack=True) and replan(pack=False); every cell runs a
form for the window of 8 iterations on two handles of the packed Problem in turn, and the same on the raw one.

Which pass a form takes, as found here: run, grad_update, run_backtracking and host_search stream the packed copy.
run_history asks every pass for the dual as well and neither packs nor reads the copy.  run_recorded, with or without the
search, packs (run_device_driven calls ensure_packed) but records ||A x_k - b||^2 through fos_fista_grad_dual, so its
iterations read the raw A: on a Problem that holds a copy these three give the raw plan's bits, which their cells assert,
while the copy stays in place."""
import numpy as np
import pytest
import torch

from tests import _data, _forms as F, _packed_probes as PP
from tests.test_gpu_fista_forms import Env, Handle, _check_searches, run_in_turn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


class PackedEnv(Env):
    """Env of tests/test_gpu_fista_forms.py on the heavy-tailed matrix, with the plans "packed" and "raw"."""

    def __init__(self, fos, cus):
        from fastoptsolver_amd import _core
        self.family, self.cus, self.spec = PP.FORMS_FAMILY, cus, F.families(cus)[PP.FORMS_FAMILY]
        self.A, self.b, self.L, self.lam = PP.forms_data(cus)
        At = torch.as_tensor(self.A.astype(np.float32)).cuda()
        assert np.array_equal(At.to(torch.float64).cpu().numpy(), self.A)
        b32 = self.b.astype(np.float32)
        self.prob = {"packed": fos.prepare(At, b32), "raw": fos.prepare(At, b32)}
        self.prob["raw"].replan(pack=False)
        bt = torch.as_tensor(b32).cuda()
        self.B = bt[:, None].repeat(1, 3).contiguous()
        self.fold_ids = _core.fold_ids_tensor(np.arange(self.spec["m"]) % 3, At.device)
        self.oracle, self.whole = {}, {}

    def fresh(self):
        """A replan drops the copy: the cell's first with-gradient pass is the one that packs."""
        self.prob["packed"].replan(pack=True)
        assert self.prob["packed"].plan()["packed"] == 0 and self.prob["packed"].plan()["pack_rows"] != 0


@pytest.fixture(scope="module")
def env(fos):
    cus = int(fos.prepare(torch.zeros(8, 68, device="cuda")).plan()["cus"])
    return PackedEnv(fos, cus)


def run_cell(env, cls, prms, steps, plan):
    """handles (weights 0 and 1) after the (form, iterations) of `steps`, call by call in turn."""
    handles = [Handle(env, cls, prms[w], w, plan) for w in (0, 1)]
    for form, iters in steps:
        assert run_in_turn(handles, form, iters) is True, (cls, form, plan, "refused")
    return handles


def amplification(env, states, a2):
    """What the window does to a rounding difference along the top singular vector of A: the gradient step multiplies it by
    |1 - tau (lambda_max + alpha2)|, and lambda_max >= L / 1.1 (make_data: L is 1.1 times a power iteration's lower bound).
    tau = 1 / (L + alpha2) in the plain and controlled classes: no growth, the factor is 1.  The backtracking class starts from
    8 / L and shrinks by 0.8 until the Armijo rule accepts: 5.12 / L in the first iteration and 2.62 / L from the second on
    (the oracle's steps, read here from its states) - a step beyond 2 / lambda_max, with which that component grows by 3.65 and
    then by 1.38 per iteration, 35 over the window (momentum, left out, only adds to it)."""
    top = env.L / 1.1 + a2
    return float(np.prod([max(1.0, s["tau"] * top - 1.0) for s in states[1:]]))


def check_cell(env, cls, prms, steps, prepack=False):
    total = sum(iters for _, iters in steps)
    assert total == F.WINDOW
    env.fresh()
    if prepack:                                             # a gradient of the Problem itself packs: the cell finds the copy there
        env.prob["packed"].gemv_pair(torch.zeros(env.spec["n"], device="cuda"))
        assert env.prob["packed"].plan()["packed"] == 1
    packed = run_cell(env, cls, prms, steps, "packed")
    assert env.prob["packed"].plan()["packed"] == 1, (steps, "the pass did not pack")
    raw = run_cell(env, cls, prms, steps, "raw")
    assert env.prob["raw"].plan()["packed"] == 0
    for h, hr in zip(packed, raw):
        o = env.states(cls, h.prm, h.w)[total]
        s, x, x_raw = h.st.status(), h.x(), hr.x()
        tag = (cls, h.prm["name"], h.w) + tuple(steps)
        assert int(s.k) == o["k"] and int(s.restarts) == o["restarts"] and int(s.stopped) == o["stopped"], \
            (tag, int(s.k), o["k"], int(s.restarts), o["restarts"], int(s.stopped), o["stopped"])
        d_pk, d_raw, d = _data.rel(x, o["x"]), _data.rel(x_raw, o["x"]), _data.rel(x, x_raw)
        print(f"{tag}: packed vs oracle {d_pk:.3e}  raw vs oracle {d_raw:.3e}  packed vs raw {d:.3e}")
        assert d_pk < F.TOL and d_raw < F.TOL, (tag, d_pk, d_raw)
        # the margin and argument of tests/test_packed_gpu.py::test_packed_full_run_against_oracle_and_raw_plan: the packed pass
        # re-associates fp32 sums of the same terms, a perturbation of the size of the raw pass's own rounding - times what the
        # window makes of such a perturbation (amplification: 1 everywhere but in the searching cells).  Measured on 256 CUs, the
        # searching cells: packed vs raw 1.65e-6 and 9.1e-7 for the two weights with d_raw = 1.96e-7 and 2.99e-7, and 1.74e-6
        # between two PACKED plans that differ in the row order alone (replan(interleave=)); through Problem.gemv_pair at the
        # oracle's y_1, y_3 and y_6 both passes were 0.8e-7 .. 2.1e-7 from fp64.  With the factor of 35 the margin of a searching
        # cell is no tighter than TOL on both sides: ONLY TOL and the oracle's shrink counts and steps, compared exactly
        # (_check_searches), guard the searching cells.  No bound tighter than TOL could be derived for them: the worst-case
        # bound of one fp32 pass on this matrix (tests/_data.fp32_pass_tolerances, or componentwise with the depths of the
        # kernel's sums) is 1e-5 .. 4e-5 of |g| at those points, and a ratio between two measured roundings is not a bound.
        amp = amplification(env, env.states(cls, h.prm, h.w), h.a2)
        assert (amp == 1.0) == (cls != "backtracking"), (tag, amp)
        assert d <= 2.0 * d_raw * amp, (tag, d, d_raw, amp)
        if all(form in DUAL_FORMS for form, _ in steps):    # every pass of the cell read the raw A: the raw plan's bits
            assert np.array_equal(x, x_raw), (tag, "a form that takes the dual pass differs from the raw plan")
    return packed


PLAIN_FORMS = ("run", "grad_update", "run_history", "run_recorded")
DUAL_FORMS = ("run_history", "run_recorded", "run_recorded_bt")      # ask every pass for the dual: never the packed pass
SEARCH_FORMS = ("run_backtracking", "run_recorded_bt", "host_search")
MIXED = (("run", "graddual_update"), ("graddual_update", "run"), ("run_multi4", "run"))


def test_the_matrix_packs(fos, env):
    case = PP.Case("forms", env.A)
    assert case.e0 == 114 and 8.5e-4 < case.share < 9.5e-4
    env.fresh()
    y = torch.zeros(env.spec["n"], device="cuda")
    env.prob["packed"].gemv_pair(y)
    assert env.prob["packed"].plan()["packed"] == 1


@pytest.mark.parametrize("form", PLAIN_FORMS)
def test_plain_forms_on_a_packed_plan(fos, env, form):
    """grad_update: the hook in launch_pass packs, not fos_fista_run.  run_history asks every pass for the dual as well
    (fos_fista_run_history: launch_pass(..., dual = true)), so it neither packs nor reads the copy: its cell runs on a Problem
    that holds one already and must leave it there."""
    prms = [F.class_params(env.family, "plain", w)[0] for w in (0, 1)]
    check_cell(env, "plain", prms, ((form, F.WINDOW),), prepack=form == "run_history")


@pytest.mark.parametrize("form", SEARCH_FORMS)
def test_searching_forms_on_a_packed_plan(fos, env, form):
    """host_search: trial_batch between grad and update, on a handle whose pass packed in grad."""
    prms = [F.class_params(env.family, "backtracking", w)[0] for w in (0, 1)]
    for h in check_cell(env, "backtracking", prms, ((form, F.WINDOW),)):
        _check_searches(h, F.WINDOW, dict(cell=(form, "packed")))      # the oracle's shrink counts and steps, exactly


def test_device_stop_on_a_packed_plan(fos, env):
    """The ratio rule stops the oracle at k = 2 of the 8 iterations asked: the three launches of every later iteration see the
    stopped flag; two more calls leave the iterate as it is, bit for bit."""
    prm = F.stop_params(env.family)
    handles = check_cell(env, "controlled", [prm, prm], (("run", F.WINDOW),))
    for h in handles:
        o = env.states("controlled", prm, h.w)[F.WINDOW]
        assert 0 < o["k"] < F.WINDOW and o["stopped"] == F.STOP_RATIO
        x, k = h.x(), int(h.st.status().k)
        for _ in range(2):
            h.st.run(3)
            assert np.array_equal(h.x(), x) and int(h.st.status().k) == k, "a stopped handle moved"


@pytest.mark.parametrize("X,Y", MIXED, ids=["/".join(c) for c in MIXED])
def test_mixed_forms_on_one_packed_handle(fos, env, X, Y):
    """The dual pass and the multi-vector pass read the raw A between packed passes of the same handle."""
    prms = [F.class_params(env.family, "plain", w)[0] for w in (0, 1)]
    check_cell(env, "plain", prms, ((X, F.WINDOW // 2), (Y, F.WINDOW // 2)))
