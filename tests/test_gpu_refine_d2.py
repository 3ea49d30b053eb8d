"""Mixed-precision solve (slu_plan_fill_a_d2 / slu_plan_refine_d2,
csrc/refine_d2.h): fp32 factors refined to the fp64 accuracy of the caller's
fp64 system, the scheme of the reference's psgsrfs_d2 (SRC/psgsrfs_d2.c) with
a power-of-two normalisation of the residual.

Matrices: the stencils' fp32 values widened and perturbed by 1e-3 relative,
so the fp64 A is not representable in fp32; b = A64 xt.

Checker: a numpy restatement of the loop -- fp64 residual, the same
normalisation, the correction from tests/lusolve.py on the downloaded fp32
factors (in fp64 arithmetic; the device sweeps in fp32, so corrections agree
to ~1e-7 relative and the converged solutions to fp64 accuracy; the device
sweep sums through float atomics, so two device runs differ likewise).  The
returned berr is compared with the componentwise backward error of the
returned x recomputed in extended precision (test_gpu_refine._berr).
"""
import numpy as np
import pytest
import scipy.sparse as sp

from gridrun_d2 import run_grid_d2, system
from lusolve import solve_1x1
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, STENCIL_3D27, Csc, Symbolic, nd_order
from test_gpu_refine import _berr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
BERR_MAX = 8 * EPS  # the bound of the fp64 refinement test


def d2_plan(S, cp, ri, v64):
    lu = S.distribute()
    p = Plan(lu)
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v64)
    assert p.factor(12.0)[0] == 0
    return p, lu


def host_refine_d2(lu, cp, ri, v64, b, x):
    """numpy restatement of slu_plan_refine_d2 on the host fp32 factors."""
    n = len(b)
    A64 = sp.csc_matrix((v64, ri, cp), shape=(n, n))
    absA = abs(A64)
    lstres, count = 3.0, 0
    x = np.array(x, dtype=np.float64)
    while True:
        r = b - A64 @ x
        s = absA @ np.abs(x) + np.abs(b)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.abs(r) / s
        be = float(np.nan if np.isnan(q).any() else q.max())
        if not (be > EPS and be * 2 <= lstres and count < 20):
            return x, be, count
        rmax = float(np.abs(r).max())
        e = int(np.frexp(rmax)[1]) if rmax > 0 and np.isfinite(rmax) else 0
        r32 = np.ldexp(r, -e).astype(np.float32)
        dx32 = solve_1x1(lu, r32).astype(np.float32)
        x = x + np.ldexp(dx32.astype(np.float64), e)
        lstres = be
        count += 1


def check_column(lu, cp, ri, v64, b, x0, x, berr, steps):
    assert berr <= BERR_MAX, berr
    assert 1 <= steps <= 20
    xh, bh, sh = host_refine_d2(lu, cp, ri, v64, b, x0)
    assert abs(int(steps) - sh) <= 1, (steps, sh)
    assert np.abs(x - xh).max() / np.abs(xh).max() < 1e-12
    # the device residual is summed in fp64: up to ~(row nnz + 1) roundings
    # relative to |A||x| + |b| (row nnz = column nnz: the pattern is symmetric)
    tol_b = 2 * (int(np.diff(cp).max()) + 1) * EPS
    assert abs(_berr(cp, ri, v64, x, b) - berr) <= tol_b


# ------------------------------------------------------------------ 1. fill
@pytest.mark.parametrize("kind,nx", [(STENCIL_3D7, 6), (STENCIL_3D27, 8)])
def test_fill_d2_is_an_exact_rounding(kind, nx):
    A, S, (cp, ri, v), v64, _, _ = system(kind, nx)
    lu, lu2 = S.distribute(), S.distribute()
    p = Plan(lu)
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v64)
    assert p.stats()["t_fill_ms"] > 0
    p.download()
    q = Plan(lu2)
    q.set_a_pattern(cp, ri)
    q.fill_a(v64.astype(np.float32))
    q.download()
    assert np.array_equal(lu.Lval, lu2.Lval) and np.array_equal(lu.Uval, lu2.Uval)
    assert np.abs(lu.Lval).max() > 0 and lu.Lval.dtype == np.float32


def test_fill_d2_duplicate_entry_keeps_last():
    A, S, (cp, ri, v), v64, _, _ = system(STENCIL_3D7, 6)
    lu = S.distribute()
    p = Plan(lu)
    j = 5
    at = cp[j + 1]  # append a duplicate of column j's first entry
    cp2 = cp.copy()
    cp2[j + 1:] += 1
    ri2 = np.insert(ri, at, ri[cp[j]])
    v2 = np.insert(v64, at, 99.0 + 2.0 ** -30)
    p.set_a_pattern(cp2, ri2)
    p.fill_a_d2(v2)
    p.download()
    L2, U2 = lu.Lval.copy(), lu.Uval.copy()
    v3 = v64.copy()
    v3[cp[j]] = 99.0 + 2.0 ** -30
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v3)
    p.download()
    assert np.array_equal(L2, lu.Lval) and np.array_equal(U2, lu.Uval)
    assert np.float32(99.0) in np.concatenate([lu.Lval, lu.Uval])


# ------------------------------------------------------------ 2, 6. refine
@pytest.mark.parametrize("kind,nx,start,amalg", [
    (STENCIL_3D7, 10, "zero", False),   # the plain plan
    (STENCIL_3D7, 12, "zero", True),    # through the coarse plan (6.)
    (STENCIL_3D27, 10, "solve", True),  # x0 = the fp32 solve, widened
])
def test_refine_d2_reaches_fp64_accuracy(kind, nx, start, amalg, monkeypatch):
    monkeypatch.setenv("SLU_AMALG", "1" if amalg else "0")
    A, S, (cp, ri, v), v64, b, xt = system(kind, nx)
    p, lu = d2_plan(S, cp, ri, v64)
    assert (p.stats()["amalg_groups"] > 0) == amalg
    p.download()
    x0 = p.solve(b.astype(np.float32)).astype(np.float64) if start == "solve" else np.zeros_like(b)
    x, berr, steps = p.refine_d2(b, x0)
    assert x.dtype == np.float64 and p.stats()["t_refine_ms"] > 0
    print(f"refine_d2 {kind} {nx}^3 {start}: berr {berr[0]:.3e} steps {steps[0]} "
          f"ferr {np.abs(x - xt).max() / np.abs(xt).max():.3e}")
    check_column(lu, cp, ri, v64, b, x0, x, berr[0], steps[0])
    # the fp32 path on the same plan: fill_a of the rounded values, fp32
    # refine of the rounded b -- its backward error against A64 stays at
    # fp32's level, so the accuracy above is the new path's doing
    p.fill_a(v64.astype(np.float32))
    assert p.factor(12.0)[0] == 0
    b32 = b.astype(np.float32)
    x32, be32, _ = p.refine(b32, p.solve(b32))
    be_vs_a64 = _berr(cp, ri, v64, x32.astype(np.float64), b)
    print(f"  fp32 refine: own berr {be32[0]:.3e}, against A64 {be_vs_a64:.3e}")
    assert be_vs_a64 > 1e-9


def test_refine_d2_several_columns():
    A, S, (cp, ri, v), v64, b, xt = system(STENCIL_3D7, 8, nrhs=3)
    assert np.linalg.matrix_rank(b) == 3
    p, lu = d2_plan(S, cp, ri, v64)
    p.download()
    x0 = np.zeros_like(b)
    x, berr, steps = p.refine_d2(b, x0)
    assert x.shape == b.shape and len(berr) == len(steps) == 3
    for j in range(3):
        check_column(lu, cp, ri, v64, b[:, j], x0[:, j], x[:, j], berr[j], steps[j])


# ------------------------------------------------------- 3. normalisation
@pytest.fixture(scope="module")
def norm_runs():
    A, S, (cp, ri, v), v64, b, xt = system(STENCIL_3D7, 8)
    p, lu = d2_plan(S, cp, ri, v64)
    out = {}
    for k in (0, -160, 130):
        x, berr, steps = p.refine_d2(np.ldexp(b, k), np.zeros_like(b))
        out[k] = (x, float(berr[0]), int(steps[0]))
    return out


@pytest.mark.parametrize("k", [-160, 130])
def test_refine_d2_is_scale_invariant(k, norm_runs):
    """b 2^k: without the scaling of the residual the first case rounds to a
    zero correction (berr stays 1) and the second overflows fp32."""
    runs = norm_runs
    x1, be1, st1 = runs[0]
    x, be, st = runs[k]
    print(f"b*2^{k}: berr {be:.3e} steps {st} (unscaled: {be1:.3e}, {st1})")
    assert be <= BERR_MAX and be1 <= BERR_MAX
    assert abs(st - st1) <= 1
    assert np.abs(np.ldexp(x, -k) - x1).max() / np.abs(x1).max() <= 1e-12


# ----------------------------------------------------------- 4. non-finite
def test_refine_d2_reports_nonfinite_backward_error():
    A, S, (cp, ri, v), v64, b, _ = system(STENCIL_3D7, 6)
    p, _ = d2_plan(S, cp, ri, v64)
    x0 = np.zeros_like(b)
    x0[5] = np.nan
    _, berr, steps = p.refine_d2(b, x0)
    assert not np.isfinite(berr[0]) and steps[0] == 0


# ------------------------------------------------- 5. state and dtype errors
def test_d2_needs_an_fp32_plan():
    A = Csc.stencil(STENCIL_3D7, 6, 6, 6)
    S = Symbolic(A, nd_order(6, 6, 6), 60, 256)
    p = Plan(S.distribute())
    cp, ri, v = A.permuted(S.perm_c).arrays()
    p.set_a_pattern(cp, ri)
    with pytest.raises(RuntimeError, match=r"fill_a_d2: fp32 plans only.*dtype is d"):
        p.fill_a_d2(v)
    p.fill_a(v)
    assert p.factor(12.0)[0] == 0
    with pytest.raises(RuntimeError, match=r"refine_d2: fp32 plans only.*dtype is d"):
        p.refine_d2(np.ones(A.n), np.zeros(A.n))
    x, berr, _ = p.refine(np.ones(A.n), np.zeros(A.n))  # the plan still works
    assert berr[0] < 1e-14


def test_d2_device_state_is_checked():
    A, S, (cp, ri, v), v64, b, _ = system(STENCIL_3D7, 6)
    p = Plan(S.distribute())
    x0 = np.zeros_like(b)
    p.set_a_pattern(cp, ri)
    with pytest.raises(ValueError, match="values for a pattern"):
        p.fill_a_d2(v64[:-1])
    p.fill_a_d2(v64)
    with pytest.raises(RuntimeError, match="factor first"):
        p.refine_d2(b, x0)
    assert p.factor(12.0)[0] == 0
    with pytest.raises(RuntimeError, match="fill_a"):   # no fp32 A for the plain refine
        p.refine(b.astype(np.float32), x0.astype(np.float32))
    _, berr, _ = p.refine_d2(b, x0)
    assert berr[0] <= BERR_MAX
    p.fill_a_d2(2 * v64)                                # refilled, not factored
    with pytest.raises(RuntimeError, match="factor first"):
        p.refine_d2(b, x0)
    assert p.factor(24.0)[0] == 0
    _, berr, _ = p.refine_d2(b, x0)
    assert berr[0] <= BERR_MAX
    p.fill_a(v64.astype(np.float32))                    # fp32 values: no fp64 A
    assert p.factor(12.0)[0] == 0
    with pytest.raises(RuntimeError, match="fill_a_d2"):
        p.refine_d2(b, x0)
    p.upload()                                          # values of unknown origin
    assert p.factor(12.0)[0] == 0
    with pytest.raises(RuntimeError, match="fill_a_d2"):
        p.refine_d2(b, x0)


@pytest.mark.parametrize("amalg", [True, False])
def test_d2_upload_forgets_the_fp64_values(amalg, monkeypatch):
    """fill_a_d2 -> factor -> upload of other values -> factor: the factors
    are of no A the plan knows, on the plain and on the coarse plan (whose
    upload is its own), so refine_d2 must refuse them."""
    monkeypatch.setenv("SLU_AMALG", "1" if amalg else "0")
    A, S, (cp, ri, v), v64, b, _ = system(STENCIL_3D7, 8)
    p, _ = d2_plan(S, cp, ri, v64)
    assert (p.stats()["amalg_groups"] > 0) == amalg
    _, berr, _ = p.refine_d2(b, np.zeros_like(b))
    assert berr[0] <= BERR_MAX
    p.upload()
    assert p.factor(12.0)[0] == 0
    with pytest.raises(RuntimeError, match="fill_a_d2"):
        p.refine_d2(b, np.zeros_like(b))


def test_d2_snapshot_restore_carry_the_values():
    """snapshot / restore keep which A the storage holds: restored d2 values
    factor and refine again; the fp32 refine still refuses them."""
    A, S, (cp, ri, v), v64, b, _ = system(STENCIL_3D7, 6)
    p = Plan(S.distribute())
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v64)
    p.snapshot()
    assert p.factor(12.0)[0] == 0
    x1, be1, st1 = p.refine_d2(b, np.zeros_like(b))
    p.restore()
    with pytest.raises(RuntimeError, match="factor first"):
        p.refine_d2(b, np.zeros_like(b))
    assert p.factor(12.0)[0] == 0
    x2, be2, st2 = p.refine_d2(b, np.zeros_like(b))
    assert be2[0] <= BERR_MAX and st2[0] == st1[0]
    assert np.abs(x2 - x1).max() <= 1e-12 * np.abs(x1).max()


# ------------------------------------------------------------ 7. 2x2 grid
def test_refine_d2_on_a_2x2_grid(tmp_path):
    out = run_grid_d2(STENCIL_3D27, 8, 2, 2, tmp_path)
    A, S, (cp, ri, v), v64, b, xt = system(STENCIL_3D27, 8)
    p, lu = d2_plan(S, cp, ri, v64)
    x1, be1, st1 = p.refine_d2(b, np.zeros_like(b))
    assert be1[0] <= BERR_MAX
    print(f"2x2: berr {[float(o['berr']) for o in out]} steps {[int(o['steps']) for o in out]}; "
          f"1x1: {be1[0]:.3e} {st1[0]}")
    for o in out:
        assert float(o["berr"]) <= BERR_MAX
        assert float(o["berr"]) == float(out[0]["berr"]) and int(o["steps"]) == int(out[0]["steps"])
        assert 1 <= int(o["steps"]) <= 20
        assert np.abs(o["x"] - x1).max() / np.abs(x1).max() <= 1e-12
