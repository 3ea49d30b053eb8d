"""Device iterative refinement of B^T y = c / B^H y = c (slu_plan_refine_t;
the loop of SRC/pdgsrfs.c:197-253 with the residual r = c - op(B)^T x,
s = |B^T||x| + |c| by columns of the CSC, csrc/solve.h k_resid_t) on the
unsymmetric 12^3 system of tests/lusolve_t.py.

Checker: a numpy restatement of the same loop on B^T (host residual, host
transposed supernodal solve on the downloaded factors).  The sums run in a
different order, so the stopping decision near eps may differ by a step: steps
within one, x to the solve tolerance (1e-12 fp64 / complex, 1e-4 fp32), berr
at most 4 eps of the type (eps = 2.2e-16 / 1.2e-7, the bound the reference
fixtures' refinement is held to in test_solve_ref.py).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from lusolve_t import op_t, solve_1x1_t, unsym_stencil
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, Symbolic, nd_order

pytestmark = pytest.mark.gpu

EPS = {0: 2.2e-16, 1: 1.2e-7, 2: 2.2e-16}          # the bound on berr: 4 EPS
UNIT = {0: 2.0 ** -53, 1: 2.0 ** -24, 2: 2.0 ** -53}  # the loop's own eps (unit roundoff)
TOL = {0: 1e-12, 1: 1e-4, 2: 1e-12}
DT = {0: np.float64, 1: np.float32, 2: np.complex128}
DIMS = (12, 12, 12)


def _abs1(v):
    return np.abs(v.real) + np.abs(v.imag) if np.iscomplexobj(v) else np.abs(v)


def host_refine_t(lu, Bt, b, x, eps, conj):
    """numpy restatement of the loop on op(B)^T = Bt (CSR), in the plan's
    element type, the correction from the host transposed solve."""
    absBt = sp.csr_matrix((_abs1(Bt.data).astype(np.float64), Bt.indices, Bt.indptr), shape=Bt.shape)
    lstres, count = 3.0, 0
    while True:
        r = (b - Bt @ x).astype(x.dtype)
        s = absBt @ _abs1(x).astype(np.float64) + _abs1(b)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = _abs1(r) / s
        be = float(np.nan if np.isnan(q).any() else q.max())
        if not (be > eps and be * 2 <= lstres and count < 20):
            return x, be, count
        x = x + solve_1x1_t(lu, r, conj).astype(x.dtype)
        lstres = be
        count += 1


@functools.lru_cache(maxsize=None)
def system(dtype):
    A = unsym_stencil(STENCIL_3D7, DIMS, dtype)
    S = Symbolic(A, nd_order(*DIMS), 60, 256)
    lu = S.distribute()
    p = Plan(lu)
    cp, ri, v = A.permuted(S.perm_c).arrays()
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(14.0)[0] == 0
    p.download()
    return p, lu, (cp, ri, v)


@pytest.mark.parametrize("dtype,trans", [(0, "T"), (1, "T"), (2, "C")])
@pytest.mark.parametrize("start", ["solve", "perturbed"])
def test_device_refine_t_matches_host_loop(dtype, trans, start):
    p, lu, (cp, ri, v) = system(dtype)
    conj = trans == "C"
    Bt = op_t(cp, ri, v, conj)
    rng = np.random.default_rng(11)
    n = len(cp) - 1
    xt = rng.standard_normal(n)
    if dtype == 2:
        xt = xt + 1j * rng.standard_normal(n)
    b = (Bt @ xt).astype(DT[dtype])
    x0 = p.solve(b, trans=trans)
    if start == "perturbed":
        x0 = (x0 * (1 + 1e-3 * rng.standard_normal(n))).astype(DT[dtype])
    x, berr, steps = p.refine(b, x0, trans=trans)
    assert x.dtype == DT[dtype] and p.stats()["t_refine_ms"] > 0
    xh, bh, sh = host_refine_t(lu, Bt, b, x0.copy(), UNIT[dtype], conj)
    print(f"dtype {dtype} {trans} {start}: berr {berr[0]:.3e} steps {steps[0]} (host {bh:.3e}, {sh})")
    assert berr[0] <= 4 * EPS[dtype], berr
    assert abs(int(steps[0]) - sh) <= 1, (steps, sh)
    if start == "perturbed":
        assert steps[0] >= 1
    assert np.abs(x - xh).max() / np.abs(xh).max() < TOL[dtype]
    # the plain refinement of the same pair heads for another solution
    xp, _, _ = p.refine(b, x0)
    assert np.abs(xp - x).max() / np.abs(x).max() > 1e-3


def test_refine_t_several_columns_and_notrans():
    p, lu, (cp, ri, v) = system(0)
    Bt = op_t(cp, ri, v)
    rng = np.random.default_rng(5)
    n = len(cp) - 1
    b = np.asfortranarray(Bt @ rng.standard_normal((n, 3)))
    x, berr, steps = p.refine(b, np.zeros_like(b), trans="T")
    assert x.shape == b.shape and len(berr) == len(steps) == 3
    assert (berr <= 4 * EPS[0]).all() and (steps >= 1).all()
    for j in range(3):
        xh = solve_1x1_t(lu, b[:, j])
        assert np.abs(x[:, j] - xh).max() / np.abs(xh).max() < TOL[0]
    # SLU_NOTRANS through slu_plan_refine_t is slu_plan_refine
    x1, be1, st1 = p.refine(b, np.zeros_like(b))
    x2, be2, st2 = p.refine(b, np.zeros_like(b), trans=0)
    assert (st1 == st2).all() and np.abs(x1 - x2).max() <= 1e-13 * np.abs(x1).max()


def test_refine_t_reports_nonfinite_backward_error():
    """A NaN in x0 must surface in berr (NaN wins the maximum), not look
    like convergence."""
    p, lu, (cp, ri, v) = system(0)
    b = np.ones(len(cp) - 1)
    x0 = p.solve(b, trans="T")
    x0[5] = np.nan
    _, berr, steps = p.refine(b, x0, trans="T")
    assert not np.isfinite(berr[0]) and steps[0] == 0


def test_refine_t_refuses_factors_of_fill_a_d2():
    """fill_a_d2 leaves no fp32 A on the device: refine_t refuses such
    factors as refine does (solve_t needs no A and still runs)."""
    A = unsym_stencil(STENCIL_3D7, (6, 6, 6), 1)
    S = Symbolic(A, nd_order(6, 6, 6), 60, 256)
    p = Plan(S.distribute())
    cp, ri, v = A.permuted(S.perm_c).arrays()
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v.astype(np.float64))
    assert p.factor(14.0)[0] == 0
    b = np.ones(A.n, dtype=np.float32)
    with pytest.raises(RuntimeError, match="fill_a"):
        p.refine(b, b, trans="T")
    assert np.isfinite(p.solve(b, trans="T")).all()
    p.fill_a(v)                                        # refilled, not factored
    with pytest.raises(RuntimeError, match="factor first"):
        p.refine(b, b, trans="T")
    assert p.factor(14.0)[0] == 0
    _, berr, _ = p.refine(b, np.zeros_like(b), trans="T")
    assert berr[0] <= 4 * EPS[1]
