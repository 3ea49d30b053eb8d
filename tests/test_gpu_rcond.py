"""Reciprocal condition estimate on the device factors (slu_plan_rcond:
Hager / Higham's estimator as LAPACK dlacn2 / zlacn2, what sequential
SuperLU's dgscon returns), at sizes where a dense inverse is cheap.

(a) the estimate of ||B^-1|| never exceeds the true norm (numpy.linalg.inv):
    exact for the algorithm, so up to the solves' accuracy -- 1e-6 relative
    for d / z, 1e-2 for s;
(b) the same loop in numpy, driven by the host solves of tests/lusolve.py and
    tests/lusolve_t.py on the downloaded factors, gives the same estimate to
    1e-8 (s: 1e-3) and takes the same number of sweeps;
(c) norm 'I' of B equals norm '1' of a plan built from B^T's values;
(d) five rows scaled by 1e-8 cost at least six orders of rcond.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from lusolve import lu_coords_matrix, solve_1x1
from lusolve_t import solve_1x1_t, unsym_stencil
from refdump import Fixture
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order

pytestmark = pytest.mark.gpu

SAFMIN = 2.2250738585072014e-308
SCALED_ROWS = (3, 100, 500, 777, 999)


def host_estimate(lu, n, norm):
    """(estimate of ||B^-1||_norm, sweeps): dlacn2 / zlacn2 restated, kase 1
    = B^-1 (norm '1') and kase 2 = B^-H, swapped for 'I'."""
    cplx = lu.Lval.dtype == np.complex128
    fwd = lambda x: solve_1x1(lu, x)                 # noqa: E731
    adj = lambda x: solve_1x1_t(lu, x, conj=cplx)    # noqa: E731
    op1, op2 = (fwd, adj) if norm == "1" else (adj, fwd)
    sweeps = 0

    def sign(x):
        if cplx:
            a = np.abs(x)
            return np.where(a > SAFMIN, x / np.where(a > SAFMIN, a, 1.0), 1.0 + 0j)
        return np.where(x >= 0, 1.0, -1.0)

    x = op1(np.full(n, 1.0 / n, dtype=np.complex128 if cplx else np.float64))
    sweeps += 1
    est = float(np.abs(x).sum())
    if n == 1:
        return est, sweeps
    sgn = sign(x)
    x = op2(sgn)
    sweeps += 1
    j = int(np.argmax(np.abs(x)))
    it = 2
    while True:
        e = np.zeros_like(x)
        e[j] = 1.0
        x = op1(e)
        sweeps += 1
        estold, est = est, float(np.abs(x).sum())
        sg = sign(x)
        if (not cplx and (sg == sgn).all()) or est <= estold:
            break
        sgn = sg
        x = op2(sg)
        sweeps += 1
        jlast, j = j, int(np.argmax(np.abs(x)))
        xl = abs(x[jlast]) if cplx else x[jlast]
        if xl != abs(x[j]) and it < 5:
            it += 1
            continue
        break
    alt = np.array([(-1.0) ** i * (1.0 + i / (n - 1)) for i in range(n)], dtype=x.dtype)
    x = op1(alt)
    sweeps += 1
    return max(est, 2.0 * float(np.abs(x).sum()) / (3.0 * n)), sweeps


def _plan_of(A, dims, anorm):
    S = Symbolic(A, nd_order(*dims), 60, 256)
    lu = S.distribute()
    p = Plan(lu)
    p.upload()
    assert p.factor(anorm)[0] == 0
    p.download()
    cp, ri, v = A.permuted(S.perm_c).arrays()
    return p, lu, sp.csc_matrix((v, ri, cp), shape=(A.n, A.n)).toarray()


def _scaled(A, dtype):
    cp, ri, v = A.arrays()
    v = v.copy()
    v[np.isin(ri, SCALED_ROWS)] *= 1e-8
    return Csc.from_arrays(A.n, cp, ri, v, dtype)


@functools.lru_cache(maxsize=None)
def case(name):
    """(plan, downloaded lu, dense B as float64 / complex128)"""
    if name in ("g20", "cd2d_24"):
        fx = Fixture(f"{name}_1x1_d")
        lu = fx.lu(0, "pre")
        p = Plan(lu, replace_tiny=fx.replace_tiny)
        cp, ri, v = lu_coords_matrix(fx)
        p.set_a_pattern(cp, ri)
        p.fill_a(v)
        assert p.factor(fx.anorm)[0] == fx.info == 0
        p.download()
        return p, lu, sp.csc_matrix((v, ri, cp), shape=(fx.n, fx.n)).toarray()
    if name == "d10":
        return _plan_of(unsym_stencil(STENCIL_3D7, (10, 10, 10), 0), (10, 10, 10), 14.0)
    if name == "d10_scaled":
        return _plan_of(_scaled(unsym_stencil(STENCIL_3D7, (10, 10, 10), 0), 0), (10, 10, 10), 14.0)
    if name == "d10_t":  # the plan of B^T's values: the same pattern and ordering
        A = unsym_stencil(STENCIL_3D7, (10, 10, 10), 0)
        cp, ri, v = A.arrays()
        At = sp.csc_matrix((v, ri, cp), shape=(A.n, A.n)).T.tocsc()
        At.sort_indices()
        return _plan_of(Csc.from_arrays(A.n, At.indptr, At.indices, At.data, 0), (10, 10, 10), 14.0)
    if name == "z8":
        return _plan_of(unsym_stencil(STENCIL_3D7, (8, 8, 8), 2), (8, 8, 8), 14.0)
    if name == "s8":
        return _plan_of(unsym_stencil(STENCIL_3D7, (8, 8, 8), 1), (8, 8, 8), 14.0)
    raise KeyError(name)


def anorm_of(B, norm):
    return float(np.abs(B).sum(axis=0 if norm == "1" else 1).max())


@pytest.mark.parametrize("norm", ["1", "I"])
@pytest.mark.parametrize("name", ["d10", "z8", "s8", "g20", "cd2d_24", "d10_scaled"])
def test_rcond_is_a_lower_bound_and_matches_the_host_loop(name, norm):
    p, lu, B = case(name)
    n = B.shape[0]
    single = lu.Lval.dtype == np.float32
    an = anorm_of(B, norm)
    rc = p.rcond(an, norm=norm)
    sweeps, ms = p.rcond_info()
    assert rc > 0 and ms > 0
    est = 1.0 / (rc * an)
    true = np.linalg.norm(np.linalg.inv(B.astype(np.complex128 if np.iscomplexobj(B) else np.float64)),
                          1 if norm == "1" else np.inf)
    he, hs = host_estimate(lu, n, norm)
    print(f"{name} {norm}: est {est:.6e} true {true:.6e} (ratio {est / true:.4f}) host {he:.6e} "
          f"rel {abs(est - he) / he:.2e} sweeps {sweeps} / {hs}")
    assert est <= true * (1 + (1e-2 if single else 1e-6))       # (a)
    assert abs(est - he) <= (1e-3 if single else 1e-8) * he      # (b)
    assert sweeps == hs and 3 <= sweeps <= 11


def test_rcond_inf_norm_is_one_norm_of_the_transposed_plan():
    p, _, B = case("d10")
    q, _, Bt = case("d10_t")
    assert np.array_equal(Bt, B.T)
    an = anorm_of(B, "I")
    assert an == pytest.approx(anorm_of(Bt, "1"), rel=1e-14)  # the same sums in another order
    r1, r2 = p.rcond(an, norm="I"), q.rcond(an, norm="1")
    print(f"rcond_I(B) {r1:.12e} rcond_1(B^T) {r2:.12e}")
    assert abs(r1 - r2) <= 1e-8 * r2
    # and the other way round
    an1 = anorm_of(B, "1")
    r3, r4 = p.rcond(an1, norm="1"), q.rcond(an1, norm="I")
    assert abs(r3 - r4) <= 1e-8 * r4


def test_rcond_sees_row_scaling():
    p, _, B = case("d10")
    q, _, Bs = case("d10_scaled")
    for norm in ("1", "I"):
        r, rs = p.rcond(anorm_of(B, norm), norm=norm), q.rcond(anorm_of(Bs, norm), norm=norm)
        print(f"norm {norm}: rcond {r:.3e}, rows scaled {rs:.3e}")
        assert 0 < rs <= 1e-6 * r


def test_rcond_degenerate_arguments():
    p, _, B = case("d10")
    assert p.rcond(0.0) == 0.0
    assert p.rcond(float("inf")) == 0.0
    assert p.rcond(float("nan")) == 0.0
