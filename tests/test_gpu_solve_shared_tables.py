"""The solve tables (csrc/engine.hip build_solve) are built lazily by
whichever entry point of the solve layer is called first, by one builder that
solve, solve_t, solve_block, refine, refine_d2 and rcond share.  No caller may
depend on a side effect of the builder that another caller skips.

For each first caller: a fresh plan on lap3d 6^3 (relax 4, maxsup 8: several
levels, supernodes with panel rows), factored, the first caller, then solve
with 3 right-hand sides and solve_block with 3 columns against the host solve
of tests/lusolve.py on the plan's downloaded factors at the fp64 tolerance of
tests/test_gpu_solve.py (1e-12 normwise), then rcond against the value of a
plan whose first call was rcond, to 1e-12 relative.
"""
import functools

import numpy as np
import pytest

from lusolve import solve_1x1
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order

pytestmark = pytest.mark.gpu

DIMS = (6, 6, 6)
TOL = 1e-12
DT = {0: np.float64, 2: np.complex128}


@functools.lru_cache(maxsize=None)
def problem(dtype):
    """(symbolic, pattern and values of B in LU coordinates, b of 3 columns, ||B||_1)"""
    kw = dict(diag=6 - 0.25, diag_im=-0.0025) if dtype == 2 else {}
    A = Csc.stencil(STENCIL_3D7, *DIMS, dtype=dtype, **kw)
    S = Symbolic(A, nd_order(*DIMS), 4, 8)
    cp, ri, v = A.permuted(S.perm_c).arrays()
    rng = np.random.default_rng(7)
    xt = rng.standard_normal((A.n, 3))
    if dtype == 2:
        xt = xt + 1j * rng.standard_normal((A.n, 3))
    b = np.zeros((A.n, 3), dtype=DT[dtype])
    anorm = 0.0
    for j in range(A.n):
        sl = slice(cp[j], cp[j + 1])
        b[ri[sl]] += np.outer(v[sl], xt[j])
        anorm = max(anorm, float(np.abs(v[sl]).sum()))
    b = np.asfortranarray(b)
    b.setflags(write=False)
    return S, (cp, ri, v), b, anorm


def fresh_plan(dtype):
    """(plan with the factors of B on the device and no solve tables yet, lu with them downloaded)"""
    S, (cp, ri, v), b, anorm = problem(dtype)
    lu = S.distribute()
    p = Plan(lu)
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(anorm) == (0, 0)
    p.download()
    return p, lu


@functools.lru_cache(maxsize=None)
def rcond_first(dtype):
    p, _ = fresh_plan(dtype)
    return p.rcond(problem(dtype)[3])


FIRST = {
    "solve": lambda p, b, an: p.solve(b[:, 0]),
    "solve_t": lambda p, b, an: p.solve(b[:, 0], trans="T"),
    "solve_conj": lambda p, b, an: p.solve(b[:, 0], trans="C"),
    "solve_block": lambda p, b, an: p.solve_block(b[:, :1]),
    "refine": lambda p, b, an: p.refine(b[:, 0], np.zeros_like(b[:, 0])),
    "rcond": lambda p, b, an: p.rcond(an),
}


@pytest.mark.parametrize("dtype,first", [(0, "solve"), (0, "solve_t"), (0, "solve_block"), (0, "refine"),
                                         (0, "rcond"), (2, "solve_conj")])
def test_tables_do_not_depend_on_the_first_caller(dtype, first):
    b, anorm = problem(dtype)[2:]
    p, lu = fresh_plan(dtype)
    st = p.stats()
    assert st["nlevels"] >= 3 and st["nsupers"] > st["nlevels"]
    FIRST[first](p, b, anorm)
    xh = np.stack([solve_1x1(lu, b[:, r]) for r in range(3)], axis=1)
    nx = np.abs(xh).max(axis=0)
    xs = p.solve(b)
    xb = p.solve_block(b)
    es = (np.abs(xs - xh).max(axis=0) / nx).max()
    eb = (np.abs(xb - xh).max(axis=0) / nx).max()
    rc, rc0 = p.rcond(anorm), rcond_first(dtype)
    print(f"{first}: solve {es:.3e} solve_block {eb:.3e} rcond {rc:.15e} rcond first {rc0:.15e} "
          f"levels {st['nlevels']} supernodes {st['nsupers']}")
    assert np.isfinite(xs).all() and np.isfinite(xb).all()
    assert es < TOL and eb < TOL
    assert rc0 > 0 and abs(rc - rc0) <= 1e-12 * rc0
