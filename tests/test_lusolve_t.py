"""The host transposed supernodal solve (tests/lusolve_t.py) pinned before
anything on the GPU relies on it: on the REFERENCE's own post-factor
LUstructs of the 1x1 refdump fixtures it solves B^T y = c (and B^H for the
complex fixture) to the accuracy of an independent sparse solve by scipy of
the fixture's matrix in LU coordinates, and the coordinate maps for a caller
who starts from A^T x = b close the loop through the fixture's R, C, perm_r
and perm_c."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from lusolve import lu_coords_matrix
from lusolve_t import from_lu_coords_t, op_t, solve_1x1_t, to_lu_coords_t
from refdump import Fixture, names

CASES = [n for n in names() if "_1x1_" in n and not n.startswith("zeropiv")]
EPS = {0: 2.2e-16, 1: 1.2e-7, 2: 2.2e-16}


def checker(fx, conj, seed=3):
    """(c, y_true, y_scipy): a generated true solution of op(B)^T y = c and
    scipy's own solve of it -- its error is the accuracy a solve can have."""
    cp, ri, v = lu_coords_matrix(fx)
    Bt = op_t(cp, ri, v.astype(np.complex128 if fx.dtype == 2 else np.float64), conj)
    rng = np.random.default_rng(seed)
    yt = rng.standard_normal(fx.n)
    if fx.dtype == 2:
        yt = yt + 1j * rng.standard_normal(fx.n)
    c = Bt @ yt
    return c, yt, spla.splu(sp.csc_matrix(Bt)).solve(c)


def factor_error(fx):
    """What the fixture's FACTORS cost a solve: the reference's own pdgstrs
    error against its generated solution (x_norefine - xtrue).  It matters
    for tinypiv, whose replaced pivot makes L U a perturbed B: B^T is then
    solved with the same perturbation, transposed."""
    xn, xt = fx.arr(0, "x_norefine"), fx.arr(0, "xtrue")
    return float(np.abs(xn - xt).max() / np.abs(xn).max())


def close(y, ys, yt, fx):
    """test_solve_ref._close: y agrees with the checker's solution to ten
    times the checker's own error against the true one (at least 50 eps),
    or ten times the error the reference's own solve has on these factors."""
    ny = np.abs(ys).max()
    return (np.abs(y - ys).max() / ny,
            max(10 * np.abs(ys - yt).max() / ny, 50 * EPS[fx.dtype], 10 * factor_error(fx)))


@pytest.mark.parametrize("name,conj", [(n, False) for n in CASES] +
                         [(n, True) for n in CASES if n.endswith("_z")])
def test_host_transposed_solve_of_reference_factors(name, conj):
    fx = Fixture(name)
    lu = fx.lu(0, "post")
    c, yt, ys = checker(fx, conj)
    y = solve_1x1_t(lu, c, conj)
    d, tol = close(y, ys, yt, fx)
    print(name, conj, d, tol)
    assert d < tol, (d, tol)
    # where op(B)^T is far from B (cg20 is complex symmetric: only its B^H
    # is), the plain sweep on the same right-hand side is far away too
    cp, ri, v = lu_coords_matrix(fx)
    B = sp.csc_matrix((v, ri, cp), shape=(fx.n, fx.n))
    if spla.norm(op_t(cp, ri, v, conj) - B) > 0.1 * spla.norm(B):
        from lusolve import solve_1x1
        assert np.abs(solve_1x1(lu, c) - ys).max() / np.abs(ys).max() > 1e-3


@pytest.mark.parametrize("name", CASES)
def test_coordinate_maps_of_the_transposed_solve(name):
    """A^T x = b through c[perm_c[j]] = C[j] b[j], B^T y = c,
    x[i] = R[i] y[perm_c[perm_r[i]]], checked against A itself: B =
    Pc Pr diag(R) A diag(C) Pc^T is undone on the fixture's matrix."""
    fx = Fixture(name)
    R, C = fx.z.get("r0_R"), fx.z.get("r0_C")
    pr, pc = fx.arr(0, "perm_r"), fx.arr(0, "perm_c")
    n = fx.n
    cp, ri, v = lu_coords_matrix(fx)
    B = sp.csc_matrix((v, ri, cp), shape=(n, n)).tocoo()
    # A[i, j] = B[perm_c[perm_r[i]], perm_c[j]] / (R[i] C[j])
    inv_row, inv_col = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    inv_row[pc[pr]] = np.arange(n)
    inv_col[pc] = np.arange(n)
    Rv = R if R is not None else np.ones(n)
    Cv = C if C is not None else np.ones(n)
    i, j = inv_row[B.row], inv_col[B.col]
    A = sp.csc_matrix((B.data / (Rv[i] * Cv[j]), (i, j)), shape=(n, n))
    rng = np.random.default_rng(5)
    xt = rng.standard_normal(n)
    b = A.T @ xt
    y = solve_1x1_t(fx.lu(0, "post"), to_lu_coords_t(b, pc, C))
    x = from_lu_coords_t(y, pr, pc, R)
    # to the accuracy of the factors (1e-8 covers the conditioning of the d / z fixtures)
    assert np.abs(x - xt).max() / np.abs(xt).max() < max(1e-8, 10 * factor_error(fx))
