"""Transposed and conjugate-transposed device solve on the HBM-resident
factors (slu_plan_solve_t; csrc/solve.h k_sv_utdiag / k_sv_utpanel /
k_sv_ltpanel / k_sv_ltdiag).

Matrices: stencils are symmetric, so a transposed solve of one proves little.
The systems are stencil PATTERNS with unsymmetric values
(lusolve_t.unsym_stencil: every off-diagonal drawn independently, dominant
diagonal); each test first asserts that B^T (and, for complex, B^H against
B^T) is far from B.

Checker: the host transposed supernodal solve of tests/lusolve_t.py (pinned
on the reference's factors by tests/test_lusolve_t.py) on the same downloaded
factors, at the project's solve tolerances (normwise 1e-12 fp64 / complex,
1e-4 fp32), plus the backward error against B^T / B^H.  The device sums
through atomics, so trans="N" against solve() is compared to the atomics'
last bits: 1e-13 in fp64 / complex, and the same multiple of the unit
roundoff in fp32 (1e-13 * 2^29).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from lusolve import lu_coords_matrix
from lusolve_t import backward_error_t, op_t, solve_1x1_t, unsym_stencil
from refdump import Fixture, names
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_2D5, STENCIL_3D7, STENCIL_3D27, Symbolic, nd_order
from superlu_dist_amd.lib import lib

pytestmark = pytest.mark.gpu

TOL = {0: 1e-12, 1: 1e-4, 2: 1e-12}
BTOL = {0: 1e-14, 1: 1e-5, 2: 1e-14}
BITS = {0: 1e-13, 1: 1e-13 * 2.0 ** 29, 2: 1e-13}
DT = {0: np.float64, 1: np.float32, 2: np.complex128}


def factored(kind, dims, dtype, relax, maxsup):
    """(plan with the factors on the device, lu with them downloaded, B's CSC)"""
    A = unsym_stencil(kind, dims, dtype)
    S = Symbolic(A, nd_order(*dims), relax, maxsup)
    lu = S.distribute()
    p = Plan(lu)
    p.upload()
    assert p.factor(28.0 if kind == STENCIL_3D27 else 14.0) == (0, 0)
    p.download()
    return p, lu, A.permuted(S.perm_c).arrays()


def assert_unsymmetric(cp, ri, v):
    n = len(cp) - 1
    B = sp.csc_matrix((v, ri, cp), shape=(n, n))
    nb = spla.norm(B, 1)
    assert spla.norm(B - B.T, 1) / nb > 0.1
    if np.iscomplexobj(v):
        assert spla.norm(B.conj().T - B.T, 1) / nb > 0.1


def rhs(cp, ri, v, dtype, nrhs, conj, seed=7):
    rng = np.random.default_rng(seed)
    n = len(cp) - 1
    xt = rng.standard_normal((n, nrhs))
    if dtype == 2:
        xt = xt + 1j * rng.standard_normal((n, nrhs))
    return np.asfortranarray((op_t(cp, ri, v, conj) @ xt).astype(DT[dtype]))


@pytest.mark.parametrize("kind,dims,dtype,relax,maxsup,nrhs,trans", [
    (STENCIL_3D7, (12, 12, 12), 0, 60, 256, 1, "T"),
    (STENCIL_3D7, (16, 16, 16), 0, 4, 24, 3, "T"),     # narrow supernodes, many levels, short U segments
    (STENCIL_3D7, (20, 20, 20), 0, 60, 320, 2, "T"),   # w > 256: two rows per thread in the plain sweep
    # supernodes whose last panel starts in the upper half of a wave (width 300 / 100)
    (STENCIL_3D7, (20, 20, 20), 2, 60, 300, 3, "C"),
    (STENCIL_3D7, (20, 20, 20), 1, 60, 300, 3, "T"),
    (STENCIL_3D7, (12, 12, 12), 0, 60, 256, 10, "T"),  # batches of 8 + 2 right-hand sides
    (STENCIL_3D7, (8, 8, 8), 2, 60, 256, 5, "T"),      # complex: batches of 2 + 2 + 1
    (STENCIL_3D7, (8, 8, 8), 2, 60, 256, 5, "C"),
    (STENCIL_3D27, (8, 8, 8), 1, 60, 256, 9, "T"),
    (STENCIL_2D5, (40, 40, 1), 0, 60, 256, 1, "T"),
])
def test_device_solve_t_matches_host_solve(kind, dims, dtype, relax, maxsup, nrhs, trans):
    p, lu, (cp, ri, v) = factored(kind, dims, dtype, relax, maxsup)
    assert_unsymmetric(cp, ri, v)
    conj = trans == "C"
    b = rhs(cp, ri, v, dtype, nrhs, conj)
    x = p.solve(b, trans=trans)
    assert x.shape == b.shape and x.dtype == DT[dtype]
    assert p.stats()["t_solve_ms"] > 0
    xn = p.solve(b)
    for r in range(nrhs):
        xh = solve_1x1_t(lu, b[:, r], conj)
        err = np.abs(x[:, r] - xh).max() / np.abs(xh).max()
        berr = backward_error_t(cp, ri, v, x[:, r].astype(xh.dtype), b[:, r].astype(xh.dtype), conj)
        print(f"col {r}: err {err:.3e} berr {berr:.3e}")
        assert err < TOL[dtype], (r, err)
        assert berr < BTOL[dtype], (r, berr)
        # a forwarder to the plain sweep fails this
        assert np.abs(x[:, r] - xn[:, r]).max() / np.abs(xn[:, r]).max() > 1e-3
    for tn in ("N", 0):  # the Python default path and slu_plan_solve_t(SLU_NOTRANS)
        x0 = p.solve(b, trans=tn)
        assert np.abs(x0 - xn).max() / np.abs(xn).max() <= BITS[dtype]
    if dtype != 2:  # SLU_CONJ on a real plan is SLU_TRANS
        xc = p.solve(b, trans="C" if trans == "T" else "T")
        assert np.abs(xc - x).max() / np.abs(x).max() <= BITS[dtype]


CASES = [n for n in names() if "_1x1_" in n and not n.startswith("zeropiv")]
EPS = {0: 2.2e-16, 1: 1.2e-7, 2: 2.2e-16}


@pytest.mark.parametrize("name,trans", [(n, "T") for n in CASES] +
                         [(n, "C") for n in CASES if n.startswith("cg20")])
def test_solve_t_on_reference_lustructs(name, trans):
    """The reference's own LUstructs (MC64 row permutations, unsymmetric
    structure, skyline U segments with fst above the block's first row):
    fill_a, factor, solve_t in LU coordinates, against an independent fp64
    sparse solve of B^T / B^H by scipy.  Tolerance: test_solve_ref._close's
    form, max(10 x that checker's own error against the generated true
    solution, 50 eps).  tinypiv's factors are those of a perturbed B (a
    replaced pivot), which scipy's exact solve does not share: there the
    error the reference's own solve has on its factors, x 10, joins the
    maximum (tests/test_lusolve_t.factor_error)."""
    from test_lusolve_t import checker, factor_error
    fx = Fixture(name)
    lu = fx.lu(0, "pre")
    p = Plan(lu, replace_tiny=fx.replace_tiny)
    cp, ri, v = lu_coords_matrix(fx)
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(fx.anorm) == (fx.info, fx.tiny)
    conj = trans == "C"
    c, yt, ys = checker(fx, conj)
    y = p.solve(c.astype(lu.Lval.dtype), trans=trans)
    ny = np.abs(ys).max()
    d = np.abs(y - ys).max() / ny
    tol = max(10 * np.abs(ys - yt).max() / ny, 50 * EPS[fx.dtype])
    if fx.tiny:
        tol = max(tol, 10 * factor_error(fx))
    print(f"{name} {trans}: {d:.3e} (tol {tol:.3e})")
    assert d < tol, (d, tol)


@pytest.mark.parametrize("amalg", [False, True])
def test_solve_t_plain_and_coarse_plan(amalg, monkeypatch):
    monkeypatch.setenv("SLU_AMALG", "1" if amalg else "0")
    p, lu, (cp, ri, v) = factored(STENCIL_3D7, (12, 12, 12), 0, 60, 256)
    assert (p.stats()["amalg_groups"] > 0) == amalg
    b = rhs(cp, ri, v, 0, 3, False)
    x = p.solve(b, trans="T")
    for r in range(3):
        xh = solve_1x1_t(lu, b[:, r])
        assert np.abs(x[:, r] - xh).max() / np.abs(xh).max() < TOL[0]
        assert backward_error_t(cp, ri, v, x[:, r], b[:, r]) < BTOL[0]
    rc = p.rcond(14.0)
    assert 0 < rc < 1 and p.rcond_info()[0] >= 3


def test_solve_t_does_not_read_stale_lds():
    """NaN in every LDS word before one solve_t (partial last panels, a
    partial batch of 3 of 8 right-hand sides, partial chunks): unchanged."""
    p, lu, (cp, ri, v) = factored(STENCIL_3D7, (20, 20, 20), 0, 60, 300)
    b = rhs(cp, ri, v, 0, 3, False)
    x1 = p.solve(b, trans="T")
    assert lib().slu_debug_poison_lds(0) == 0
    x2 = p.solve(b, trans="T")
    assert np.isfinite(x2).all()
    assert np.abs(x2 - x1).max() / np.abs(x1).max() <= BITS[0]
    assert lib().slu_debug_poison_lds(0) == 0
    y1 = p.solve(b[:, 0], trans="T")
    assert np.abs(y1 - x1[:, 0]).max() / np.abs(x1).max() <= BITS[0]


def test_solve_t_refusals_in_process():
    A = unsym_stencil(STENCIL_3D7, (6, 6, 6), 0)
    S = Symbolic(A, nd_order(6, 6, 6), 60, 256)
    p = Plan(S.distribute())
    p.upload()
    b = np.ones(A.n)
    with pytest.raises(RuntimeError, match="factor first"):
        p.solve(b, trans="T")
    with pytest.raises(RuntimeError, match="factor first"):
        p.rcond(14.0)
    assert p.factor(14.0) == (0, 0)
    with pytest.raises(RuntimeError, match="trans = 7"):
        p.solve(b, trans=7)
    with pytest.raises(RuntimeError, match="trans = -1"):
        p.refine(b, b, trans=-1)
    with pytest.raises(ValueError, match="trans"):
        p.solve(b, trans="X")
    with pytest.raises(RuntimeError, match="fill_a"):   # factors of values the plan never saw
        p.refine(b, b, trans="T")
    with pytest.raises(ValueError, match="norm"):
        p.rcond(14.0, norm="F")
    x = p.solve(b, trans="T")  # the plan still works
    assert np.isfinite(x).all()


@pytest.mark.parametrize("pr,pc,pz,word", [(2, 2, 1, "2x2 grid"), (1, 1, 2, "3D")])
def test_solve_t_refused_on_grids(pr, pc, pz, word, tmp_path):
    """2x2 over the host p2p transport and a 3D plan: solve_t, refine_t and
    rcond raise with the message on every rank, nothing hangs or crashes,
    and the 2D plan's own solve still works afterwards."""
    from gridrun_t import run_grid_t
    out = run_grid_t(pr, pc, pz, tmp_path)
    assert len(out) == pr * pc * pz
    for o in out:
        assert int(o["info"]) == 0
        for what in ("solve", "refine", "rcond"):
            assert word in str(o[what]) and "1x1" in str(o[what]), (what, str(o[what]))
        if pz == 1:
            assert 0 <= float(o["resid"]) < 1e-12


def test_solve_t_empty_rhs():
    p, lu, (cp, ri, v) = factored(STENCIL_3D7, (6, 6, 6), 0, 60, 256)
    x = p.solve(np.zeros((len(cp) - 1, 0)), trans="T")
    assert x.shape == (len(cp) - 1, 0)
