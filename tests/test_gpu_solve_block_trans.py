"""Block solve with the transpose for many right-hand sides
(slu_plan_solve_block_t; csrc/solve_block_t.h k_svb_utdiag / k_svb_utpanel /
k_svb_ltpanel / k_svb_ltdiag on MFMA).

Matrices: stencil patterns with unsymmetric values (lusolve_t.unsym_stencil)
under assert_unsymmetric, so a forwarder to the untransposed sweep cannot
pass.  Checker: the host transposed supernodal solve of tests/lusolve_t.py on
the same downloaded factors, column by column, at the tolerances of
tests/test_gpu_solve_block.py (normwise 1e-12 / 1e-4 / 1e-12, backward error
by backward_error_t 1e-14 / 1e-5 / 1e-14); every case also compares with
Plan.solve(b, trans=...) at the normwise tolerance and must be farther than
1e-3 from Plan.solve_block(b).  A case's matrix is factored once and its
reference solutions are computed once per operation.
"""
import ctypes as C
import functools

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
from test_gpu_solve_block import BTOL, DT, SVB_NR, TOL
from test_gpu_solve_trans import BITS, assert_unsymmetric

pytestmark = pytest.mark.gpu

SMALL = (STENCIL_3D7, (12, 12, 12), 0, 60, 256)
NARROW = (STENCIL_3D7, (16, 16, 16), 0, 4, 24)   # K below a fragment, w % 4 != 0, many levels
WIDE = (STENCIL_3D7, (20, 20, 20), 0, 60, 320)   # supernodes wider than 256
MID_S = (STENCIL_3D7, (20, 20, 20), 1, 60, 300)  # the last panel of the widest supernodes starts mid-wave
MID_Z = (STENCIL_3D7, (20, 20, 20), 2, 60, 300)
Z8 = (STENCIL_3D7, (8, 8, 8), 2, 60, 256)


@functools.lru_cache(maxsize=None)
def factored(kind, dims, dtype, relax, maxsup):
    """(plan with the factors on the device, lu with them downloaded, B's CSC arrays)"""
    A = unsym_stencil(kind, dims, dtype)
    S = Symbolic(A, nd_order(*dims), relax, maxsup)
    lu = S.distribute()
    p = Plan(lu)
    p.upload()
    assert p.factor(28.0 if kind == STENCIL_3D27 else 14.0) == (0, 0)
    p.download()
    cp, ri, v = A.permuted(S.perm_c).arrays()
    assert_unsymmetric(cp, ri, v)
    return p, lu, (cp, ri, v)


@functools.lru_cache(maxsize=None)
def reference(case, trans, ncols):
    """(b, host solutions) of `ncols` right-hand sides of op(B)^T x = b: computed once."""
    p, lu, (cp, ri, v) = factored(*case)
    dtype, conj = case[2], trans == "C"
    rng = np.random.default_rng(7)
    n = len(cp) - 1
    xt = rng.standard_normal((n, ncols))
    if dtype == 2:
        xt = xt + 1j * rng.standard_normal((n, ncols))
    b = np.asfortranarray((op_t(cp, ri, v, conj) @ xt).astype(DT[dtype]))
    xh = np.stack([solve_1x1_t(lu, b[:, r], conj) for r in range(ncols)], axis=1)
    b.setflags(write=False)
    xh.setflags(write=False)
    return b, xh


def colrel(x, y):
    return np.abs(x - y).max(axis=0) / np.abs(y).max(axis=0)


def check(case, trans, nrhs, ncols, x=None):
    """solve_block(trans) on the first nrhs of the case's ncols reference columns."""
    p, lu, (cp, ri, v) = factored(*case)
    dtype, conj = case[2], trans == "C"
    bf, xhf = reference(case, trans, ncols)
    b, xh = np.asfortranarray(bf[:, :nrhs]), xhf[:, :nrhs]
    if x is None:
        x = p.solve_block(b, trans=trans)
    assert x.shape == b.shape and x.dtype == DT[dtype]
    assert np.isfinite(x).all()
    err = colrel(x, xh)
    berr = np.array([backward_error_t(cp, ri, v, x[:, r].astype(xh.dtype), b[:, r].astype(xh.dtype), conj)
                     for r in range(nrhs)])
    dif = colrel(x, p.solve(b, trans=trans))
    far = colrel(x, p.solve_block(b))
    print(f"{trans} nrhs {nrhs}: err {err.max():.3e} berr {berr.max():.3e} against solve_t {dif.max():.3e} "
          f"from solve_block {far.min():.3e}")
    assert (err < TOL[dtype]).all(), err
    assert (berr < BTOL[dtype]).all(), berr
    assert (dif < TOL[dtype]).all(), dif
    assert (far > 1e-3).all(), far  # a forwarder to the untransposed sweep fails this
    return x


# 1. shapes: (case, trans, nrhs, columns of the case's shared reference)
SHAPES = [(SMALL, "T", k, 70) for k in (1, 31, 32, 33, 70)] + [   # one pass, an exact pass, tails
    (NARROW, "T", 33, 33),
    (WIDE, "T", 5, 33),
    (MID_S, "T", 17, 17),
    (MID_Z, "C", 17, 17),
    ((STENCIL_2D5, (40, 40, 1), 0, 60, 256), "T", 32, 32),
    ((STENCIL_3D27, (8, 8, 8), 1, 60, 256), "T", 40, 40),
] + [(Z8, tr, k, 35) for tr in ("T", "C") for k in (16, 17, 35)]  # the complex pass is 16 wide


@pytest.mark.parametrize("case,trans,nrhs,ncols", SHAPES)
def test_solve_block_t_matches_host_solve(case, trans, nrhs, ncols):
    x = check(case, trans, nrhs, ncols)
    p = factored(*case)[0]
    assert p.stats()["t_solve_ms"] > 0
    if case[2] == 2:  # B^H is not B^T
        other = p.solve_block(np.asfortranarray(reference(case, trans, ncols)[0][:, :nrhs]),
                              trans="T" if trans == "C" else "C")
        assert (colrel(other, x) > 1e-3).all()


@pytest.mark.parametrize("case", [SMALL, (STENCIL_3D27, (8, 8, 8), 1, 60, 256), Z8], ids=["d", "s", "z"])
def test_solve_block_t_same_codes(case):
    """trans="N" and trans=0 are solve_block(b); SLU_CONJ on a real plan is
    SLU_TRANS: to the atomics' last bits."""
    p = factored(*case)[0]
    dtype = case[2]
    nrhs = SVB_NR[dtype] + 1
    b = np.asfortranarray(reference(case, "T", 70 if case == SMALL else 35 if case == Z8 else 40)[0][:, :nrhs])
    xn = p.solve_block(b)
    for tn in ("N", 0):
        assert colrel(p.solve_block(b, trans=tn), xn).max() <= BITS[dtype]
    if dtype != 2:
        assert colrel(p.solve_block(b, trans="C"), p.solve_block(b, trans="T")).max() <= BITS[dtype]
        assert colrel(p.solve_block(b, trans=2), p.solve_block(b, trans=1)).max() <= BITS[dtype]


# 2. skyline U segments and MC64 permutations: the reference's own LUstructs
REF_CASES = [n for n in names() if "_1x1_" in n and not n.startswith("zeropiv")]
EPS = {0: 2.2e-16, 1: 1.2e-7, 2: 2.2e-16}


@pytest.mark.parametrize("name,trans", [(n, "T") for n in REF_CASES] +
                         [(n, "C") for n in REF_CASES if n.startswith("cg20")])
def test_solve_block_t_on_reference_lustructs(name, trans):
    """fill_a, factor, solve_block(trans) of 33 columns in LU coordinates
    against an independent fp64 sparse solve of op(B)^T by scipy; tolerance
    of test_solve_t_on_reference_lustructs: max(10 x scipy's own error
    against the generated solution, 50 eps), and for tinypiv 10 x the error
    the reference's own solve has on its factors."""
    from test_lusolve_t import factor_error
    fx = Fixture(name)
    lu = fx.lu(0, "pre")
    p = Plan(lu, replace_tiny=fx.replace_tiny)
    cp, ri, v = lu_coords_matrix(fx)
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(fx.anorm) == (fx.info, fx.tiny)
    wide = np.complex128 if fx.dtype == 2 else np.float64
    Bt = op_t(cp, ri, v.astype(wide), trans == "C")
    rng = np.random.default_rng(3)
    yt = rng.standard_normal((fx.n, 33))
    if fx.dtype == 2:
        yt = yt + 1j * rng.standard_normal((fx.n, 33))
    c = Bt @ yt
    ys = spla.splu(sp.csc_matrix(Bt)).solve(c)
    y = p.solve_block(c.astype(lu.Lval.dtype), trans=trans)
    ny = np.abs(ys).max(axis=0)
    d = (np.abs(y - ys).max(axis=0) / ny).max()
    tol = max(10 * (np.abs(ys - yt).max(axis=0) / ny).max(), 50 * EPS[fx.dtype])
    if fx.tiny:
        tol = max(tol, 10 * factor_error(fx))
    print(f"{name} {trans}: {d:.3e} (tol {tol:.3e})")
    assert d < tol, (d, tol)


# 3. untouched memory
@pytest.mark.parametrize("nrhs", [5, 33])
def test_solve_block_t_leaves_the_rest_of_b_alone(nrhs):
    """b inside an (n + 7) x (nrhs + 3) array of sentinels, ldb = n + 7."""
    p, lu, (cp, ri, v) = factored(*SMALL)
    n = len(cp) - 1
    bf, _ = reference(SMALL, "T", 70)
    sent = np.float64(-7.25e300)
    big = np.full((n + 7, nrhs + 3), sent, order="F")
    big[:n, :nrhs] = bf[:, :nrhs]
    assert lib().slu_plan_solve_block_t(p.ptr, 1, big.ctypes.data_as(C.c_void_p), n + 7, nrhs, 0) == 0
    assert (big[n:, :].view(np.uint64) == sent.view(np.uint64)).all()
    assert (big[:, nrhs:].view(np.uint64) == sent.view(np.uint64)).all()
    check(SMALL, "T", nrhs, 70, x=np.asfortranarray(big[:n, :nrhs]))


def test_solve_block_t_empty_and_vector_rhs():
    p, lu, (cp, ri, v) = factored(*SMALL)
    n = len(cp) - 1
    x = p.solve_block(np.zeros((n, 0)), trans="T")
    assert x.shape == (n, 0) and p.solve_block_info()[0] == 0
    bf, xhf = reference(SMALL, "T", 70)
    x = p.solve_block(np.array(bf[:, 0]), trans="T")
    assert x.shape == (n,)
    assert np.abs(x - xhf[:, 0]).max() / np.abs(xhf[:, 0]).max() < TOL[0]


# 4. the coarse plan
@pytest.mark.parametrize("amalg", [False, True])
def test_solve_block_t_plain_and_coarse_plan(amalg, monkeypatch):
    monkeypatch.setenv("SLU_AMALG", "1" if amalg else "0")
    p, lu, (cp, ri, v) = factored.__wrapped__(*SMALL)
    assert (p.stats()["amalg_groups"] > 0) == amalg
    bf, _ = reference(SMALL, "T", 70)
    b = np.asfortranarray(bf[:, :33])
    x = p.solve_block(b, trans="T")
    assert p.solve_block_info()[0] == 2 and p.stats()["t_solve_ms"] == p.solve_block_info()[2] > 0
    xs = p.solve(b, trans="T")
    for r in range(33):
        xh = solve_1x1_t(lu, b[:, r])
        assert np.abs(x[:, r] - xh).max() / np.abs(xh).max() < TOL[0]
        assert np.abs(x[:, r] - xs[:, r]).max() / np.abs(xs[:, r]).max() < TOL[0]
        assert backward_error_t(cp, ri, v, x[:, r], b[:, r]) < BTOL[0]


# 5. poisoned LDS
@pytest.mark.parametrize("case", [NARROW, WIDE], ids=["narrow16", "wide20"])
@pytest.mark.parametrize("nrhs", [1, 33])
def test_solve_block_t_does_not_read_stale_lds(case, nrhs):
    """NaN in every LDS word immediately before a call (partial panels,
    partial strips and chunks, a partial last pass)."""
    p = factored(*case)[0]
    bf, _ = reference(case, "T", 33)
    assert lib().slu_debug_poison_lds(0) == 0
    x = p.solve_block(np.asfortranarray(bf[:, :nrhs]), trans="T")
    assert np.isfinite(x).all()
    check(case, "T", nrhs, 33, x=x)


# 6. device pointer
def test_solve_block_t_device_pointer():
    """A column-major torch tensor on the device with ldb > n through
    solve_block_dev(..., trans="T") in a child process, at the normwise
    tolerance (the atomics' order is free)."""
    from gridrun_block_t import run_device_pointer_t
    o = run_device_pointer_t()
    xh, xd = o["x_host"], o["x_dev"]
    assert xh.shape == xd.shape and np.isfinite(xd).all()
    assert (colrel(xd, xh) < TOL[0]).all()
    assert (colrel(xd, o["x_ref"]) < TOL[0]).all()
    assert bool(o["sentinels_ok"])
    assert int(o["passes"]) == 2 and float(o["ms"]) > 0


# 7. info
@pytest.mark.parametrize("case", [SMALL, (STENCIL_3D27, (8, 8, 8), 1, 60, 256), Z8], ids=["d", "s", "z"])
@pytest.mark.parametrize("nrhs", [1, 33, 70])
def test_solve_block_t_info(case, nrhs):
    """passes = ceil(nrhs / SVB_NR); as many launches as the untransposed call
    on the same plan (same levels, same chunk lists)."""
    p = factored(*case)[0]
    n = len(factored(*case)[2][0]) - 1
    b = np.ones((n, nrhs), dtype=DT[case[2]])
    p.solve_block(b)
    ref = p.solve_block_info()
    p.solve_block(b, trans="T")
    passes, launches, ms = p.solve_block_info()
    assert passes == -(-nrhs // SVB_NR[case[2]]) == ref[0]
    assert launches == ref[1] > 0
    assert ms > 0 and ms == p.stats()["t_solve_ms"]


# 8. zero pivot
def test_solve_block_t_zero_pivot_is_not_hidden():
    """A singular U_kk (the zeropiv fixture, info > 0): the diagonal is
    divided, so the columns solve(trans="T") returns non-finite are
    non-finite from solve_block(trans="T") too, and the call is no error."""
    name = next(n for n in names() if n.startswith("zeropiv") and "_1x1_" in n)
    fx = Fixture(name)
    p = Plan(fx.lu(0, "pre"), replace_tiny=fx.replace_tiny)
    p.upload()
    info, _ = p.factor(fx.anorm)
    assert info > 0 and info == fx.info
    b = np.random.default_rng(5).standard_normal((fx.n, 33))
    xs = p.solve(b, trans="T")
    xb = p.solve_block(b, trans="T")
    bad_s = ~np.isfinite(xs).all(axis=0)
    bad_b = ~np.isfinite(xb).all(axis=0)
    assert bad_s.any()
    assert (bad_b == bad_s).all(), (bad_s, bad_b)


# 9. refusals
def test_solve_block_t_refusals_in_process():
    A = unsym_stencil(STENCIL_3D7, (6, 6, 6), 0)
    S = Symbolic(A, nd_order(6, 6, 6), 60, 256)
    p = Plan(S.distribute())
    p.upload()
    b = np.ones((A.n, 3), order="F")
    keep = b.copy()
    with pytest.raises(RuntimeError, match="solve_block_t.*factor first"):
        p.solve_block(b, trans="T")
    assert p.factor(14.0) == (0, 0)
    for trans, ldb, nrhs in ((1, A.n - 1, 3), (2, A.n, -1), (3, A.n, 3), (-1, A.n, 3)):
        assert lib().slu_plan_solve_block_t(p.ptr, trans, b.ctypes.data_as(C.c_void_p), ldb, nrhs, 0) != 0
        assert "solve_block_t" in lib().slu_last_error().decode()
        assert (b == keep).all()
    with pytest.raises(RuntimeError, match="trans = 7"):
        p.solve_block(b, trans=7)
    with pytest.raises(ValueError, match="trans"):
        p.solve_block(b, trans="X")
    x = p.solve_block(b, trans="T")  # the plan still works
    assert np.isfinite(x).all() and (b == keep).all()


@pytest.mark.parametrize("pr,pc,pz,word", [(2, 2, 1, "2x2 grid"), (1, 1, 2, "3D")])
def test_block_t_refused_on_grids(pr, pc, pz, word, tmp_path):
    """2x2 over the host p2p transport and a 3D plan: solve_block_t and
    refine_block_t raise in the words of the block sweep on every rank before
    any device work and leave b and x unchanged; the 2D plan's own solve still
    works afterwards."""
    from gridrun_block_t import run_grid_block_t
    out = run_grid_block_t(pr, pc, pz, tmp_path)
    assert len(out) == pr * pc * pz
    for o in out:
        assert int(o["info"]) == 0
        for key, what in (("msg_solve", "solve_block_t"), ("msg_refine", "refine_block_t")):
            m = str(o[key])
            assert what in m and word in m and "1x1" in m and "block sweep" in m, m
        assert bool(o["unchanged"])
        if pz == 1:
            assert 0 <= float(o["resid"]) < 1e-12


# 10. the tables do not depend on the first caller
def test_solve_block_t_as_the_first_solve_call():
    """solve_block(trans="T") builds the tables when it is the plan's first
    solve call; every later call agrees with a plan whose first call was solve."""
    p1 = factored.__wrapped__(STENCIL_3D7, (6, 6, 6), 0, 60, 256)[0]
    p2, lu, (cp, ri, v) = factored.__wrapped__(STENCIL_3D7, (6, 6, 6), 0, 60, 256)
    n = len(cp) - 1
    b = np.asfortranarray(op_t(cp, ri, v) @ np.random.default_rng(3).standard_normal((n, 33)))
    xt1 = p1.solve_block(b, trans="T")
    p2.solve(b[:, 0])
    xt2 = p2.solve_block(b, trans="T")
    assert colrel(xt1, xt2).max() <= BITS[0]
    for r in (0, 32):
        xh = solve_1x1_t(lu, b[:, r])
        assert np.abs(xt1[:, r] - xh).max() / np.abs(xh).max() < TOL[0]
    assert colrel(p1.solve(b), p2.solve(b)).max() <= BITS[0]
    assert colrel(p1.solve_block(b), p2.solve_block(b)).max() <= BITS[0]
    assert colrel(p1.solve(b, trans="T"), xt1).max() < TOL[0]
