"""Block solve for many right-hand sides on the device factors
(slu_plan_solve_block; csrc/solve_block.h k_svb_ldiag / k_svb_lpanel /
k_svb_upanel / k_svb_udiag on MFMA, 32 columns per pass over the factors, 16
in complex).

Checker: the host supernodal solve of tests/lusolve.py on the same
downloaded factors, column by column, at the tolerances of
tests/test_gpu_solve.py (only the summation order differs from
slu_plan_solve): normwise 1e-12 fp64 / complex and 1e-4 fp32, backward error
below 1e-14 / 1e-5.  Every numbered case also compares solve_block with
Plan.solve on the same b at the normwise tolerance.  A case's matrix is
factored once and its reference solutions are computed once; the tests that
share a case take leading columns of the same b.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from lusolve import lu_coords_matrix, solve_1x1
from refdump import Fixture, names
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_2D5, STENCIL_3D7, STENCIL_3D27, Csc, Symbolic, nd_order
from superlu_dist_amd.lib import lib

pytestmark = pytest.mark.gpu

TOL = {0: 1e-12, 1: 1e-4, 2: 1e-12}
BTOL = {0: 1e-14, 1: 1e-5, 2: 1e-14}
DT = {0: np.float64, 1: np.float32, 2: np.complex128}
SVB_NR = {0: 32, 1: 32, 2: 16}

NARROW = (STENCIL_3D7, (16, 16, 16), 0, 4, 24)   # K below a fragment, w % 4 != 0, many levels
WIDE = (STENCIL_3D7, (20, 20, 20), 0, 60, 320)   # supernodes wider than 256


@functools.lru_cache(maxsize=None)
def factored(kind, dims, dtype, relax, maxsup):
    """(plan with the factors on the device, lu with them downloaded, B as scipy CSC)"""
    kw = dict(diag=6 - 0.25, diag_im=-0.0025) if dtype == 2 else {}
    A = Csc.stencil(kind, *dims, dtype=dtype, **kw)
    S = Symbolic(A, nd_order(*dims), relax, maxsup)
    lu = S.distribute()
    p = Plan(lu)
    p.upload()
    assert p.factor(12.0) == (0, 0)
    p.download()
    cp, ri, v = A.permuted(S.perm_c).arrays()
    return p, lu, sp.csc_matrix((v, ri, cp), shape=(A.n, A.n))


@functools.lru_cache(maxsize=None)
def reference(case, ncols):
    """(b, host solutions) of `ncols` right-hand sides of a case: computed once."""
    p, lu, B = factored(*case)
    dtype = case[2]
    rng = np.random.default_rng(7)
    xt = rng.standard_normal((B.shape[0], ncols))
    if dtype == 2:
        xt = xt + 1j * rng.standard_normal((B.shape[0], ncols))
    b = np.asfortranarray((B @ xt).astype(DT[dtype]))
    xh = np.stack([solve_1x1(lu, b[:, r]) for r in range(ncols)], axis=1)
    b.setflags(write=False)
    xh.setflags(write=False)
    return b, xh


def backward_errors(B, x, b):
    """lusolve.backward_error per column: ||B x - b|| / (||B|| ||x||), inf norms."""
    r = np.abs(B @ x - b).max(axis=0)
    return r / (abs(B).sum(axis=1).max() * np.abs(x).max(axis=0))


def check(case, nrhs, ncols, x=None):
    """solve_block on the first nrhs of the case's ncols reference columns."""
    p, lu, B = factored(*case)
    dtype = case[2]
    bf, xhf = reference(case, ncols)
    b, xh = np.asfortranarray(bf[:, :nrhs]), xhf[:, :nrhs]
    if x is None:
        x = p.solve_block(b)
    assert x.shape == b.shape and x.dtype == DT[dtype]
    nx = np.abs(xh).max(axis=0)
    err = np.abs(x - xh).max(axis=0) / nx
    wide = np.complex128 if dtype == 2 else np.float64
    berr = backward_errors(B, x.astype(wide), b.astype(wide))
    xs = p.solve(b)
    dif = np.abs(x - xs).max(axis=0) / np.abs(xs).max(axis=0)
    print(f"nrhs {nrhs}: err {err.max():.3e} berr {berr.max():.3e} against solve {dif.max():.3e}")
    assert np.isfinite(x).all()
    assert (err < TOL[dtype]).all(), err
    assert (berr < BTOL[dtype]).all(), berr
    assert (dif < TOL[dtype]).all(), dif
    return x


# 1. shapes: (case, nrhs, columns of the case's shared reference)
SMALL = (STENCIL_3D7, (12, 12, 12), 0, 60, 256)
SHAPES = [(SMALL, k, 70) for k in (1, 31, 32, 33, 70)] + [   # one pass, an exact pass, tails
    (NARROW, 33, 33),
    (WIDE, 5, 33),
    # the last 32- / 16-column panel of the widest supernodes starts mid-wave (width 300 / 100)
    ((STENCIL_3D7, (20, 20, 20), 1, 60, 300), 17, 17),
    ((STENCIL_3D7, (20, 20, 20), 2, 60, 300), 17, 17),
    ((STENCIL_2D5, (40, 40, 1), 0, 60, 256), 32, 32),
    ((STENCIL_3D27, (8, 8, 8), 1, 60, 256), 40, 40),
] + [((STENCIL_3D7, (8, 8, 8), 2, 60, 256), k, 35) for k in (16, 17, 35)]  # the complex pass is 16 wide


@pytest.mark.parametrize("case,nrhs,ncols", SHAPES)
def test_solve_block_matches_host_solve(case, nrhs, ncols):
    check(case, nrhs, ncols)
    p = factored(*case)[0]
    assert p.stats()["t_solve_ms"] > 0


def test_solve_block_vector_rhs():
    """b of shape (n,) comes back as (n,), as from Plan.solve."""
    p, lu, B = factored(*SMALL)
    bf, xhf = reference(SMALL, 70)
    x = p.solve_block(np.array(bf[:, 0]))
    assert x.shape == (B.shape[0],)
    assert np.abs(x - xhf[:, 0]).max() / np.abs(xhf[:, 0]).max() < TOL[0]


# 2. skyline U segments and MC64 permutations: the reference's own LUstructs
REF_CASES = [n for n in names() if "_1x1_" in n and not n.startswith("zeropiv") and n[-1] in "dz"]
EPS = {0: 2.2e-16, 1: 1.2e-7, 2: 2.2e-16}


@pytest.mark.parametrize("name", REF_CASES)
def test_solve_block_on_reference_lustructs(name):
    """fill_a, factor, solve_block of 33 columns in LU coordinates against an
    independent fp64 sparse solve of B by scipy.  Tolerance as in
    tests/test_gpu_solve_trans.py: max(10 x scipy's own error against the
    generated solution, 50 eps), and for tinypiv (factors of a perturbed B)
    10 x the error the reference's own solve has on its factors."""
    from test_lusolve_t import factor_error
    fx = Fixture(name)
    lu = fx.lu(0, "pre")
    p = Plan(lu, replace_tiny=fx.replace_tiny)
    cp, ri, v = lu_coords_matrix(fx)
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(fx.anorm) == (fx.info, fx.tiny)
    wide = np.complex128 if fx.dtype == 2 else np.float64
    B = sp.csc_matrix((v.astype(wide), ri, cp), shape=(fx.n, fx.n))
    rng = np.random.default_rng(3)
    yt = rng.standard_normal((fx.n, 33))
    if fx.dtype == 2:
        yt = yt + 1j * rng.standard_normal((fx.n, 33))
    c = B @ yt
    ys = spla.splu(B).solve(c)
    y = p.solve_block(c.astype(lu.Lval.dtype))
    ny = np.abs(ys).max(axis=0)
    d = (np.abs(y - ys).max(axis=0) / ny).max()
    tol = max(10 * (np.abs(ys - yt).max(axis=0) / ny).max(), 50 * EPS[fx.dtype])
    if fx.tiny:
        tol = max(tol, 10 * factor_error(fx))
    yv = p.solve(c.astype(lu.Lval.dtype))
    dv = (np.abs(y - yv).max(axis=0) / np.abs(yv).max(axis=0)).max()
    print(f"{name}: {d:.3e} (tol {tol:.3e}), against solve {dv:.3e}")
    assert d < tol, (d, tol)
    assert dv < max(TOL[fx.dtype], tol)


# 3. untouched memory
@pytest.mark.parametrize("nrhs", [5, 33])
def test_solve_block_leaves_the_rest_of_b_alone(nrhs):
    """b inside an (n + 7) x (nrhs + 3) array of sentinels, ldb = n + 7: the
    extra rows and columns are bit-identical afterwards."""
    import ctypes as C
    p, lu, B = factored(*SMALL)
    n = B.shape[0]
    bf, _ = reference(SMALL, 70)
    sent = np.float64(-7.25e300)
    big = np.full((n + 7, nrhs + 3), sent, order="F")
    big[:n, :nrhs] = bf[:, :nrhs]
    assert lib().slu_plan_solve_block(p.ptr, big.ctypes.data_as(C.c_void_p), n + 7, nrhs, 0) == 0
    assert (big[n:, :].view(np.uint64) == sent.view(np.uint64)).all()
    assert (big[:, nrhs:].view(np.uint64) == sent.view(np.uint64)).all()
    check(SMALL, nrhs, 70, x=np.asfortranarray(big[:n, :nrhs]))


def test_solve_block_empty_rhs():
    p, lu, B = factored(*SMALL)
    x = p.solve_block(np.zeros((B.shape[0], 0)))
    assert x.shape == (B.shape[0], 0)
    assert p.solve_block_info()[0] == 0


# 4. the coarse plan
@pytest.mark.parametrize("amalg", [False, True])
def test_solve_block_plain_and_coarse_plan(amalg, monkeypatch):
    """The engine-side amalgamated plan of a reference-partition LUstruct
    forwards solve_block to its coarse plan, as it forwards solve."""
    from lusolve_t import unsym_stencil
    monkeypatch.setenv("SLU_AMALG", "1" if amalg else "0")
    A = unsym_stencil(STENCIL_3D7, (12, 12, 12), 0)
    S = Symbolic(A, nd_order(12, 12, 12), 60, 256)
    lu = S.distribute()
    p = Plan(lu)
    p.upload()
    assert p.factor(14.0) == (0, 0)
    p.download()
    assert (p.stats()["amalg_groups"] > 0) == amalg
    cp, ri, v = A.permuted(S.perm_c).arrays()
    B = sp.csc_matrix((v, ri, cp), shape=(A.n, A.n))
    b = np.asfortranarray(B @ np.random.default_rng(7).standard_normal((A.n, 33)))
    x = p.solve_block(b)
    assert p.solve_block_info()[0] == 2 and p.stats()["t_solve_ms"] == p.solve_block_info()[2] > 0
    xs = p.solve(b)
    for r in range(33):
        xh = solve_1x1(lu, b[:, r])
        assert np.abs(x[:, r] - xh).max() / np.abs(xh).max() < TOL[0]
        assert np.abs(x[:, r] - xs[:, r]).max() / np.abs(xs[:, r]).max() < TOL[0]
    assert (backward_errors(B, x, b) < BTOL[0]).all()


# 5. poisoned LDS
@pytest.mark.parametrize("case", [NARROW, WIDE], ids=["narrow16", "wide20"])
@pytest.mark.parametrize("nrhs", [1, 33])
def test_solve_block_does_not_read_stale_lds(case, nrhs):
    """NaN in every LDS word immediately before a solve_block (partial
    panels, partial strips and chunks, a partial last pass): finite and
    within tolerance."""
    p, lu, B = factored(*case)
    bf, _ = reference(case, 33)
    b = np.asfortranarray(bf[:, :nrhs])
    assert lib().slu_debug_poison_lds(0) == 0
    x = p.solve_block(b)
    assert np.isfinite(x).all()
    check(case, nrhs, 33, x=x)


# 6. device pointer
def test_solve_block_device_pointer(tmp_path):
    """A column-major torch tensor on the device with ldb > n through
    solve_block_dev, in a child process (torch brings its own HIP runtime,
    which has to be loaded before the engine).  The panel updates of
    different supernodes meet in X through atomics whose order is free, so
    two runs are not bit-identical at any shape with more than one
    contributor per row (two host runs in a row differ in the last bits as
    well): the comparison is at the normwise tolerance, against solve_block
    on the same host data and against the host solve.  The padding rows and
    the extra column of the tensor keep their sentinel."""
    from gridrun_block import run_device_pointer
    o = run_device_pointer(tmp_path)
    xh, xd, x1 = o["x_host"], o["x_dev"], o["x_host2"]
    assert xh.shape == xd.shape and np.isfinite(xd).all()
    nx = np.abs(xh).max(axis=0)
    print("device pointer against host b:", (np.abs(xd - xh).max(axis=0) / nx).max(),
          "host b twice:", (np.abs(x1 - xh).max(axis=0) / nx).max())
    assert (np.abs(xd - xh).max(axis=0) / nx < TOL[0]).all()
    assert (np.abs(x1 - xh).max(axis=0) / nx < TOL[0]).all()
    assert (np.abs(xd - o["x_ref"]).max(axis=0) / nx < TOL[0]).all()
    assert bool(o["sentinels_ok"])
    assert int(o["passes"]) == 2 and float(o["ms"]) > 0


# 7. info
@pytest.mark.parametrize("case", [SMALL, (STENCIL_3D27, (8, 8, 8), 1, 60, 256),
                                  (STENCIL_3D7, (8, 8, 8), 2, 60, 256)], ids=["d", "s", "z"])
@pytest.mark.parametrize("nrhs", [1, 32, 33, 70])
def test_solve_block_info(case, nrhs):
    p, lu, B = factored(*case)
    b = np.ones((B.shape[0], nrhs), dtype=DT[case[2]])
    p.solve_block(b)
    passes, launches, ms = p.solve_block_info()
    assert passes == -(-nrhs // SVB_NR[case[2]])
    assert launches > 0 and launches % passes == 0
    assert ms > 0 and ms == p.stats()["t_solve_ms"]


# 8. zero pivot
def test_solve_block_zero_pivot_is_not_hidden():
    """A singular U_kk (the zeropiv fixture, info > 0): the diagonal is
    divided, not multiplied by a reciprocal, so every column Plan.solve
    returns non-finite is non-finite from solve_block too."""
    name = next(n for n in names() if n.startswith("zeropiv") and "_1x1_" in n)
    fx = Fixture(name)
    p = Plan(fx.lu(0, "pre"), replace_tiny=fx.replace_tiny)
    p.upload()
    info, _ = p.factor(fx.anorm)
    assert info > 0 and info == fx.info
    b = np.random.default_rng(5).standard_normal((fx.n, 33))
    xs = p.solve(b)
    xb = p.solve_block(b)
    bad_s = ~np.isfinite(xs).all(axis=0)
    bad_b = ~np.isfinite(xb).all(axis=0)
    assert bad_s.any()
    assert (bad_b | ~bad_s).all(), (bad_s, bad_b)


# 9. refusals
def test_solve_block_refusals_in_process():
    import ctypes as C
    A = Csc.stencil(STENCIL_3D7, 6, 6, 6)
    S = Symbolic(A, nd_order(6, 6, 6), 60, 256)
    p = Plan(S.distribute())
    p.upload()
    b = np.ones((A.n, 3), order="F")
    keep = b.copy()
    with pytest.raises(RuntimeError, match="factor first"):
        p.solve_block(b)
    assert p.factor(12.0) == (0, 0)
    for ldb, nrhs in ((A.n - 1, 3), (A.n, -1)):
        assert lib().slu_plan_solve_block(p.ptr, b.ctypes.data_as(C.c_void_p), ldb, nrhs, 0) != 0
        assert "solve_block" in lib().slu_last_error().decode()
        assert (b == keep).all()
    x = p.solve_block(b)  # the plan still works
    assert np.isfinite(x).all() and (b == keep).all()


@pytest.mark.parametrize("pr,pc,pz,word", [(2, 2, 1, "2x2 grid"), (1, 1, 2, "3D")])
def test_solve_block_refused_on_grids(pr, pc, pz, word, tmp_path):
    """2x2 over the host p2p transport and a 3D plan: solve_block raises with
    the message on every rank before any device work and leaves b unchanged;
    the 2D plan's own solve still works afterwards."""
    from gridrun_block import run_grid_block
    out = run_grid_block(pr, pc, pz, tmp_path)
    assert len(out) == pr * pc * pz
    for o in out:
        assert int(o["info"]) == 0
        assert "solve_block" in str(o["msg"]) and word in str(o["msg"]) and "1x1" in str(o["msg"]), str(o["msg"])
        assert bool(o["b_unchanged"])
        if pz == 1:
            assert 0 <= float(o["resid"]) < 1e-12
