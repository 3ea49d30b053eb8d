"""Block iterative refinement for many right-hand sides
(slu_plan_refine_block / slu_plan_refine_block_d2; csrc/refine_block.h
k_rfb_resid, k_rfb_mask, k_rfb_axpy, k_rfb_scale_cvt_d2, k_rfb_axpy_d2 around
the block sweep of csrc/solve_block.h: 32 columns per pass, 16 in complex).

Checkers, imported from the per-column tests: the numpy restatements of the
loop (test_gpu_refine._host_refine, test_gpu_refine_d2.host_refine_d2 with
check_column) on the downloaded factors, and the backward error of the
returned x recomputed in extended precision (test_gpu_refine._berr).
Tolerances are those of test_device_refine_matches_host_loop and
check_column: x within 1e-12 (1e-5 in fp32) of the host loop's, steps within
one of it, berr <= 8 eps (1e-6 in fp32), |berr - _berr(x)| <=
2 (max row nnz + 1) eps.  Each system is factored once per module and its
host references are computed once.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from gridrun_d2 import system
from lusolve import solve_1x1  # noqa: F401  (the host sweep behind the imported checkers)
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, STENCIL_3D27, Csc, Symbolic, nd_order
from superlu_dist_amd.lib import lib
from test_gpu_refine import _berr, _host_refine
from test_gpu_refine_d2 import check_column

pytestmark = pytest.mark.gpu

EPS = {0: 2.0 ** -53, 1: 2.0 ** -24, 2: 2.0 ** -53}
DT = {0: np.float64, 1: np.float32, 2: np.complex128}
SVB_NR = {0: 32, 1: 32, 2: 16}
XTOL = {0: 1e-12, 1: 1e-5, 2: 1e-12}
BMAX = {0: 8 * EPS[0], 1: 1e-6, 2: 8 * EPS[2]}

# n = 729: neither 8 nor 16 rows per workgroup of the residual divide it
CASES = {"d": (STENCIL_3D7, (9, 9, 9), 0), "s": (STENCIL_3D27, (8, 8, 8), 1), "z": (STENCIL_3D7, (8, 8, 8), 2),
         "f": (STENCIL_3D7, (3, 5, 5), 0)}  # the frozen-column test's: n = 75
NCOL = {"d": 33, "s": 33, "z": 17}


def make_plan(kind, dims, dtype):
    """(plan with factors of fill_a's values, lu with them downloaded, (cp, ri, v))"""
    kw = dict(diag=6 - 0.25, diag_im=-0.0025) if dtype == 2 else {}  # test_gpu_refine's complex diagonal
    A = Csc.stencil(kind, *dims, dtype=dtype, **kw)
    S = Symbolic(A, nd_order(*dims), 60, 256)
    lu = S.distribute()
    p = Plan(lu)
    cp, ri, v = A.permuted(S.perm_c).arrays()
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(12.0)[0] == 0
    p.download()
    return p, lu, (cp, ri, v)


def rhs(cp, ri, v, dtype, ncols, seed=11):
    n = len(cp) - 1
    rng = np.random.default_rng(seed)
    xt = rng.standard_normal((n, ncols))
    if dtype == 2:
        xt = xt + 1j * rng.standard_normal((n, ncols))
    return np.asfortranarray((sp.csc_matrix((v, ri, cp), shape=(n, n)) @ xt).astype(DT[dtype]))


@functools.lru_cache(maxsize=None)
def factored(key):
    return make_plan(*CASES[key])


@functools.lru_cache(maxsize=None)
def reference(key):
    """(b, x0 = solve_block(b), the host loop's (x, steps) per column from x0): computed once."""
    p, lu, (cp, ri, v) = factored(key)
    dtype = CASES[key][2]
    b = rhs(cp, ri, v, dtype, NCOL[key])
    x0 = p.solve_block(b)
    host = [_host_refine(lu, cp, ri, v, b[:, j], x0[:, j].copy(), EPS[dtype]) for j in range(b.shape[1])]
    xh = np.stack([h[0] for h in host], axis=1)
    sh = np.array([h[2] for h in host])
    for a in (b, x0, xh, sh):
        a.setflags(write=False)
    return b, x0, xh, sh


def check_columns(cp, ri, v, dtype, b, x, berr, steps, xh, sh, cols=None):
    """test 1's bounds on the columns `cols` of a result"""
    tol_b = 2 * (int(np.diff(cp).max()) + 1) * EPS[dtype]
    for j in range(b.shape[1]) if cols is None else cols:
        err = np.abs(x[:, j] - xh[:, j]).max() / np.abs(xh[:, j]).max()
        own = _berr(cp, ri, v, x[:, j], b[:, j])
        print(f"col {j}: steps {steps[j]} (host {sh[j]}) berr {berr[j]:.3e} (recomputed {own:.3e}) err {err:.3e}")
        assert np.isfinite(x[:, j]).all()
        assert err < XTOL[dtype], (j, err)
        assert abs(int(steps[j]) - int(sh[j])) <= 1, (j, steps[j], sh[j])
        assert berr[j] <= BMAX[dtype], (j, berr[j])
        assert abs(own - berr[j]) <= tol_b, (j, own, berr[j])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# 1. parity per column with the host loop and with refine
@pytest.mark.parametrize("key,nrhs", [(k, n) for k in "dsz"
                                      for n in ((15, 16, 17) if k == "z" else (1, 31, 32, 33))])
def test_refine_block_matches_host_loop_and_refine(key, nrhs):
    p, lu, (cp, ri, v) = factored(key)
    dtype = CASES[key][2]
    bf, x0f, xh, sh = reference(key)
    b, x0 = np.asfortranarray(bf[:, :nrhs]), np.asfortranarray(x0f[:, :nrhs])
    x, berr, steps = p.refine_block(b, x0)
    assert x.shape == b.shape and x.dtype == DT[dtype] and len(berr) == len(steps) == nrhs
    assert p.stats()["t_refine_ms"] > 0
    check_columns(cp, ri, v, dtype, b, x, berr, steps, xh, sh)
    xr, ber, str_ = p.refine(b, x0)
    dif = np.abs(x - xr).max(axis=0) / np.abs(xr).max(axis=0)
    print(f"against refine: {dif.max():.3e}, steps {steps} / {str_}")
    assert (dif < XTOL[dtype]).all(), dif
    assert (np.abs(steps.astype(int) - str_.astype(int)) <= 1).all()


# 2. frozen columns and mixed stopping times
def test_refine_block_freezes_stopped_columns():
    """One pass of 32 columns of four kinds, j % 4: (a) x0 = what a prior
    refine returned, (b) x0 = 0, (c) b = 0 and x0 = 0, (d) a NaN in x0.

    (a): a refine that ends because berr no longer halves returns an x whose
    berr is above eps = 1.1e-16 (1.2e-16 .. 2.1e-16 at 9^3, where the maximum
    runs over 729 rows), and a second refine of it starts over with lstres = 3
    and takes a step.  Only an x returned with berr <= eps takes none.  At
    3 x 5 x 5 (n = 75: ten workgroups of the residual, the last one partial)
    most refined columns end that way (164 of 256 on the MI355X), so the
    columns of kind (a) are the first 8 of 256 refined candidates whose
    reported berr is <= eps."""
    p, lu, (cp, ri, v) = factored("f")
    b = rhs(cp, ri, v, 0, 32)
    x0 = p.solve_block(b)
    ka, kb, kc, kd = (np.arange(k, 32, 4) for k in range(4))
    bc = rhs(cp, ri, v, 0, 256, seed=5)
    xc, bec, _ = p.refine(bc, p.solve_block(bc))
    sel = np.flatnonzero(bec <= EPS[0])[:8]
    print(f"{(bec <= EPS[0]).sum()} of 256 refined candidates have berr <= eps")
    assert len(sel) == 8
    b[:, ka] = bc[:, sel]
    x0[:, ka] = xc[:, sel]
    x0[:, kb] = 0.0
    b[:, kc] = 0.0
    x0[:, kc] = 0.0
    x0[5, kd] = np.nan
    _, be_ref, st_ref = p.refine(b[:, ka], x0[:, ka])  # the per-column call on the same x0
    assert (st_ref == 0).all() and (be_ref > 0).all()
    x, berr, steps = p.refine_block(b, x0)
    passes, sweeps, resids, ms = p.refine_block_info()
    print("steps", steps, "berr", berr)
    for j in range(32):
        if steps[j] == 0:
            assert np.array_equal(bits(x[:, j]), bits(x0[:, j])), j
    assert (steps[ka] == 0).all()
    assert np.array_equal(bits(berr[ka]), bits(be_ref)), (berr[ka], be_ref)
    assert (steps[kb] >= 1).all()
    assert (steps[kc] == 0).all() and (berr[kc] == 0).all() and (x[:, kc] == 0).all()
    assert (steps[kd] == 0).all() and not np.isfinite(berr[kd]).any()
    # the NaN columns leave the others finite and within test 1's bounds
    good = np.concatenate([ka, kb])
    host = {j: _host_refine(lu, cp, ri, v, b[:, j], x0[:, j].copy(), EPS[0]) for j in good}
    xh = np.stack([host[j][0] if j in host else x0[:, j] for j in range(32)], axis=1)
    sh = np.array([host[j][2] if j in host else 0 for j in range(32)])
    check_columns(cp, ri, v, 0, b, x, berr, steps, xh, sh, cols=good)
    assert passes == 1 and sweeps == steps.max() and resids == sweeps + 1


# 3. counters over several passes
@pytest.mark.parametrize("key,nrhs", [("d", 70), ("s", 70), ("z", 40)])
def test_refine_block_info_over_passes(key, nrhs):
    p, lu, (cp, ri, v) = factored(key)
    dtype = CASES[key][2]
    nrb = SVB_NR[dtype]
    b = rhs(cp, ri, v, dtype, nrhs, seed=3)
    x0 = p.solve_block(b)
    x0[:, 1::3] = 0  # mixed stopping times within every pass
    x, berr, steps = p.refine_block(b, x0)
    passes, sweeps, resids, ms = p.refine_block_info()
    assert (berr <= BMAX[dtype]).all()
    assert passes == -(-nrhs // nrb)
    assert sweeps == sum(int(steps[r0:r0 + nrb].max()) for r0 in range(0, nrhs, nrb)) and sweeps >= passes
    assert resids == sweeps + passes
    assert ms > 0 and ms == p.stats()["t_refine_ms"]


def test_refine_block_empty_and_vector_rhs():
    p, lu, (cp, ri, v) = factored("d")
    bf, x0f, xh, _ = reference("d")
    x, berr, steps = p.refine_block(np.zeros((len(cp) - 1, 0)), np.zeros((len(cp) - 1, 0)))
    assert x.shape == (len(cp) - 1, 0) and len(berr) == len(steps) == 0
    assert p.refine_block_info() == (0, 0, 0, 0.0)
    x, berr, steps = p.refine_block(np.array(bf[:, 0]), np.array(x0f[:, 0]))
    assert x.shape == (len(cp) - 1,) and len(berr) == 1
    assert np.abs(x - xh[:, 0]).max() / np.abs(xh[:, 0]).max() < XTOL[0]


# 4. d2 on fp32 plans
@functools.lru_cache(maxsize=None)
def d2_factored(kind, nx):
    A, S, (cp, ri, v), v64, b, xt = system(kind, nx, nrhs=33)
    lu = S.distribute()
    p = Plan(lu)
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v64)
    assert p.factor(12.0)[0] == 0
    p.download()
    return p, lu, (cp, ri, v64), b


@pytest.mark.parametrize("kind,nx", [(STENCIL_3D7, 10), (STENCIL_3D27, 8)])
def test_refine_block_d2_reaches_fp64_accuracy(kind, nx):
    """33 columns: x0 = 0 for the first 16, the widened fp32 solve_block for
    the rest; columns 1 and 2 are column 0's b times 2^40 and 2^-40, which
    only a per-column exponent brings through fp32's range together."""
    p, lu, (cp, ri, v64), bf = d2_factored(kind, nx)
    b = np.array(bf, order="F")
    b[:, 1] = np.ldexp(b[:, 0], 40)
    b[:, 2] = np.ldexp(b[:, 0], -40)
    x0 = p.solve_block(b.astype(np.float32)).astype(np.float64)
    x0[:, :16] = 0.0
    x, berr, steps = p.refine_block_d2(b, x0)
    assert x.dtype == np.float64 and x.shape == b.shape and p.stats()["t_refine_ms"] > 0
    print("steps", steps, "berr max", berr.max())
    for j in range(33):
        check_column(lu, cp, ri, v64, b[:, j], x0[:, j], x[:, j], berr[j], steps[j])
    for j, k in ((1, 40), (2, -40)):
        assert abs(int(steps[j]) - int(steps[0])) <= 1, steps[:3]
        assert np.abs(np.ldexp(x[:, j], -k) - x[:, 0]).max() / np.abs(x[:, 0]).max() <= 1e-12
    passes, sweeps, resids, ms = p.refine_block_info()
    assert passes == 2 and sweeps == steps[:32].max() + steps[32] and resids == sweeps + 2


def test_refine_block_d2_freezes_a_nan_column():
    p, lu, (cp, ri, v64), bf = d2_factored(STENCIL_3D7, 10)
    b = np.array(bf[:, :5], order="F")
    x0 = np.zeros_like(b)
    x0[5, 3] = np.nan
    x, berr, steps = p.refine_block_d2(b, x0)
    assert steps[3] == 0 and not np.isfinite(berr[3])
    assert np.array_equal(bits(x[:, 3]), bits(x0[:, 3]))
    for j in (0, 1, 2, 4):
        check_column(lu, cp, ri, v64, b[:, j], x0[:, j], x[:, j], berr[j], steps[j])


# 5. memory discipline
@pytest.mark.parametrize("nrhs", [5, 33])
def test_refine_block_leaves_the_rest_alone(nrhs):
    """b and x inside (n + 3) x (nrhs + 2) arrays of sentinels, ld = n + 3: the
    sentinels and all of b are bit-identical afterwards."""
    p, lu, (cp, ri, v) = factored("d")
    n = len(cp) - 1
    bf, x0f, xh, sh = reference("d")
    sent = np.float64(-7.25e300)
    bb = np.full((n + 3, nrhs + 2), sent, order="F")
    xx = np.full((n + 3, nrhs + 2), sent, order="F")
    bb[:n, :nrhs] = bf[:, :nrhs]
    xx[:n, :nrhs] = x0f[:, :nrhs]
    keep = bb.copy()
    berr, steps = np.zeros(nrhs), np.zeros(nrhs, dtype=np.int32)
    assert lib().slu_plan_refine_block(p.ptr, bb.ctypes.data_as(C.c_void_p), xx.ctypes.data_as(C.c_void_p),
                                       n + 3, nrhs, 0, berr.ctypes.data_as(C.POINTER(C.c_double)),
                                       steps.ctypes.data_as(C.POINTER(C.c_int))) == 0
    assert np.array_equal(bits(bb), bits(keep))
    assert (bits(xx[n:, :]) == sent.view(np.uint64)).all()
    assert (bits(xx[:, nrhs:]) == sent.view(np.uint64)).all()
    check_columns(cp, ri, v, 0, bf[:, :nrhs], xx[:n, :nrhs], berr, steps, xh, sh)


# 6. the coarse plan
@pytest.mark.parametrize("amalg", [False, True])
def test_refine_block_plain_and_coarse_plan(amalg, monkeypatch):
    """The engine-side amalgamated plan forwards refine_block and its
    counters to its coarse plan, as it forwards solve_block and refine."""
    monkeypatch.setenv("SLU_AMALG", "1" if amalg else "0")
    p, lu, (cp, ri, v) = make_plan(STENCIL_3D7, (10, 10, 10), 0)
    assert (p.stats()["amalg_groups"] > 0) == amalg
    b = rhs(cp, ri, v, 0, 33)
    x0 = p.solve_block(b)
    x0[:, ::2] = 0.0
    x, berr, steps = p.refine_block(b, x0)
    passes, sweeps, resids, ms = p.refine_block_info()
    assert passes == 2 and sweeps == steps[:32].max() + steps[32] and resids == sweeps + 2
    assert ms == p.stats()["t_refine_ms"] > 0
    host = [_host_refine(lu, cp, ri, v, b[:, j], x0[:, j].copy(), EPS[0]) for j in range(33)]
    check_columns(cp, ri, v, 0, b, x, berr, steps, np.stack([h[0] for h in host], axis=1),
                  np.array([h[2] for h in host]))


# 7. poisoned LDS
@pytest.mark.parametrize("key", ["d", "z"])
@pytest.mark.parametrize("nrhs", [1, 33])
def test_refine_block_does_not_read_stale_lds(key, nrhs):
    """NaN in every LDS word immediately before the call (a partial last
    workgroup of the residual, a partial last pass): results as in test 1."""
    p, lu, (cp, ri, v) = factored(key)
    dtype = CASES[key][2]
    nrhs = min(nrhs, NCOL[key])
    bf, x0f, xh, sh = reference(key)
    b, x0 = np.asfortranarray(bf[:, :nrhs]), np.asfortranarray(x0f[:, :nrhs])
    assert lib().slu_debug_poison_lds(0) == 0
    x, berr, steps = p.refine_block(b, x0)
    check_columns(cp, ri, v, dtype, b, x, berr, steps, xh, sh)


@pytest.mark.parametrize("nrhs", [1, 33])
def test_refine_block_d2_does_not_read_stale_lds(nrhs):
    p, lu, (cp, ri, v64), bf = d2_factored(STENCIL_3D27, 8)
    b = np.array(bf[:, :nrhs], order="F")
    x0 = np.zeros_like(b)
    assert lib().slu_debug_poison_lds(0) == 0
    x, berr, steps = p.refine_block_d2(b, x0)
    for j in range(nrhs):
        check_column(lu, cp, ri, v64, b[:, j], x0[:, j], x[:, j], berr[j], steps[j])


# 8. device pointers
def test_refine_block_device_pointers(tmp_path):
    """Column-major torch tensors on the device with ld > n, refined in place
    through refine_block_dev, fp64 and d2, in a child process (torch brings
    its own HIP runtime, which has to be loaded before the engine).  The
    sweep's atomics are unordered, so the comparison with the host-array call
    on the same data is at test 1's tolerance, not bit for bit.  b and the
    padding rows and the extra column of x keep their values."""
    from gridrun_refine_block import run_device_pointer
    o = run_device_pointer(tmp_path)
    for pre in ("", "d2_"):
        xh, xd = o[pre + "x_host"], o[pre + "x_dev"]
        assert xh.shape == xd.shape and np.isfinite(xd).all()
        dif = np.abs(xd - xh).max(axis=0) / np.abs(xh).max(axis=0)
        print(pre or "fp64", "device pointer against host arrays:", dif.max(), o[pre + "steps_dev"],
              o[pre + "steps_host"])
        assert (dif < XTOL[0]).all()
        assert (o[pre + "berr_dev"] <= BMAX[0]).all() and (o[pre + "berr_host"] <= BMAX[0]).all()
        assert (np.abs(o[pre + "steps_dev"].astype(int) - o[pre + "steps_host"].astype(int)) <= 1).all()
        assert bool(o[pre + "ok"])
    assert (o["steps_host"][::2] >= 1).all() and (o["d2_steps_host"] >= 1).all()
    assert int(o["info"][0]) == 2 and float(o["info"][3]) > 0


# 9. refusals
def small(dtype=0):
    A = Csc.stencil(STENCIL_3D7, 6, 6, 6, dtype=dtype)
    S = Symbolic(A, nd_order(6, 6, 6), 60, 256)
    return A, Plan(S.distribute()), A.permuted(S.perm_c).arrays()


def test_refine_block_refusals_in_process():
    A, p, (cp, ri, v) = small()
    n = A.n
    b, x = np.ones((n, 3), order="F"), np.zeros((n, 3), order="F")
    p.upload()
    with pytest.raises(RuntimeError, match="refine_block.*factor first"):
        p.refine_block(b, x)
    with pytest.raises(RuntimeError, match="refine_block_d2.*factor first"):
        p.refine_block_d2(b, x)
    assert p.factor(12.0) == (0, 0)
    with pytest.raises(RuntimeError, match="refine_block needs.*fill_a"):  # uploaded values: of no A
        p.refine_block(b, x)
    with pytest.raises(RuntimeError, match=r"refine_block_d2: fp32 plans only.*dtype is d"):
        p.refine_block_d2(b, x)
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    with pytest.raises(RuntimeError, match="refine_block.*factor first"):  # refilled, not factored
        p.refine_block(b, x)
    assert p.factor(12.0)[0] == 0
    keep = x.copy()
    args = (b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p))
    for ld, nrhs in ((n - 1, 3), (n, -1)):
        assert lib().slu_plan_refine_block(p.ptr, *args, ld, nrhs, 0, None, None) != 0
        msg = lib().slu_last_error().decode()
        assert "refine_block" in msg and "ld" in msg and "nrhs" in msg
        assert (x == keep).all() and (b == 1).all()
    x1, berr, _ = p.refine_block(b, x)  # the plan still works
    assert (berr <= BMAX[0]).all() and (b == 1).all()


def test_refine_block_d2_refusals_in_process():
    A, S, (cp, ri, v), v64, b, _ = system(STENCIL_3D7, 6, nrhs=3)
    p = Plan(S.distribute())
    x = np.zeros_like(b)
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(12.0)[0] == 0
    with pytest.raises(RuntimeError, match="refine_block_d2 needs.*fill_a_d2"):  # fp32 values: no fp64 A
        p.refine_block_d2(b, x)
    _, berr, _ = p.refine_block(b.astype(np.float32), x.astype(np.float32))
    assert (berr <= BMAX[1]).all()
    p.fill_a_d2(v64)
    with pytest.raises(RuntimeError, match="refine_block_d2.*factor first"):
        p.refine_block_d2(b, x)
    assert p.factor(12.0)[0] == 0
    with pytest.raises(RuntimeError, match="refine_block needs.*fill_a"):  # no fp32 A for the plain loop
        p.refine_block(b.astype(np.float32), x.astype(np.float32))
    args = (b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p))
    for ld, nrhs in ((A.n - 1, 3), (A.n, -1)):
        assert lib().slu_plan_refine_block_d2(p.ptr, *args, ld, nrhs, 0, None, None) != 0
        msg = lib().slu_last_error().decode()
        assert "refine_block_d2" in msg and "ld" in msg and "nrhs" in msg
        assert (x == 0).all()
    _, berr, steps = p.refine_block_d2(b, x)
    assert (berr <= BMAX[0]).all() and (steps >= 1).all()


@pytest.mark.parametrize("pr,pc,pz,word", [(2, 2, 1, "2x2 grid"), (1, 1, 2, "3D")])
def test_refine_block_refused_on_grids(pr, pc, pz, word, tmp_path):
    """2x2 over the host p2p transport and a 3D plan: both calls raise with
    the message on every rank before any device work and leave b and x alone."""
    from gridrun_refine_block import run_grid_refine_block
    out = run_grid_refine_block(pr, pc, pz, tmp_path)
    assert len(out) == pr * pc * pz
    for o in out:
        assert int(o["info"]) == 0
        for k, name in (("msg", "refine_block:"), ("msg_d2", "refine_block_d2:")):
            assert name in str(o[k]) and word in str(o[k]) and "1x1" in str(o[k]), str(o[k])
        assert bool(o["unchanged"])
