"""Block iterative refinement with the transpose for many right-hand sides
(slu_plan_refine_block_t; csrc/refine_block.h k_rfb_resid_t around the
transposed block sweep of csrc/solve_block_t.h).

Systems: stencil patterns with unsymmetric values (lusolve_t.unsym_stencil)
under assert_unsymmetric.  Checkers: test_gpu_refine_trans.host_refine_t
column by column on the downloaded factors, and the per-column device call
Plan.refine(b, x, trans=...).  Bounds are the constants of
tests/test_gpu_refine_block.py: berr <= BMAX, x within XTOL of both, steps
equal to the per-column call's (and within one of the host loop's, as
test_gpu_refine_trans allows its host loop).  Each system is factored once
per module and its references are computed once.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from lusolve_t import op_t, unsym_stencil
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, STENCIL_3D27, Symbolic, nd_order
from superlu_dist_amd.lib import lib
from test_gpu_refine_block import BMAX, DT, EPS, SVB_NR, XTOL, bits
from test_gpu_refine_trans import host_refine_t
from test_gpu_solve_trans import assert_unsymmetric

pytestmark = pytest.mark.gpu

# n = 729: neither 8 nor 16 columns per workgroup of the residual divide it
CASES = {"d": (STENCIL_3D7, (9, 9, 9), 0, "T"), "s": (STENCIL_3D27, (8, 8, 8), 1, "T"),
         "z": (STENCIL_3D7, (8, 8, 8), 2, "C"), "f": (STENCIL_3D7, (3, 5, 5), 0, "T")}
NCOL = {"d": 33, "s": 33, "z": 17}


def make_plan(kind, dims, dtype):
    A = unsym_stencil(kind, dims, dtype)
    S = Symbolic(A, nd_order(*dims), 60, 256)
    lu = S.distribute()
    p = Plan(lu)
    cp, ri, v = A.permuted(S.perm_c).arrays()
    assert_unsymmetric(cp, ri, v)
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(28.0 if kind == STENCIL_3D27 else 14.0)[0] == 0
    p.download()
    return p, lu, (cp, ri, v)


@functools.lru_cache(maxsize=None)
def factored(key):
    return make_plan(*CASES[key][:3])


def rhs(key, ncols, seed=11):
    cp, ri, v = factored(key)[2]
    dtype, trans = CASES[key][2:]
    n = len(cp) - 1
    rng = np.random.default_rng(seed)
    xt = rng.standard_normal((n, ncols))
    if dtype == 2:
        xt = xt + 1j * rng.standard_normal((n, ncols))
    return np.asfortranarray((op_t(cp, ri, v, trans == "C") @ xt).astype(DT[dtype]))


@functools.lru_cache(maxsize=None)
def reference(key):
    """(b, x0, host loop's x and steps, refine(trans)'s x, berr and steps) per
    column; x0 = the block solve, every third column perturbed so that it has
    steps to take.  Computed once."""
    p, lu, (cp, ri, v) = factored(key)
    dtype, trans = CASES[key][2:]
    Bt = op_t(cp, ri, v, trans == "C")
    b = rhs(key, NCOL[key])
    x0 = p.solve_block(b, trans=trans)
    rng = np.random.default_rng(5)
    x0[:, 1::3] = (x0[:, 1::3] * (1 + 1e-3 * rng.standard_normal(x0[:, 1::3].shape))).astype(DT[dtype])
    host = [host_refine_t(lu, Bt, b[:, j], x0[:, j].copy(), EPS[dtype], trans == "C") for j in range(b.shape[1])]
    xh = np.stack([h[0] for h in host], axis=1)
    sh = np.array([h[2] for h in host])
    xr, ber, sr = p.refine(b, x0, trans=trans)
    for a in (b, x0, xh, sh, xr, ber, sr):
        a.setflags(write=False)
    return b, x0, xh, sh, xr, ber, sr


def check_columns(key, x, berr, steps, ncols):
    dtype = CASES[key][2]
    b, x0, xh, sh, xr, ber, sr = reference(key)
    for j in range(ncols):
        eh = np.abs(x[:, j] - xh[:, j]).max() / np.abs(xh[:, j]).max()
        er = np.abs(x[:, j] - xr[:, j]).max() / np.abs(xr[:, j]).max()
        print(f"col {j}: steps {steps[j]} (host {sh[j]}, refine {sr[j]}) berr {berr[j]:.3e} "
              f"(refine {ber[j]:.3e}) err host {eh:.3e} refine {er:.3e}")
        assert np.isfinite(x[:, j]).all()
        assert berr[j] <= BMAX[dtype], (j, berr[j])
        assert eh < XTOL[dtype] and er < XTOL[dtype], (j, eh, er)
        assert int(steps[j]) == int(sr[j]), (j, steps[j], sr[j])
        assert abs(int(steps[j]) - int(sh[j])) <= 1, (j, steps[j], sh[j])


# 1. parity per column with the host loop and with refine(trans)
@pytest.mark.parametrize("key,nrhs", [(k, n) for k in "dsz" for n in ((1, 5, 17) if k == "z" else (1, 5, 33))])
def test_refine_block_t_matches_host_loop_and_refine(key, nrhs):
    p = factored(key)[0]
    dtype, trans = CASES[key][2:]
    bf, x0f = reference(key)[:2]
    b, x0 = np.asfortranarray(bf[:, :nrhs]), np.asfortranarray(x0f[:, :nrhs])
    x, berr, steps = p.refine_block(b, x0, trans=trans)
    assert x.shape == b.shape and x.dtype == DT[dtype] and len(berr) == len(steps) == nrhs
    assert p.stats()["t_refine_ms"] > 0
    check_columns(key, x, berr, steps, nrhs)
    if nrhs > 1:
        assert (steps[1::3] >= 1).all()
        # the untransposed loop on the same pair heads for another solution
        xn = p.refine_block(b, x0)[0]
        assert (np.abs(xn - x).max(axis=0) / np.abs(x).max(axis=0) > 1e-3).all()


def test_refine_block_t_same_codes():
    """trans="N" and 0 are refine_block(b, x); "C" on a real plan is "T"."""
    p = factored("d")[0]
    b, x0 = reference("d")[:2]
    x1, be1, st1 = p.refine_block(b, x0)
    for tn in ("N", 0):
        x2, be2, st2 = p.refine_block(b, x0, trans=tn)
        assert (st1 == st2).all() and np.abs(x1 - x2).max() <= 1e-13 * np.abs(x1).max()
    xt, bet, stt = p.refine_block(b, x0, trans="T")
    xc, bec, stc = p.refine_block(b, x0, trans="C")
    assert (stt == stc).all() and np.abs(xt - xc).max() <= 1e-13 * np.abs(xt).max()


# 2. frozen columns and mixed stopping times
def test_refine_block_t_freezes_stopped_columns():
    """test_refine_block_freezes_stopped_columns with the transpose: one pass
    of 32 columns of four kinds, j % 4: (a) x0 = what a prior refine(trans="T")
    returned with berr <= eps (takes no step), (b) x0 = 0, (c) b = 0 and
    x0 = 0, (d) a NaN in x0."""
    p, lu, (cp, ri, v) = factored("f")
    Bt = op_t(cp, ri, v)
    b = rhs("f", 32)
    x0 = p.solve_block(b, trans="T")
    ka, kb, kc, kd = (np.arange(k, 32, 4) for k in range(4))
    bc = rhs("f", 256, seed=5)
    xc, bec, _ = p.refine(bc, p.solve_block(bc, trans="T"), trans="T")
    sel = np.flatnonzero(bec <= EPS[0])[:8]
    print(f"{(bec <= EPS[0]).sum()} of 256 refined candidates have berr <= eps")
    assert len(sel) == 8
    b[:, ka] = bc[:, sel]
    x0[:, ka] = xc[:, sel]
    x0[:, kb] = 0.0
    b[:, kc] = 0.0
    x0[:, kc] = 0.0
    x0[5, kd] = np.nan
    _, be_ref, st_ref = p.refine(b[:, ka], x0[:, ka], trans="T")  # the per-column call on the same x0
    assert (st_ref == 0).all() and (be_ref > 0).all()
    x, berr, steps = p.refine_block(b, x0, trans="T")
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
    # a stopped column's berr is refine(trans)'s on the same returned x, as bits
    _, be_again, st_again = p.refine(b[:, kb], x[:, kb], trans="T")
    stopped = st_again == 0
    assert np.array_equal(bits(be_again[stopped]), bits(berr[kb][stopped]))
    # the NaN columns leave the others finite and within test 1's bounds
    for j in kb:
        xh, _, sh = host_refine_t(lu, Bt, b[:, j], x0[:, j].copy(), EPS[0], False)
        assert np.isfinite(x[:, j]).all() and berr[j] <= BMAX[0]
        assert np.abs(x[:, j] - xh).max() / np.abs(xh).max() < XTOL[0]
        assert abs(int(steps[j]) - sh) <= 1
    assert passes == 1 and sweeps == steps.max() and resids == sweeps + 1


# 3. counters over several passes
@pytest.mark.parametrize("key,nrhs", [("d", 70), ("z", 40)])
def test_refine_block_t_info_over_passes(key, nrhs):
    p = factored(key)[0]
    dtype, trans = CASES[key][2:]
    nrb = SVB_NR[dtype]
    b = rhs(key, nrhs, seed=3)
    x0 = p.solve_block(b, trans=trans)
    x0[:, 1::3] = 0  # mixed stopping times within every pass
    x, berr, steps = p.refine_block(b, x0, trans=trans)
    passes, sweeps, resids, ms = p.refine_block_info()
    assert (berr <= BMAX[dtype]).all()
    assert passes == -(-nrhs // nrb)
    assert sweeps == sum(int(steps[r0:r0 + nrb].max()) for r0 in range(0, nrhs, nrb)) and sweeps >= passes
    assert resids == sweeps + passes
    assert ms > 0 and ms == p.stats()["t_refine_ms"]


# 4. memory discipline
@pytest.mark.parametrize("nrhs", [5, 33])
def test_refine_block_t_leaves_the_rest_alone(nrhs):
    """b and x inside (n + 3) x (nrhs + 2) arrays of sentinels, ld = n + 3: the
    sentinels and all of b are bit-identical afterwards."""
    p, lu, (cp, ri, v) = factored("d")
    n = len(cp) - 1
    bf, x0f = reference("d")[:2]
    sent = np.float64(-7.25e300)
    bb = np.full((n + 3, nrhs + 2), sent, order="F")
    xx = np.full((n + 3, nrhs + 2), sent, order="F")
    bb[:n, :nrhs] = bf[:, :nrhs]
    xx[:n, :nrhs] = x0f[:, :nrhs]
    keep = bb.copy()
    berr, steps = np.zeros(nrhs), np.zeros(nrhs, dtype=np.int32)
    assert lib().slu_plan_refine_block_t(p.ptr, 1, bb.ctypes.data_as(C.c_void_p), xx.ctypes.data_as(C.c_void_p),
                                         n + 3, nrhs, 0, berr.ctypes.data_as(C.POINTER(C.c_double)),
                                         steps.ctypes.data_as(C.POINTER(C.c_int))) == 0
    assert np.array_equal(bits(bb), bits(keep))
    assert (bits(xx[n:, :]) == sent.view(np.uint64)).all()
    assert (bits(xx[:, nrhs:]) == sent.view(np.uint64)).all()
    check_columns("d", np.asfortranarray(xx[:n, :nrhs]), berr, steps, nrhs)


# 5. poisoned LDS
@pytest.mark.parametrize("key", ["d", "z"])
def test_refine_block_t_does_not_read_stale_lds(key):
    """NaN in every LDS word immediately before the call (a partial last
    workgroup of the residual, a partial last pass): results as in test 1."""
    p = factored(key)[0]
    b, x0 = reference(key)[:2]
    assert lib().slu_debug_poison_lds(0) == 0
    x, berr, steps = p.refine_block(b, x0, trans=CASES[key][3])
    check_columns(key, x, berr, steps, NCOL[key])


# 6. device pointers
def test_refine_block_t_device_pointers():
    """Column-major torch tensors on the device with ld > n, refined in place
    through refine_block_dev(..., trans="T") in a child process; compared
    with the host-array call at test 1's tolerance (the sweep's atomics are
    unordered).  b and the padding of x keep their values."""
    from gridrun_block_t import run_device_pointer_t
    o = run_device_pointer_t()
    xh, xd = o["r_x_host"], o["r_x_dev"]
    assert xh.shape == xd.shape and np.isfinite(xd).all()
    assert (np.abs(xd - xh).max(axis=0) / np.abs(xh).max(axis=0) < XTOL[0]).all()
    assert (o["r_berr_dev"] <= BMAX[0]).all() and (o["r_berr_host"] <= BMAX[0]).all()
    assert (np.abs(o["r_steps_dev"].astype(int) - o["r_steps_host"].astype(int)) <= 1).all()
    assert (o["r_steps_host"][::2] >= 1).all()
    assert bool(o["r_ok"])
    assert int(o["r_info"][0]) == 2 and float(o["r_info"][3]) > 0


# 7. refusals
def test_refine_block_t_refusals_in_process():
    A = unsym_stencil(STENCIL_3D7, (6, 6, 6), 0)
    S = Symbolic(A, nd_order(6, 6, 6), 60, 256)
    p = Plan(S.distribute())
    cp, ri, v = A.permuted(S.perm_c).arrays()
    n = A.n
    b, x = np.ones((n, 3), order="F"), np.zeros((n, 3), order="F")
    p.upload()
    with pytest.raises(RuntimeError, match="refine_block_t.*factor first"):
        p.refine_block(b, x, trans="T")
    assert p.factor(14.0) == (0, 0)
    with pytest.raises(RuntimeError, match="refine_block_t needs.*fill_a"):  # uploaded values: of no A
        p.refine_block(b, x, trans="T")
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(14.0)[0] == 0
    args = (b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p))
    for trans, ld, nrhs, word in ((1, n - 1, 3, "ld"), (2, n, -1, "nrhs"), (3, n, 3, "trans = 3"),
                                  (-1, n, 3, "trans = -1")):
        assert lib().slu_plan_refine_block_t(p.ptr, trans, *args, ld, nrhs, 0, None, None) != 0
        msg = lib().slu_last_error().decode()
        assert "refine_block_t" in msg and word in msg, msg
        assert (x == 0).all() and (b == 1).all()
    with pytest.raises(ValueError, match="trans"):
        p.refine_block(b, x, trans="X")
    with pytest.raises(ValueError, match="d2"):
        p.refine_block_dev(0, 0, n, 3, d2=True, trans="T")
    x1, berr, _ = p.refine_block(b, x, trans="T")  # the plan still works; berr and steps may be NULL
    assert (berr <= BMAX[0]).all() and (b == 1).all()
    assert lib().slu_plan_refine_block_t(p.ptr, 1, *args, n, 3, 0, None, None) == 0


def test_refine_block_t_refuses_factors_of_fill_a_d2():
    """fill_a_d2 leaves no fp32 A on the device: refused as refine_t refuses
    such factors (solve_block_t needs no A and still runs)."""
    A = unsym_stencil(STENCIL_3D7, (6, 6, 6), 1)
    S = Symbolic(A, nd_order(6, 6, 6), 60, 256)
    p = Plan(S.distribute())
    cp, ri, v = A.permuted(S.perm_c).arrays()
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v.astype(np.float64))
    assert p.factor(14.0)[0] == 0
    b = np.ones((A.n, 2), dtype=np.float32, order="F")
    with pytest.raises(RuntimeError, match="refine_block_t needs.*fill_a"):
        p.refine_block(b, b, trans="T")
    assert np.isfinite(p.solve_block(b, trans="T")).all()
