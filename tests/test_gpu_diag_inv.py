"""DiagInv for the block sweeps (slu_plan_set_diag_inv; csrc/solve_block_inv.h):
k_svb_inv inverts every supernode's diagonal block once per factorization,
k_svb_minv applies L_kk^-1 / U_kk^-1 as one MFMA product per supernode where
solve_block, refine_block and refine_block_d2 substitute without the mode.

Shapes: the synthetic families of tests/synth.py under SLU_AMALG=0, so the
plans sweep the prescribed partition:

  frag_star      widths 1, 2, 7, 15, 16, 47, 48, 49, 96: less than one
                 fragment, w % 16 in {0, 1, 15}, the 16-column complex panel
  edge_chain     65, 127, 128, 129, 200
  wide_chain     255 / 256 / 257
  max_inner      512: every fragment round of the 8 waves full
  max511_inner   511: a partial last panel (31 columns, complex 15), an odd
                 number of fragments

each in d, s and z, on synth.rhs's 33 right-hand sides (17 in complex): a
full pass and a pass with one live column.  The plans are this module's own:
the mode is never switched on for a plan another module's cache can reach.

Reference: long double (synth.ld_solution, synth.reference).  Tolerance per
column: max(10 x e_cpu, 50 eps), test_gpu_solve_shapes.tol_of's form, never
more than test_gpu_solve.TOL (asserted).  e_cpu is the error against the same
long-double solution of a CPU restatement of the reference's DiagInv scheme
(scheme_errors below): the oracle's factors in the plan's dtype
(synth.oracle_lu), each diagonal block's triangles inverted in that dtype by
scipy's solve_triangular on the identity, the inverses multiplied in the
block sweep's order.  The inverses themselves (test_inverses) are compared
normwise, L part and U part apart, with the long-double inverse of the
long-double factors' block, at 10 x the error of that scipy inverse of the
oracle's block, at least 50 eps.

e_cpu on the CPU, max over the columns, and the largest error of solve_block
with the mode on seen on an MI355X against long double (the tests print
both, with synth.cpu_errors' substitution pipeline beside them, in lines
that start with "DIAGINV"):

  family         e_cpu d    z          s         | MI355X d   z          s
  frag_star      8.6e-16    8.3e-16    4.1e-7    | 8.3e-16    7.3e-16    4.1e-7
  edge_chain     1.3e-15    1.3e-15    7.5e-7    | 1.5e-15    2.2e-15    7.0e-7
  wide_chain     1.7e-15    1.2e-15    1.4e-6    | 1.7e-15    1.8e-15    1.4e-6
  max_inner      1.9e-15    1.4e-15    9.7e-7    | 1.8e-15    1.7e-15    9.7e-7
  max511_inner   1.5e-15    1.4e-15    7.2e-7    | 1.0e-15    1.5e-15    5.5e-7

so the tolerance is 1.1e-14 to 1.9e-14 for d and z and 6.0e-6 to 1.4e-5 for
s, below the caps of 1e-12 and 1e-4.  Substitution's error on the same
columns is 9.8e-16 to 2.4e-15 (d, z) and 3.1e-7 to 8.2e-7 (s).  After
refine_block the error is 1.2e-15 to 1.5e-15 (d, z) and 8.8e-7 (s), after
refine_block_d2 1.2e-15 to 1.4e-15.  The inverses, max over all blocks
(scipy's inverse of the oracle's block in brackets): L part 1.7e-17 (2.5e-17)
d, 1.2e-17 (2.1e-17) z, 1.2e-8 (1.3e-8) s; U part 2.9e-15 (2.9e-15) d,
3.4e-15 (3.4e-15) z, 1.7e-6 (1.7e-6) s.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import synth
from refdump import Fixture, names
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
from superlu_dist_amd.lib import lib
from test_gpu_refine_block import BMAX
from test_gpu_solve import TOL
from test_gpu_solve_block import BTOL, backward_errors
from test_gpu_solve_shapes import plan_of
from test_solve_ref import EPS

pytestmark = pytest.mark.gpu

FAMS = ["frag_star", "edge_chain", "wide_chain", "max_inner", "max511_inner"]
PAIRS = [(f, d) for f in FAMS for d in (0, 1, 2)]
DT = {0: np.float64, 1: np.float32, 2: np.complex128}
NRHS = {0: 33, 1: 33, 2: 17}


# ------------------------------------------------------------------ the CPU yardstick
def block_inverses(M, xs):
    """Per supernode, (inverse of the unit lower triangle, inverse of the
    upper triangle) of the diagonal block of the packed factors M, in M's
    dtype: solve_triangular on the identity, what dtrtri gives the reference."""
    out = []
    for f, l in zip(xs[:-1], xs[1:]):
        D = M[f:l, f:l]
        I = np.eye(l - f, dtype=M.dtype)
        out.append((sla.solve_triangular(D, I, lower=True, unit_diagonal=True).astype(M.dtype),
                    sla.solve_triangular(D, I, lower=False).astype(M.dtype)))
    return out


def scheme_solve(M, xs, b):
    """The reference's DiagInv scheme in M's dtype: forward, X_k = L_kk^-1 X_k,
    then the rows below minus L(below, k) X_k; backward, X_k minus U(k, right)
    X(right), then X_k = U_kk^-1 X_k."""
    inv = block_inverses(M, xs)
    x = np.array(b, dtype=M.dtype, order="F")
    ns = len(xs) - 1
    for k in range(ns):
        f, l = xs[k], xs[k + 1]
        x[f:l] = inv[k][0] @ x[f:l]
        x[l:] -= M[l:, f:l] @ x[f:l]
    for k in range(ns - 1, -1, -1):
        f, l = xs[k], xs[k + 1]
        x[f:l] -= M[f:l, l:] @ x[l:]
        x[f:l] = inv[k][1] @ x[f:l]
    return x


@functools.lru_cache(maxsize=None)
def oracle_dense(family, dtype):
    lu = synth.oracle_lu(family, dtype)
    return synth.lu_to_dense(lu, synth.case(family, dtype)[0].n)


@functools.lru_cache(maxsize=None)
def scheme_errors(family, dtype):
    """e_cpu per column of synth.rhs (read-only)."""
    xs = synth.offsets(synth.FAMILIES[family])
    x = scheme_solve(oracle_dense(family, dtype), xs, synth.rhs(family, dtype))
    e = synth.col_errors(x, synth.ld_solution(family, dtype))
    e.setflags(write=False)
    return e


def cap(t, dtype):
    t = np.maximum(t, 50 * EPS[dtype])
    assert (t <= TOL[dtype]).all(), t
    return t


def tol_of(family, dtype, ncols):
    """Per column: max(10 x e_cpu, 50 eps), capped by TOL."""
    return cap(10 * scheme_errors(family, dtype)[:ncols], dtype)


def against_ld(what, family, dtype, x, xld=None, tol=None):
    k = x.shape[1]
    assert x.dtype == DT[dtype] and np.isfinite(x).all()
    err = synth.col_errors(x, (synth.ld_solution(family, dtype) if xld is None else xld)[:, :k])
    tol = tol_of(family, dtype, k) if tol is None else tol[:k]
    print(f"DIAGINV {what} dtype {dtype} {family} nrhs {k}: err {err.max():.3e} tol {tol.min():.3e} "
          f"e_cpu {scheme_errors(family, dtype)[:k].max():.3e} substitution {synth.cpu_errors(family, dtype)[:k].max():.3e}")
    assert (err < tol).all(), (err, tol)
    return err


# ------------------------------------------------------------------ the plans
def fresh(family, dtype, values=None):
    """A new plan of the family with A's values (or `values`) filled, not factored."""
    A, S, V, an = synth.case(family, dtype)
    p = plan_of(S.distribute())
    cp, ri, v = A.arrays()
    p.set_a_pattern(cp, ri)
    p.fill_a(v if values is None else values)
    return p, (cp, ri, v), an


@functools.lru_cache(maxsize=None)
def built(family, dtype):
    """(factored plan of this module, B's CSC arrays); one per (family, dtype).
    Tests set the mode they need first and leave the factors alone."""
    p, csc, an = fresh(family, dtype)
    assert p.factor(an) == (0, 0)
    assert p.stats()["nsupers"] == len(synth.FAMILIES[family]) and p.stats()["amalg_groups"] == 0
    return p, csc


def b_of(family, dtype):
    return synth.rhs(family, dtype)[:, :NRHS[dtype]]


def widths(p):
    """(fst, w) of every supernode the plan sweeps, from diag_inv_block."""
    out, k, n = [], 0, p.lu.n
    while not out or out[-1][0] + out[-1][1] < n:
        fst, w = C.c_int(), C.c_int()
        assert lib().slu_plan_diag_inv_block(p.ptr, k, C.byref(fst), C.byref(w), None, 0) == 0
        out.append((fst.value, w.value))
        k += 1
    return out


# ------------------------------------------------------------------ 1: the inverses
def ld_tri_inverses(D):
    """(inverse of D's unit lower triangle, of its upper triangle) in D's
    long-double type, by substitution on the identity."""
    w = D.shape[0]
    Li, Ui = np.eye(w, dtype=D.dtype), np.eye(w, dtype=D.dtype)
    for j in range(w - 1):
        Li[j + 1:, :j + 1] -= np.outer(D[j + 1:, j], Li[j, :j + 1])
    for j in range(w - 1, -1, -1):
        Ui[j, j:] /= D[j, j]
        Ui[:j, j:] -= np.outer(D[:j, j], Ui[j, j:])
    return Li, Ui


def tri_errors(Li, Ui, LiR, UiR):
    """Normwise errors of a unit lower and an upper inverse against long double."""
    eL = float(np.abs(np.tril(Li, -1).astype(LiR.dtype) - np.tril(LiR, -1)).max() / np.abs(LiR).max())
    eU = float(np.abs(np.triu(Ui).astype(UiR.dtype) - UiR).max() / np.abs(UiR).max())
    return eL, eU


@pytest.mark.parametrize("family,dtype", PAIRS)
def test_inverses(family, dtype):
    """Every supernode's packed inverse from k_svb_inv: L_kk^-1 strictly below
    the diagonal, U_kk^-1 on and above it."""
    p, _ = built(family, dtype)
    p.set_diag_inv(True)
    xs = synth.offsets(synth.FAMILIES[family])
    R = synth.reference(family, dtype)[0]
    cpu = block_inverses(oracle_dense(family, dtype), xs)
    assert widths(p) == [(int(f), int(l - f)) for f, l in zip(xs[:-1], xs[1:])]
    for k, (f, l) in enumerate(zip(xs[:-1], xs[1:])):
        fst, Mi = p.diag_inv_block(k)
        assert fst == f and Mi.shape == (l - f, l - f) and Mi.dtype == DT[dtype]
        assert np.isfinite(Mi).all()
        LiR, UiR = ld_tri_inverses(R[f:l, f:l])
        cL, cU = tri_errors(cpu[k][0], cpu[k][1], LiR, UiR)
        eL, eU = tri_errors(Mi, Mi, LiR, UiR)
        tL, tU = max(10 * cL, 50 * EPS[dtype]), max(10 * cU, 50 * EPS[dtype])
        print(f"DIAGINV inverse dtype {dtype} {family} w {l - f}: L {eL:.3e} (cpu {cL:.3e}) U {eU:.3e} (cpu {cU:.3e})")
        assert eL < tL and eU < tU, (k, l - f, eL, tL, eU, tU)
    assert p.diag_inv_info()[:2] == (True, True)


# ------------------------------------------------------------------ 2: solve_block
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_solve_block(family, dtype):
    p, _ = built(family, dtype)
    b = b_of(family, dtype)
    p.set_diag_inv(False)
    x0 = p.solve_block(b)
    info0 = p.solve_block_info()
    p.set_diag_inv(True)
    x = p.solve_block(b)
    info = p.solve_block_info()
    assert x.shape == b.shape
    against_ld("solve_block", family, dtype, x)
    dif = np.abs(x - x0).max(axis=0) / np.abs(x0).max(axis=0)
    assert (dif < tol_of(family, dtype, b.shape[1])).all(), dif
    assert info[0] == info0[0] == 2 and info[1] == info0[1] and info[1] % 2 == 0
    assert p.stats()["t_solve_ms"] == info[2] > 0


# ------------------------------------------------------------------ 3: stale inverses
def halved(family, dtype):
    """The family's matrix with its off-diagonal entries halved (exact in every
    dtype; still diagonally dominant): (values in the pattern's order, e_cpu
    per column and the long-double solution of synth.rhs for it)."""
    A, S, V, an = synth.case(family, dtype)
    cp, ri, v = A.arrays()
    cols = np.repeat(np.arange(A.n), np.diff(cp))
    v2 = np.where(ri == cols, v, v * DT[dtype](0.5))
    A2 = Csc.from_arrays(A.n, cp, ri, v2, dtype)
    S2 = synth.symbolic(A2)
    assert np.array_equal(S2.perm_c, np.arange(A.n))
    import cases
    import pyoracle
    lu = S2.distribute()
    o = pyoracle.oracle_factor([lu], 1, 1, A.n, False, cases.anorm(A2))
    assert o["info"] == 0 and o["tiny"] == 0
    b = synth.rhs(family, dtype)
    xld = synth.ld_solve(synth.dense_lu_ref(A2.to_dense())[0], b)
    xs = synth.offsets(synth.FAMILIES[family])
    e = synth.col_errors(scheme_solve(synth.lu_to_dense(lu, A.n), xs, b), xld)
    return v2, cases.anorm(A2), e, xld


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_stale_inverses(dtype):
    """Whatever changes the device factor storage invalidates the inverses:
    fill_a + factor with other values, snapshot / restore, upload."""
    family = "frag_star"
    p, (cp, ri, v), an = fresh(family, dtype)
    p.snapshot()
    assert p.factor(an) == (0, 0)
    p.set_diag_inv(True)
    assert p.diag_inv_info()[:4] == (True, False, 0, 0)
    b = b_of(family, dtype)
    k = b.shape[1]
    against_ld("stale: first", family, dtype, p.solve_block(b))
    on, valid, nbytes, computes, ms = p.diag_inv_info()
    assert (on, valid, computes) == (True, True, 1) and nbytes > 0 and ms > 0

    v2, an2, e2, xld2 = halved(family, dtype)
    tol2 = cap(10 * e2, dtype)
    p.fill_a(v2)
    assert p.diag_inv_info()[:2] == (True, False)
    assert p.factor(an2) == (0, 0)
    assert p.diag_inv_info()[:2] == (True, False)
    x2 = p.solve_block(b)
    against_ld("stale: new values", family, dtype, x2, xld=xld2, tol=tol2)
    old = synth.col_errors(x2, synth.ld_solution(family, dtype)[:, :k])
    assert (old >= tol_of(family, dtype, k)).all(), old   # no column passes as the old system's: stale inverses would show
    assert p.diag_inv_info()[1:4] == (True, nbytes, 2)

    p.restore()                                    # the snapshot: A's first values, not factored
    assert p.diag_inv_info()[1] is False
    assert p.factor(an) == (0, 0)
    against_ld("stale: restored", family, dtype, p.solve_block(b))
    assert p.diag_inv_info()[1:4] == (True, nbytes, 3)
    p.upload()                                     # the LUstruct's host values: A again
    assert p.diag_inv_info()[1] is False
    assert p.factor(an) == (0, 0)
    against_ld("stale: uploaded", family, dtype, p.solve_block(b))
    assert p.diag_inv_info()[1:4] == (True, nbytes, 4)


# ------------------------------------------------------------------ 4: off again
def test_off_again():
    family, dtype = "edge_chain", 0
    p, _ = built(family, dtype)
    b = b_of(family, dtype)
    p.set_diag_inv(True)
    against_ld("on", family, dtype, p.solve_block(b))
    on, valid, nbytes, computes, _ = p.diag_inv_info()
    assert on and valid and nbytes > 0
    p.set_diag_inv(False)
    assert p.diag_inv_info()[:4] == (False, False, 0, computes)
    against_ld("off", family, dtype, p.solve_block(b))
    assert p.diag_inv_info()[:4] == (False, False, 0, computes)
    p.set_diag_inv(True)
    assert p.diag_inv_info()[:4] == (True, False, 0, computes)
    against_ld("on again", family, dtype, p.solve_block(b))
    assert p.diag_inv_info()[:4] == (True, True, nbytes, computes + 1)
    p.set_diag_inv(True)                           # already on: nothing is recomputed
    p.solve_block(b)
    assert p.diag_inv_info()[3] == computes + 1


def test_mode_on_an_unfactored_plan():
    p, _, an = fresh("frag_star", 0)
    p.set_diag_inv(True)
    assert p.diag_inv_info() == (True, False, 0, 0, 0.0)
    b = b_of("frag_star", 0)
    with pytest.raises(RuntimeError, match="factor first"):
        p.solve_block(b)
    with pytest.raises(RuntimeError, match="diag_inv_block.*factor first"):
        p.diag_inv_block(0)
    assert p.diag_inv_info() == (True, False, 0, 0, 0.0)
    assert p.factor(an) == (0, 0)
    against_ld("late factor", "frag_star", 0, p.solve_block(b))


# ------------------------------------------------------------------ 5: refinement
@pytest.mark.parametrize("family", ["edge_chain", "max511_inner"])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_refine_block(family, dtype):
    """refine_block from the block solve (even columns) and from zeros (odd
    columns), against the same call with the mode off."""
    p, _ = built(family, dtype)
    b = b_of(family, dtype)
    out = {}
    for on in (False, True):
        p.set_diag_inv(on)
        x0 = p.solve_block(b)
        x0[:, 1::2] = 0
        out[on] = p.refine_block(b, x0)
        assert p.stats()["t_refine_ms"] == p.refine_block_info()[3] > 0
    x, berr, steps = out[True]
    print(f"DIAGINV refine_block dtype {dtype} {family}: steps {steps} (off {out[False][2]}) berr {berr.max():.3e}")
    assert (berr <= BMAX[dtype]).all(), berr
    assert (steps[1::2] >= 1).all() and (steps <= 20).all()
    assert (np.abs(steps.astype(int) - out[False][2].astype(int)) <= 1).all(), (steps, out[False][2])
    against_ld("refine_block", family, dtype, x)


@pytest.mark.parametrize("family", ["edge_chain", "max511_inner"])
def test_refine_block_d2(family):
    """The fp32 plan filled from the fp64 family's values, refined from zeros
    to the fp64 family's tolerance."""
    A, S, V, an = synth.case(family, 1)
    A0, _, _, an0 = synth.case(family, 0)
    cp, ri, _ = A.arrays()
    cp0, ri0, v0 = A0.arrays()
    assert np.array_equal(cp, cp0) and np.array_equal(ri, ri0)
    p = plan_of(S.distribute())
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v0)
    assert p.factor(an0) == (0, 0)
    b = b_of(family, 0)
    out = {}
    for on in (False, True):
        p.set_diag_inv(on)
        out[on] = p.refine_block_d2(b, np.zeros_like(b))
    x, berr, steps = out[True]
    print(f"DIAGINV refine_block_d2 {family}: steps {steps} (off {out[False][2]}) berr {berr.max():.3e}")
    assert p.diag_inv_info()[:2] == (True, True) and p.diag_inv_info()[3] == 1
    assert (berr <= BMAX[0]).all(), berr
    assert (steps >= 1).all() and (steps <= 20).all()
    assert (np.abs(steps.astype(int) - out[False][2].astype(int)) <= 1).all(), (steps, out[False][2])
    against_ld("refine_block_d2", family, 0, x)


# ------------------------------------------------------------------ 6: zero pivot
def test_zero_pivot_is_not_hidden():
    """A singular U_kk (the zeropiv fixture, info > 0): k_svb_inv divides by
    the diagonal, so every column Plan.solve returns non-finite is non-finite
    from solve_block with the mode on too."""
    name = next(n for n in names() if n.startswith("zeropiv") and "_1x1_" in n)
    fx = Fixture(name)
    p = Plan(fx.lu(0, "pre"), replace_tiny=fx.replace_tiny)
    p.upload()
    info, _ = p.factor(fx.anorm)
    assert info > 0 and info == fx.info
    b = np.random.default_rng(5).standard_normal((fx.n, 33))
    xs = p.solve(b)
    p.set_diag_inv(True)
    xb = p.solve_block(b)
    assert p.diag_inv_info()[:2] == (True, True)
    bad_s = ~np.isfinite(xs).all(axis=0)
    bad_b = ~np.isfinite(xb).all(axis=0)
    assert bad_s.any()
    assert (bad_b | ~bad_s).all(), (bad_s, bad_b)


# ------------------------------------------------------------------ 7: poisoned LDS
@pytest.mark.parametrize("family,dtype", [("max511_inner", 0), ("frag_star", 2)])
def test_poisoned_lds(family, dtype):
    """NaN in every LDS word right before the inversion and again right
    before a solve_block: finite and within tolerance."""
    p, _ = built(family, dtype)
    b = b_of(family, dtype)
    p.set_diag_inv(False)
    p.set_diag_inv(True)                           # the inverses are gone
    computes = p.diag_inv_info()[3]
    assert lib().slu_debug_poison_lds(0) == 0
    last = len(synth.FAMILIES[family]) - 1
    assert np.isfinite(p.diag_inv_block(last)[1]).all()
    assert p.diag_inv_info()[1:4:2] == (True, computes + 1)
    assert lib().slu_debug_poison_lds(0) == 0
    x = p.solve_block(b)
    assert p.diag_inv_info()[3] == computes + 1
    against_ld("poisoned", family, dtype, x)


# ------------------------------------------------------------------ 8: the coarse plan
def test_coarse_plan(monkeypatch):
    """The amalgamated plan forwards the mode to its inner plan, whose
    partition is the one swept (test_solve_block_plain_and_coarse_plan's case)."""
    from lusolve import solve_1x1
    from lusolve_t import unsym_stencil
    monkeypatch.setenv("SLU_AMALG", "1")
    A = unsym_stencil(STENCIL_3D7, (12, 12, 12), 0)
    S = Symbolic(A, nd_order(12, 12, 12), 60, 256)
    lu = S.distribute()
    p = Plan(lu)
    p.upload()
    assert p.factor(14.0) == (0, 0)
    p.download()
    assert p.stats()["amalg_groups"] > 0
    cp, ri, v = A.permuted(S.perm_c).arrays()
    B = sp.csc_matrix((v, ri, cp), shape=(A.n, A.n))
    b = np.asfortranarray(B @ np.random.default_rng(7).standard_normal((A.n, 33)))
    p.set_diag_inv(True)
    x = p.solve_block(b)
    ws = widths(p)
    assert len(ws) < S.nsupers and sum(w for _, w in ws) == A.n
    assert p.diag_inv_info()[:4] == (True, True, 8 * sum(w * w for _, w in ws), 1)
    assert p.solve_block_info()[0] == 2 and p.stats()["t_solve_ms"] == p.solve_block_info()[2] > 0
    for r in range(33):
        xh = solve_1x1(lu, b[:, r])
        assert np.abs(x[:, r] - xh).max() / np.abs(xh).max() < TOL[0]
    assert (backward_errors(B, x, b) < BTOL[0]).all()


# ------------------------------------------------------------------ 9: info
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_info(dtype):
    family = "frag_star"
    p, _ = built(family, dtype)
    p.set_diag_inv(False)
    p.set_diag_inv(True)
    p.solve_block(b_of(family, dtype))
    on, valid, nbytes, computes, ms = p.diag_inv_info()
    assert on and valid and computes >= 1 and ms > 0
    assert nbytes == np.dtype(DT[dtype]).itemsize * sum(w * w for w, _ in synth.FAMILIES[family])
    assert p.stats()["t_solve_ms"] == p.solve_block_info()[2] > 0


# ------------------------------------------------------------------ 10: refusals
def test_bad_arguments():
    p, _ = built("frag_star", 0)
    p.set_diag_inv(True)
    ns = len(synth.FAMILIES["frag_star"])
    out = np.zeros((96, 96), order="F")
    vp = out.ctypes.data_as(C.c_void_p)
    for k, ldo in ((-1, 96), (ns, 96), (ns - 1, 95)):
        assert lib().slu_plan_diag_inv_block(p.ptr, k, None, None, vp, ldo) != 0
        assert "diag_inv_block" in lib().slu_last_error().decode()
        assert (out == 0).all()
    assert lib().slu_plan_diag_inv_block(p.ptr, ns - 1, None, None, vp, 96) == 0  # the plan still works
    assert np.isfinite(out).all() and out[0, 0] != 0


@pytest.mark.parametrize("pr,pc,pz,word", [(2, 2, 1, "2x2 grid"), (1, 1, 2, "3D")])
def test_refused_on_grids(pr, pc, pz, word, tmp_path):
    """2x2 over the host p2p transport and a 3D plan: set_diag_inv(1) fails
    with the block sweep's message on every rank, on the plan without values
    (so before any device work) and after the factorization; the mode stays
    off and the 2D plan's own solve still works."""
    from gridrun_diag_inv import run_grid_diag_inv
    out = run_grid_diag_inv(pr, pc, pz, tmp_path)
    assert len(out) == pr * pc * pz
    for o in out:
        assert int(o["info"]) == 0
        for rc, msg in ((o["rc0"], str(o["msg0"])), (o["rc"], str(o["msg"]))):
            assert int(rc) != 0
            assert "set_diag_inv" in msg and word in msg and "block sweep" in msg and "1x1" in msg, msg
        assert not bool(o["on"]) and not bool(o["valid"]) and int(o["bytes"]) == 0 and int(o["computes"]) == 0
        if pz == 1:
            assert 0 <= float(o["resid"]) < 1e-12
