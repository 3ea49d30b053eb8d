"""Solve-kernel parity on synthetic supernode shapes against long double: the
sweeps of csrc/solve.h (k_sv_*), the MFMA block solve of csrc/solve_block.h
(k_svb_*), refinement (refine_loop, csrc/refine_d2.h) and the condition
estimate on matrices whose supernode widths and panel heights are chosen on
purpose (tests/synth.py), where every other solve test takes what nested
dissection of a stencil gives it (at most 320 columns):

  frag_star        widths 1, 2, 7 (the G < SVT_G groups of k_sv_utpanel), 15 /
                   16 and 47 / 48 / 49 (the 16-column complex panel, the 16-row
                   MFMA fragments)
  narrow_star, mixed_star, edge_chain
                   31 / 32 / 33, 63 / 64 / 65, 127 / 128 / 129
  wide_chain, wide_inner
                   255 / 256 / 257, 300: the second row per thread of k_sv_upanel
  lpanel256_star, lpanel257_star
                   L panels of exactly 256 and 257 rows: the second 256-row
                   chunk of k_sv_lpanel / k_sv_ltpanel / k_svb_lpanel holds one row
  max_inner, max511_inner
                   512 and 511 wide blocks with panels: every thread of the
                   512-thread diagonal solves live, last panel at j0 = 480

Reference: synth.ld_solve, forward and back substitution in long double with
the long-double LU of the same matrix (synth.reference) -- factors the device
never saw.  The plans run under SLU_AMALG=0, so they sweep the prescribed
partition; the downloaded factors are checked once against that LU
(test_factors), so a failure belongs to the factorization or to the sweep.

Tolerance, per column and op: max(10 x e_cpu, 50 eps) (test_solve_ref._close's
form), e_cpu = the error against ld_solve of the CPU pipeline on the same b
(the oracle's factors in the plan's dtype, then lusolve / lusolve_t;
synth.cpu_errors), never more than test_gpu_solve.TOL.  Errors are normwise
per column, max|x - x_ld| / max|x_ld|.

CPU yardstick on the 33 right-hand sides used here (max over the families):
d 2.9e-15, z 2.4e-15, s 8.3e-7, so the tolerance is 1.1e-14 to 2.9e-14 for d
and z and 6.0e-6 to 8.3e-6 for s.  Largest error seen on an MI355X against
long double, over all families (the factors: 2.8e-15 / 3.2e-15 / 1.5e-6):

  entry point            d          z          s
  solve                  2.6e-15    2.4e-15    1.7e-6
  solve trans="T"        2.3e-15    1.8e-15    1.5e-6
  solve trans="C"        -          2.4e-15    -
  solve_block            2.1e-15    1.7e-15    1.1e-6
  refine                 1.2e-15    1.6e-15    7.1e-7
  refine trans="T"       1.4e-15    1.5e-15    7.0e-7
  refine trans="C"       -          1.4e-15    -
  refine_d2 (s plan)     1.2e-15 against the fp64 matrix
  rcond vs host loop     1.0e-15    1.8e-15    1.9e-7   (relative)

Mutations these tests were checked to catch (each skips work, none committed):
k_sv_upanel without its second row per thread fails solve / solve_block-vs-
solve / rcond on wide_inner, max_inner and max511_inner (wide_chain's only
block wider than 256 is the root, which has no U panel); k_sv_lpanel without
its last panel row fails solve on every family; k_sv_utpanel without the
atomics of groups of fewer than 4 lanes fails the transposed cases of
frag_star only.  Refinement converges through such a sweep, so the refine
cases do not see them: they pin the loop, ld > n and the berr word.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import synth
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.lib import TRANS_CODE, lib
from test_gpu_refine import EPS as EPS_R
from test_gpu_refine import _berr
from test_gpu_rcond import anorm_of, host_estimate
from test_gpu_solve import TOL
from test_gpu_solve_trans import BITS, assert_unsymmetric
from test_oracle import TOL as FTOL
from test_solve_ref import EPS

pytestmark = pytest.mark.gpu

FAMS = ["narrow_star", "frag_star", "mixed_star", "edge_chain", "wide_chain", "wide_inner",
        "lpanel256_star", "lpanel257_star", "max_inner", "max511_inner"]
PAIRS = [(f, d) for f in FAMS for d in (0, 1, 2)]
DT = {0: np.float64, 1: np.float32, 2: np.complex128}
SENT = {0: -7.25e30, 1: -7.25e30, 2: -7.25e30 + 3.5e30j}
OPS = {0: (None, "T"), 1: (None, "T"), 2: (None, "T", "C")}
vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def plan_of(lu):
    """A plan of the prescribed partition (no amalgamation)."""
    old = os.environ.get("SLU_AMALG")
    os.environ["SLU_AMALG"] = "0"
    try:
        return Plan(lu)
    finally:
        if old is None:
            del os.environ["SLU_AMALG"]
        else:
            os.environ["SLU_AMALG"] = old


@functools.lru_cache(maxsize=None)
def factored(family, dtype):
    """(plan with A's values and the factors on the device, lu with the
    factors downloaded, B's CSC arrays, dense B); one per (family, dtype)."""
    A, S, V, an = synth.case(family, dtype)
    assert np.array_equal(S.perm_c, np.arange(A.n))
    lu = S.distribute()
    p = plan_of(lu)
    cp, ri, v = A.arrays()
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    assert p.factor(an) == (0, 0)
    p.download()
    st = p.stats()
    assert st["nsupers"] == len(synth.FAMILIES[family]) and st["amalg_groups"] == 0
    return p, lu, (cp, ri, v), V


def tol_of(family, dtype, trans, ncols):
    """Per column: max(10 x the CPU pipeline's error, 50 eps), capped by TOL."""
    t = np.maximum(10 * synth.cpu_errors(family, dtype, trans)[:ncols], 50 * EPS[dtype])
    assert (t <= TOL[dtype]).all(), t
    return t


def against_ld(what, family, dtype, trans, x):
    """Asserts x (n, k) within tolerance of the long-double solution of the
    family's first k right-hand sides; returns the errors."""
    k = x.shape[1]
    assert x.dtype == DT[dtype] and np.isfinite(x).all()
    err = synth.col_errors(x, synth.ld_solution(family, dtype, trans)[:, :k])
    tol = tol_of(family, dtype, trans, k)
    print(f"SHAPES {what} {trans or 'N'} dtype {dtype} {family} nrhs {k}: err {err.max():.3e} "
          f"tol {tol.min():.3e} cpu {synth.cpu_errors(family, dtype, trans)[:k].max():.3e}")
    assert (err < tol).all(), (err, tol)
    return err


def rel(x, y):
    return float(np.abs(x - y).max() / np.abs(y).max())


# ------------------------------------------------------------------ the factors
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_factors(family, dtype):
    p, lu, _, V = factored(family, dtype)
    R, info, tiny = synth.reference(family, dtype)
    eL, eU = synth.lu_errors(synth.lu_to_dense(lu, V.shape[0]), R)
    print(f"SHAPES factor N dtype {dtype} {family}: L {eL:.3e} U {eU:.3e}")
    assert info == 0 and tiny == 0
    assert max(eL, eU) < FTOL[dtype], (eL, eU)


# ------------------------------------------------------------------ 1, 2: the sweeps
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_solve(family, dtype):
    """NR = 1; real: a full batch of 8 and a batch of 3 live columns; complex
    (SvNr = 2): a full batch and a batch of one."""
    p = factored(family, dtype)[0]
    b = synth.rhs(family, dtype)
    for nrhs in (1, 3 if dtype == 2 else 11):
        x = p.solve(b[:, :nrhs])
        assert x.shape == (b.shape[0], nrhs)
        against_ld("solve", family, dtype, None, x)


@pytest.mark.parametrize("family,dtype", PAIRS)
def test_solve_trans(family, dtype):
    p, lu, (cp, ri, v), V = factored(family, dtype)
    assert_unsymmetric(cp, ri, v)
    b = synth.rhs(family, dtype)
    for nrhs in (1, 3 if dtype == 2 else 11):
        xt = p.solve(b[:, :nrhs], trans="T")
        against_ld("solve_t", family, dtype, "T", xt)
        xc = p.solve(b[:, :nrhs], trans="C")
        if dtype == 2:
            against_ld("solve_t", family, dtype, "C", xc)
        else:  # SLU_CONJ on a real plan is SLU_TRANS
            assert rel(xc, xt) <= BITS[dtype]


# ------------------------------------------------------------------ 3: the block solve
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_solve_block(family, dtype):
    """A full pass of 32 (complex: 16) columns and a pass with one live column."""
    p = factored(family, dtype)[0]
    nrhs = 17 if dtype == 2 else 33
    b = synth.rhs(family, dtype)[:, :nrhs]
    x = p.solve_block(b)
    assert p.solve_block_info()[0] == 2
    against_ld("solve_block", family, dtype, None, x)
    xs = p.solve(b)
    dif = np.abs(x - xs).max(axis=0) / np.abs(xs).max(axis=0)
    assert (dif < tol_of(family, dtype, None, nrhs)).all(), dif


# ------------------------------------------------------------------ 4: refinement
def op_csc(cp, ri, v, trans):
    """CSC arrays of op(B) and its largest number of entries in a row."""
    if trans is not None:
        n = len(cp) - 1
        M = sp.csc_matrix((v, ri, cp), shape=(n, n))
        M = (M.conj().T if trans == "C" else M.T).tocsc()
        M.sort_indices()
        cp, ri, v = M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data
    return cp, ri, v, int(np.bincount(ri).max())


def padded(a, ld, dtype):
    out = np.full((ld, a.shape[1]), SENT[dtype], dtype=DT[dtype], order="F")
    out[:a.shape[0]] = a
    return out


def refine_abi(p, dtype, trans, b, x0, pad=5, d2=False):
    """slu_plan_refine / _t / _d2 with ld = n + pad; b untouched and the rows
    n .. ld - 1 of x bit-identical afterwards.  Returns (x, berr, steps)."""
    n, nrhs = b.shape
    ld = n + pad
    B, X = padded(b, ld, dtype), padded(x0, ld, dtype)
    B0, X0 = B.copy(order="F"), X.copy(order="F")
    berr = np.full(nrhs, -1.0)
    steps = np.full(nrhs, -1, dtype=np.int32)
    tail = (ld, nrhs, berr.ctypes.data_as(C.POINTER(C.c_double)), steps.ctypes.data_as(C.POINTER(C.c_int)))
    if d2:
        rc = lib().slu_plan_refine_d2(p.ptr, vp(B), vp(X), *tail)
    elif trans is None:
        rc = lib().slu_plan_refine(p.ptr, vp(B), vp(X), *tail)
    else:
        rc = lib().slu_plan_refine_t(p.ptr, TRANS_CODE[trans], vp(B), vp(X), *tail)
    assert rc == 0, lib().slu_last_error().decode()
    assert B.tobytes(order="F") == B0.tobytes(order="F")
    assert X[n:].tobytes() == X0[n:].tobytes()
    return np.asfortranarray(X[:n]), berr, steps


@pytest.mark.parametrize("family,dtype", PAIRS)
def test_refine(family, dtype):
    """Three columns through one refine_loop with ld = n + 5: from the solve,
    from zeros, and a copy of the first; each also alone."""
    p, lu, (cp, ri, v), V = factored(family, dtype)
    n = V.shape[0]
    bb = synth.rhs(family, dtype)
    b = np.asfortranarray(bb[:, [0, 1, 0]])
    for trans in OPS[dtype]:
        x0 = np.zeros_like(b)
        x0[:, 0] = x0[:, 2] = p.solve(b[:, 0], trans=trans or "N")
        x, berr, steps = refine_abi(p, dtype, trans, b, x0)
        assert ((0 <= steps) & (steps <= 20)).all(), steps
        assert steps[1] >= 1
        ocp, ori, ov, rownnz = op_csc(cp, ri, v, trans)
        tol_b = 2 * (rownnz + 1) * EPS_R[dtype]
        for j in range(3):
            be = _berr(ocp, ori, ov, x[:, j], b[:, j])
            assert abs(be - berr[j]) <= tol_b, (j, be, berr[j], tol_b)
        against_ld("refine", family, dtype, trans, np.asfortranarray(x[:, :2]))
        assert rel(x[:, 2], x[:, 0]) <= BITS[dtype] and abs(int(steps[2]) - int(steps[0])) <= 1
        for j in range(3):  # nothing carries from one column of refine_loop to the next
            x1, b1, s1 = refine_abi(p, dtype, trans, b[:, j:j + 1], x0[:, j:j + 1])
            assert rel(x[:, j], x1[:, 0]) <= BITS[dtype], (j, rel(x[:, j], x1[:, 0]))
            assert abs(int(steps[j]) - int(s1[0])) <= 1, (j, steps, s1)
            assert abs(berr[j] - b1[0]) <= tol_b


# ------------------------------------------------------------------ 5: mixed-precision refinement
@functools.lru_cache(maxsize=None)
def factored_d2(family):
    """The fp32 plan of a family with the fp64 family's values (fill_a_d2)."""
    A, S, V, an = synth.case(family, 1)
    A0, _, V0, an0 = synth.case(family, 0)
    cp, ri, _ = A.arrays()
    cp0, ri0, v0 = A0.arrays()
    assert np.array_equal(cp, cp0) and np.array_equal(ri, ri0)
    p = plan_of(S.distribute())
    p.set_a_pattern(cp, ri)
    p.fill_a_d2(v0)
    assert p.factor(an0) == (0, 0)
    assert p.stats()["nsupers"] == len(synth.FAMILIES[family])
    return p


@pytest.mark.parametrize("family", FAMS)
def test_refine_d2(family):
    """fp32 factors of the fp64 matrix, refined from zero to the fp64
    tolerance of the family against the fp64 matrix's long-double solution."""
    p = factored_d2(family)
    b = np.asfortranarray(synth.rhs(family, 0)[:, :2])
    x, berr, steps = refine_abi(p, 0, None, b, np.zeros_like(b), d2=True)
    assert (steps >= 1).all() and (steps <= 20).all(), steps
    assert (berr <= 8 * 2.0 ** -53).all(), berr
    against_ld("refine_d2", family, 0, None, x)


# ------------------------------------------------------------------ 6: the condition estimate
@functools.lru_cache(maxsize=None)
def true_inverse_norms(family, dtype):
    """{'1', 'I'}: the norms of B^-1 from the long-double factors."""
    inv = np.abs(synth.ld_inverse(synth.reference(family, dtype)[0]))
    return {"1": float(inv.sum(axis=0).max()), "I": float(inv.sum(axis=1).max())}


@pytest.mark.parametrize("norm", ["1", "I"])
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_rcond(family, dtype, norm):
    p, lu, _, V = factored(family, dtype)
    n = V.shape[0]
    an = anorm_of(V.astype(np.complex128 if dtype == 2 else np.float64), norm)
    rc = p.rcond(an, norm=norm)
    sweeps, ms = p.rcond_info()
    assert rc > 0 and ms > 0
    est = 1.0 / (rc * an)
    true = true_inverse_norms(family, dtype)[norm]
    he, hs = host_estimate(lu, n, norm)
    print(f"SHAPES rcond {norm} dtype {dtype} {family}: est {est:.6e} true {true:.6e} host {he:.6e} "
          f"rel {abs(est - he) / he:.2e} sweeps {sweeps} / {hs}")
    assert est <= true * (1 + (1e-2 if dtype == 1 else 1e-6))
    assert abs(est - he) <= (1e-3 if dtype == 1 else 1e-8) * he
    assert sweeps == hs and 3 <= sweeps <= 11


# ------------------------------------------------------------------ 7: ldb > n
@pytest.mark.parametrize("dtype", [0, 2])
def test_solve_ldb(dtype):
    """b inside an (n + 7) x (nrhs + 2) array of sentinels, ldb = n + 7: the
    extra rows and columns are bit-identical afterwards."""
    family = "edge_chain"
    p = factored(family, dtype)[0]
    nrhs = 3 if dtype == 2 else 11
    b = synth.rhs(family, dtype)[:, :nrhs]
    n = b.shape[0]
    for trans in OPS[dtype]:
        big = np.full((n + 7, nrhs + 2), SENT[dtype], dtype=DT[dtype], order="F")
        keep = big.copy(order="F")
        big[:n, :nrhs] = b
        if trans is None:
            rc = lib().slu_plan_solve(p.ptr, vp(big), n + 7, nrhs)
        else:
            rc = lib().slu_plan_solve_t(p.ptr, TRANS_CODE[trans], vp(big), n + 7, nrhs)
        assert rc == 0, lib().slu_last_error().decode()
        assert big[n:].tobytes() == keep[n:].tobytes()
        assert big[:, nrhs:].tobytes() == keep[:, nrhs:].tobytes()
        against_ld("solve_ldb", family, dtype, trans, np.asfortranarray(big[:n, :nrhs]))


# ------------------------------------------------------------------ 8: stale LDS
@pytest.mark.parametrize("family,dtype", [("max511_inner", 0), ("frag_star", 2)])
def test_stale_lds(family, dtype):
    """NaN in every LDS word before a sweep with partial batches and partial
    last panels: finite and unchanged."""
    p = factored(family, dtype)[0]
    bb = synth.rhs(family, dtype)
    b = bb[:, :3]
    for trans in ("N", "T"):
        x1 = p.solve(b, trans=trans)
        assert lib().slu_debug_poison_lds(0) == 0
        x2 = p.solve(b, trans=trans)
        assert np.isfinite(x2).all()
        assert rel(x2, x1) <= BITS[dtype], (trans, rel(x2, x1))
    y1 = p.solve_block(bb)
    assert lib().slu_debug_poison_lds(0) == 0
    y2 = p.solve_block(bb)
    assert np.isfinite(y2).all()
    dif = np.abs(y2 - y1).max(axis=0) / np.abs(y1).max(axis=0)
    assert (dif < tol_of(family, dtype, None, 33)).all(), dif
    against_ld("solve_block_lds", family, dtype, None, y2)
