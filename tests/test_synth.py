"""The synthetic supernode matrices (tests/synth.py) and their long-double
reference, checked on the CPU before the GPU tests lean on them
(tests/test_gpu_kernel_paths.py):

* the reference symbolic stage gives exactly the requested partition with the
  identity perm_c, and the U panels are ragged (segments that start below
  their block's first row);
* the oracle (oracle/oracle.c) agrees with dense_lu_ref within the project's
  tolerances (test_oracle.TOL), so the two checkers of the GPU tests do not
  contradict each other;
* planted zero and tiny pivots: info and the tiny count of the oracle and of
  dense_lu_ref agree, and so do the factors, as far as they are well defined
  (synth.final_upto; replaced pivots are factored with synth.PIVOT_ANORM, where
  the reasons are written down);
* synth.ld_solve (N / T / C) leaves a residual below 1e-17 against the dense
  matrix, and the CPU pipeline the solve tests are judged against
  (tests/test_gpu_solve_shapes.py: the oracle's factors in the family's dtype,
  then lusolve / lusolve_t) agrees with it within test_oracle.TOL.

Largest oracle-vs-long-double error seen on these families (max over L and U
of max|oracle - ref| / max|ref|): d 2.8e-15, z 2.1e-15, s 1.4e-6; with the
planted pivots d 2.7e-15, z 1.2e-15, s 1.0e-6.  Largest error of the CPU solve
pipeline against ld_solve (normwise per column, 3 columns, N / T / C): d
1.9e-15, z 2.0e-15, s 8.5e-7; ld_solve's own residual at most 4.4e-19.
"""
import numpy as np
import pytest

import pyoracle
import synth
from test_oracle import TOL

FAMILY_DTYPES = [(f, d) for f in synth.FAMILIES for d in (0, 1, 2)]

# (family, dtype, column): every block the GPU pivot cases aim at
#   narrow32_star 40: column 20 of the 31-wide leaf; narrow_star 259: column 40
#   of the 64-wide leaf; pivot_chain 80 / 204 / 594: column 40 of the 64-wide,
#   100 of the 200-wide and 290 of the 300-wide block
PIVOT_SITES = [("narrow32_star", 0, 40), ("narrow_star", 0, 259), ("pivot_chain", 0, 80),
               ("pivot_chain", 0, 204), ("pivot_chain", 0, 594), ("pivot_chain", 2, 204),
               ("pivot_chain", 1, 204), ("pivot_chain", 1, 594)]
TWO_TINY = ((80, 1e-30), (204, 1e-30))


def oracle_vs_ref(family, dtype, pivot=None, replace_tiny=False):
    A, S, V, an = synth.case(family, dtype, pivot)
    lu = S.distribute()
    o = pyoracle.oracle_factor([lu], 1, 1, A.n, replace_tiny, synth.norm_for(an, replace_tiny))
    R, info, tiny = synth.reference(family, dtype, pivot, replace_tiny)
    eL, eU = synth.lu_errors(synth.lu_to_dense(lu, A.n), R, upto=synth.final_upto(pivot, replace_tiny))
    print(f"{family} dtype {dtype} pivot {pivot} replace {replace_tiny}: info {o['info']} / {info}, "
          f"tiny {o['tiny']} / {tiny}, oracle vs long double L {eL:.3e} U {eU:.3e}")
    return o, info, tiny, max(eL, eU)


@pytest.mark.parametrize("family,dtype", FAMILY_DTYPES)
def test_partition_is_the_request(family, dtype):
    A, S, V, an = synth.case(family, dtype)
    assert list(np.diff(S.xsup)) == [w for w, _ in synth.FAMILIES[family]]
    assert np.array_equal(S.perm_c, np.arange(A.n))
    fr = synth.u_first_rows(S.distribute())
    assert any(r > 0 for _, r in fr), "no U segment starts below its block's first row"
    # A's dense copy is the CSC's
    assert np.array_equal(A.to_dense(), V)


@pytest.mark.parametrize("family,rows", [("schur128_star", 128), ("schur129_star", 129)])
def test_schur_edge_families_have_the_panel_heights(family, rows):
    """The leaves' L panels are exactly 128 / 129 rows high, and their U
    panels have at least 128 columns: a Schur update on the 128-row edge."""
    lu = synth.case(family, 0)[1].distribute()
    for k in range(lu.nsupers - 1):
        w = lu.xsup[k + 1] - lu.xsup[k]
        assert lu.Lidx[lu.Loff[k] + 1] - w == rows
        assert sum(1 for kk, _ in synth.u_first_rows(lu) if kk == k) >= 128


@pytest.mark.parametrize("family,rows", [("lpanel256_star", 256), ("lpanel257_star", 257)])
def test_lpanel_edge_families_have_the_panel_heights(family, rows):
    """The leaves' L panels are exactly 256 / 257 rows high: one full 256-row
    chunk of the solve's panel kernels, and a second chunk of a single row."""
    lu = synth.case(family, 0)[1].distribute()
    for k in range(lu.nsupers - 1):
        w = lu.xsup[k + 1] - lu.xsup[k]
        assert lu.Lidx[lu.Loff[k] + 1] - w == rows


OPS = [None, "T", "C"]


@pytest.mark.parametrize("trans", OPS)
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("family", ["frag_star", "max_inner"])
def test_ld_solve_residual(family, dtype, trans):
    """||op(A) x - b||_inf / (||op(A)||_inf ||x||_inf) of ld_solve in long
    double against the dense V, vector and matrix b."""
    A, S, V, an = synth.case(family, dtype)
    R = synth.reference(family, dtype)[0]
    M = np.array(V, dtype=R.dtype)
    M = M.T if trans else M
    M = np.conj(M) if trans == "C" else M
    b = synth.rhs(family, dtype)[:, :3]
    x = synth.ld_solve(R, b, trans)
    assert x.shape == b.shape and x.dtype == R.dtype
    res = (np.abs(M @ x - b).max(axis=0) / (np.abs(M).sum(axis=1).max() * np.abs(x).max(axis=0))).max()
    print(f"{family} dtype {dtype} {trans}: residual {float(res):.3e}")
    assert res < 1e-17, res
    x0 = synth.ld_solve(R, b[:, 0], trans)
    assert x0.shape == (A.n,) and np.array_equal(x0, x[:, 0])
    if dtype != 2:
        assert np.array_equal(synth.ld_solve(R, b, "C"), synth.ld_solve(R, b, "T"))
    if family == "frag_star" and trans is None:   # ld_inverse is ld_solve of the identity
        assert np.array_equal(synth.ld_inverse(R), synth.ld_solve(R, np.eye(A.n)))


@pytest.mark.parametrize("family,dtype", FAMILY_DTYPES)
def test_cpu_pipeline_against_long_double(family, dtype):
    """The yardstick of tests/test_gpu_solve_shapes.py: the oracle's factors
    in the family's dtype, the host solves of lusolve / lusolve_t on them,
    normwise error per column against ld_solve (3 columns, N / T / C)."""
    worst = 0.0
    for trans in OPS:
        if trans == "C" and dtype != 2:
            continue
        e = synth.cpu_errors(family, dtype, trans, 3)
        print(f"{family} dtype {dtype} {trans}: CPU pipeline vs long double {e.max():.3e}")
        worst = max(worst, float(e.max()))
    assert worst < TOL[dtype], worst


def test_pivot_keeps_the_partition():
    base = synth.case("pivot_chain", 0)[1]
    S = synth.case("pivot_chain", 0, (204, 0.0))[1]
    assert np.array_equal(S.xsup, base.xsup) and np.array_equal(S.perm_c, base.perm_c)


@pytest.mark.parametrize("family,dtype", FAMILY_DTYPES)
def test_oracle_matches_long_double(family, dtype):
    o, info, tiny, err = oracle_vs_ref(family, dtype)
    assert o["info"] == info == 0 and o["tiny"] == tiny == 0
    assert err < TOL[dtype], err


@pytest.mark.parametrize("replace_tiny", [False, True])
@pytest.mark.parametrize("value", [0.0, 1e-30])
@pytest.mark.parametrize("family,dtype,column", PIVOT_SITES)
def test_oracle_pivots_match_long_double(family, dtype, column, value, replace_tiny):
    o, info, tiny, err = oracle_vs_ref(family, dtype, (column, value), replace_tiny)
    assert tiny == int(replace_tiny) and o["tiny"] == tiny
    if value == 0.0 or replace_tiny:      # (an unreplaced 1e-30: synth.final_upto)
        assert info == (0 if replace_tiny else column + 1)
        assert o["info"] == info
    assert err < TOL[dtype], err


@pytest.mark.parametrize("family,dtype,column", PIVOT_SITES)
def test_oracle_negative_tiny_pivot_keeps_its_sign(family, dtype, column):
    """A replaced pivot takes the sign of its real part: -1e-30 -> -thresh."""
    o, info, tiny, err = oracle_vs_ref(family, dtype, (column, -1e-30), True)
    assert o["info"] == info == 0 and o["tiny"] == tiny == 1
    assert err < TOL[dtype], err
    R = synth.reference(family, dtype, (column, -1e-30), True)[0]
    assert R[column, column].real == -float(np.float32(synth.S_EPS * synth.PIVOT_ANORM) if dtype == 1
                                            else synth.S_EPS * synth.PIVOT_ANORM)


def test_oracle_two_tiny_pivots_match_long_double():
    o, info, tiny, err = oracle_vs_ref("pivot_chain", 0, TWO_TINY, True)
    assert o["info"] == info == 0 and o["tiny"] == tiny == 2
    assert err < TOL[0], err


def test_dense_lu_ref_reconstructs_the_matrix():
    """L U = A in long double, far below the tolerances it referees."""
    A, S, V, an = synth.case("narrow32_star", 0)
    R, info, tiny = synth.reference("narrow32_star", 0)
    n = A.n
    L = np.tril(R, -1) + np.eye(n, dtype=R.dtype)
    assert np.abs(L @ np.triu(R) - V).max() / np.abs(V).max() < 1e-17
