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

* the mergeable families (synth.SYM_FAMILIES, synth_sym): the partition is the
  request, the engine's amalgamation (Amalgamation, csrc/amalg.h) merges the
  groups written down here, and every shape the device relayout tests
  (tests/test_gpu_amalg_shapes.py) rely on -- U chunks of exactly 256 and 257
  values, L block columns of 255 / 256 / 257 rows, a block column of more
  than 65536 values, both destination kinds in one chunk -- is recomputed from
  the LUstruct; the host relayout is bit-exact and the oracle on the coarse
  LUstruct agrees with dense_lu_ref.  None of the families of synth.FAMILIES
  merges at all.

Largest oracle-vs-long-double error seen on these families (max over L and U
of max|oracle - ref| / max|ref|): d 2.8e-15, z 2.1e-15, s 1.4e-6; with the
planted pivots d 2.7e-15, z 1.2e-15, s 1.0e-6.  Largest error of the CPU solve
pipeline against ld_solve (normwise per column, 3 columns, N / T / C): d
1.9e-15, z 2.0e-15, s 8.5e-7; ld_solve's own residual at most 4.4e-19.  The
oracle on the coarse LUstructs of the mergeable families against long double:
d 2.0e-15, z 2.2e-15, s 1.1e-6.
"""
import functools

import numpy as np
import pytest

import pyoracle
import synth
from superlu_dist_amd.frontend import Amalgamation
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


# ------------------------------------------------------------------ mergeable families
# family: (coarse widths, merged groups, U chunks per level of the coarse plan)
SYM_EXPECT = {
    "amalg_w256": ([256, 64], 1, [5, 0]),
    "amalg_w257": ([160, 137, 64], 2, [8, 3, 0]),
    "amalg_mixed": ([61, 20, 10, 256, 300], 3, [35, 0]),
    "amalg_uchunk": ([71, 45, 47, 105], 4, [10, 9]),
    "amalg_dense": ([256, 64], 1, [10, 0]),
    "amalg_ones": ([12, 70, 150], 2, [29, 0]),
}
SYM_DTYPES = [(f, d) for f in synth.SYM_FAMILIES for d in (0, 1, 2)]
FAST_MAXW = 256   # csrc: the widest coarse supernode


def u_chunks(lu, am):
    """The k_amalg_u programs of a LUstruct, recomputed from its index arrays:
    per U block row with a non-empty segment, the chunks of at most 64
    non-empty segments in storage order, each a list of (segment length,
    lands in the coarse L: its column is in the row's own group)."""
    xs, x2 = lu.xsup, am.merged.xsup
    grp = lambda col: int(np.searchsorted(x2, col, side="right")) - 1  # noqa: E731
    out = {}
    for k in range(lu.nsupers):
        if lu.Uoff[k] < 0:
            continue
        idx = lu.Uidx[lu.Uoff[k]:]
        segs, p = [], 3
        for _ in range(idx[0]):
            jb = idx[p]
            for c in range(xs[jb + 1] - xs[jb]):
                fst = idx[p + 2 + c]
                if fst < xs[k + 1]:
                    segs.append((int(xs[k + 1] - fst), grp(xs[jb]) == grp(xs[k])))
            p += 2 + xs[jb + 1] - xs[jb]
        if segs:
            out[k] = [segs[i:i + 64] for i in range(0, len(segs), 64)]
    # synth.u_first_rows walks the same segments in the same order
    fr = synth.u_first_rows(lu)
    assert [(k, int(xs[k + 1] - xs[k]) - n) for k in out for ch in out[k] for n, _ in ch] == fr
    return out


def total(ch):
    return sum(n for n, _ in ch)


def ragged(ch):
    return len({n for n, _ in ch}) > 1


def both_kinds(ch):
    return len({kind for _, kind in ch}) == 2


def nsupr(lu, k):
    return int(lu.Lidx[lu.Loff[k] + 1])


def l_rows(lu, k):
    """Global rows of L block column k in storage order."""
    idx = lu.Lidx[lu.Loff[k]:]
    rows, p = [], 2
    for _ in range(idx[0]):
        rows.extend(int(r) for r in idx[p + 2:p + 2 + idx[p + 1]])
        p += 2 + idx[p + 1]
    return rows


@functools.lru_cache(maxsize=None)
def sym_amalg(family):
    """(fine LUstruct, Amalgamation, chunks) of a mergeable family (dtype d:
    the structure does not depend on the dtype, test_sym_partition)."""
    lu = synth.case(family, 0)[1].distribute()
    am = Amalgamation(lu)
    return lu, am, u_chunks(lu, am)


@pytest.mark.parametrize("family,dtype", SYM_DTYPES)
def test_sym_partition(family, dtype):
    """The prescribed partition with the identity perm_c, and what the
    amalgamation makes of it."""
    A, S, V, an = synth.case(family, dtype)
    assert list(np.diff(S.xsup)) == synth.sym_widths(synth.SYM_FAMILIES[family])
    assert np.array_equal(S.perm_c, np.arange(A.n))
    assert np.array_equal(A.to_dense(), V)
    lu = S.distribute()
    if dtype:   # one structure for every dtype
        lu0 = sym_amalg(family)[0]
        assert np.array_equal(lu.Lidx, lu0.Lidx) and np.array_equal(lu.Uidx, lu0.Uidx)
    am = Amalgamation(lu)
    widths, groups, _ = SYM_EXPECT[family]
    assert am.ns1 == lu.nsupers and am.ns2 == len(widths) and am.groups == groups
    assert list(np.diff(am.merged.xsup)) == widths
    assert max(widths) <= FAST_MAXW or max(synth.sym_widths(synth.SYM_FAMILIES[family])) == max(widths)
    # the explicit zeros are the coarse storage minus the caller's.  A member
    # without some row of its parent's leaves zeros in the coarse panel (drop,
    # keep); amalg_dense, whose members the symbolic stage's width limit cut
    # out of one dense chain, has every row and leaves none
    assert am.zeros == am.lval2 + am.uval2 - (lu.Lval.size - 1) - (lu.Uval.size - 1)
    assert (am.zeros == 0) == (family == "amalg_dense") and am.zeros >= 0


def test_sym_edges_width_limit():
    """A group of exactly FAST_MAXW columns merges; at 257 the walk stops and
    a new group starts at the block that did not fit."""
    lu, am, ch = sym_amalg("amalg_w256")
    assert list(np.diff(lu.xsup))[:2] == [100, 156] and am.merged.xsup[1] == FAST_MAXW
    # the same width without explicit zeros: four 64-wide members cut out of
    # one dense chain by the symbolic stage's maxsup = 64
    lu, am, ch = sym_amalg("amalg_dense")
    assert list(np.diff(lu.xsup)) == [64] * 5 and list(am.merged.xsup) == [0, FAST_MAXW, 320] and am.zeros == 0
    assert synth.SYM_FAMILIES["amalg_dense"]["maxsup"] == 64
    lu, am, ch = sym_amalg("amalg_w257")
    assert list(np.diff(lu.xsup))[:3] == [60, 100, 97] and sum(np.diff(lu.xsup)[:3]) == FAST_MAXW + 1
    assert list(am.merged.xsup[:3]) == [0, 160, 297]   # [60, 100] | [97, 40] | root
    # the 300-wide root of amalg_mixed is wider than a group may become and stays alone
    lu, am, ch = sym_amalg("amalg_mixed")
    assert np.diff(am.merged.xsup)[-1] == 300 and np.diff(lu.xsup)[-1] == 300


def test_sym_edges_levels():
    """amalg_mixed: merged groups, unmerged blocks and four groups in the
    first level, so a level's range of the relayout programs holds several
    L items and the chunks of several U rows."""
    lu, am, ch = sym_amalg("amalg_mixed")
    xs, x2 = lu.xsup, am.merged.xsup
    members = np.diff(np.searchsorted(xs, x2))
    assert list(members) == [3, 1, 3, 2, 1]
    lev = synth.levels(am.merged)
    assert list(lev) == [0, 0, 0, 0, 1]
    grp = np.searchsorted(x2, xs[:-1], side="right") - 1
    assert [int((lev[grp] == L).sum()) for L in (0, 1)] == [9, 1]   # U rows (and L block columns) per level


@pytest.mark.parametrize("family", list(synth.SYM_FAMILIES))
def test_sym_edges_idle_waves(family):
    """k_amalg_u runs four chunks per workgroup.  The U chunks per level of
    the coarse plan (synth.levels), as written down in SYM_EXPECT: the count
    of a whole relayout is no multiple of 4 in any family, and neither is a
    level's where the overlapped download compresses level by level;
    amalg_uchunk and amalg_w257 have chunks beyond the first level, so a
    level's launch starts inside the chunk table."""
    lu, am, ch = sym_amalg(family)
    lev = synth.levels(am.merged)
    grp = np.searchsorted(am.merged.xsup, lu.xsup[:-1], side="right") - 1
    per_level = [sum(len(ch[k]) for k in ch if lev[grp[k]] == L) for L in range(lev.max() + 1)]
    assert per_level == SYM_EXPECT[family][2]
    assert sum(per_level) % 4 != 0 and any(c % 4 for c in per_level)
    if family in ("amalg_uchunk", "amalg_w257"):
        assert per_level[0] > 0 and per_level[1] > 0


def test_sym_edges_u_chunks():
    """The chunk totals around the total <= 256 switch of k_amalg_u."""
    lu, am, ch = sym_amalg("amalg_uchunk")
    w = list(np.diff(lu.xsup))
    assert w[:6] == [4, 67, 5, 40, 17, 30]
    # [4, 67] "top": 129 = 2 x 64 + 1 segments of 4: 256, 256 and a chunk of one column
    assert [(len(c), total(c)) for c in ch[0]] == [(64, 256), (64, 256), (1, 4)]
    assert not any(ragged(c) for c in ch[0])
    assert not both_kinds(ch[0][0]) and both_kinds(ch[0][1])          # short path, both kinds
    assert [kind for _, kind in ch[0][1]] == [True] + [False] * 63
    # [5, 40]: 5 + 63 x 4 = 257 on the long path, both kinds; then 38 ragged columns, short path
    assert [n for n, _ in ch[2][0]] == [5] + [4] * 63 and total(ch[2][0]) == 257
    assert both_kinds(ch[2][0])
    assert len(ch[2]) == 2 and len(ch[2][1]) == 38 and total(ch[2][1]) < 200 and ragged(ch[2][1])
    assert {n for n, _ in ch[2][1]} == {1, 2, 3, 4, 5}
    # [17, 30]: ragged, far above 256, both kinds; a short last chunk of 28 columns
    assert len(ch[4][0]) == 64 and total(ch[4][0]) > 400 and ragged(ch[4][0]) and both_kinds(ch[4][0])
    assert len(ch[4][1]) == 28 and ragged(ch[4][1])
    # width 1: 64 segments of one value (the production shape's chunks)
    assert [(len(c), total(c)) for c in ch[6]] == [(64, 64)]
    # amalg_w256: the 100-wide member's ragged chunks of thousands of values,
    # and a last chunk of 4 ragged columns on the short path
    lu, am, ch = sym_amalg("amalg_w256")
    assert all(len(c) == 64 and total(c) > 2000 and ragged(c) for c in ch[0][:-1])
    assert len(ch[0][-1]) == 4 and total(ch[0][-1]) <= 256 and ragged(ch[0][-1])


def test_sym_edges_l_items():
    """k_amalg_l: block columns of 255 / 256 / 257 stored rows (its i += 256
    loop), one of more than 65536 values (AmalgPlan::build_programs cuts it
    into items of 65536 / nsupr columns), and row maps that are not the
    identity."""
    lu, am, ch = sym_amalg("amalg_mixed")
    w = [int(x) for x in np.diff(lu.xsup)]
    assert w == [4, 16, 41, 20, 1, 2, 7, 200, 56, 300]
    assert (nsupr(lu, 0), nsupr(lu, 1), nsupr(lu, 8)) == (257, 255, 256)
    assert (w[7], nsupr(lu, 7)) == (200, 454) and w[7] * nsupr(lu, 7) > 65536
    assert 65536 // nsupr(lu, 7) == 144 < w[7]            # items of 144 and 56 columns
    assert w[9] * nsupr(lu, 9) > 65536 and 65536 // nsupr(lu, 9) == 218 < w[9]
    # the row map of every member of a merged group: position of its stored
    # rows in the coarse block column
    for fam in synth.SYM_FAMILIES:
        lu, am, ch = sym_amalg(fam)
        m = am.merged
        grp = np.searchsorted(m.xsup, lu.xsup[:-1], side="right") - 1
        moved = 0
        for k in range(lu.nsupers):
            J = grp[k]
            pos = {r: i for i, r in enumerate(l_rows(m, J))}
            rows = l_rows(lu, k)
            assert set(rows) <= set(pos)
            mp = [pos[r] for r in rows]
            assert len(set(mp)) == len(mp)
            moved += mp != list(range(len(mp)))
        assert moved >= am.groups, (fam, moved)


def test_sym_edges_ones_chain():
    """amalg_ones: twelve width-1 supernodes, each without one row of its
    parent's, in one group: explicit zeros in the coarse panel."""
    lu, am, ch = sym_amalg("amalg_ones")
    assert list(np.diff(lu.xsup))[:12] == [1] * 12 and am.merged.xsup[1] == 12
    rows = [set(l_rows(lu, k)) for k in range(12)]
    for k in range(11):
        assert k + 1 in rows[k] and len(rows[k + 1] - rows[k]) == 1   # the row left out
    # and nine of them that merge with the 96-wide root
    lu, am, ch = sym_amalg("amalg_uchunk")
    assert list(np.diff(lu.xsup))[6:] == [1] * 9 + [96] and np.diff(am.merged.xsup)[-1] == 105


@pytest.mark.parametrize("family,dtype", SYM_DTYPES)
def test_sym_host_roundtrip(family, dtype):
    """Amalgamation.expand / compress with random values in every position
    of Lval / Uval: bit for bit."""
    lu = synth.case(family, dtype)[1].distribute()
    am = Amalgamation(lu)
    rng = np.random.default_rng(5)
    for a in (lu.Lval, lu.Uval):
        a[:] = rng.standard_normal(a.size) + (1j * rng.standard_normal(a.size) if dtype == 2 else 0)
    am.expand()
    L, U = np.full_like(lu.Lval, np.nan), np.full_like(lu.Uval, np.nan)
    am.compress(L, U)
    np.testing.assert_array_equal(L[:-1], lu.Lval[:-1])
    np.testing.assert_array_equal(U[:-1], lu.Uval[:-1])
    nz = np.count_nonzero(am.merged.Lval) + np.count_nonzero(am.merged.Uval)
    assert nz == np.count_nonzero(lu.Lval[:-1]) + np.count_nonzero(lu.Uval[:-1])


@pytest.mark.parametrize("family,dtype", SYM_DTYPES)
def test_sym_coarse_oracle_matches_long_double(family, dtype):
    """The oracle on the coarse LUstruct, compressed into the caller's
    layout, against dense_lu_ref: the CPU yardstick of the GPU factor tests
    of tests/test_gpu_amalg_shapes.py."""
    A, S, V, an = synth.case(family, dtype)
    lu = S.distribute()
    am = Amalgamation(lu)
    am.expand()
    o = pyoracle.oracle_factor([am.merged], 1, 1, A.n, False, an)
    assert o["info"] == 0 and o["tiny"] == 0
    lu.Lval[:] = np.nan
    lu.Uval[:] = np.nan
    am.compress(lu.Lval, lu.Uval)
    R, info, tiny = synth.reference(family, dtype)
    eL, eU = synth.lu_errors(synth.lu_to_dense(lu, A.n), R)
    print(f"{family} dtype {dtype}: coarse oracle vs long double L {eL:.3e} U {eU:.3e}")
    assert info == 0 and tiny == 0
    assert max(eL, eU) < TOL[dtype], (eL, eU)


@pytest.mark.parametrize("family", list(synth.FAMILIES))
def test_ragged_families_do_not_merge(family):
    """synth()'s ragged U rows lack columns their L columns have as rows, so
    no chain passes the symmetry test of amalg_chains: under the default
    environment these families run the plain plan
    (tests/test_gpu_kernel_paths.py::test_default_amalgamation)."""
    lu = synth.case(family, 0)[1].distribute()
    with pytest.raises(RuntimeError, match="nothing merges"):
        Amalgamation(lu)
