"""Fused Schur updates of chained supernode pairs (SLU_SCHUR_PAIR, csrc/engine.hip
build_pairs; k_schur_big's two K segments, csrc/kernels.h).

A supernode k and its parent k' one level up form a pair when the rows and U
columns of k beyond block k' are exactly those of k'; the far x far tiles of
k whose twin tile of k' is a rest tile then run one level later, as a first K
segment of the twin.  The families of tests/synth.py do not nest exactly
(their parents take half the rows), so this file builds its own matrices:
dense diagonally dominant blocks under the reference symbolic stage with
maxsup = W, where a dense chain splits into W-wide supernodes whose far
structures are equal by construction.

Every case is one factorization of n <= about 1000 on one process with
SLU_AMALG=0, checked as test_gpu_kernel_paths.run does -- info and the tiny
count exact, L and U within test_oracle.TOL of the long-double LU and of the
oracle -- and run once more with SLU_SCHUR_PAIR=0, where both counters are 0.
The pairs the plan forms are also counted here from the LUstruct's row and
column lists (pairs_by_rule), independently of the engine.

Largest GPU-vs-long-double error seen on an MI355X with fused tiles: d 1.4e-15,
z 7.6e-16, s 7.8e-7.  The stencil cases run at 17^3 / 18^3, the smallest cubes
that form a fused tile (STENCIL_NX below).  Plans on process grids pair nothing
(Plan::build_pairs returns at once for them): the last case runs the dense
chain on a 2x2 grid over the host transport (tests/gridrun_pair.py).  The
issue speaks of five full members for n = 769, W = 128; 769 = 6 * 128 + 1, so
the chain has six 128-wide members and one column: five updates with big
tiles (641 ... 129 rows), two pairs and an odd one out, as the issue counts.
"""
import functools
import os

import numpy as np
import pytest

import cases
import pyoracle
import synth
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
from superlu_dist_amd.lib import DTYPES, SLU_Z
from gridrun_pair import run_grid_pair
from test_oracle import TOL

pytestmark = pytest.mark.gpu

BIG_BN = {0: 128, 1: 128, 2: 64}  # columns of a big tile (BigCfg<T>::BN)


# ------------------------------------------------------------------ matrices
def from_pattern(P, seed, dtype, pivot=None):
    """(Csc, dense V) with the boolean pattern P (full diagonal): uniform
    off-diagonal values, a dominant diagonal of random sign / phase, planted
    pivots as synth.synth plants them."""
    rng = np.random.default_rng(seed)
    n = P.shape[0]
    npt = DTYPES[dtype]
    V = rng.uniform(-1.0, 1.0, (n, n))
    if dtype == SLU_Z:
        V = V + 1j * rng.uniform(-1.0, 1.0, (n, n))
    V = np.where(P, V, 0).astype(npt)
    np.fill_diagonal(V, 0)
    a = np.abs(V).astype(np.float64)
    d = 1.05 * np.maximum(a.sum(axis=1), a.sum(axis=0)) + 1.0
    d = d * (np.exp(2j * np.pi * rng.random(n)) if dtype == SLU_Z else rng.choice([-1.0, 1.0], n))
    V[np.arange(n), np.arange(n)] = d.astype(npt)
    if pivot is not None:
        col, val = pivot
        V[col, :col] = 0      # stays in the pattern: explicit stored zeros
        V[col, col] = val
    colptr = np.zeros(n + 1, dtype=np.int64)
    ri, vv = [], []
    for j in range(n):
        r = np.nonzero(P[:, j])[0]
        ri.append(r)
        vv.append(V[r, j])
        colptr[j + 1] = colptr[j] + len(r)
    return Csc.from_arrays(n, colptr, np.concatenate(ri), np.concatenate(vv), dtype), V


def chain(n):
    return np.ones((n, n), dtype=bool)


def ragged_chain(n, w, seed=3):
    """Dense chain whose first block's U columns right of the block start at a
    random row s_c >= 5 of the block (the last row kept): kmin > 0 and a
    ragged ct0 for the first member, full segments (fill) for the second."""
    rng = np.random.default_rng(seed)
    P = chain(n)
    for c in range(w, n):
        P[:rng.integers(5, w), c] = False
    return P


def two_chains(w, members, border):
    """Two dense chains on the diagonal plus a dense border they both update."""
    m = w * members
    n = 2 * m + border
    P = np.zeros((n, n), dtype=bool)
    P[:m, :m] = P[m:2 * m, m:2 * m] = True
    P[2 * m:, :] = P[:, 2 * m:] = True
    return P


# name -> (pattern builder, maxsup)
FAMILIES = {
    "chain128": (lambda: chain(769), 128),      # 6 full members + 1 column: updates of 641 ... 129 rows
    "chain65": (lambda: chain(647), 65),        # K = 65 + 65, far offset 65; second members of 517, 387, 257 rows
    "chain200": (lambda: chain(740), 200),      # K = 200 + 200: both segments end in a partial stage
    "ragged128": (lambda: ragged_chain(513, 128), 128),
    "two_chains": (lambda: two_chains(128, 3, 260), 128),   # n = 1028
    "chain24": (lambda: chain(409), 24),        # a 128-row tile spans 6 destination blocks: table walk
    "pivot128": (lambda: chain(513), 128),
}


@functools.lru_cache(maxsize=None)
def case(name, dtype, pivot=None):
    """(A, S, anorm) of a family; cached, read-only."""
    build, maxsup = FAMILIES[name]
    A, V = from_pattern(build(), 11, dtype, pivot)
    S = Symbolic(A, np.arange(A.n, dtype=np.int64), relax=1, maxsup=maxsup, reference=True)
    return A, S, cases.anorm(A)


@functools.lru_cache(maxsize=None)
def reference(name, dtype, pivot=None, replace_tiny=False):
    A, S, an = case(name, dtype, pivot)
    B = A.permuted(S.perm_c).to_dense()
    return synth.dense_lu_ref(B, synth.S_EPS * synth.norm_for(an, True) if replace_tiny else None)


@functools.lru_cache(maxsize=None)
def oracle_dense(name, dtype, pivot=None, replace_tiny=False):
    A, S, an = case(name, dtype, pivot)
    ref = S.distribute()
    o = pyoracle.oracle_factor([ref], 1, 1, A.n, replace_tiny, synth.norm_for(an, replace_tiny))
    return synth.lu_to_dense(ref, A.n), o


# ------------------------------------------------------------------ the rule, from the index arrays
def structure(lu):
    """Per supernode: (global rows below the diagonal block, their blocks,
    global columns of the nonempty U segments, their blocks)."""
    xs = lu.xsup
    out = []
    for k in range(lu.nsupers):
        idx = lu.Lidx[lu.Loff[k]:]
        rows, rblk, p = [], [], 2
        for _ in range(idx[0]):
            gb, nr = int(idx[p]), int(idx[p + 1])
            if gb != k:
                rows.extend(int(r) for r in idx[p + 2:p + 2 + nr])
                rblk.extend([gb] * nr)
            p += 2 + nr
        cols, cblk = [], []
        if lu.Uoff[k] >= 0:
            idx = lu.Uidx[lu.Uoff[k]:]
            p = 3
            for _ in range(idx[0]):
                jb = int(idx[p])
                for c in range(int(xs[jb + 1] - xs[jb])):
                    if idx[p + 2 + c] < xs[k + 1]:
                        cols.append(int(xs[jb]) + c)
                        cblk.append(jb)
                p += 2 + int(xs[jb + 1] - xs[jb])
        out.append((rows, rblk, cols, cblk))
    return out


def levels(st):
    lv = [0] * len(st)
    for k, (_, rblk, _, cblk) in enumerate(st):
        for b in set(rblk) | set(cblk):
            lv[b] = max(lv[b], lv[k] + 1)
    return lv


def pairs_by_rule(lu, dtype):
    """The pairs of the issue's rule, greedily from the first member of every
    chain; also the supernodes whose far structure differs from their
    parent's although both run big tiles (for the non-matching case)."""
    st = structure(lu)
    lv = levels(st)
    bn = BIG_BN[dtype]
    taken, pairs, mismatched = set(), [], []
    for k, (rows, rblk, cols, cblk) in enumerate(st):
        if k in taken or len(rows) < 128 or len(cols) < bn:
            continue
        kp = rblk[0]
        if cblk[0] != kp or lv[kp] != lv[k] + 1 or kp in taken:
            continue
        nr0, nc0 = rblk.count(kp), cblk.count(kp)
        prow, _, pcol, _ = st[kp]
        if len(rows) - nr0 < 128 or len(cols) - nc0 < bn:
            continue
        if rows[nr0:] == prow and cols[nc0:] == pcol:
            pairs.append((k, kp))
            taken.update((k, kp))
        else:
            mismatched.append((k, kp))
    return pairs, mismatched


# ------------------------------------------------------------------ one factorization
def factor(S, an, replace_tiny=False):
    gpu = S.distribute()
    p = Plan(gpu, replace_tiny=replace_tiny)
    p.upload()
    info, tiny = p.factor(synth.norm_for(an, replace_tiny))
    p.download()
    return gpu, info, tiny, p.path_counts()


def run(name, dtype, pivot=None, replace_tiny=False):
    """As test_gpu_kernel_paths.run, on this file's families."""
    A, S, an = case(name, dtype, pivot)
    gpu, info, tiny, pc = factor(S, an, replace_tiny)
    R, rinfo, rtiny = reference(name, dtype, pivot, replace_tiny)
    upto = synth.final_upto(pivot, replace_tiny)
    M = synth.lu_to_dense(gpu, A.n)
    eL, eU = synth.lu_errors(M, R, upto=upto)
    O, o = oracle_dense(name, dtype, pivot, replace_tiny)
    oL, oU = synth.lu_errors(M, O.astype(R.dtype), upto=upto)
    print(f"{name} dtype {dtype} pivot {pivot} replace {replace_tiny} pair {os.environ.get('SLU_SCHUR_PAIR', '1')}: "
          f"info {info} / {rinfo}, tiny {tiny} / {rtiny}, GPU vs long double L {eL:.3e} U {eU:.3e}, vs oracle "
          f"L {oL:.3e} U {oU:.3e}; pairs {pc['schur_pairs']} fused {pc['schur_fused_tiles']} "
          f"big {pc['schur_big']} small {pc['schur_small']}")
    assert tiny == rtiny == o["tiny"]
    assert max(eL, eU) < TOL[dtype], (eL, eU)
    assert max(oL, oU) < TOL[dtype], (oL, oU)
    if pivot is None:
        assert info == rinfo == o["info"] == 0
    return info, tiny, pc


def on_and_off(monkeypatch, name, dtype, pivot=None, replace_tiny=False):
    """The case with the default setting, then with SLU_SCHUR_PAIR=0 (today's
    schedule: both counters 0); returns the first run's (info, tiny, counters)."""
    monkeypatch.setenv("SLU_AMALG", "0")
    monkeypatch.delenv("SLU_SCHUR_PAIR", raising=False)
    out = run(name, dtype, pivot, replace_tiny)
    monkeypatch.setenv("SLU_SCHUR_PAIR", "0")
    info0, tiny0, pc0 = run(name, dtype, pivot, replace_tiny)
    assert pc0["schur_pairs"] == 0 and pc0["schur_fused_tiles"] == 0, pc0
    assert (info0, tiny0) == out[:2]
    return out


def expected_pairs(name, dtype):
    A, S, an = case(name, dtype)
    return pairs_by_rule(S.distribute(), dtype)[0]


# ------------------------------------------------------------------ cases
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_dense_chain_128(dtype, monkeypatch):
    """Updates of 641, 513, 385, 257 and 129 rows (and one of a single row):
    two pairs and an odd one out; the second members' tile grids end in a
    tile of one row and one column."""
    A, S, an = case("chain128", dtype)
    lu = S.distribute()
    assert [int(w) for w in np.diff(lu.xsup)] == [128] * 6 + [1]
    _, _, pc = on_and_off(monkeypatch, "chain128", dtype)
    assert len(expected_pairs("chain128", dtype)) == 2
    assert pc["schur_pairs"] == 2 and pc["schur_fused_tiles"] > 0, pc


@pytest.mark.parametrize("dtype", [0, 1])
def test_dense_chain_65(dtype, monkeypatch):
    """K = 65 per segment (no multiple of the stage depth), an odd far offset,
    and a second member of 257 rows: its fused tiles include the one-row one."""
    A, S, an = case("chain65", dtype)
    lu = S.distribute()
    assert set(int(w) for w in np.diff(lu.xsup)[:-1]) == {65}
    pairs = expected_pairs("chain65", dtype)
    assert any(len(structure(lu)[kp][0]) == 257 for _, kp in pairs)
    _, _, pc = on_and_off(monkeypatch, "chain65", dtype)
    assert pc["schur_pairs"] == len(pairs) == 3 and pc["schur_fused_tiles"] > 0, pc


def test_dense_chain_200(monkeypatch):
    """K = 200 + 200: the last stage of each segment is partial."""
    _, _, pc = on_and_off(monkeypatch, "chain200", 0)
    assert pc["schur_pairs"] == len(expected_pairs("chain200", 0)) == 1 and pc["schur_fused_tiles"] > 0, pc


@pytest.mark.parametrize("dtype", [0, 1])
def test_ragged_first_segment(dtype, monkeypatch):
    A, S, an = case("ragged128", dtype)
    first = synth.u_first_rows(S.distribute())
    s0 = [t for k, t in first if k == 0]
    assert min(s0) >= 5 and len(set(s0)) > 20, "the first member's skyline is not ragged"
    assert all(t == 0 for k, t in first if k == 1), "the second member's segments are not full"
    _, _, pc = on_and_off(monkeypatch, "ragged128", dtype)
    assert pc["schur_pairs"] == 1 and pc["schur_fused_tiles"] > 0, pc


def level_log(S, an, capfd):
    """One more factorization with the per-level table (timing 2, stderr):
    the rows as lists of numbers (level, nsup, diag, trsm, big, small, atomic,
    ..., wall_ms, fused)."""
    gpu = S.distribute()
    p = Plan(gpu, timing=2)
    p.upload()
    capfd.readouterr()
    p.factor(an)
    p.stats()
    rows = []
    for line in capfd.readouterr().err.splitlines():
        tok = line.split()
        if line.startswith("[slu rank 0]") and len(tok) > 10 and tok[3].isdigit():
            rows.append([float(x) for x in tok[3:]])
    return rows


@pytest.mark.parametrize("dtype", [0, 1])
def test_two_chains_into_one_border(dtype, monkeypatch, capfd):
    """The members of both chains share levels and destinations (atomic
    KInfos); there are pairs in both chains."""
    A, S, an = case("two_chains", dtype)
    pairs = expected_pairs("two_chains", dtype)
    firsts = {k for k, _ in pairs}
    assert 0 in firsts and 3 in firsts, pairs     # the first members of the two chains
    _, _, pc = on_and_off(monkeypatch, "two_chains", dtype)
    assert pc["schur_pairs"] == len(pairs) and pc["schur_fused_tiles"] > 0, pc
    # the level log: tiles of colliding KInfos on the chains' levels, and the
    # fused column adds up to the counter
    monkeypatch.delenv("SLU_SCHUR_PAIR", raising=False)
    rows = level_log(S, an, capfd)
    assert rows, "no level log"
    assert sum(r[6] for r in rows[:3]) > 0, rows          # atomic tiles on levels 0-2
    assert sum(r[-1] for r in rows) == pc["schur_fused_tiles"], rows


def test_slow_path_tile(monkeypatch):
    """24-wide members: a 128-row tile spans six destination blocks, more than
    the epilogue tables hold, so the fused tiles scatter by the table walk."""
    _, _, pc = on_and_off(monkeypatch, "chain24", 0)
    assert pc["schur_pairs"] == len(expected_pairs("chain24", 0)) > 0 and pc["schur_fused_tiles"] > 0, pc


PIVOT_COL = 128 + 50   # column 50 of the second member of the pair (0, 1)


@pytest.mark.parametrize("replace_tiny", [False, True])
@pytest.mark.parametrize("value", [0.0, 1e-30])
def test_pivot_in_second_member(value, replace_tiny, monkeypatch):
    info, tiny, pc = on_and_off(monkeypatch, "pivot128", 0, (PIVOT_COL, value), replace_tiny)
    assert tiny == int(replace_tiny)
    if value == 0.0 or replace_tiny:
        assert info == (0 if replace_tiny else PIVOT_COL + 1)
    assert pc["schur_pairs"] == 1 and pc["schur_fused_tiles"] > 0, pc


def test_non_matching_parent(monkeypatch):
    """synth's edge_chain: every parent takes half of its child's rows, so no
    far structure equals the parent's and nothing pairs."""
    monkeypatch.setenv("SLU_AMALG", "0")
    A, S, V, an = synth.case("edge_chain", 0)
    pairs, mismatched = pairs_by_rule(S.distribute(), 0)
    assert pairs == [] and mismatched, (pairs, mismatched)
    gpu, info, tiny, pc = factor(S, an)
    R, rinfo, rtiny = synth.reference("edge_chain", 0)
    eL, eU = synth.lu_errors(synth.lu_to_dense(gpu, A.n), R)
    assert (info, tiny) == (0, 0) and max(eL, eU) < TOL[0], (info, tiny, eL, eU)
    assert pc["schur_big"] > 0 and pc["schur_pairs"] == 0 and pc["schur_fused_tiles"] == 0, pc


# 16^3 forms no fused tile: on the reference structure (SLU_AMALG=0) the rows
# inside a block are not sorted, so almost no far row list equals the parent's
# entry for entry, and the one pair of the amalgamated 16^3 has only critical
# twins.  The smallest cubes with a fused tile (pairs_by_rule on the CPU, nx =
# 16 ... 32): 17^3 on the reference structure, 18^3 with the default
# amalgamation (17^3 has none there; 25^3 is the first with both).
STENCIL_NX = {"0": 17, "default": 18}


@functools.lru_cache(maxsize=None)
def stencil(nx):
    """7-point stencil on the reference structure with maxsup 64, with the oracle's factors."""
    A = Csc.stencil(STENCIL_3D7, nx, nx, nx)
    S = Symbolic(A, nd_order(nx, nx, nx), 60, 64, reference=True)
    ref = S.distribute()
    an = cases.anorm(A)
    o = pyoracle.oracle_factor([ref], 1, 1, A.n, False, an)
    assert o["info"] == 0
    return A, S, an, (ref.Lval.copy(), ref.Uval.copy())


@pytest.mark.parametrize("amalg", ["default", "0"])
def test_stencil(amalg, monkeypatch):
    if amalg == "0":
        monkeypatch.setenv("SLU_AMALG", "0")
    nx = STENCIL_NX[amalg]
    A, S, an, ref = stencil(nx)
    for pair in ("1", "0"):
        monkeypatch.setenv("SLU_SCHUR_PAIR", pair)
        gpu = S.distribute()
        p = Plan(gpu)
        p.upload()
        assert p.factor(an) == (0, 0)
        p.download()
        pc = p.path_counts()
        err = cases.factor_error([gpu], [ref])
        print(f"stencil {nx}^3 amalg {amalg} pair {pair}: err {err:.3e}, pairs {pc['schur_pairs']} "
              f"fused {pc['schur_fused_tiles']} big {pc['schur_big']}")
        assert err < TOL[0], err
        if pair == "1":
            assert pc["schur_fused_tiles"] > 0, pc
        else:
            assert pc["schur_pairs"] == 0 and pc["schur_fused_tiles"] == 0, pc


class _Fac:
    def __init__(self, d):
        self.Lval, self.Uval = d["L"], d["U"]


def test_grid_plan_pairs_nothing(monkeypatch, tmp_path):
    """2x2 grid on the host transport, the switch on: both counters 0 on every
    rank (the chain forms two pairs on one process), factors as the oracle's."""
    monkeypatch.setenv("SLU_AMALG", "0")
    monkeypatch.delenv("SLU_SCHUR_PAIR", raising=False)
    out = run_grid_pair(2, 2, "chain128", 0, tmp_path)
    A, S, an = case("chain128", 0)
    lus = [S.distribute(2, 2, r, c) for r in range(2) for c in range(2)]
    o = pyoracle.oracle_factor(lus, 2, 2, A.n, False, an)
    assert o["info"] == 0 and all(int(x["info"]) == 0 and int(x["tiny"]) == 0 for x in out)
    for x in out:
        assert int(x["schur_pairs"]) == 0 and int(x["schur_fused_tiles"]) == 0, x
    assert sum(int(x["schur_big"]) + int(x["schur_small"]) for x in out) > 0
    err = cases.factor_error([_Fac(x) for x in out], [(lu.Lval, lu.Uval) for lu in lus])
    assert err < TOL[0], err
