"""Fused Schur updates of mapped supernode pairs (SLU_SCHUR_PAIR_MAP, csrc/engine.hip
build_pairs second pass; k_schur_big<T, 2>, csrc/kernels.h).

Among the supernodes the exact rule of tests/test_gpu_schur_pair.py leaves
free, k and its parent k' one level up also pair where the far rows and
columns of k are in-order subsequences of the rows and columns of k': k' has
rows of other subtrees besides.  A rest tile of k' that holds a row and a
column of k then runs the far part of k through a row map and mapped column
tables as its first K segment.

The matrices (bordered below) are a dense chain of W-wide members M1, M2, ...
over a dense border.  Every member is connected to the border part B1; a leaf
(min(64, W) columns) is connected to M2 and to the border part B2, so M2 and
the later members gain B2 by fill and M1 lacks it: (M1, M2) is the mapped pair.
Two things differ from the issue's sketch of the pattern, both because the
rule itself would otherwise form another pair:
  * the leaf stands between M1 and M2, not before the chain: the mapped pass
    goes by ascending k, and a leaf numbered before M1 would take M2 for itself
    (its own far rows, B2, are a subsequence of M2's too);
  * a second leaf between M2 and M3, connected to M3 and to a third border
    part B3 of 100 rows (too few for a pair of its own), gives M3 rows that M2
    lacks; with M2's far rows equal to M3's rows the exact pass, which runs
    first, would pair (M2, M3) and leave M1 without a free parent.

Every case is one factorization of n <= about 1100 on one process with
SLU_AMALG=0, checked as test_gpu_schur_pair.run does -- info and the tiny count
exact, L and U within test_oracle.TOL of the long-double LU and of the oracle
-- and run once more with SLU_SCHUR_PAIR_MAP=0, where the map counters are 0
(schur_big / schur_small count launches, and the mapped tiles of a level are
one more launch, so those are not compared).  The exact counters equal
pairs_by_rule's of the existing file in both runs; the mapped pairs are
counted here from the LUstruct's lists (mapped_pairs_by_rule), independently
of the engine.

Largest GPU-vs-long-double error seen on an MI355X with mapped fused tiles:
d 9.1e-16, z 6.8e-16, s 4.3e-7.

Padding.  A fused tile of k' computes its first segment on all its rows and
columns; the share computed for nothing is what SLU_SCHUR_PAIR_MAP_WASTE caps
(default 0.05).  With 150-row border parts no family stays under 5 %, so
every family names the cap it runs under (WASTE below), and PADDED records the
padded share of its mapped pair (whole-tile work of the tiles of k' that hold
a row and a column of k, over the far part's own, minus 1; computed on the
CPU by padded_share, asserted in test_rule_and_padding).  The rule alone
decides: each family's share lies on the stated side of its cap by a margin.
"""
import numpy as np
import pytest

import cases
import pyoracle
import synth
import gridrun_pair
import gridrun_pair_map
import test_gpu_schur_pair as tp
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import Amalgamation
from test_oracle import TOL

pytestmark = pytest.mark.gpu

BIG_BN = tp.BIG_BN


# ------------------------------------------------------------------ matrices
def bordered(w, members=3, b1=150, b2=150, b3=100, interleave=False, rows=True, cols=True, ragged=False):
    """M1 | leaf | M2 | leaf2 | M3 [| M4 ...] | border (B1, B2, B3), see the
    module docstring.  interleave: the rows of B1 and B2 alternate.  rows /
    cols: whether M2 gains B2 in L (rows) / in U (columns); with one of them
    off the pattern is unsymmetric.  ragged: the U columns of M1 right of its
    block start at a random row >= 5 of the block (as tp.ragged_chain)."""
    lw = min(64, w)
    sizes = [w, lw, w, lw] + [w] * (members - 2)
    off = np.concatenate([[0], np.cumsum(sizes)])
    m0 = int(off[-1])
    n = m0 + b1 + b2 + b3
    blk = lambda i: np.arange(off[i], off[i + 1])  # noqa: E731
    chain = np.concatenate([blk(0), blk(2)] + [blk(i) for i in range(4, len(sizes))])
    leaf, leaf2, M2, M3 = blk(1), blk(3), blk(2), blk(4)
    b12 = np.arange(m0, m0 + b1 + b2)
    if interleave:
        assert b1 == b2
        B1, B2 = b12[0::2], b12[1::2]
    else:
        B1, B2 = b12[:b1], b12[b1:]
    B3 = np.arange(m0 + b1 + b2, n)
    border = np.arange(m0, n)
    P = np.zeros((n, n), dtype=bool)

    def sym(a, b):
        P[np.ix_(a, b)] = True
        P[np.ix_(b, a)] = True

    sym(chain, chain)
    sym(border, border)
    sym(chain, B1)
    sym(leaf, leaf)
    sym(leaf, M2)
    if rows:
        P[np.ix_(B2, leaf)] = True   # L(B2, leaf): with U(leaf, M2), fill in L(B2, M2)
    if cols:
        P[np.ix_(leaf, B2)] = True   # U(leaf, B2): with L(M2, leaf), fill in U(M2, B2)
    sym(leaf2, leaf2)
    sym(leaf2, M3)
    sym(leaf2, B3)
    if ragged:
        rng = np.random.default_rng(3)
        for c in range(w, n):
            if P[0, c]:
                P[:rng.integers(5, w), c] = False
    return P


# name -> (pattern builder, maxsup); registered with the existing file's
# families, so that its case / reference / oracle_dense / run serve these too
FAMILIES = {
    "trail128": (lambda: bordered(128), 128),                                   # n = 912
    "inter128": (lambda: bordered(128, interleave=True), 128),
    "inter128_rows": (lambda: bordered(128, interleave=True, cols=False), 128),
    "inter128_cols": (lambda: bordered(128, interleave=True, rows=False), 128),
    "edge128": (lambda: bordered(128, b1=129, b2=128), 128),    # M2 has 128 + 129 + 128 = 385 rows: tiles of one row
    "trail65": (lambda: bordered(65, members=4), 65),           # both segments end in a partial stage
    "mragged128": (lambda: bordered(128, ragged=True), 128),    # ragged first segment under the column tables
    "trail24": (lambda: bordered(24, members=4), 24),           # table-walk epilogue
    "four128": (lambda: bordered(128, members=4), 128),         # n = 1040
    "mpivot128": (lambda: bordered(128), 128),
}
assert all(tp.FAMILIES.get(k, v) is v for k, v in FAMILIES.items()), "family names clash"
tp.FAMILIES.update(FAMILIES)

# the cap every family runs under (PADDED below: the padded shares)
WASTE = {name: "4" for name in FAMILIES}


# ------------------------------------------------------------------ the rule, from the index arrays
def subsequence_map(sub, full):
    """Per entry of full: its index in sub, or -1; None unless sub is an in-order subsequence."""
    out, p = [-1] * len(full), 0
    for q, v in enumerate(full):
        if p < len(sub) and v == sub[p]:
            out[q] = p
            p += 1
    return out if p == len(sub) else None


def tile_facts(st, lv, k, kp, bn):
    """(rmap, cmap, whole-tile work, far elements in fused tiles, fused tiles,
    one critical row range and one critical column range?) of the candidate (k, kp)."""
    rows, rblk, cols, cblk = st[k]
    prow, prblk, pcol, pcblk = st[kp]
    nr0, nc0 = rblk.count(kp), cblk.count(kp)
    rmap, cmap = subsequence_map(rows[nr0:], prow), subsequence_map(cols[nc0:], pcol)
    if rmap is None or cmap is None:
        return None
    tm, tn = -(-len(prow) // 128), -(-len(pcol) // bn)
    rc = [sum(q >= 0 for q in rmap[i * 128:(i + 1) * 128]) for i in range(tm)]
    cc = [sum(q >= 0 for q in cmap[j * bn:(j + 1) * bn]) for j in range(tn)]
    crow = [any(lv[b] == lv[kp] + 1 for b in prblk[i * 128:(i + 1) * 128]) for i in range(tm)]
    ccol = [any(lv[b] == lv[kp] + 1 for b in pcblk[j * bn:(j + 1) * bn]) for j in range(tn)]

    def one_range(m, crit, B):
        q = [v for i, v in enumerate(m) if v >= 0 and crit[i // B]]
        return not q or max(q) - min(q) + 1 == len(q)

    work = fused_el = fused = 0
    for i in range(tm):
        for j in range(tn):
            if rc[i] and cc[j]:
                work += min(128, len(prow) - i * 128) * min(bn, len(pcol) - j * bn)
                if not crow[i] and not ccol[j]:
                    fused_el += rc[i] * cc[j]
                    fused += 1
    return rmap, cmap, work, fused_el, fused, one_range(rmap, crow, 128) and one_range(cmap, ccol, bn)


def mapped_pairs_by_rule(lu, dtype, waste):
    """(exact pairs, mapped pairs as (k, kp, fused tiles, padded share)): the
    exact pass of tp.pairs_by_rule, then the mapped pass over the supernodes
    it left free, ascending k: same size and level conditions, the
    subsequence test, one critical range each way, a fused tile at all, and
    the tile-level padding cap."""
    st = tp.structure(lu)
    lv = tp.levels(st)
    bn = BIG_BN[dtype]
    exact, _ = tp.pairs_by_rule(lu, dtype)
    taken = {k for p in exact for k in p}
    mapped = []
    for k, (rows, rblk, cols, cblk) in enumerate(st):
        if k in taken or len(rows) < 128 or len(cols) < bn:
            continue
        kp = rblk[0]
        if cblk[0] != kp or lv[kp] != lv[k] + 1 or kp in taken:
            continue
        fm, fn = len(rows) - rblk.count(kp), len(cols) - cblk.count(kp)
        if fm < 128 or fn < bn:
            continue
        f = tile_facts(st, lv, k, kp, bn)
        if f is None or not f[5] or not f[4] or f[2] > (1.0 + waste) * fm * fn:
            continue
        mapped.append((k, kp, f[4], f[2] / (fm * fn) - 1.0))
        taken.update((k, kp))
    return exact, mapped


def padded_share(name, dtype):
    """Padded share of the family's pair (0, 2) = (M1, M2), whatever the cap."""
    A, S, an = tp.case(name, dtype)
    lu = S.distribute()
    st = tp.structure(lu)
    rows, rblk, cols, cblk = st[0]
    f = tile_facts(st, tp.levels(st), 0, 2, BIG_BN[dtype])
    return f[2] / ((len(rows) - rblk.count(2)) * (len(cols) - cblk.count(2))) - 1.0


def expected(name, dtype, waste):
    A, S, an = tp.case(name, dtype)
    return mapped_pairs_by_rule(S.distribute(), dtype, waste)


# ------------------------------------------------------------------ one case, map on and off
def on_and_off(monkeypatch, name, dtype, pivot=None, replace_tiny=False, waste=None):
    """The case with the family's cap, then with SLU_SCHUR_PAIR_MAP=0 (the
    parent schedule); both against the rule; returns the first run's (info, tiny, counters)."""
    monkeypatch.setenv("SLU_AMALG", "0")
    monkeypatch.delenv("SLU_SCHUR_PAIR", raising=False)
    monkeypatch.delenv("SLU_SCHUR_PAIR_MAP", raising=False)
    waste = WASTE[name] if waste is None else waste
    if waste == "default":
        monkeypatch.delenv("SLU_SCHUR_PAIR_MAP_WASTE", raising=False)
    else:
        monkeypatch.setenv("SLU_SCHUR_PAIR_MAP_WASTE", waste)
    exact, mapped = expected(name, dtype, 0.05 if waste == "default" else float(waste))
    info, tiny, pc = tp.run(name, dtype, pivot, replace_tiny)
    print(f"{name} dtype {dtype} waste {waste}: map pairs {pc['schur_map_pairs']} map fused "
          f"{pc['schur_map_fused_tiles']}; rule: exact {exact} mapped {mapped}")
    assert pc["schur_pairs"] == len(exact), (pc, exact)
    assert pc["schur_map_pairs"] == len(mapped), (pc, mapped)
    assert pc["schur_map_fused_tiles"] == sum(m[2] for m in mapped), (pc, mapped)
    monkeypatch.setenv("SLU_SCHUR_PAIR_MAP", "0")
    info0, tiny0, pc0 = tp.run(name, dtype, pivot, replace_tiny)
    assert pc0["schur_map_pairs"] == 0 and pc0["schur_map_fused_tiles"] == 0, pc0
    assert pc0["schur_pairs"] == len(exact), (pc0, exact)
    assert (info0, tiny0) == (info, tiny)
    return info, tiny, pc, pc0


def members_k2_tiles(name, dtype):
    A, S, an = tp.case(name, dtype)
    rows, _, cols, _ = tp.structure(S.distribute())[2]
    return -(-len(rows) // 128) * -(-len(cols) // BIG_BN[dtype])


# ------------------------------------------------------------------ cases
# padded share of (M1, M2) per family, fp64 tiles (128 x 128); the complex
# tiles (128 x 64) of trail128: 0.590
PADDED = {"trail128": 0.908, "inter128": 1.370, "inter128_rows": 0.540, "inter128_cols": 0.540, "edge128": 1.233,
          "trail65": 0.881, "mragged128": 0.908, "trail24": 0.672, "four128": 0.590, "mpivot128": 0.908}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_rule_and_padding(name):
    """CPU side of case 1: the recorded padded shares, each well inside its
    family's cap of 4 and well beyond the default 0.05, and (M1, M2) is what
    the rule forms under the cap and nothing under the default."""
    share = padded_share(name, 0)
    print(f"{name}: padded share {share:.3f}")
    assert abs(share - PADDED[name]) < 0.01, share
    assert 0.05 * 2 < share < 4.0 / 2
    exact, mapped = expected(name, 0, 4.0)
    assert [(k, kp) for k, kp, _, _ in mapped] == [(0, 2)], mapped
    assert (0, 2) not in [(k, kp) for k, kp, _, _ in expected(name, 0, 0.05)[1]]


def test_pair_under_the_default_cap(monkeypatch):
    """edge128 under the default cap: (M1, M2) pads too much, and the leaf,
    next in line, pairs with M2 instead: its 128 far rows are the last rows of
    M2 (a map of -1, then the identity; padded share 0.016)."""
    exact, mapped = expected("edge128", 0, 0.05)
    assert [(k, kp) for k, kp, _, _ in mapped] == [(1, 2)] and mapped[0][3] < 0.02, mapped
    _, _, pc, _ = on_and_off(monkeypatch, "edge128", 0, waste="default")
    assert pc["schur_map_pairs"] == 1 and pc["schur_map_fused_tiles"] > 0, pc


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_trailing_extras(dtype, monkeypatch):
    """Case 2: the maps are the identity, then -1; the tiles of M2 wholly inside B2 stay plain."""
    A, S, an = tp.case("trail128", dtype)
    lu = S.distribute()
    st = tp.structure(lu)
    f = tile_facts(st, tp.levels(st), 0, 2, BIG_BN[dtype])
    nfar = len(st[0][0]) - st[0][1].count(2)
    assert f[0] == list(range(nfar)) + [-1] * (len(st[2][0]) - nfar), "row map: identity, then -1"
    _, _, pc, _ = on_and_off(monkeypatch, "trail128", dtype)
    assert pc["schur_map_pairs"] == 1
    assert 0 < pc["schur_map_fused_tiles"] < members_k2_tiles("trail128", dtype), pc


@pytest.mark.parametrize("name", ["inter128", "inter128_rows", "inter128_cols"])
def test_interleaved_extras(name, monkeypatch):
    """Case 3: every tile row (column) of M2 is half absent; rows only and U
    columns only are unsymmetric patterns.  Under the default cap the same
    matrix forms no mapped pair and gives the same factors."""
    A, S, an = tp.case(name, 0)
    st = tp.structure(S.distribute())
    (r0, _, c0, _), (r2, _, c2, _) = st[0], st[2]
    extra_r, extra_c = len(r2) - (len(r0) - 128), len(c2) - (len(c0) - 128)
    assert (extra_r > 0) == (name != "inter128_cols") and (extra_c > 0) == (name != "inter128_rows"), (extra_r, extra_c)
    _, _, pc, _ = on_and_off(monkeypatch, name, 0)
    assert pc["schur_map_pairs"] == 1 and pc["schur_map_fused_tiles"] > 0, pc
    _, _, pcd, _ = on_and_off(monkeypatch, name, 0, waste="default")
    assert pcd["schur_map_pairs"] == 0, pcd


@pytest.mark.parametrize("name,dtype", [("edge128", 0), ("trail65", 0), ("trail65", 1), ("mragged128", 0),
                                        ("mragged128", 1), ("trail24", 0)])
def test_edges(name, dtype, monkeypatch):
    """Case 4: one-row and one-column tiles, partial last stages in both
    segments, a ragged first segment, the table-walk epilogue."""
    if name == "mragged128":
        A, S, an = tp.case(name, dtype)
        s0 = [t for k, t in synth.u_first_rows(S.distribute()) if k == 0]
        assert min(s0) >= 5 and len(set(s0)) > 20, "the first member's skyline is not ragged"
    if name == "edge128":
        A, S, an = tp.case(name, dtype)
        assert len(tp.structure(S.distribute())[2][0]) % 128 == 1
    _, _, pc, _ = on_and_off(monkeypatch, name, dtype)
    assert pc["schur_map_pairs"] == 1 and pc["schur_map_fused_tiles"] > 0, pc


def level_log(S, an, capfd):
    """As tp.level_log; the rows end (..., wall_ms, mapped, fused)."""
    return tp.level_log(S, an, capfd)


def test_critical_region(monkeypatch, capfd):
    """Case 5: four members; the far part of M1 has destinations in the panels
    of M3, two levels up, which must be added at M1's own level."""
    _, _, pc, _ = on_and_off(monkeypatch, "four128", 0)
    assert pc["schur_map_pairs"] == 1
    A, S, an = tp.case("four128", 0)
    monkeypatch.delenv("SLU_SCHUR_PAIR_MAP", raising=False)
    rows = level_log(S, an, capfd)
    assert rows, "no level log"
    assert rows[0][4] > 0, rows[0]                                  # big tiles on level 0
    assert sum(r[-2] for r in rows) == pc["schur_map_fused_tiles"] > 0, rows
    assert rows[1][-2] == pc["schur_map_fused_tiles"], rows[1]      # all on the level of M2
    assert sum(r[-1] for r in rows) == pc["schur_fused_tiles"], rows


PIVOT_COL = 128 + 64 + 50   # column 50 of M2


@pytest.mark.parametrize("replace_tiny", [False, True])
@pytest.mark.parametrize("value", [0.0, 1e-30])
def test_pivot_in_second_member(value, replace_tiny, monkeypatch):
    """Case 6."""
    info, tiny, pc, _ = on_and_off(monkeypatch, "mpivot128", 0, (PIVOT_COL, value), replace_tiny)
    assert tiny == int(replace_tiny)
    if value == 0.0 or replace_tiny:
        assert info == (0 if replace_tiny else PIVOT_COL + 1)
    assert pc["schur_map_pairs"] == 1 and pc["schur_map_fused_tiles"] > 0, pc


# Case 7.  The smallest cubes (7-point, ND order, maxsup 64) that form a mapped
# fused tile under the default cap, found with mapped_pairs_by_rule on the CPU
# over nx = 6 ... 32.  On the reference structure (SLU_AMALG=0) the subsequence
# test does find pairs, from 10^3 on (two of one fused tile each, padded
# 1.6 %; every size above has some).  On the amalgamated structure
# (Amalgamation(lu).merged) the default cap admits a pair only at 25^3 (one
# pair, 9 fused tiles, no padding) and at 32^3 (two); with a cap of 4 there
# are pairs from 16^3 on (1, 5, 8, 8, 8, 12, ... pairs).
STENCIL_NX = {"default": 25, "0": 10}


@pytest.mark.parametrize("amalg", ["default", "0"])
def test_stencil(amalg, monkeypatch):
    nx = STENCIL_NX[amalg]
    if amalg == "0":
        monkeypatch.setenv("SLU_AMALG", "0")
    monkeypatch.delenv("SLU_SCHUR_PAIR_MAP_WASTE", raising=False)
    A, S, an, ref = tp.stencil(nx)
    lu = S.distribute()
    exact, mapped = mapped_pairs_by_rule(lu if amalg == "0" else Amalgamation(lu).merged, 0, 0.05)
    assert mapped and (nx, len(mapped), sum(m[2] for m in mapped)) in ((25, 1, 9), (10, 2, 2)), mapped
    for sw in ("1", "0"):
        monkeypatch.setenv("SLU_SCHUR_PAIR_MAP", sw)
        gpu = S.distribute()
        p = Plan(gpu)
        p.upload()
        assert p.factor(an) == (0, 0)
        p.download()
        pc = p.path_counts()
        err = cases.factor_error([gpu], [ref])
        print(f"stencil {nx}^3 amalg {amalg} map {sw}: err {err:.3e}, map pairs {pc['schur_map_pairs']} "
              f"map fused {pc['schur_map_fused_tiles']} pairs {pc['schur_pairs']} big {pc['schur_big']}")
        assert err < TOL[0], err
        assert pc["schur_pairs"] == len(exact), (pc, exact)
        if sw == "1":
            assert pc["schur_map_pairs"] == len(mapped), (pc, mapped)
            assert pc["schur_map_fused_tiles"] == sum(m[2] for m in mapped) > 0, pc
        else:
            assert pc["schur_map_pairs"] == 0 and pc["schur_map_fused_tiles"] == 0, pc


def test_non_nesting_parent(monkeypatch):
    """Case 8: synth's edge_chain, whose parents have fewer rows than their
    children: no far list is a subsequence of the parent's, nothing pairs."""
    monkeypatch.setenv("SLU_AMALG", "0")
    monkeypatch.setenv("SLU_SCHUR_PAIR_MAP_WASTE", "4")
    A, S, V, an = synth.case("edge_chain", 0)
    exact, mapped = mapped_pairs_by_rule(S.distribute(), 0, 4.0)
    assert exact == [] and mapped == [], (exact, mapped)
    gpu, info, tiny, pc = tp.factor(S, an)
    R, rinfo, rtiny = synth.reference("edge_chain", 0)
    eL, eU = synth.lu_errors(synth.lu_to_dense(gpu, A.n), R)
    assert (info, tiny) == (0, 0) and max(eL, eU) < TOL[0], (info, tiny, eL, eU)
    assert pc["schur_big"] > 0 and pc["schur_map_pairs"] == 0 and pc["schur_map_fused_tiles"] == 0, pc


def test_grid_plan_pairs_nothing(monkeypatch, tmp_path):
    """Case 9: the trailing-extras matrix on a 2x2 grid over the host
    transport: all four counters 0 on every rank, factors as the oracle's."""
    monkeypatch.setenv("SLU_AMALG", "0")
    monkeypatch.setenv("SLU_SCHUR_PAIR_MAP_WASTE", "4")
    monkeypatch.delenv("SLU_SCHUR_PAIR", raising=False)
    monkeypatch.delenv("SLU_SCHUR_PAIR_MAP", raising=False)
    monkeypatch.setattr(gridrun_pair, "_worker", gridrun_pair_map._worker)
    out = gridrun_pair.run_grid_pair(2, 2, "trail128", 0, tmp_path)
    A, S, an = tp.case("trail128", 0)
    lus = [S.distribute(2, 2, r, c) for r in range(2) for c in range(2)]
    o = pyoracle.oracle_factor(lus, 2, 2, A.n, False, an)
    assert o["info"] == 0 and all(int(x["info"]) == 0 and int(x["tiny"]) == 0 for x in out)
    for x in out:
        assert all(int(x[c]) == 0 for c in ("schur_pairs", "schur_fused_tiles", "schur_map_pairs",
                                            "schur_map_fused_tiles")), x
    assert sum(int(x["schur_big"]) + int(x["schur_small"]) for x in out) > 0
    err = cases.factor_error([tp._Fac(x) for x in out], [(lu.Lval, lu.Uval) for lu in lus])
    assert err < TOL[0], err
