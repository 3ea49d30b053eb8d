"""Kernel-path parity: the engine on matrices whose supernode widths are chosen
on purpose (tests/synth.py), against an unpivoted long-double LU, with the
plan's launch counters (Plan.path_counts()) proving which kernel ran.

Every case is one factorization of n <= 800 on one process: info and the tiny
count exact, L and U within test_oracle.TOL of dense_lu_ref (error = max|mine -
ref| / max|ref|, L and U separately), and where info == 0 also within TOL of
the oracle.  The width sweeps run with SLU_AMALG=0 so that the plan factors the
prescribed partition; some run once more in the default environment, where
nothing of them merges and the plain plan runs again (test_default_amalgamation),
and two mergeable families of synth_sym run through the amalgamated plan
(test_merging_amalgamation).

Which case asserts which counter non-zero:

  diag_generic       wide_chain (root 257), wide_inner, pivot 594 of pivot_chain
  diag_f             edge_chain under SLU_DIAG_STRIPS=0; z families
  diag_f_small       narrow_star z; pivot 259 under SLU_DIAG_WAVE=0
  diag_wave32        narrow32_star; pivot 40 of narrow32_star
  diag_wave64        narrow_star; pivot 259 of narrow_star
  diag_strips        edge_chain, mixed_star, wide_chain; pivot 204 of pivot_chain
  trsm_reg64_pf      narrow_star
  trsm_reg128_pf     edge_chain, mixed_star
  trsm_reg256_pf     edge_chain (129), wide_chain; SLU_TRSM_NARROW=0
  trsm_reg*_nopf     SLU_TRSM_PF=0 on narrow_star (64), edge_chain (128, 256)
  trsm_blk           z families
  trsm_generic       wide_inner (a 300-wide block with panels)
  schur_big          edge_chain, wide_chain; schur128_star / schur129_star (L panels
                     of exactly 128 and 129 rows; d, s, z)
  schur_small        narrow_star
  ksplit_kinfos      ksplit_chain under SLU_KSPLIT_TILES=64

Largest GPU-vs-long-double error seen on an MI355X: d 2.8e-15, z 1.9e-15,
s 1.4e-6 ("Kernel-path parity on synthetic supernodes").
"""
import functools

import numpy as np
import pytest

import cases
import pyoracle
import synth
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
from test_oracle import TOL
from test_synth import TWO_TINY

pytestmark = pytest.mark.gpu

TRSM_REG = [f"trsm_reg{w}_{f}" for w in (64, 128, 256) for f in ("pf", "nopf")]


@functools.lru_cache(maxsize=None)
def oracle_dense(family, dtype, pivot, replace_tiny):
    """The oracle's factors of a family as a dense matrix (cached, read-only)."""
    A, S, V, an = synth.case(family, dtype, pivot)
    ref = S.distribute()
    o = pyoracle.oracle_factor([ref], 1, 1, A.n, replace_tiny, synth.norm_for(an, replace_tiny))
    return synth.lu_to_dense(ref, A.n), o


def run(family, dtype, pivot=None, replace_tiny=False, stats=None):
    """One factorization checked against the long-double LU and the oracle;
    returns (info, tiny, path counts).  Pivot cases compare what
    synth.final_upto calls well defined; info is pinned by the callers.
    stats: a dict that receives the plan's stats."""
    A, S, V, an = synth.case(family, dtype, pivot)
    gpu = S.distribute()
    p = Plan(gpu, replace_tiny=replace_tiny)
    p.upload()
    info, tiny = p.factor(synth.norm_for(an, replace_tiny))
    p.download()
    pc = p.path_counts()
    if stats is not None:
        stats.update(p.stats())
    R, rinfo, rtiny = synth.reference(family, dtype, pivot, replace_tiny)
    upto = synth.final_upto(pivot, replace_tiny)
    M = synth.lu_to_dense(gpu, A.n)
    eL, eU = synth.lu_errors(M, R, upto=upto)
    O, o = oracle_dense(family, dtype, pivot, replace_tiny)
    oL, oU = synth.lu_errors(M, O.astype(R.dtype), upto=upto)
    print(f"{family} dtype {dtype} pivot {pivot} replace {replace_tiny}: info {info} / {rinfo}, "
          f"tiny {tiny} / {rtiny}, GPU vs long double L {eL:.3e} U {eU:.3e}, vs oracle L {oL:.3e} "
          f"U {oU:.3e}; { {k: v for k, v in pc.items() if v} }")
    assert tiny == rtiny == o["tiny"]
    assert max(eL, eU) < TOL[dtype], (eL, eU)
    assert max(oL, oU) < TOL[dtype], (oL, oU)
    if pivot is None:
        assert info == rinfo == o["info"] == 0
    return info, tiny, pc


def fine(monkeypatch):
    monkeypatch.setenv("SLU_AMALG", "0")


def only(pc, keys, among):
    """Of the counters ``among``, exactly ``keys`` are non-zero."""
    assert {k for k in among if pc[k]} == set(keys), pc


DIAG = ["diag_generic", "diag_f", "diag_f_small", "diag_wave32", "diag_wave64", "diag_strips"]


# ------------------------------------------------------------------ width sweeps
@pytest.mark.parametrize("dtype", [0, 1])
def test_narrow_star(dtype, monkeypatch):
    fine(monkeypatch)
    _, _, pc = run("narrow_star", dtype)
    only(pc, ["diag_wave64", "diag_strips"], DIAG)      # the leaves' level, the 130-wide root
    assert pc["diag_wave64"] == 1 and pc["diag_strips"] == 1
    only(pc, ["trsm_reg64_pf"], TRSM_REG)
    assert pc["trsm_reg64_pf"] == 2                     # the L and the U panels
    assert pc["schur_small"] > 0 and pc["schur_big"] == 0   # fewer than 128 rows
    assert pc["trsm_generic"] == pc["trsm_blk"] == 0


@pytest.mark.parametrize("dtype", [0, 1])
def test_narrow32_star(dtype, monkeypatch):
    fine(monkeypatch)
    _, _, pc = run("narrow32_star", dtype)
    only(pc, ["diag_wave32", "diag_strips"], DIAG)
    assert pc["diag_wave32"] == 1
    only(pc, ["trsm_reg64_pf"], TRSM_REG)


@pytest.mark.parametrize("strips", ["1", "0"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_edge_chain(dtype, strips, monkeypatch):
    """65 -> 127 -> 128 -> 129 -> 200: just past the 64-wide diagonal kernels,
    around the 128-wide TRSM instantiation, Schur panels past 128 rows."""
    fine(monkeypatch)
    monkeypatch.setenv("SLU_DIAG_STRIPS", strips)
    _, _, pc = run("edge_chain", dtype)
    only(pc, ["diag_strips" if strips == "1" else "diag_f"], DIAG)
    assert pc["diag_strips"] + pc["diag_f"] == 5
    only(pc, ["trsm_reg128_pf", "trsm_reg256_pf"], TRSM_REG)
    assert pc["trsm_reg128_pf"] == 6 and pc["trsm_reg256_pf"] == 2   # 65, 127, 128 | 129
    assert pc["schur_big"] > 0


@pytest.mark.parametrize("dtype", [0, 1])
def test_wide_chain(dtype, monkeypatch):
    fine(monkeypatch)
    _, _, pc = run("wide_chain", dtype)
    only(pc, ["diag_strips", "diag_generic"], DIAG)     # 255, 256 | the 257-wide root
    assert pc["diag_strips"] == 2 and pc["diag_generic"] == 1
    only(pc, ["trsm_reg256_pf"], TRSM_REG)
    assert pc["trsm_generic"] == 0 and pc["schur_big"] > 0


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_wide_inner(dtype, monkeypatch):
    """300 -> 260: a block wider than 256 that has L and U panels."""
    fine(monkeypatch)
    _, _, pc = run("wide_inner", dtype)
    only(pc, ["diag_generic"], DIAG)
    assert pc["diag_generic"] == 2 and pc["trsm_generic"] == 2
    only(pc, [], TRSM_REG)
    assert pc["trsm_blk"] == 0 and pc["schur_big"] > 0


@pytest.mark.parametrize("strips", ["1", "0"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_mixed_star(dtype, strips, monkeypatch):
    """5, 70, 128 and 64 wide blocks in one level: the widest picks the
    kernel for all of them."""
    fine(monkeypatch)
    monkeypatch.setenv("SLU_DIAG_STRIPS", strips)
    _, _, pc = run("mixed_star", dtype)
    only(pc, ["diag_strips" if strips == "1" else "diag_f", "diag_generic"], DIAG)
    assert pc["diag_strips"] + pc["diag_f"] == 1 and pc["diag_generic"] == 1
    only(pc, ["trsm_reg128_pf"], TRSM_REG)
    assert pc["trsm_reg128_pf"] == 2


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("family", ["schur128_star", "schur129_star"])
def test_schur_tile_edge(family, dtype, monkeypatch):
    """L panels of exactly 128 and 129 rows (test_synth pins the heights):
    the threshold of the 128-row tiles, and a tile of one row."""
    fine(monkeypatch)
    _, _, pc = run(family, dtype)
    assert pc["schur_big"] > 0 and pc["schur_small"] == 0, pc


@pytest.mark.parametrize("family", ["narrow_star", "edge_chain"])
def test_complex(family, monkeypatch):
    fine(monkeypatch)
    _, _, pc = run(family, 2)
    if family == "narrow_star":
        only(pc, ["diag_f_small", "diag_f"], DIAG)      # the leaves | the 130-wide root
        assert pc["schur_small"] > 0
    else:
        only(pc, ["diag_f"], DIAG)
        assert pc["diag_f"] == 5 and pc["schur_big"] > 0
    only(pc, [], TRSM_REG)
    assert pc["trsm_blk"] > 0 and pc["trsm_generic"] == 0


@pytest.mark.parametrize("family,dtype", [(f, d) for f in ("narrow_star", "edge_chain", "wide_chain",
                                                          "mixed_star") for d in (0, 1)] +
                         [("narrow_star", 2), ("edge_chain", 2)])
def test_default_amalgamation(family, dtype, monkeypatch):
    """The default environment on structures that do not merge: synth()'s
    ragged U rows fail the symmetry test of the amalgamation
    (tests/test_synth.py::test_ragged_families_do_not_merge), AmalgPlan::make
    finds no chain and the plain plan runs the prescribed partition."""
    monkeypatch.delenv("SLU_AMALG", raising=False)
    monkeypatch.delenv("SLU_AMALG_ZERO", raising=False)
    st = {}
    run(family, dtype, stats=st)
    assert st["amalg_groups"] == 0 and st["nsupers"] == st["nsupers_in"] == len(synth.FAMILIES[family])


@pytest.mark.parametrize("family,dtype", [(f, d) for f in ("amalg_mixed", "amalg_uchunk") for d in (0, 1, 2)])
def test_merging_amalgamation(family, dtype, monkeypatch):
    """The default environment on structures that merge (synth_sym): the
    amalgamated plan factors the coarse partition, the factors come back in
    the caller's layout (tests/test_gpu_amalg_shapes.py has the relayout's
    own tests)."""
    monkeypatch.delenv("SLU_AMALG", raising=False)
    monkeypatch.delenv("SLU_AMALG_ZERO", raising=False)
    st = {}
    run(family, dtype, stats=st)
    assert st["amalg_groups"] > 0 and st["nsupers"] < st["nsupers_in"]
    assert st["nsupers_in"] == len(synth.sym_widths(synth.SYM_FAMILIES[family]))


# ------------------------------------------------------------------ pivots
# (family, dtype, column, environment, the diagonal kernel that meets the pivot)
PIVOT_CASES = [
    ("narrow32_star", 0, 40, {}, "diag_wave32"),                       # column 20 of the 31-wide leaf
    ("narrow_star", 0, 259, {}, "diag_wave64"),                        # column 40 of the 64-wide leaf
    ("narrow_star", 0, 259, {"SLU_DIAG_WAVE": "0"}, "diag_f_small"),
    ("pivot_chain", 0, 204, {}, "diag_strips"),                        # column 100 of 200: strip 3
    ("pivot_chain", 0, 204, {"SLU_DIAG_STRIPS": "0"}, "diag_f"),
    ("pivot_chain", 0, 594, {}, "diag_generic"),                       # column 290 of 300
    ("pivot_chain", 2, 204, {}, "diag_f"),
    ("pivot_chain", 1, 204, {}, "diag_strips"),
    ("pivot_chain", 1, 594, {}, "diag_generic"),
]


@pytest.mark.parametrize("replace_tiny", [False, True])
@pytest.mark.parametrize("value", [0.0, 1e-30])
@pytest.mark.parametrize("family,dtype,column,env,kernel", PIVOT_CASES)
def test_pivot(family, dtype, column, env, kernel, value, replace_tiny, monkeypatch):
    """One planted pivot, met by one diagonal kernel: a zero pivot without
    replacement gives info = column + 1 exactly; the tiny count is exact
    everywhere, and the factors are the long-double LU's as far as they are
    well defined (all of them with replacement, synth.final_upto without)."""
    fine(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    info, tiny, pc = run(family, dtype, (column, value), replace_tiny)
    assert tiny == int(replace_tiny)
    if value == 0.0 or replace_tiny:      # (an unreplaced 1e-30: synth.final_upto)
        assert info == (0 if replace_tiny else column + 1)
    # the pivot's block went through that kernel: a level is one launch, and
    # the family has one level of that kind (the stars' leaves; pivot_chain:
    # 40 and 64 | 200 | 300 wide, each a level)
    assert pc[kernel] == 1, pc
    if family == "pivot_chain":
        assert pc["diag_generic"] == 1, pc


@pytest.mark.parametrize("family,dtype,column,env,kernel", PIVOT_CASES)
def test_negative_tiny_pivot_keeps_its_sign(family, dtype, column, env, kernel, monkeypatch):
    """A replaced pivot takes the sign of its real part (-1e-30 -> -thresh):
    with the wrong sign the pivot's whole L column flips, far outside TOL."""
    fine(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    info, tiny, pc = run(family, dtype, (column, -1e-30), True)
    assert (info, tiny) == (0, 1)
    assert pc[kernel] == 1, pc


def test_two_tiny_pivots(monkeypatch):
    """Two tiny pivots in two blocks (the 64-wide and the 200-wide)."""
    fine(monkeypatch)
    info, tiny, pc = run("pivot_chain", 0, TWO_TINY, True)
    assert (info, tiny) == (0, 2)
    assert pc["diag_wave64"] == 2 and pc["diag_strips"] == 1     # 40 | 64 | 200


# ------------------------------------------------------------------ runtime branches
BRANCHES = [("SLU_TRSM_PF", "0"), ("SLU_TRSM_2STREAM", "0"), ("SLU_TRSM_NARROW", "0"),
            ("SLU_TRSM_NARROW", "1"), ("SLU_DIAG_WAVE", "0"), ("SLU_REST_SPLIT", "0"),
            ("SLU_REST_SPLIT", "100")]


def check_branch(var, val, pc):
    pf = [k for k in TRSM_REG if k.endswith("_pf")]
    nopf = [k for k in TRSM_REG if k.endswith("_nopf")]
    if var == "SLU_TRSM_PF":
        assert not any(pc[k] for k in pf) and any(pc[k] for k in nopf), pc
    else:
        assert not any(pc[k] for k in nopf) and any(pc[k] for k in pf), pc
    if var == "SLU_TRSM_NARROW":
        assert pc["trsm_reg128_pf"] == 0, pc
        if val == "0":
            assert pc["trsm_reg64_pf"] == 0 and pc["trsm_reg256_pf"] > 0, pc
    if var == "SLU_DIAG_WAVE":
        assert pc["diag_wave32"] == pc["diag_wave64"] == 0, pc


@pytest.mark.parametrize("var,val", BRANCHES)
@pytest.mark.parametrize("family", ["edge_chain", "mixed_star", "narrow_star"])
def test_runtime_branch(family, var, val, monkeypatch):
    fine(monkeypatch)
    monkeypatch.setenv(var, val)
    _, _, pc = run(family, 0)
    check_branch(var, val, pc)
    if var == "SLU_TRSM_PF":
        want = {"edge_chain": ["trsm_reg128_nopf", "trsm_reg256_nopf"], "mixed_star": ["trsm_reg128_nopf"],
                "narrow_star": ["trsm_reg64_nopf"]}[family]
        only(pc, want, TRSM_REG)
    if var == "SLU_TRSM_NARROW":
        # every level's TRSM moves to the 256-wide instantiation, but for the
        # narrow star's leaves under 1 (the 64-wide one stays on)
        only(pc, ["trsm_reg64_pf" if (family, val) == ("narrow_star", "1") else "trsm_reg256_pf"], TRSM_REG)
    if (family, var) == ("narrow_star", "SLU_DIAG_WAVE"):
        only(pc, ["diag_f_small", "diag_strips"], DIAG)


@functools.lru_cache(maxsize=None)
def stencil16():
    """16^3 7-point stencil on the reference structure, with the oracle's factors."""
    A = Csc.stencil(STENCIL_3D7, 16, 16, 16)
    S = Symbolic(A, nd_order(16, 16, 16), 60, 256, reference=True)
    ref = S.distribute()
    an = cases.anorm(A)
    o = pyoracle.oracle_factor([ref], 1, 1, A.n, False, an)
    assert o["info"] == 0
    return A, S, an, (ref.Lval.copy(), ref.Uval.copy())


@pytest.mark.parametrize("var,val", BRANCHES)
def test_runtime_branch_stencil(var, val, monkeypatch):
    monkeypatch.setenv(var, val)
    A, S, an, ref = stencil16()
    gpu = S.distribute()
    p = Plan(gpu)
    p.upload()
    assert p.factor(an) == (0, 0)
    p.download()
    err = cases.factor_error([gpu], [ref])
    assert err < TOL[0], err
    check_branch(var, val, p.path_counts())


@pytest.mark.parametrize("dtype", [0, 1])
def test_ksplit(dtype, monkeypatch):
    """SLU_KSPLIT_TILES: the K range of a near-root update cut into chunks that
    add into the same destinations atomically (parity only: the order of the
    additions is not reproducible)."""
    fine(monkeypatch)
    monkeypatch.setenv("SLU_KSPLIT_TILES", "64")
    _, _, pc = run("ksplit_chain", dtype)
    assert pc["ksplit_kinfos"] > 1 and pc["schur_big"] > 0, pc


def test_ksplit_off_by_default(monkeypatch):
    fine(monkeypatch)
    _, _, pc = run("ksplit_chain", 0)
    assert pc["ksplit_kinfos"] == 0
