"""The amalgamated plan on synthetic merging chains: AmalgPlan
(csrc/plan_amalg.h), its device relayout k_amalg_l / k_amalg_u
(csrc/amalg_dev.h) and the program builder AmalgPlan::build_programs, on the
mergeable families of tests/synth.py (synth_sym, SYM_FAMILIES), whose shapes
are chosen and pinned on the CPU (tests/test_synth.py, test_sym_*):

  amalg_w256    one group of exactly 256 columns; ragged U chunks of thousands
                of values and a last chunk of 4 columns
  amalg_w257    60 + 100 + 97 = 257: the greedy walk stops and starts again
  amalg_mixed   merged groups, unmerged blocks, four groups in one level; L
                block columns of 255 / 256 / 257 rows; 200 x 454 and 300 x 300
                values: two k_amalg_l items each
  amalg_uchunk  U chunks of exactly 256 (short path) and 257 values (long
                path), a chunk of one column, ragged chunks on both paths,
                coarse-L and coarse-U destinations in one chunk
  amalg_dense   four 64-wide members of one dense chain (the symbolic stage's
                maxsup = 64 cut it) in a group of 256 columns: no explicit zeros
  amalg_ones    twelve width-1 supernodes in one group (the production shape)

Every plan is built with SLU_AMALG and SLU_AMALG_ZERO out of the environment
and its stats say that the amalgamated plan ran (check_plan).  The relayout is
a copy, so the round trip and the fill are compared bit for bit; the factors
are compared with the long-double LU of synth.reference within
test_oracle.TOL, the solves with synth.ld_solve within
test_gpu_solve_shapes.tol_of.  No tolerance is this module's own.

Largest error seen on an MI355X against long double, over the families:

  entry point                     d          z          s
  factors after upload()          1.9e-15    2.2e-15    1.1e-6
  factors after fill_a            1.9e-15    2.2e-15    1.1e-6
  factors, overlapped copies      1.9e-15    2.2e-15    -
  solve                           1.7e-15    1.3e-15    8.4e-7
  solve trans="T"                 1.5e-15    9.7e-16    9.2e-7
  solve trans="C"                 -          1.5e-15    -
  solve_block                     1.3e-15    9.8e-16    7.4e-7
  solve_block trans="T"           1.5e-15    9.8e-16    7.8e-7
  solve_block trans="C"           -          1.0e-15    -
  refine                          8.0e-16    1.1e-15    5.6e-7
  refine trans="T"                7.0e-16    8.2e-16    6.5e-7
  refine trans="C"                -          7.9e-16    -

(the CPU pipeline on the same right-hand sides: d 2.2e-15, z 2.0e-15, s
5.7e-7; the oracle on the coarse LUstruct: tests/test_synth.py).  The round
trip and the fill are exact.

Mutations these tests were checked to catch (each skips work, none writes or
reads out of bounds, none committed):

  k_amalg_u's short path stops at total - 1
      test_device_roundtrip, test_fill_equals_host_distribute, test_factors
      and test_overlapped_copies on amalg_w256, amalg_mixed, amalg_uchunk and
      amalg_ones (amalg_w257 and amalg_dense have no chunk of 256 values or
      fewer); test_overlapped_copies on those of them it runs
  k_amalg_u's long path stops at C.nc - 1
      the same four tests on every family
  k_amalg_l handles only i < 256
      the same four on amalg_w256, amalg_w257, amalg_mixed and amalg_dense
      (the block columns of the other two have fewer than 256 rows)
  AmalgPlan::build_programs emits only the first item of a split block column
      the same four on amalg_mixed only, the family with block columns of
      more than 65536 values
  relayout_levels ends its L items at lx_lev[L1] - 1
      the same four on every family

test_device_roundtrip fails under every one of them.  The solves and the
refinement run on the coarse layout after fill_a and never call the relayout,
so they pass under all five: they pin the sweeps over 256-wide coarse
supernodes with explicit zeros in their panels.
"""
import functools
import os

import numpy as np
import pytest

import synth
from superlu_dist_amd.engine import Plan
from superlu_dist_amd.frontend import Amalgamation
from test_gpu_solve_shapes import DT, OPS, against_ld, refine_abi
from test_oracle import TOL as FTOL

pytestmark = pytest.mark.gpu

FAMS = list(synth.SYM_FAMILIES)
PAIRS = [(f, d) for f in FAMS for d in (0, 1, 2)]


def default_plan(lu, **kw):
    """A plan under the default amalgamation settings, whatever the caller's
    environment says."""
    saved = {k: os.environ.pop(k, None) for k in ("SLU_AMALG", "SLU_AMALG_ZERO")}
    try:
        return Plan(lu, **kw)
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def coarse(family):
    """(blocks, coarse supernodes, merged groups, explicit zeros) of a family
    from the host analysis (the structure is the same for every dtype)."""
    lu = synth.case(family, 0)[1].distribute()
    am = Amalgamation(lu)
    assert am.groups > 0 and am.ns2 < am.ns1 == len(synth.sym_widths(synth.SYM_FAMILIES[family]))
    return am.ns1, am.ns2, am.groups, am.zeros


def check_plan(p, family):
    """a. The amalgamated plan ran, on the coarse partition of the host analysis."""
    ns1, ns2, groups, zeros = coarse(family)
    st = p.stats()
    assert st["nsupers_in"] == ns1 and st["nsupers"] == ns2, st
    assert st["amalg_groups"] == groups and st["amalg_zeros"] == zeros, st
    return st


def random_values(rng, a):
    v = rng.standard_normal(a.size)
    if np.iscomplexobj(a):
        v = v + 1j * rng.standard_normal(a.size)
    return v.astype(a.dtype)


def errors(what, family, dtype, lu):
    """The factors in lu against the long-double LU: no NaN left, L and U
    within test_oracle.TOL, exact zeros where the reference has them."""
    n = lu.n
    R, info, tiny = synth.reference(family, dtype)
    assert info == 0 and tiny == 0
    assert np.isfinite(lu.Lval[:-1]).all() and np.isfinite(lu.Uval[:-1]).all()
    M = synth.lu_to_dense(lu, n)
    eL, eU = synth.lu_errors(M, R)
    print(f"SHAPES {what} N dtype {dtype} {family}: L {eL:.3e} U {eU:.3e}")
    assert max(eL, eU) < FTOL[dtype], (eL, eU)
    assert not M[R == 0].any()
    return eL, eU


# ------------------------------------------------------------------ b: the round trip
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_device_roundtrip(family, dtype):
    """expand (upload) and compress (download) on the device, no
    factorization: R1 goes up and is snapshotted in the coarse layout; R2
    goes up over it, so the caller-layout device copies hold R2; restore puts
    R1 back into the coarse storage and download compresses it.  A position
    the compress skips comes back as R2 or NaN, a value the expand misplaced
    as a wrong R1."""
    lu = synth.case(family, dtype)[1].distribute()
    rng = np.random.default_rng(17)
    r1 = [random_values(rng, a) for a in (lu.Lval, lu.Uval)]
    r2 = [random_values(rng, a) for a in (lu.Lval, lu.Uval)]
    p = default_plan(lu)
    lu.Lval[:], lu.Uval[:] = r1
    p.upload()
    p.snapshot()
    lu.Lval[:], lu.Uval[:] = r2
    p.upload()
    p.restore()
    lu.Lval[:] = np.nan
    lu.Uval[:] = np.nan
    p.download()
    check_plan(p, family)
    for what, got, want in (("L", lu.Lval, r1[0]), ("U", lu.Uval, r1[1])):
        bad = np.nonzero(~(got[:-1] == want[:-1]))[0]
        assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------ c: fill_a
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_fill_equals_host_distribute(family, dtype):
    """fill_a scatters A into the coarse layout; downloaded (compressed) it is
    the front-end's host distribution of the same matrix, bit for bit.  NaN
    goes up first, so a position that fill_a or the compress leaves out comes
    back as NaN and not as whatever fresh device memory holds."""
    A, S, V, an = synth.case(family, dtype)
    lu = S.distribute()
    p = default_plan(lu)
    lu.Lval[:] = np.nan
    lu.Uval[:] = np.nan
    p.upload()
    cp, ri, v = A.arrays()
    p.set_a_pattern(cp, ri)
    p.fill_a(v)
    p.download()
    check_plan(p, family)
    ref = S.distribute()
    assert np.array_equal(lu.Lval[:-1], ref.Lval[:-1]) and np.array_equal(lu.Uval[:-1], ref.Uval[:-1])


# ------------------------------------------------------------------ d: the factors
@functools.lru_cache(maxsize=None)
def factored(family, dtype, fill):
    """(plan with the factors on the device, lu with the factors downloaded
    over NaN); fill: the values come from fill_a, else from upload()."""
    A, S, V, an = synth.case(family, dtype)
    assert np.array_equal(S.perm_c, np.arange(A.n))
    lu = S.distribute()
    p = default_plan(lu)
    if fill:
        cp, ri, v = A.arrays()
        p.set_a_pattern(cp, ri)
        p.fill_a(v)
    else:
        p.upload()
    assert p.factor(an) == (0, 0)
    lu.Lval[:] = np.nan
    lu.Uval[:] = np.nan
    p.download()
    check_plan(p, family)
    return p, lu


@pytest.mark.parametrize("fill", [False, True], ids=["upload", "fill_a"])
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_factors(family, dtype, fill):
    p, lu = factored(family, dtype, fill)
    errors("amalg factor " + ("fill_a" if fill else "upload"), family, dtype, lu)


# ------------------------------------------------------------------ e: overlapped copies
@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("family", ["amalg_mixed", "amalg_w256", "amalg_uchunk", "amalg_dense"])
def test_overlapped_copies(family, dtype, monkeypatch):
    """The drop-in path's copies on the amalgamated plan: the values go up
    beside the plan build, and every level is compressed and written back
    while later levels run (AmalgPlan::build_d2h, relayout_levels(1,
    compressed_to, L + 1)), through 64 KB slots.  amalg_uchunk has U chunks
    in its second level, so that level's k_amalg_u starts inside the chunk
    table; amalg_dense is the plan without explicit zeros."""
    monkeypatch.setenv("SLU_D2H_SLOT_KB", "64")
    A, S, V, an = synth.case(family, dtype)
    lu = S.distribute()
    p = default_plan(lu, overlap_upload=True, overlap_download=True)
    p.upload()
    lu.Lval[:] = np.nan
    lu.Uval[:] = np.nan
    assert p.factor(an) == (0, 0)
    p.download()                           # a no-op: already written back
    st = check_plan(p, family)
    errors("amalg overlapped", family, dtype, lu)
    vb = (lu.Lval.size - 1 + lu.Uval.size - 1) * lu.Lval.itemsize
    assert st["d2h_bytes"] == vb and st["h2d_bytes"] == vb


# ------------------------------------------------------------------ f: the solves
@pytest.mark.parametrize("family,dtype", PAIRS)
def test_solves(family, dtype):
    """solve, solve_block and their transposed forms sweep the coarse
    supernodes (256 wide, explicit zeros in their panels)."""
    p = factored(family, dtype, True)[0]
    b = synth.rhs(family, dtype)
    nb = 17 if dtype == 2 else 33
    for trans in OPS[dtype]:
        t = trans or "N"
        for nrhs in (1, 3 if dtype == 2 else 11):
            x = p.solve(b[:, :nrhs], trans=t)
            assert x.shape == (b.shape[0], nrhs)
            against_ld("amalg solve", family, dtype, trans, x)
        x = p.solve_block(b[:, :nb], trans=t)
        assert x.dtype == DT[dtype]
        against_ld("amalg solve_block", family, dtype, trans, x)


@pytest.mark.parametrize("family,dtype", PAIRS)
def test_refine(family, dtype):
    """One refinement call per op, two columns from zero, ld = n + 5."""
    p = factored(family, dtype, True)[0]
    b = np.asfortranarray(synth.rhs(family, dtype)[:, :2])
    for trans in OPS[dtype]:
        x, berr, steps = refine_abi(p, dtype, trans, b, np.zeros_like(b))
        assert ((1 <= steps) & (steps <= 20)).all(), steps
        against_ld("amalg refine", family, dtype, trans, x)
