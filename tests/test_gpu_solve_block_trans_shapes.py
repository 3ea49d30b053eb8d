"""Kernel parity of the transposed block solve (csrc/solve_block_t.h,
k_svb_ut* / k_svb_lt*) on the synthetic supernode shapes of tests/synth.py
against long double, next to tests/test_gpu_solve_shapes.py: the same
families, plans (SLU_AMALG=0, the prescribed partition), right-hand sides,
reference (synth.ld_solution) and tolerance (tol_of: max(10 x the CPU
pipeline's error, 50 eps) capped by TOL, pinned in tests/test_synth.py).

What the families carry for these kernels: widths 1 / 2 / 7, 15 / 16 / 17,
47 / 48 / 49, 255 / 256 / 257 and 511 / 512 (fragment tails, the tails of a
lane's K run in both panel kernels and in the rows above a partial last
panel of k_svb_ltdiag, the complex 16-column panel, the second round of
k_svb_ltpanel over supernodes wider than 256) and L panels of exactly 256 and
257 rows (a second chunk of one row in the pull).
"""
import numpy as np
import pytest

import synth
from superlu_dist_amd.lib import lib
from test_gpu_solve_shapes import FAMS, OPS, against_ld, factored, tol_of
from test_gpu_solve_trans import assert_unsymmetric

pytestmark = pytest.mark.gpu

CASES = [(f, d, t) for f in FAMS for d in (0, 1, 2) for t in OPS[d] if t]


def ncols_of(dtype):
    """one full pass and a pass with one live column"""
    return 17 if dtype == 2 else 33


@pytest.mark.parametrize("family,dtype,trans", CASES)
def test_solve_block_trans(family, dtype, trans):
    p, lu, (cp, ri, v), V = factored(family, dtype)
    assert_unsymmetric(cp, ri, v)
    nrhs = ncols_of(dtype)
    b = synth.rhs(family, dtype)[:, :nrhs]
    x = p.solve_block(b, trans=trans)
    assert p.solve_block_info()[0] == 2
    against_ld("solve_block_t", family, dtype, trans, x)
    xs = p.solve(b, trans=trans)
    dif = np.abs(x - xs).max(axis=0) / np.abs(xs).max(axis=0)
    assert (dif < tol_of(family, dtype, trans, nrhs)).all(), dif


@pytest.mark.parametrize("family,dtype", [("max511_inner", 0), ("frag_star", 2)])
def test_stale_lds(family, dtype):
    """NaN in every LDS word before a transposed block sweep with partial
    panels, strips, chunks and a partial last pass: finite and within
    tolerance of the run before and of long double."""
    p = factored(family, dtype)[0]
    nrhs = ncols_of(dtype)
    b = synth.rhs(family, dtype)[:, :nrhs]
    for trans in (t for t in OPS[dtype] if t):
        y1 = p.solve_block(b, trans=trans)
        assert lib().slu_debug_poison_lds(0) == 0
        y2 = p.solve_block(b, trans=trans)
        assert np.isfinite(y2).all()
        dif = np.abs(y2 - y1).max(axis=0) / np.abs(y1).max(axis=0)
        assert (dif < tol_of(family, dtype, trans, nrhs)).all(), dif
        against_ld("solve_block_t_lds", family, dtype, trans, y2)
