"""Fused Schur tiles whose two K segments run through one stage loop
(k_schur_big<T, 1> and <T, 2>, csrc/kernels.h; BigCfg<T>::FLAT).

The loop iteration that consumes the first segment's last stage rewrites the
operand pointers and prefetches the second segment's first stage, so what can
go wrong is decided by the stage counts of the two segments.  The shapes here
put them at the boundary (BK = 16 for fp64 / fp32, 8 for complex):

  * dense chains with maxsup = W, both segments K = W: W = 16 (one stage each:
    the only loop iteration is the switching one), W = 8 (fp64 / fp32: that
    stage is partial), W = 17 (two stages, the second of one k), W = 33; complex
    W = 8, 9, 17.  n is about 18 W + 1 (22 W + 1 for W = 8, 20 W + 1 for complex
    W = 9: the third member must keep 129 far rows), so at least two pairs
    form.  A 128-row tile spans more than four destination blocks: these run
    the table-walk epilogue.
  * unequal stage counts: tp.ragged_chain(385, 32) and (513, 128), whose first
    member has kmin = 5 (kw = 27 | 32 and 123 | 128).  The seed moves the
    skyline but not its lowest start, which is 5 for every seed once there are
    a few hundred columns: these cases have two stages before two, and eight
    before eight with a different partial last stage.  A first segment of a
    single stage before a second of several needs starts of at least W - 16:
    deep_ragged_chain draws them from [20, 32) (kw = 12 | 32).
  * the mapped form, tm.bordered(w) under SLU_SCHUR_PAIR_MAP_WASTE=4 with
    w = 16, 17, 40 in all three types, one interleaved and one ragged case
    (bordered(17, ragged=True): kw = 12 | 17, one stage before two).
  * a zero and a tiny pivot in the second member of a W = 16 chain.

Every case is one factorization of n <= about 600 with SLU_AMALG=0, checked as
test_gpu_schur_pair.run checks its own (info and the tiny count exact, L and U
within test_oracle.TOL of the long-double LU and of the oracle), run again
with SLU_SCHUR_PAIR=0, and the plan's pairs are those of the CPU rule.  fp32
keeps one stage loop per segment (BigCfg<float>::FLAT = false); its cases run
the same shapes through that form.

Largest GPU-vs-long-double error seen on an MI355X: d 1.2e-15, z 8.7e-16, s 6.4e-7.
"""
import numpy as np
import pytest

import synth
import test_gpu_schur_pair as tp
import test_gpu_schur_pair_map as tm

pytestmark = pytest.mark.gpu


def deep_ragged_chain(n, w, lo, seed):
    """tp.ragged_chain with the first block's U columns starting at a row in [lo, w)."""
    rng = np.random.default_rng(seed)
    P = tp.chain(n)
    for c in range(w, n):
        P[:rng.integers(lo, w), c] = False
    return P


# W -> n of the dense chains (fp64 / fp32, complex)
CHAIN_N = {16: 289, 8: 177, 17: 307, 33: 595}
CHAIN_N_Z = {8: 177, 9: 181, 17: 307}

FAMILIES = {
    "flat_ragged32_s3": (lambda: tp.ragged_chain(385, 32, seed=3), 32),
    "flat_ragged32_s5": (lambda: tp.ragged_chain(385, 32, seed=5), 32),
    "flat_ragged128_s5": (lambda: tp.ragged_chain(513, 128, seed=5), 128),
    "flat_ragged128_s7": (lambda: tp.ragged_chain(513, 128, seed=7), 128),
    "flat_deep32": (lambda: deep_ragged_chain(385, 32, 20, 3), 32),
    "flat_map16": (lambda: tm.bordered(16), 16),
    "flat_map17": (lambda: tm.bordered(17), 17),
    "flat_map40": (lambda: tm.bordered(40), 40),
    "flat_map_inter16": (lambda: tm.bordered(16, interleave=True), 16),
    "flat_map_ragged17": (lambda: tm.bordered(17, ragged=True), 17),
    "flat_pivot16": (lambda: tp.chain(CHAIN_N[16]), 16),
}
for _w, _n in CHAIN_N.items():
    FAMILIES[f"flat_chain{_w}"] = (lambda n=_n: tp.chain(n), _w)
for _w, _n in CHAIN_N_Z.items():
    FAMILIES[f"flat_zchain{_w}"] = (lambda n=_n: tp.chain(n), _w)
assert all(tp.FAMILIES.get(k, v) is v for k, v in FAMILIES.items()), "family names clash"
tp.FAMILIES.update(FAMILIES)


def segment_widths(name, dtype):
    """Per supernode kw = W - kmin (kmin: the lowest start of its U segments)."""
    A, S, an = tp.case(name, dtype)
    lu = S.distribute()
    w = np.diff(lu.xsup)
    kmin = {}
    for k, t in synth.u_first_rows(lu):
        kmin[k] = min(kmin.get(k, int(w[k])), t)
    return {k: int(w[k]) - t for k, t in kmin.items()}


def stages(kw, dtype):
    bk = 8 if dtype == 2 else 16
    return -(-kw // bk)


def exact_case(monkeypatch, name, dtype, pivot=None, replace_tiny=False, min_pairs=1):
    """tp.on_and_off, the plan's pairs against the CPU rule; returns (info, tiny, counters, pairs)."""
    pairs = tp.expected_pairs(name, dtype)
    kw = segment_widths(name, dtype)
    print(f"{name} dtype {dtype}: pairs {pairs}, kw {[(kw[k], kw[kp]) for k, kp in pairs]}")
    assert len(pairs) >= min_pairs, pairs
    info, tiny, pc = tp.on_and_off(monkeypatch, name, dtype, pivot, replace_tiny)
    assert pc["schur_pairs"] == len(pairs) and pc["schur_fused_tiles"] > 0, (pc, pairs)
    return info, tiny, pc, pairs


# ------------------------------------------------------------------ dense chains
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("W", [16, 8, 17, 33])
def test_dense_chain(W, dtype, monkeypatch):
    name = f"flat_chain{W}"
    A, S, an = tp.case(name, dtype)
    lu = S.distribute()
    assert set(int(w) for w in np.diff(lu.xsup)[:-1]) == {W}
    kw = segment_widths(name, dtype)
    _, _, _, pairs = exact_case(monkeypatch, name, dtype, min_pairs=2)
    assert all(kw[k] == kw[kp] == W for k, kp in pairs), kw


@pytest.mark.parametrize("W", [8, 9, 17])
def test_dense_chain_complex(W, monkeypatch):
    name = f"flat_zchain{W}"
    A, S, an = tp.case(name, 2)
    lu = S.distribute()
    assert set(int(w) for w in np.diff(lu.xsup)[:-1]) == {W}
    kw = segment_widths(name, 2)
    _, _, _, pairs = exact_case(monkeypatch, name, 2, min_pairs=2)
    assert all(kw[k] == kw[kp] == W for k, kp in pairs), kw


# ------------------------------------------------------------------ unequal stage counts
@pytest.mark.parametrize("name,dtype,kws", [("flat_ragged32_s3", 0, (27, 32)), ("flat_ragged32_s5", 0, (27, 32)),
                                            ("flat_ragged32_s5", 2, (27, 32)), ("flat_ragged128_s5", 0, (123, 128)),
                                            ("flat_ragged128_s7", 0, (123, 128)), ("flat_ragged128_s7", 1, (123, 128)),
                                            ("flat_deep32", 0, (12, 32)), ("flat_deep32", 1, (12, 32)),
                                            ("flat_deep32", 2, (12, 32))])
def test_ragged_first_segment(name, dtype, kws, monkeypatch):
    """The pair (0, 1): the first member has kmin > 0 and a kw that is not the second's."""
    kw = segment_widths(name, dtype)
    assert (kw[0], kw[1]) == kws, kw
    A, S, an = tp.case(name, dtype)
    s0 = [t for k, t in synth.u_first_rows(S.distribute()) if k == 0]
    assert len(set(s0)) > 5, "the first member's skyline is not ragged"
    _, _, _, pairs = exact_case(monkeypatch, name, dtype)
    assert (0, 1) in pairs, pairs


def test_single_stage_before_several():
    """CPU side: flat_deep32 is the case of one stage before several, in every type."""
    for dtype in (0, 1, 2):
        kw = segment_widths("flat_deep32", dtype)
        if dtype != 2:
            assert stages(kw[0], dtype) == 1 and stages(kw[1], dtype) == 2, kw
        else:
            assert stages(kw[0], dtype) == 2 and stages(kw[1], dtype) == 4, kw
    kw = segment_widths("flat_map_ragged17", 0)
    assert stages(kw[0], 0) == 1 and stages(kw[2], 0) == 2, kw


# ------------------------------------------------------------------ mapped form
def mapped_case(monkeypatch, name, dtype):
    kw = segment_widths(name, dtype)
    print(f"{name} dtype {dtype}: kw of (M1, M2) {(kw[0], kw[2])}")
    info, tiny, pc, _ = tm.on_and_off(monkeypatch, name, dtype, waste="4")
    assert pc["schur_map_pairs"] == 1 and pc["schur_map_fused_tiles"] > 0, pc
    monkeypatch.delenv("SLU_SCHUR_PAIR_MAP", raising=False)
    monkeypatch.setenv("SLU_SCHUR_PAIR", "0")
    info0, tiny0, pc0 = tp.run(name, dtype)
    assert all(pc0[c] == 0 for c in ("schur_pairs", "schur_fused_tiles", "schur_map_pairs",
                                     "schur_map_fused_tiles")), pc0
    assert (info0, tiny0) == (info, tiny)


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("w", [16, 17, 40])
def test_mapped(w, dtype, monkeypatch):
    """The first segment goes through the row map, with absent rows and empty
    columns; the second is the tile's own."""
    name = f"flat_map{w}"
    exact, mapped = tm.expected(name, dtype, 4.0)
    assert [(k, kp) for k, kp, _, _ in mapped] == [(0, 2)], mapped
    mapped_case(monkeypatch, name, dtype)


@pytest.mark.parametrize("name", ["flat_map_inter16", "flat_map_ragged17"])
def test_mapped_interleaved_and_ragged(name, monkeypatch):
    exact, mapped = tm.expected(name, 0, 4.0)
    assert [(k, kp) for k, kp, _, _ in mapped] == [(0, 2)], mapped
    mapped_case(monkeypatch, name, 0)


# ------------------------------------------------------------------ planted pivot
PIVOT_COL = 16 + 5   # column 5 of the second member of the pair (0, 1)


@pytest.mark.parametrize("replace_tiny", [False, True])
@pytest.mark.parametrize("value", [0.0, 1e-30])
def test_pivot_in_second_member(value, replace_tiny, monkeypatch):
    info, tiny, pc = tp.on_and_off(monkeypatch, "flat_pivot16", 0, (PIVOT_COL, value), replace_tiny)
    assert tiny == int(replace_tiny)
    if value == 0.0 or replace_tiny:
        assert info == (0 if replace_tiny else PIVOT_COL + 1)
    assert pc["schur_pairs"] == len(tp.expected_pairs("flat_pivot16", 0)) >= 2 and pc["schur_fused_tiles"] > 0, pc
