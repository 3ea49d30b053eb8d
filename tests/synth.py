"""Synthetic matrices with prescribed supernodes, and a long-double reference
LU for them (test helpers).

``synth`` builds an unsymmetric, diagonally dominant sparse matrix whose
supernode partition under the reference symbolic stage
(``Symbolic(A, arange(n), relax=1, maxsup=512, reference=True)``) is exactly a
requested list of widths on a requested tree, so a test picks the kernel a
block meets (the engine dispatches on block widths, csrc/engine.hip) instead
of taking whatever nested dissection of a stencil gives it.  ``pivot`` plants
an exact pivot value at any column.

``dense_lu_ref`` is an unpivoted right-looking LU in ``np.longdouble`` with
the tiny-pivot rule of oracle/oracle_impl.h; ``lu_to_dense`` scatters a
factored 1x1 LUstruct into a dense matrix to compare with it.
"""
import functools

import numpy as np

import cases
from superlu_dist_amd.frontend import Csc, Symbolic
from superlu_dist_amd.lib import DTYPES, SLU_S, SLU_Z

S_EPS = 5.9604644775390625e-08  # FLT_EPSILON * 0.5, smach_dist("Epsilon") for every type

# Families of the kernel-path tests: (width, parent) leaf to root, postorder.
_STAR = lambda leaves, root: [(w, len(leaves)) for w in leaves] + [(root, None)]  # noqa: E731
_CHAIN = lambda ws: [(w, i + 1) for i, w in enumerate(ws[:-1])] + [(ws[-1], None)]  # noqa: E731
FAMILIES = {
    "narrow_star": _STAR([3, 17, 31, 32, 33, 40, 63, 64], 130),
    "narrow32_star": _STAR([3, 17, 31, 32], 130),
    "edge_chain": _CHAIN([65, 127, 128, 129, 200]),
    "wide_chain": _CHAIN([255, 256, 257]),
    "mixed_star": _STAR([5, 70, 128, 64], 257),
    "pivot_chain": _CHAIN([40, 64, 200, 300]),   # the pivot cases' blocks
    "wide_inner": _CHAIN([300, 260]),            # a > 256-wide block with panels
    "ksplit_chain": _CHAIN([256, 300]),
    # the leaves' L panels have exactly 128 / 129 rows (2/3 of the root): one
    # full 128-row Schur tile, and one more tile of a single row
    "schur128_star": _STAR([96, 70], 192),
    "schur129_star": _STAR([96, 70], 194),
}
MAXSUP = 512


def offsets(blocks):
    return np.concatenate([[0], np.cumsum([w for w, _ in blocks])]).astype(np.int64)


def synth(blocks, seed, dtype, pivot=None):
    """Returns (Csc, dense matrix).  pivot: (column, value) or a sequence of
    such pairs; every structural entry of row ``column`` left of the diagonal
    becomes an explicit stored zero and the diagonal entry ``value``, so the
    pivot met at elimination is exactly ``value``."""
    rng = np.random.default_rng(seed)
    xs = offsets(blocks)
    n = int(xs[-1])
    nb = len(blocks)
    root = nb - 1
    assert blocks[root][1] is None
    P = np.zeros((n, n), dtype=bool)
    rr = np.arange(xs[root], xs[root + 1])
    rootset = np.sort(rng.choice(rr, size=max(1, (2 * len(rr)) // 3), replace=False))

    def ragged_u(b, t):
        """U(b, t): each column of block t gets, with probability 0.7-0.8, one
        entry at a random row of block b."""
        p = rng.uniform(0.7, 0.8)
        for c in range(xs[t], xs[t + 1]):
            if rng.random() < p:
                P[rng.integers(xs[b], xs[b + 1]), c] = True

    for b, (w, par) in enumerate(blocks):
        f, l = xs[b], xs[b + 1]
        P[f:l, f:l] = True
        if b == root:
            continue
        assert par is not None and b < par <= root, "blocks must be in postorder"
        P[np.ix_(rootset, np.arange(f, l))] = True
        if par != root:
            pr = np.arange(xs[par], xs[par + 1])
            half = np.sort(rng.choice(pr, size=max(1, len(pr) // 2), replace=False))
            P[np.ix_(half, np.arange(f, l))] = True
            ragged_u(b, par)
        ragged_u(b, root)
    npt = DTYPES[dtype]
    V = rng.uniform(-1.0, 1.0, (n, n))
    if dtype == SLU_Z:
        V = V + 1j * rng.uniform(-1.0, 1.0, (n, n))
    V = np.where(P, V, 0).astype(npt)
    np.fill_diagonal(V, 0)
    a = np.abs(V).astype(np.float64)
    d = 1.05 * np.maximum(a.sum(axis=1), a.sum(axis=0)) + 1.0
    if dtype == SLU_Z:
        d = d * np.exp(2j * np.pi * rng.random(n))
    else:
        d = d * rng.choice([-1.0, 1.0], n)
    V[np.arange(n), np.arange(n)] = d.astype(npt)
    if pivot is not None:
        pv = [pivot] if np.isscalar(pivot[0]) else list(pivot)
        for col, val in pv:
            V[col, :col] = 0      # stays in the pattern P: explicit stored zeros
            V[col, col] = val
    colptr = np.zeros(n + 1, dtype=np.int64)
    ri, vv = [], []
    for j in range(n):
        r = np.nonzero(P[:, j])[0]
        ri.append(r)
        vv.append(V[r, j])
        colptr[j + 1] = colptr[j] + len(r)
    A = Csc.from_arrays(n, colptr, np.concatenate(ri), np.concatenate(vv), dtype)
    return A, V


def symbolic(A):
    """The reference symbolic stage on the natural order; the front-end's own
    partitions these matrices differently."""
    return Symbolic(A, np.arange(A.n, dtype=np.int64), relax=1, maxsup=MAXSUP, reference=True)


def dense_lu_ref(V, thresh=None):
    """Unpivoted right-looking LU of the dense matrix V in long double.
    thresh: replace a pivot with |piv| < thresh by +-thresh (sign of its real
    part; |.| = |re| + |im| for complex; an fp32 matrix stores thresh rounded
    to fp32), oracle/oracle_impl.h:38-39.  A zero pivot records info = j + 1
    (the last one wins) and its column is left unscaled.  Returns (packed
    factors: L strictly lower, U upper; info; tiny count)."""
    cplx = np.iscomplexobj(V)
    single = V.dtype == np.float32
    M = np.array(V, dtype=np.clongdouble if cplx else np.longdouble)
    n = M.shape[0]
    info = tiny = 0
    stored = float(np.float32(thresh)) if thresh is not None and single else thresh
    for j in range(n):
        piv = M[j, j]
        if thresh is not None:
            mag = abs(piv.real) + abs(piv.imag) if cplx else abs(piv)
            if mag < thresh:
                piv = M[j, j] = -stored if piv.real < 0 else stored
                tiny += 1
        if piv == 0:
            info = j + 1
        else:
            M[j + 1:, j] /= piv
        if j + 1 < n:
            M[j + 1:, j + 1:] -= np.outer(M[j + 1:, j], M[j, j + 1:])
    return M, info, tiny


def lu_to_dense(lu, n):
    """The factors of a 1x1 LUstruct as one dense matrix (L strictly lower, U
    upper, both from the diagonal blocks and the panels)."""
    xs = lu.xsup
    M = np.zeros((n, n), dtype=lu.Lval.dtype)
    for k in range(lu.nsupers):
        f, l = int(xs[k]), int(xs[k + 1])
        w = l - f
        idx = lu.Lidx[lu.Loff[k]:]
        ld = int(idx[1])
        blk = lu.Lval[lu.Lvoff[k]:lu.Lvoff[k] + ld * w].reshape(w, ld).T
        rows, p = [], 2
        for _ in range(idx[0]):
            nr = idx[p + 1]
            rows.extend(idx[p + 2:p + 2 + nr])
            p += 2 + nr
        M[np.ix_(np.array(rows, dtype=np.int64), np.arange(f, l))] = blk
        if lu.Uoff[k] >= 0:
            idx = lu.Uidx[lu.Uoff[k]:]
            v = lu.Uval[lu.Uvoff[k]:]
            p, q = 3, 0
            for _ in range(idx[0]):
                jb = idx[p]
                for c in range(xs[jb + 1] - xs[jb]):
                    fst = idx[p + 2 + c]
                    seg = l - fst
                    if seg:
                        M[fst:l, xs[jb] + c] = v[q:q + seg]
                    q += seg
                p += 2 + xs[jb + 1] - xs[jb]
    return M


def u_first_rows(lu):
    """(block, first row of the segment - first row of the block) of every
    nonempty U segment."""
    xs = lu.xsup
    out = []
    for k in range(lu.nsupers):
        if lu.Uoff[k] < 0:
            continue
        idx = lu.Uidx[lu.Uoff[k]:]
        p = 3
        for _ in range(idx[0]):
            jb = idx[p]
            for c in range(xs[jb + 1] - xs[jb]):
                fst = idx[p + 2 + c]
                if fst < xs[k + 1]:
                    out.append((k, int(fst - xs[k])))
            p += 2 + xs[jb + 1] - xs[jb]
    return out


def lu_errors(M, R, upto=None):
    """(error of L, error of U) = max|mine - ref| / max|ref| over the strictly
    lower and the upper triangle.  upto (a zero pivot's column): only what is
    final before that column is eliminated -- L's columns left of it, U's rows
    above it; the rest holds divisions by the zero pivot."""
    assert M.shape == R.shape
    M = np.asarray(M, dtype=R.dtype)
    out = []
    for m, r in ((np.tril(M, -1)[:, :upto], np.tril(R, -1)[:, :upto]),
                 (np.triu(M)[:upto], np.triu(R)[:upto])):
        if m.size == 0:
            out.append(0.0)
        elif not np.isfinite(m).all():
            out.append(float("inf"))   # max() below would drop a NaN
        else:
            out.append(float(np.abs(m - r).max() / max(float(np.abs(r).max()), 1e-300)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case(family, dtype, pivot=None, seed=7):
    """(A, S, dense V, anorm) of a family; cached, treat as read-only."""
    A, V = synth(FAMILIES[family], seed, dtype, pivot)
    return A, symbolic(A), V, cases.anorm(A)


# The norm the pivot cases hand to the factorization where tiny pivots are
# replaced: thresh = S_EPS * anorm = 1.0133 (not a power of two, so its fp32
# rounding and its sign are visible in the factors).  With the matrices' true
# norm (about 600) a replaced pivot is 3.6e-5 and its L column grows to 3e4;
# everything eliminated after it then carries rounding errors amplified by
# the square of that growth, and the oracle itself is 4e-11 (d) / 1e-2 (s)
# away from the long-double LU: the comparison would measure the conditioning
# of the replaced system, not the kernel.  A replaced pivot of about 1 keeps
# the growth at 1, and the kernels' compare / replace / count logic runs the same.
PIVOT_ANORM = 1.7e7


def norm_for(an, replace_tiny):
    return PIVOT_ANORM if replace_tiny else an


def final_upto(pivot, replace_tiny):
    """How much of the factors of a pivot case is well defined, as lu_errors'
    ``upto``.  Replaced pivots: everything (None).  A zero pivot: what is
    final before its column (the rest holds divisions by zero).  An
    unreplaced 1e-30: through its column -- its L column is about 1e30, so
    the Schur complement behind it is a rank-one matrix plus rounding noise
    of 1e14, and neither the later factors nor whether a later pivot cancels
    to exactly zero (info) are properties of the algorithm."""
    if pivot is None or replace_tiny:
        return None
    pv = [pivot] if np.isscalar(pivot[0]) else list(pivot)
    col, val = min(pv)
    return col if val == 0.0 else col + 1


@functools.lru_cache(maxsize=None)
def reference(family, dtype, pivot=None, replace_tiny=False, seed=7):
    """dense_lu_ref of a family's matrix in the LUstruct's coordinates
    (cached): (packed long-double factors, info, tiny)."""
    A, S, V, an = case(family, dtype, pivot, seed)
    B = A.permuted(S.perm_c).to_dense()
    return dense_lu_ref(B, S_EPS * norm_for(an, True) if replace_tiny else None)
