"""Synthetic matrices with prescribed supernodes, and a long-double reference
LU for them (test helpers).

``synth`` builds an unsymmetric, diagonally dominant sparse matrix whose
supernode partition under the reference symbolic stage
(``Symbolic(A, arange(n), relax=1, maxsup=512, reference=True)``) is exactly a
requested list of widths on a requested tree, so a test picks the kernel a
block meets (the engine dispatches on block widths, csrc/engine.hip) instead
of taking whatever nested dissection of a stencil gives it.  ``pivot`` plants
an exact pivot value at any column.

``synth_sym`` builds structurally symmetric, nested matrices on arms of chained
blocks, again with exactly the requested partition: the chains the engine's
amalgamation merges (csrc/amalg.h), which ``synth``'s ragged U never does.

``dense_lu_ref`` is an unpivoted right-looking LU in ``np.longdouble`` with
the tiny-pivot rule of oracle/oracle_impl.h; ``lu_to_dense`` scatters a
factored 1x1 LUstruct into a dense matrix to compare with it; ``ld_solve``
solves with its factors (plain, transposed, conjugate transposed) in long
double, the reference of the solve kernels' tests.
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
    # the solve kernels' edges (tests/test_gpu_solve_shapes.py): width 1 and the
    # G = 1, 2, 8 lane groups of k_sv_utpanel, widths around the 16-column
    # complex panel and the 16-row MFMA fragments (w % 16 in {0, 1, 15})
    "frag_star": _STAR([1, 2, 7, 15, 16, 47, 48, 49], 96),
    # the leaves' L panels have exactly 256 / 257 rows (2/3 of the root): one
    # full 256-row chunk of the panel kernels, and a second chunk of one row
    "lpanel256_star": _STAR([40, 100], 384),
    "lpanel257_star": _STAR([40, 100], 386),
    # a block of the largest width with L and U panels: every thread of the
    # 512-thread diagonal solves is live; 511: a partial last panel of 31
    # (complex: 15) columns that starts mid-wave in the last wavefront
    "max_inner": _CHAIN([512, 200]),
    "max511_inner": _CHAIN([511, 150]),
}
# Families of synth_sym (structurally symmetric and nested: the engine's
# amalgamation merges their chains; tests/test_synth.py pins every edge named
# here by recomputing it from the LUstruct; tests/test_gpu_amalg_shapes.py).
_U257 = [0] + [1] * 63 + [0, 1, 2, 3, 4] * 8   # a 5-wide block's U first rows: 5 + 63 x 4 = 257, then 5 .. 1
SYM_FAMILIES = {
    # one group of exactly 256 columns (FAST_MAXW); the 100-wide member's U
    # row: ragged chunks of 3000 values and a last chunk of 4 columns
    "amalg_w256": {"arms": [[100, 156]], "root": 64},
    # 60 + 100 + 97 = 257: the greedy walk stops at 160 and starts again at
    # the 97-wide block, which takes the 40-wide one
    "amalg_w257": {"arms": [[60, 100, 97, 40]], "root": 64},
    # merged groups of 61, 10 and 256 columns, an unmerged 20-wide block (20 +
    # 300 > 256) and the 300-wide root: four groups in the first level.  L
    # block columns of 257, 255 and 256 stored rows (the 4-, 16- and 56-wide
    # blocks); 200 x 454 and 300 x 300 values: two k_amalg_l items each.  The
    # keep makes the U chunks of the first level 35, not a multiple of 4
    "amalg_mixed": {"arms": [[4, 16, 41], [20], {"widths": [1, 2, 7], "keep": -10}, [200, 56]], "root": 300},
    # the U chunk edges of k_amalg_u.  [4, 67] "top": 129 = 2 x 64 + 1 columns
    # of length 4, chunks of 256, 256 and 4 values, the second with one column
    # in the coarse L and 63 in the coarse U.  [5, 40] with _U257: a chunk of
    # 257 values over 38 columns of the coarse L and 26 of the coarse U, then
    # 38 ragged columns on the short path.  [17, 30]: ragged on the long path,
    # both kinds.  Nine width-1 blocks that merge with the root
    "amalg_uchunk": {"arms": [{"widths": [4, 67], "ufirst": "top"}, {"widths": [5, 40], "ufirst": _U257},
                              [17, 30], {"widths": [1] * 9, "drop": 0, "keep": -1}], "root": 96},
    # no explicit zeros: a dense chain of 256 columns (drop = 0, "top") that the
    # symbolic stage cuts at its supernode width limit, maxsup = 64, and the
    # amalgamation joins again into one group of exactly FAST_MAXW columns in
    # which every member row is present
    "amalg_dense": {"arms": [{"widths": [64, 64, 64, 64], "drop": 0, "ufirst": "top"}], "root": 64, "maxsup": 64},
    # the production shape: a chain of twelve width-1 supernodes, each
    # without one row of its parent's, merged into one group
    "amalg_ones": {"arms": [{"widths": [1] * 12, "drop": 0, "keep": -1}, [30, 40]], "root": 150},
}
MAXSUP = 512


def offsets(blocks):
    return np.concatenate([[0], np.cumsum([w for w, _ in blocks])]).astype(np.int64)


def _valued(P, rng, dtype, pivot):
    """(Csc, dense matrix) with the pattern P: random values, a dominant
    diagonal, planted pivots (synth's docstring)."""
    n = P.shape[0]
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
    return _valued(P, rng, dtype, pivot)


def sym_widths(spec):
    """The prescribed partition of a synth_sym family: the arms' widths in
    order, then the root."""
    arms = [a["widths"] if isinstance(a, dict) else a for a in spec["arms"]]
    return [w for a in arms for w in a] + [spec["root"]]


def synth_sym(spec, seed, dtype, pivot=None):
    """Returns (Csc, dense matrix) of a structurally symmetric, nested matrix
    whose chains the engine's amalgamation merges (csrc/amalg.h; synth()'s
    ragged U never does: U(s,:) lacks columns that L(:,s) has as rows).

    spec: {"arms": [...], "root": width, the defaults "drop" (2), "keep"
    (None), "ufirst" ("ragged"), and "maxsup", the symbolic stage's widest
    supernode for this family (synth.case; 512 if absent)}; an arm is a list of widths, or a dict with
    "widths" and its own drop / keep / ufirst.  Every arm is a chain of blocks
    whose last block hangs on the root.  The rows of L(:,b) below the
    diagonal block:

      last block of an arm   a random 2/3 of the root's columns;
      other blocks           cols(b+1) without ``drop`` random columns (at
                             least one stays; with drop = 0 the symbolic stage
                             makes b and b+1 one supernode unless the
                             family's maxsup cuts them apart), plus the next block's row set --
                             with ``keep``, only that many of it (negative:
                             all but that many), which leaves explicit zeros
                             in the coarse storage and keeps a width-1 block
                             apart from a width-1 parent (drop = 0 there).

    U(b,:) has exactly these columns, one entry of A in each: at a random row
    of b ("ragged"), at b's first row ("top"), or at the given offsets from
    b's first row (an array, cycled over the columns in ascending order; the
    arm's first block only, the others "top").  Elimination of block b - 1
    fills the columns it shares with b from b's first row that b - 1 holds,
    so prescribed first rows are exact in an arm's first block.
    The first column of the next block (of the root) is always among the
    rows: every block then hangs on its parent's first column in the
    elimination tree, whose postorder is the order written, so perm_c is the
    identity and the partition comes out as requested (with a later first row
    the symbolic stage's postorder moves the arm).  Values, pivot: as synth()."""
    rng = np.random.default_rng(seed)
    arms = [dict(a) if isinstance(a, dict) else {"widths": a} for a in spec["arms"]]
    widths = sym_widths(spec)
    xs = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    n = int(xs[-1])
    root = len(widths) - 1
    P = np.zeros((n, n), dtype=bool)
    P[xs[root]:, xs[root]:] = True
    rr = np.arange(xs[root], xs[root + 1])
    b0 = 0
    for arm in arms:
        nb = len(arm["widths"])
        drop, keep, ufirst = (arm.get(k, spec.get(k, d)) for k, d in
                              (("drop", 2), ("keep", None), ("ufirst", "ragged")))
        below = None
        for b in range(b0 + nb - 1, b0 - 1, -1):       # from the arm's last block up
            f, l = int(xs[b]), int(xs[b + 1])
            if below is None:
                rows = np.sort(np.concatenate([rr[:1], rng.choice(rr[1:], size=max(1, (2 * len(rr)) // 3) - 1,
                                                                     replace=False)]))
            else:
                nxt = np.arange(xs[b + 1], xs[b + 2])
                d = min(drop, len(nxt) - 1)              # (at least one row of the parent stays)
                assert d or keep is not None or "maxsup" in spec, \
                    "drop = 0 without keep or a maxsup: the symbolic stage merges b and b + 1"
                if d:
                    nxt = np.sort(np.concatenate([nxt[:1], rng.choice(nxt[1:], size=len(nxt) - d - 1,
                                                                      replace=False)]))
                if keep is not None:
                    k = keep if keep >= 0 else len(below) + keep
                    below = np.sort(rng.choice(below, size=max(1, min(k, len(below))), replace=False))
                rows = np.concatenate([nxt, below])
            P[f:l, f:l] = True
            P[np.ix_(rows, np.arange(f, l))] = True
            if isinstance(ufirst, str):
                assert ufirst in ("ragged", "top")
                off = rng.integers(0, l - f, len(rows)) if ufirst == "ragged" else np.zeros(len(rows), int)
            else:
                off = np.resize(np.asarray(ufirst, dtype=int), len(rows)) if b == b0 else np.zeros(len(rows), int)
                assert ((0 <= off) & (off < l - f)).all()
            P[f + off, rows] = True
            below = rows
        b0 += nb
    return _valued(P, rng, dtype, pivot)


def symbolic(A, maxsup=MAXSUP):
    """The reference symbolic stage on the natural order; the front-end's own
    partitions these matrices differently.  maxsup: the widest supernode (a
    family of SYM_FAMILIES may set its own)."""
    return Symbolic(A, np.arange(A.n, dtype=np.int64), relax=1, maxsup=maxsup, reference=True)


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


def ld_solve(R, b, trans=None):
    """Solve op(B) x = b in long double with the packed factors of
    dense_lu_ref (L strictly lower and unit, U upper), column-oriented.
    trans None: B x = b (L forward, U backward); "T": B^T x = b (U^T forward
    along U's rows, L^T backward along L's rows); "C": the same on conj(R).
    b: (n,) or (n, nrhs); returns x of b's shape in R's dtype."""
    assert trans in (None, "T", "C")
    if trans == "C":
        R = np.conj(R)
    n = R.shape[0]
    b = np.asarray(b)
    x = np.array(b.reshape(n, -1), dtype=R.dtype)
    if trans is None:
        for j in range(n - 1):                  # L y = b
            x[j + 1:] -= np.outer(R[j + 1:, j], x[j])
        for j in range(n - 1, -1, -1):          # U x = y
            x[j] /= R[j, j]
            x[:j] -= np.outer(R[:j, j], x[j])
    else:
        for j in range(n):                      # U^T z = b
            x[j] /= R[j, j]
            x[j + 1:] -= np.outer(R[j, j + 1:], x[j])
        for j in range(n - 1, 0, -1):           # L^T x = z
            x[:j] -= np.outer(R[j, :j], x[j])
    return x.reshape(b.shape)


def ld_inverse(R):
    """B^-1 in long double from the packed factors: ld_solve(R, I), with the
    forward sweep kept to the columns of L^-1 that are non-zero so far."""
    n = R.shape[0]
    x = np.eye(n, dtype=R.dtype)
    for j in range(n - 1):
        x[j + 1:, :j + 1] -= np.outer(R[j + 1:, j], x[j, :j + 1])
    for j in range(n - 1, -1, -1):
        x[j] /= R[j, j]
        x[:j] -= np.outer(R[:j, j], x[j])
    return x


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


def levels(lu):
    """Level of every supernode of a 1x1 LUstruct as the plan counts them
    (csrc/engine.hip: a supernode comes one level after the last one that
    updates it, i.e. that has it among its L block rows or U block columns)."""
    xs = lu.xsup
    lev = np.zeros(lu.nsupers, dtype=np.int64)
    for k in range(lu.nsupers):
        tg = set()
        idx = lu.Lidx[lu.Loff[k]:]
        p = 2
        for _ in range(idx[0]):
            tg.add(int(idx[p]))
            p += 2 + idx[p + 1]
        if lu.Uoff[k] >= 0:
            idx = lu.Uidx[lu.Uoff[k]:]
            p = 3
            for _ in range(idx[0]):
                jb = int(idx[p])
                tg.add(jb)
                p += 2 + xs[jb + 1] - xs[jb]
        for t in tg - {k}:
            lev[t] = max(lev[t], lev[k] + 1)
    return lev


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
    if family in SYM_FAMILIES:
        A, V = synth_sym(SYM_FAMILIES[family], seed, dtype, pivot)
        return A, symbolic(A, SYM_FAMILIES[family].get("maxsup", MAXSUP)), V, cases.anorm(A)
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


# ---- the yardstick of the solve tests: the CPU pipeline against ld_solve
@functools.lru_cache(maxsize=None)
def oracle_lu(family, dtype):
    """A family's 1x1 LUstruct holding the oracle's factors in the family's
    own dtype (cached, read-only)."""
    import pyoracle
    A, S, V, an = case(family, dtype)
    lu = S.distribute()
    o = pyoracle.oracle_factor([lu], 1, 1, A.n, False, an)
    assert o["info"] == 0 and o["tiny"] == 0
    return lu


def rhs(family, dtype, ncols=33):
    """ncols random right-hand sides rounded to the family's dtype (cached,
    read-only, Fortran order)."""
    return _rhs(family, dtype, ncols)


def ld_solution(family, dtype, trans=None, ncols=33):
    """ld_solve of rhs(family, dtype, ncols) with the family's long-double
    factors (cached, read-only)."""
    return _ld_solution(family, dtype, trans, ncols)


def cpu_errors(family, dtype, trans=None, ncols=33):
    """Per column, the error against ld_solution of the CPU pipeline on the
    same right-hand sides and op: the oracle's factors in the family's dtype,
    then the host supernodal solve of lusolve / lusolve_t (which promotes to
    fp64).  Cached, read-only."""
    return _cpu_errors(family, dtype, trans, ncols)


@functools.lru_cache(maxsize=None)
def _rhs(family, dtype, ncols, seed=11):
    """ncols random right-hand sides rounded to the family's dtype (cached,
    read-only, Fortran order)."""
    n = case(family, dtype)[0].n
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((n, ncols))
    if dtype == SLU_Z:
        b = b + 1j * rng.standard_normal((n, ncols))
    b = np.asfortranarray(b.astype(DTYPES[dtype]))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _ld_solution(family, dtype, trans, ncols):
    x = ld_solve(reference(family, dtype)[0], rhs(family, dtype, ncols), trans)
    x.setflags(write=False)
    return x


def col_errors(x, xref):
    """Normwise error per column, max|x - xref| / max|xref|, in xref's precision."""
    x = np.asarray(x).reshape(xref.shape[0], -1)
    xr = xref.reshape(xref.shape[0], -1)
    if not np.isfinite(x).all():
        return np.full(xr.shape[1], np.inf)
    return (np.abs(x.astype(xr.dtype) - xr).max(axis=0) / np.abs(xr).max(axis=0)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _cpu_errors(family, dtype, trans, ncols):
    from lusolve_t import solve_1x1, solve_1x1_t
    lu = oracle_lu(family, dtype)
    b = rhs(family, dtype, ncols)
    cols = [solve_1x1(lu, b[:, r]) if trans is None else solve_1x1_t(lu, b[:, r], conj=trans == "C")
            for r in range(ncols)]
    e = col_errors(np.stack(cols, axis=1), ld_solution(family, dtype, trans, ncols))
    e.setflags(write=False)
    return e
