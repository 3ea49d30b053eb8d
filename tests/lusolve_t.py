"""Host-side TRANSPOSED supernodal solve on a factored 1x1 LUstruct (the
checker of the device's solve_t), the coordinate maps of a transposed solve
for a caller who starts from A, and the unsymmetric test systems.

The LUstruct factors B = Pc Pr diag(R) A diag(C) Pc^T = L U, so
B^T = U^T L^T: U^T z = c is a forward sweep over the supernodes (solve with
the transposed diagonal block, then push along U's row segments), L^T y = z a
backward sweep (pull down L's panel rows, then solve).  Mirrors
lusolve.solve_1x1."""
import numpy as np
import scipy.sparse as sp
from scipy.linalg import solve_triangular

from lusolve import solve_1x1  # noqa: F401  (re-exported for the callers of both)


def solve_1x1_t(lu, b, conj=False):
    """Solve B^T x = b (conj: B^H x = b) with the factors held in lu (1x1 grid)."""
    xs = lu.xsup
    cplx = lu.Lval.dtype == np.complex128
    x = np.array(b, dtype=np.result_type(lu.Lval.dtype, np.complex128 if cplx else np.float64)).copy()
    ns = lu.nsupers
    tr = "C" if conj else "T"
    cj = np.conj if conj else (lambda a: a)
    cols = []
    for k in range(ns):
        w = xs[k + 1] - xs[k]
        idx = lu.Lidx[lu.Loff[k]:]
        ld = idx[1]
        blk = lu.Lval[lu.Lvoff[k]:lu.Lvoff[k] + ld * w].reshape(w, ld).T
        rows, p = [], 2
        for _ in range(idx[0]):
            nr = idx[p + 1]
            rows.extend(idx[p + 2:p + 2 + nr])
            p += 2 + nr
        cols.append((blk, np.array(rows)))
    for k in range(ns):  # forward: U^T z = b
        f, l = xs[k], xs[k + 1]
        blk, rows = cols[k]
        w = l - f
        x[f:l] = solve_triangular(blk[:w], x[f:l], lower=False, trans=tr)
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
                        x[xs[jb] + c] -= cj(v[q:q + seg]) @ x[fst:l]
                    q += seg
                p += 2 + xs[jb + 1] - xs[jb]
    for k in range(ns - 1, -1, -1):  # backward: L^T y = z
        f, l = xs[k], xs[k + 1]
        blk, rows = cols[k]
        w = l - f
        if len(rows) > w:
            x[f:l] -= cj(blk[w:]).T @ x[rows[w:]]
        x[f:l] = solve_triangular(blk[:w], x[f:l], lower=True, unit_diagonal=True, trans=tr)
    return x


def to_lu_coords_t(b, perm_c, C=None):
    """Right-hand side of A^T x = b -> c of B^T y = c: c[perm_c[j]] = C[j] b[j]
    (column j of A is column perm_c[j] of B)."""
    bb = np.asarray(b) * (C if C is not None else 1.0)
    out = np.empty_like(bb)
    out[perm_c] = bb
    return out


def from_lu_coords_t(y, perm_r, perm_c, R=None):
    """Solution of B^T y = c -> x of A^T x = b: x[i] = R[i] y[perm_c[perm_r[i]]]
    (row i of A is row perm_c[perm_r[i]] of B)."""
    x = np.asarray(y)[perm_c[perm_r]]
    return x * (R if R is not None else 1.0)


def op_t(cp, ri, v, conj=False):
    """B^T (or B^H) as a scipy CSR matrix from B's CSC arrays."""
    n = len(cp) - 1
    B = sp.csc_matrix((v, ri, cp), shape=(n, n))
    return (B.conj().T if conj else B.T).tocsr()


def backward_error_t(cp, ri, v, x, b, conj=False):
    """||B^T x - b|| / (||B^T|| ||x||) (inf norms; B^H with conj)."""
    Bt = op_t(cp, ri, v, conj)
    r = Bt @ x - b
    return float(np.abs(r).max() / (abs(Bt).sum(axis=1).max() * np.abs(x).max()))


def unsym_stencil(kind, dims, dtype, seed=13):
    """A stencil's pattern with unsymmetric values: every off-diagonal drawn
    independently from U(-1, -0.1) (complex: an independent imaginary part of
    the same size), the diagonal 7 (7-point and 5-point patterns) or 27
    (27-point), so every row and column is diagonally dominant and no
    pivoting is needed.  Returns the Csc."""
    from superlu_dist_amd.frontend import STENCIL_3D27, Csc
    from superlu_dist_amd.lib import DTYPES
    P = Csc.stencil(kind, *dims, dtype=dtype)
    cp, ri, v = P.arrays()
    n = P.n
    rng = np.random.default_rng(seed)
    val = rng.uniform(-1.0, -0.1, len(ri)).astype(np.complex128 if dtype == 2 else np.float64)
    if dtype == 2:
        val = val + 1j * rng.uniform(-1.0, -0.1, len(ri))
    col = np.repeat(np.arange(n), np.diff(cp))
    val[ri == col] = 27.0 if kind == STENCIL_3D27 else 7.0
    return Csc.from_arrays(n, cp, ri, val.astype(DTYPES[dtype]), dtype)
