"""Transposed block solve and refinement against the per-column transposed
calls on one GPU, with the protocol of
tools/solve_block_prof.py and tools/refine_block_prof.py: lap3d nx^3 through
the front end, one plan per leg, and on that plan, for each nrhs of the leg,
the two calls alternate on the same b after a warm-up of each, `reps`
repetitions:
  (d) fp64, trans "T", nrhs 1, 8, 32, 64: solve(trans) against
      solve_block(trans); the untransposed solve_block runs in the same
      alternation, for the ratio of a transposed to an untransposed pass and
      for the difference of the two results (the stencil is symmetric, so
      they solve the same system),
  (s) fp32, "T", nrhs 64,
  (z) complex, "C", nrhs 16 and 64, at --nxz (a size that fits the host),
  (r) fp64, "T", nrhs 8, 32, 64: fill_a, factor, x0 = solve_block(b, "T"),
      refine(trans) against refine_block(trans).
The yardstick of a block call is the per-column call on the same plan in the
same run; the times are the HIP-event device times the plan reports
(t_solve_ms, t_refine_ms).  `won` says whether the block call's minimum is
below the per-column call's by more than the larger of the two spreads (max -
min over the repetitions).
Each leg runs in a child process of its own with its own time limit, in the
order given; nothing more is started after a leg fails.  Prints one JSON
line.  --leg d64 (not part of the default run) is one 64-column fp64
solve_block(trans="T") and one refine_block(trans="T") from x0 = 0 alone, for
a kernel trace of its own."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"d": (0, "T", (1, 8, 32, 64)), "s": (1, "T", (64,)), "z": (2, "C", (16, 64)),
        "r": (0, "T", (8, 32, 64)), "d64": (0, "T", (64,))}
DT = {0: np.float64, 1: np.float32, 2: np.complex128}
BERR_MAX = 8 * 2.0 ** -53


def stats_of(t, a, b):
    """minimum of each, the larger spread, and whether b won against a"""
    ma, mb = min(t[a]), min(t[b])
    spread = max(max(t[a]) - ma, max(t[b]) - mb)
    return ma, mb, spread, bool(ma - mb > spread)


def leg(which, nx, reps):
    import scipy.sparse as sp
    from superlu_dist_amd.engine import Plan
    from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
    dtype, trans, cols = LEGS[which]
    kw = dict(diag=6 - 0.25, diag_im=-0.0025) if dtype == 2 else {}
    A = Csc.stencil(STENCIL_3D7, nx, nx, nx, dtype=dtype, **kw)
    S = Symbolic(A, nd_order(nx, nx, nx), 60, 256)
    p = Plan(S.distribute())
    refine = which in ("r", "d64")
    rng = np.random.default_rng(1)
    if refine:
        cp, ri, v = A.permuted(S.perm_c).arrays()
        B = sp.csc_matrix((v, ri, cp), shape=(A.n, A.n))
        p.set_a_pattern(cp, ri)
        p.fill_a(v)
    else:
        p.upload()
    info, _ = p.factor(12.0)
    p.sync()
    assert info == 0, info
    st = p.stats()
    out = {"nx": nx, "n": A.n, "dtype": "dsz"[dtype], "trans": trans, "nsupers": st["nsupers"],
           "nlevels": st["nlevels"], "lu_bytes": st["lu_bytes"], "nrhs": {}}
    for nrhs in cols:
        b = rng.standard_normal((A.n, nrhs))
        if dtype == 2:
            b = b + 1j * rng.standard_normal((A.n, nrhs))
        b = np.asfortranarray(b.astype(DT[dtype]))
        if which == "d64":
            for _ in range(2):
                p.solve_block(b, trans=trans)
            o = dict(zip(("passes", "launches", "block_ms"), p.solve_block_info()))
            bb = np.asfortranarray(B.T @ b)
            x, berr, steps = p.refine_block(bb, np.zeros_like(bb), trans=trans)
            o.update(zip(("refine_passes", "refine_sweeps", "refine_resids", "refine_ms"), p.refine_block_info()))
            o.update(steps=steps.tolist(), berr_max=float(berr.max()))
            out["nrhs"][nrhs] = o
        elif refine:
            bb = np.asfortranarray(B.T @ b)
            x0 = p.solve_block(bb, trans=trans)
            calls = {"column": p.refine, "block": p.refine_block}
            t = {k: [] for k in calls}
            res = {}
            for k in range(reps + 1):  # the first round warms up
                for name, fn in calls.items():
                    res[name] = fn(bb, x0, trans=trans)
                    if k:
                        t[name].append(p.stats()["t_refine_ms"])
            passes, sweeps, resids, _ = p.refine_block_info()
            mc, mb, spread, won = stats_of(t, "column", "block")
            xc, xb = res["column"][0], res["block"][0]
            out["nrhs"][nrhs] = {
                "column_ms": t["column"], "block_ms": t["block"], "column_ms_min": mc, "block_ms_min": mb,
                "column_over_block": mc / mb, "spread_ms": spread, "won": won,
                "passes": passes, "sweeps": sweeps, "resids": resids,
                "column_steps": res["column"][2].tolist(), "block_steps": res["block"][2].tolist(),
                "column_berr_max": float(res["column"][1].max()), "block_berr_max": float(res["block"][1].max()),
                "berr_ok": bool((res["block"][1] <= BERR_MAX).all() and (res["column"][1] <= BERR_MAX).all()),
                "block_minus_column": float((np.abs(xb - xc).max(axis=0) / np.abs(xc).max(axis=0)).max()),
            }
        else:
            calls = {"solve": lambda: p.solve(b, trans=trans), "block": lambda: p.solve_block(b, trans=trans),
                     "block_n": lambda: p.solve_block(b)}
            t = {k: [] for k in calls}
            x = {}
            for k in range(reps + 1):  # the first round warms up
                for name, fn in calls.items():
                    x[name] = fn()
                    if k:
                        t[name].append(p.stats()["t_solve_ms"])
            passes, launches, _ = p.solve_block_info()
            ms, mb, spread, won = stats_of(t, "solve", "block")
            rel = lambda u, w: float((np.abs(u - w).max(axis=0) / np.abs(w).max(axis=0)).max())  # noqa: E731
            o = {
                "solve_ms": t["solve"], "block_ms": t["block"], "block_n_ms": t["block_n"],
                "solve_ms_min": ms, "block_ms_min": mb, "block_n_ms_min": min(t["block_n"]),
                "solve_over_block": ms / mb, "spread_ms": spread, "won": won,
                "trans_over_notrans_pass": mb / min(t["block_n"]), "passes": passes, "launches": launches,
                "block_minus_solve": rel(x["block"], x["solve"]),
            }
            if dtype != 2:  # the real stencil is symmetric: B^T = B (the complex one is not Hermitian)
                o["block_t_minus_block_n"] = rel(x["block"], x["block_n"])
            out["nrhs"][nrhs] = o
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--nxz", type=int, default=64, help="nx of the complex leg")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="d,s,z,r")
    ap.add_argument("--leg", choices=sorted(LEGS), help="(internal) run one leg in this process")
    ap.add_argument("--leg-timeout", type=float, default=420.0, help="seconds per leg")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.nx, a.reps)
        return 0
    res = {"kind": "lap3d"}
    for which in a.legs.split(","):
        nx = a.nxz if which == "z" else a.nx
        cmd = [sys.executable, os.path.abspath(__file__), "--nx", str(nx), "--reps", str(a.reps),
               "--leg", which]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            print(f"leg ({which}) ran into its time limit of {a.leg_timeout:.0f} s", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"leg ({which}) failed with exit status {r.returncode}", file=sys.stderr)
            return 1
        res[which] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"leg ({which}): {json.dumps(res[which])}", file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
