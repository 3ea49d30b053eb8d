"""Mixed-precision solve against the fp64 solve on one GPU:
the same fp64 system A x = b through
  (a) an fp64 plan: fill_a, factor, solve, refine;
  (b) an fp32 plan: fill_a_d2, factor, refine_d2 from x0 = 0.
A = the stencil's values perturbed by 1e-3 relative (not representable in
fp32), b = A xt.  Each leg runs in a child process of its own with its own
time limit, (a) first; nothing more is started after a leg fails.  Prints one
JSON line: per leg the device times of the phases, the refinement steps, the
componentwise backward error against the fp64 A, the forward error against
xt and the bytes of L and U."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = {"lap3d": "STENCIL_3D7", "st27": "STENCIL_3D27"}


def leg(which, kind, nx):
    import scipy.sparse as sp
    from superlu_dist_amd import frontend
    from superlu_dist_amd.engine import Plan
    from superlu_dist_amd.frontend import Csc, Symbolic, nd_order
    mixed = which == "b"
    A = Csc.stencil(getattr(frontend, KINDS[kind]), nx, nx, nx, dtype=1 if mixed else 0)
    S = Symbolic(A, nd_order(nx, nx, nx), 60, 256)
    cp, ri, v = A.permuted(S.perm_c).arrays()
    rng = np.random.default_rng(1)
    v64 = v.astype(np.float64) * (1 + 1e-3 * rng.standard_normal(len(v)))
    B = sp.csc_matrix((v64, ri, cp), shape=(A.n, A.n))
    xt = rng.standard_normal(A.n)
    b = B @ xt
    anorm = float(abs(B).sum(axis=0).max())
    p = Plan(S.distribute(), timing=1)
    p.set_a_pattern(cp, ri)
    out = {"dtype": "s" if mixed else "d"}
    if mixed:
        p.fill_a_d2(v64)
    else:
        p.fill_a(v64)
    out["t_fill_ms"] = p.stats()["t_fill_ms"]
    info, tiny = p.factor(anorm)
    p.sync()
    assert info == 0, info
    out["t_factor_ms"] = p.stats()["t_total_ms"]
    if mixed:
        x, berr, steps = p.refine_d2(b, np.zeros_like(b))
        out["t_solve_ms"] = 0.0
    else:
        x0 = p.solve(b)
        out["t_solve_ms"] = p.stats()["t_solve_ms"]
        x, berr, steps = p.refine(b, x0)
    st = p.stats()
    out["t_refine_ms"] = st["t_refine_ms"]
    out["t_sum_ms"] = out["t_fill_ms"] + out["t_factor_ms"] + out["t_solve_ms"] + out["t_refine_ms"]
    out["steps"] = int(steps[0])
    out["berr_device"] = float(berr[0])
    r = np.abs((b - B @ x).astype(np.float64))
    out["berr"] = float((r / (abs(B) @ np.abs(x) + np.abs(b))).max())
    out["fwd_err"] = float(np.abs(x - xt).max() / np.abs(xt).max())
    out["lu_bytes"] = st["lu_bytes"]
    out["tiny"] = tiny
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--kind", choices=sorted(KINDS), default="lap3d")
    ap.add_argument("--leg", choices=["a", "b"], help="(internal) run one leg in this process")
    ap.add_argument("--leg-timeout", type=float, default=420.0, help="seconds per leg")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.kind, a.nx)
        return 0
    res = {"nx": a.nx, "kind": a.kind}
    for which in ("a", "b"):
        cmd = [sys.executable, os.path.abspath(__file__), "--nx", str(a.nx), "--kind", a.kind,
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
    res["b_over_a_time"] = res["b"]["t_sum_ms"] / res["a"]["t_sum_ms"]
    res["b_over_a_lu_bytes"] = res["b"]["lu_bytes"] / res["a"]["lu_bytes"]
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
