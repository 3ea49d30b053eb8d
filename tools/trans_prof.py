"""Transposed solve against the plain solve, and the condition estimate, on
one GPU: lap3d nx^3 through the front end, factored once
per leg, then on that one plan
  (n1) solve and solve_t of 1 right-hand side,
  (n8) solve and solve_t of 8 right-hand sides (one batch),
  (rc) rcond, norm '1' and 'I'.
The yardstick of solve_t is slu_plan_solve on the same plan in the same run:
the two alternate, after a warm-up of each, and the times are the HIP-event
device times the plan reports (t_solve_ms; rcond: slu_plan_rcond_info).
Each leg runs in a child process of its own with its own time limit, in the
order above; nothing more is started after a leg fails.  Prints one JSON
line."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = ("n1", "n8", "rc")


def leg(which, nx, reps):
    from superlu_dist_amd.engine import Plan
    from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
    A = Csc.stencil(STENCIL_3D7, nx, nx, nx)
    S = Symbolic(A, nd_order(nx, nx, nx), 60, 256)
    p = Plan(S.distribute())
    p.upload()
    info, _ = p.factor(12.0)
    p.sync()
    assert info == 0, info
    st = p.stats()
    out = {"n": A.n, "nsupers": st["nsupers"], "nlevels": st["nlevels"], "lu_bytes": st["lu_bytes"]}
    rng = np.random.default_rng(1)
    if which == "rc":
        for norm in ("1", "I"):
            p.rcond(12.0, norm=norm)  # warm-up: tables, code objects
            ms = []
            for _ in range(reps):
                rc = p.rcond(12.0, norm=norm)
                sweeps, t = p.rcond_info()
                ms.append(t)
            out[f"rcond_{norm}"] = {"rcond": rc, "sweeps": sweeps, "ms": ms, "ms_min": min(ms)}
        p.solve(rng.standard_normal(A.n))
        p.solve(rng.standard_normal(A.n))
        out["t_solve_ms"] = p.stats()["t_solve_ms"]
    else:
        nrhs = int(which[1:])
        b = np.asfortranarray(rng.standard_normal((A.n, nrhs)))
        t = {"N": [], "T": []}
        x = {}
        for k in range(reps + 1):  # the first round warms up
            for tr in ("N", "T"):
                x[tr] = p.solve(b, trans=tr)
                if k:
                    t[tr].append(p.stats()["t_solve_ms"])
        out["nrhs"] = nrhs
        out["solve_ms"], out["solve_t_ms"] = t["N"], t["T"]
        out["solve_ms_min"], out["solve_t_ms_min"] = min(t["N"]), min(t["T"])
        out["t_over_n"] = min(t["T"]) / min(t["N"])
        # the stencil is symmetric: both solve the same system
        out["t_minus_n"] = float(np.abs(x["T"] - x["N"]).max() / np.abs(x["N"]).max())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg", choices=LEGS, help="(internal) run one leg in this process")
    ap.add_argument("--leg-timeout", type=float, default=300.0, help="seconds per leg")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.nx, a.reps)
        return 0
    res = {"nx": a.nx, "kind": "lap3d"}
    for which in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--nx", str(a.nx), "--reps", str(a.reps),
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
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
