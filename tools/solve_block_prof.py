"""Block solve against the plain solve on one GPU: lap3d
nx^3 through the front end, factored once per leg, then on that one plan,
for each nrhs of the leg, slu_plan_solve and slu_plan_solve_block alternate
on the same b after a warm-up of each, `reps` repetitions:
  (d) fp64, nrhs 1, 8, 32, 64,
  (s) fp32, nrhs 64,
  (z) complex, nrhs 16 and 64, at --nxz (a size that fits the host).
The yardstick of solve_block is slu_plan_solve on the same plan in the same
run; the times are the HIP-event device times the plan reports (t_solve_ms).
`won` says whether solve_block's minimum is below solve's by more than the
larger of the two spreads (max - min over the repetitions).
Each leg runs in a child process of its own with its own time limit, in the
order above; nothing more is started after a leg fails.  Prints one JSON
line.  --leg d64 (not part of the default run) is the 64-column fp64 block
solve alone, for a kernel trace of its own."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"d": (0, (1, 8, 32, 64)), "s": (1, (64,)), "z": (2, (16, 64)), "d64": (0, (64,))}
DT = {0: np.float64, 1: np.float32, 2: np.complex128}


def leg(which, nx, reps):
    from superlu_dist_amd.engine import Plan
    from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
    dtype, cols = LEGS[which]
    kw = dict(diag=6 - 0.25, diag_im=-0.0025) if dtype == 2 else {}
    A = Csc.stencil(STENCIL_3D7, nx, nx, nx, dtype=dtype, **kw)
    S = Symbolic(A, nd_order(nx, nx, nx), 60, 256)
    p = Plan(S.distribute())
    p.upload()
    info, _ = p.factor(12.0)
    p.sync()
    assert info == 0, info
    st = p.stats()
    out = {"nx": nx, "n": A.n, "dtype": "dsz"[dtype], "nsupers": st["nsupers"], "nlevels": st["nlevels"],
           "lu_bytes": st["lu_bytes"], "nrhs": {}}
    rng = np.random.default_rng(1)
    for nrhs in cols:
        b = rng.standard_normal((A.n, nrhs))
        if dtype == 2:
            b = b + 1j * rng.standard_normal((A.n, nrhs))
        b = np.asfortranarray(b.astype(DT[dtype]))
        if which == "d64":
            for _ in range(2):
                p.solve_block(b)
            out["nrhs"][nrhs] = dict(zip(("passes", "launches", "block_ms"), p.solve_block_info()))
            continue
        t = {"solve": [], "block": []}
        x = {}
        for k in range(reps + 1):  # the first round warms up
            x["solve"] = p.solve(b)
            if k:
                t["solve"].append(p.stats()["t_solve_ms"])
            x["block"] = p.solve_block(b)
            if k:
                t["block"].append(p.stats()["t_solve_ms"])
        passes, launches, _ = p.solve_block_info()
        ms, mb = min(t["solve"]), min(t["block"])
        spread = max(max(t["solve"]) - ms, max(t["block"]) - mb)
        out["nrhs"][nrhs] = {
            "solve_ms": t["solve"], "block_ms": t["block"], "solve_ms_min": ms, "block_ms_min": mb,
            "solve_over_block": ms / mb, "spread_ms": spread, "won": bool(ms - mb > spread),
            "passes": passes, "launches": launches,
            "block_minus_solve": float(np.abs(x["block"] - x["solve"]).max() / np.abs(x["solve"]).max()),
        }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--nxz", type=int, default=64, help="nx of the complex leg")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="d,s,z")
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
