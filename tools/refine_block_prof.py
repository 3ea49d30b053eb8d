"""Block refinement against the per-column refinement on one GPU (DESIGN
section 24): lap3d nx^3 through the front end, one plan per leg,
  (d)  an fp64 plan: fill_a, factor, x0 = solve_block(b), refine against
       refine_block;
  (d2) an fp32 plan: fill_a_d2, factor, x0 = 0, refine_d2 against
       refine_block_d2;
b = A xt for a random xt, nrhs 8, 32 and 64.  On that one plan the per-column
call and the block call alternate on the same b and x0 after a warm-up of
each, `reps` repetitions.  The yardstick of the block call is the per-column
call on the same plan in the same run; the times are the HIP-event device
times the plan reports (t_refine_ms).  `won` says whether the block call's
minimum is below the per-column call's by more than the larger of the two
spreads (max - min over the repetitions).  Per column the steps and berr of
both calls are recorded, and `berr_ok` says whether every berr is within
8 eps (the bound of tests/test_gpu_refine_block.py).
Each leg runs in a child process of its own with its own time limit;
nothing more is started after a leg fails.  Prints one JSON line.  --leg d64
(not part of the default run) is one 64-column fp64 refine_block alone, from
x0 = 0 so that every pass takes steps, for a kernel trace of its own."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"d": (False, (8, 32, 64)), "d2": (True, (8, 32, 64)), "d64": (False, (64,))}
BERR_MAX = 8 * 2.0 ** -53


def leg(which, nx, reps):
    import scipy.sparse as sp
    from superlu_dist_amd.engine import Plan
    from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
    mixed, cols = LEGS[which]
    A = Csc.stencil(STENCIL_3D7, nx, nx, nx, dtype=1 if mixed else 0)
    S = Symbolic(A, nd_order(nx, nx, nx), 60, 256)
    cp, ri, v = A.permuted(S.perm_c).arrays()
    rng = np.random.default_rng(1)
    v64 = v.astype(np.float64)
    if mixed:  # not representable in fp32, as tools/mixed_prof.py
        v64 = v64 * (1 + 1e-3 * rng.standard_normal(len(v)))
    B = sp.csc_matrix((v64, ri, cp), shape=(A.n, A.n))
    p = Plan(S.distribute())
    p.set_a_pattern(cp, ri)
    if mixed:
        p.fill_a_d2(v64)
    else:
        p.fill_a(v64)
    info, _ = p.factor(float(abs(B).sum(axis=0).max()))
    p.sync()
    assert info == 0, info
    st = p.stats()
    out = {"nx": nx, "n": A.n, "dtype": "s+d2" if mixed else "d", "nsupers": st["nsupers"],
           "nlevels": st["nlevels"], "lu_bytes": st["lu_bytes"], "nrhs": {}}
    calls = {"column": p.refine_d2 if mixed else p.refine, "block": p.refine_block_d2 if mixed else p.refine_block}
    for nrhs in cols:
        b = np.asfortranarray(B @ rng.standard_normal((A.n, nrhs)))
        if which == "d64":
            p.solve_block(b)  # warms the sweep's kernels
            x, berr, steps = p.refine_block(b, np.zeros_like(b))
            out["nrhs"][nrhs] = dict(zip(("passes", "sweeps", "resids", "block_ms"), p.refine_block_info()))
            out["nrhs"][nrhs].update(steps=steps.tolist(), berr_max=float(berr.max()))
            continue
        x0 = np.zeros_like(b) if mixed else p.solve_block(b)
        t = {k: [] for k in calls}
        res = {}
        for k in range(reps + 1):  # the first round warms up
            for name, fn in calls.items():
                res[name] = fn(b, x0)
                if k:
                    t[name].append(p.stats()["t_refine_ms"])
        passes, sweeps, resids, _ = p.refine_block_info()
        mc, mb = min(t["column"]), min(t["block"])
        spread = max(max(t["column"]) - mc, max(t["block"]) - mb)
        xc, xb = res["column"][0], res["block"][0]
        out["nrhs"][nrhs] = {
            "column_ms": t["column"], "block_ms": t["block"], "column_ms_min": mc, "block_ms_min": mb,
            "column_over_block": mc / mb, "spread_ms": spread, "won": bool(mc - mb > spread),
            "passes": passes, "sweeps": sweeps, "resids": resids,
            "column_steps": res["column"][2].tolist(), "block_steps": res["block"][2].tolist(),
            "column_berr": res["column"][1].tolist(), "block_berr": res["block"][1].tolist(),
            "berr_ok": bool((res["block"][1] <= BERR_MAX).all() and (res["column"][1] <= BERR_MAX).all()),
            "block_minus_column": float((np.abs(xb - xc).max(axis=0) / np.abs(xc).max(axis=0)).max()),
        }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="d,d2")
    ap.add_argument("--leg", choices=sorted(LEGS), help="(internal) run one leg in this process")
    ap.add_argument("--leg-timeout", type=float, default=420.0, help="seconds per leg")
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.nx, a.reps)
        return 0
    res = {"kind": "lap3d"}
    for which in a.legs.split(","):
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
        print(f"leg ({which}): {json.dumps(res[which])}", file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
