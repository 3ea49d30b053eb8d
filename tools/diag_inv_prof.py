"""DiagInv against substitution in the block sweeps on one GPU (DESIGN section
27): lap3d nx^3 through the front end, one plan per leg, factored once; then
on that one plan, for each nrhs of the leg, the same call with the mode off
and with the mode on alternates on the same b after a warm-up of each, `reps`
repetitions.  The legs are those of DESIGN section 21:
  (d)  fp64 solve_block, nrhs 32 and 64,
  (s)  fp32 solve_block, nrhs 64,
  (z)  complex solve_block, nrhs 16 and 64, at --nxz (a size that fits the host),
  (r)  fp64 refine_block, nrhs 32, x0 = solve_block(b),
  (d2) fp32 factors of an fp64 matrix, refine_block_d2, nrhs 32, x0 = 0.
The yardstick of the mode is the mode-off call on the same plan in the same
run; the times are the HIP-event device times the plan reports (t_solve_ms,
t_refine_ms), which leave the inversion out.  `won` says whether the mode-on
minimum is below the mode-off minimum by more than the larger of the two
spreads (max - min over the repetitions); `lost` the same the other way.
Every leg also records the device time of one inversion (min over the
repetitions: the mode is switched off and on again each round, so every
round inverts) and the bytes the inverses hold beside the factors' bytes.
Each leg runs in a child process of its own with its own time limit, in the
order above; nothing more is started after a leg fails.  Prints one JSON
line.  --leg d64 (not part of the default run) is the 64-column fp64
solve_block with the mode on alone, for a kernel trace of its own."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# leg -> (plan dtype, call, columns)
LEGS = {"d": (0, "solve", (32, 64)), "s": (1, "solve", (64,)), "z": (2, "solve", (16, 64)),
        "r": (0, "refine", (32,)), "d2": (1, "refine_d2", (32,)), "d64": (0, "solve", (64,))}
DT = {0: np.float64, 1: np.float32, 2: np.complex128}


def leg(which, nx, reps):
    import scipy.sparse as sp
    from superlu_dist_amd.engine import Plan
    from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
    dtype, call, cols = LEGS[which]
    kw = dict(diag=6 - 0.25, diag_im=-0.0025) if dtype == 2 else {}
    A = Csc.stencil(STENCIL_3D7, nx, nx, nx, dtype=dtype, **kw)
    S = Symbolic(A, nd_order(nx, nx, nx), 60, 256)
    cp, ri, v = A.permuted(S.perm_c).arrays()
    rng = np.random.default_rng(1)
    p = Plan(S.distribute())
    p.set_a_pattern(cp, ri)
    if call == "refine_d2":  # not representable in fp32, as tools/mixed_prof.py
        v = v.astype(np.float64) * (1 + 1e-3 * rng.standard_normal(len(v)))
        p.fill_a_d2(v)
    else:
        p.fill_a(v)
    B = sp.csc_matrix((v, ri, cp), shape=(A.n, A.n))
    info, _ = p.factor(float(abs(B).sum(axis=0).max()))
    p.sync()
    assert info == 0, info
    st = p.stats()
    out = {"nx": nx, "n": A.n, "dtype": "s+d2" if call == "refine_d2" else "dsz"[dtype], "call": call,
           "nsupers": st["nsupers"], "nlevels": st["nlevels"], "lu_bytes": st["lu_bytes"], "nrhs": {}}
    bt = np.float64 if call == "refine_d2" else DT[dtype]
    inv_ms = []
    for nrhs in cols:
        xt = rng.standard_normal((A.n, nrhs))
        if dtype == 2:
            xt = xt + 1j * rng.standard_normal((A.n, nrhs))
        b = np.asfortranarray((B @ xt).astype(bt))
        if which == "d64":
            p.set_diag_inv(True)
            for _ in range(2):
                p.solve_block(b)
            out["nrhs"][nrhs] = dict(zip(("passes", "launches", "on_ms"), p.solve_block_info()))
            continue
        p.set_diag_inv(False)
        x0 = p.solve_block(b) if call == "refine" else np.zeros_like(b)
        t = {"off": [], "on": []}
        res = {}
        for k in range(reps + 1):  # the first round warms up
            for name in ("off", "on"):
                p.set_diag_inv(name == "on")
                if call == "solve":
                    res[name] = (p.solve_block(b),)
                    ms = p.stats()["t_solve_ms"]
                else:
                    res[name] = (p.refine_block_d2 if call == "refine_d2" else p.refine_block)(b, x0)
                    ms = p.stats()["t_refine_ms"]
                if k:
                    t[name].append(ms)
                    if name == "on":
                        inv_ms.append(p.diag_inv_info()[4])
        m0, m1 = min(t["off"]), min(t["on"])
        spread = max(max(t["off"]) - m0, max(t["on"]) - m1)
        x_off, x_on = res["off"][0], res["on"][0]
        o = {"off_ms": t["off"], "on_ms": t["on"], "off_ms_min": m0, "on_ms_min": m1, "off_over_on": m0 / m1,
             "spread_ms": spread, "won": bool(m0 - m1 > spread), "lost": bool(m1 - m0 > spread),
             "on_minus_off": float((np.abs(x_on - x_off).max(axis=0) / np.abs(x_off).max(axis=0)).max())}
        if call == "solve":
            o.update(zip(("passes", "launches"), p.solve_block_info()[:2]))
        else:
            o.update(zip(("passes", "sweeps", "resids"), p.refine_block_info()[:3]))
            o.update(off_steps=res["off"][2].tolist(), on_steps=res["on"][2].tolist(),
                     off_berr_max=float(res["off"][1].max()), on_berr_max=float(res["on"][1].max()))
        out["nrhs"][nrhs] = o
    on, valid, nbytes, computes, ms = p.diag_inv_info()
    out.update(inv_bytes=nbytes, inv_computes=computes, inv_ms=inv_ms, inv_ms_min=min(inv_ms) if inv_ms else ms)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--nxz", type=int, default=64, help="nx of the complex leg")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="d,s,z,r,d2")
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
