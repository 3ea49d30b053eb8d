"""Worker of the refusal tests of the transposed calls on plans that are not
1x1 (tests/test_gpu_solve_trans.py): every rank of a Pr x Pc (x Pz) grid on
one GPU, over the point-to-point host transport of tests/gridrun.py, factors
a small stencil and records what solve(trans="T"), refine(trans="T") and
rcond raise.  The refusals come before any exchange, so no rank waits for
another; the plain solve afterwards (2D) shows the plan is still usable."""
import os
import traceback

import numpy as np

from gridrun import GlooGrid, free_port


def _worker(rank, world, port, pr, pc, pz, out_dir, device):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("SLU_WATCHDOG_S", "120")  # the library's watchdog is opt-in
    try:
        import torch.distributed as dist  # before the engine: see gridrun.run_grid
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from superlu_dist_amd.engine import Comm, Plan
        from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
        gg = GlooGrid(rank, pr, pc, pz)
        A = Csc.stencil(STENCIL_3D7, 8, 8, 8)
        S = Symbolic(A, nd_order(8, 8, 8), 60, 256)
        lu = S.distribute(pr, pc, gg.myrow, gg.mycol)
        if pz > 1:
            comm = Comm.host_p2p3d(pr, pc, pz, rank, device, gg.p2p)
        else:
            comm = Comm.host_p2p(pr, pc, rank, device, gg.p2p)
        p = Plan(lu, comm=comm)
        p.upload()
        info, _ = p.factor(12.0)
        b = np.ones(A.n)
        msgs = {}
        for what, call in (("solve", lambda: p.solve(b, trans="T")),
                           ("refine", lambda: p.refine(b, b, trans="T")),
                           ("rcond", lambda: p.rcond(12.0))):
            try:
                call()
                msgs[what] = ""
            except RuntimeError as e:
                msgs[what] = str(e)
        resid = -1.0
        if pz == 1:  # collective; every rank gets the whole x
            x = p.solve(b)
            cp, ri, v = A.permuted(S.perm_c).arrays()
            r = -b
            for j in range(A.n):
                r[ri[cp[j]:cp[j + 1]]] += v[cp[j]:cp[j + 1]] * x[j]
            resid = float(np.abs(r).max())
        del p
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), info=info, resid=resid, **msgs)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


def run_grid_t(pr, pc, pz, out_dir, device=0, timeout=240):
    """Per-rank dicts (info, resid, the three messages); the parent never
    imports torch and joins with a timeout, as gridrun.run_grid."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    world = pr * pc * pz
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, pr, pc, pz, str(out_dir), device))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
    bad = []
    for r, p in enumerate(procs):
        if p.is_alive():
            p.kill()
            p.join()
            bad.append(f"rank {r}: timed out")
        elif p.exitcode != 0:
            err = os.path.join(out_dir, f"rank{r}.err")
            msg = open(err).read() if os.path.exists(err) else ""
            bad.append(f"rank {r}: exit {p.exitcode}\n{msg}")
    if bad:
        raise RuntimeError("grid run failed:\n" + "\n".join(bad))
    out = []
    for r in range(world):
        z = np.load(os.path.join(out_dir, f"rank{r}.npz"))
        out.append({k: z[k] for k in z.files})
    return out
