"""Child processes of tests/test_gpu_diag_inv.py.

run_grid_diag_inv: every rank of a Pr x Pc (x Pz) grid on one GPU, over the
point-to-point host transport of tests/gridrun.py, builds the plan of a small
stencil and records what set_diag_inv(1) raises -- before the plan holds any
values and again after the factorization.  The refusal comes before any device
work or exchange, so no rank waits for another; the mode stays off, and the
plain solve afterwards (2D) shows the plan is still usable."""
import os
import traceback

import numpy as np

from gridrun import GlooGrid, free_port
from gridrun_block import _join


def _worker(rank, world, port, pr, pc, pz, out_dir, device):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("SLU_WATCHDOG_S", "120")  # the library's watchdog is opt-in
    try:
        import torch.distributed as dist  # before the engine: see gridrun.run_grid
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from superlu_dist_amd.engine import Comm, Plan
        from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
        from superlu_dist_amd.lib import lib
        gg = GlooGrid(rank, pr, pc, pz)
        A = Csc.stencil(STENCIL_3D7, 8, 8, 8)
        S = Symbolic(A, nd_order(8, 8, 8), 60, 256)
        lu = S.distribute(pr, pc, gg.myrow, gg.mycol)
        if pz > 1:
            comm = Comm.host_p2p3d(pr, pc, pz, rank, device, gg.p2p)
        else:
            comm = Comm.host_p2p(pr, pc, rank, device, gg.p2p)
        p = Plan(lu, comm=comm)
        rc0 = lib().slu_plan_set_diag_inv(p.ptr, 1)
        msg0 = lib().slu_last_error().decode() if rc0 != 0 else ""
        p.upload()
        info, _ = p.factor(12.0)
        rc = lib().slu_plan_set_diag_inv(p.ptr, 1)
        msg = lib().slu_last_error().decode() if rc != 0 else ""
        state = p.diag_inv_info()
        resid = -1.0
        if pz == 1:  # collective; every rank gets the whole x
            b = np.ones(A.n)
            x = p.solve(b)
            cp, ri, v = A.permuted(S.perm_c).arrays()
            r = -b.copy()
            for j in range(A.n):
                r[ri[cp[j]:cp[j + 1]]] += v[cp[j]:cp[j + 1]] * x[j]
            resid = float(np.abs(r).max())
        del p
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), info=info, resid=resid, rc0=rc0, msg0=msg0, rc=rc,
                 msg=msg, on=state[0], valid=state[1], bytes=state[2], computes=state[3])
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


def run_grid_diag_inv(pr, pc, pz, out_dir, device=0, timeout=240):
    """Per-rank dicts; the parent never imports torch and joins with a
    timeout, as gridrun.run_grid."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    world = pr * pc * pz
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, pr, pc, pz, str(out_dir), device))
             for r in range(world)]
    for p in procs:
        p.start()
    _join(procs, str(out_dir), timeout)
    out = []
    for r in range(world):
        z = np.load(os.path.join(out_dir, f"rank{r}.npz"))
        out.append({k: z[k] for k in z.files})
    return out
