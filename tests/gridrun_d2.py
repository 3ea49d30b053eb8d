"""The mixed-precision test systems and their 2D-grid worker
(tests/test_gpu_refine_d2.py): every rank of a Pr x Pc grid on one GPU, over
the point-to-point host transport of tests/gridrun.py, fills its fp32 factor
storage from the whole fp64 A (slu_plan_fill_a_d2), factors and refines
x0 = 0 (slu_plan_refine_d2, collective)."""
import os
import traceback

import numpy as np

from gridrun import GlooGrid, free_port


def system(kind, nx, nrhs=1, seed=5):
    """(A: the fp32 stencil, its Symbolic, (cp, ri, v): A in the LUstruct's
    permuted coordinates, v64: v widened and perturbed by 1e-3 relative --
    not representable in fp32 --, b = A64 xt, xt)."""
    import scipy.sparse as sp
    from superlu_dist_amd.frontend import Csc, Symbolic, nd_order
    A = Csc.stencil(kind, nx, nx, nx, dtype=1)
    S = Symbolic(A, nd_order(nx, nx, nx), 60, 256)
    cp, ri, v = A.permuted(S.perm_c).arrays()
    rng = np.random.default_rng(seed)
    v64 = v.astype(np.float64) * (1 + 1e-3 * rng.standard_normal(len(v)))
    xt = rng.standard_normal((A.n, nrhs))
    b = sp.csc_matrix((v64, ri, cp), shape=(A.n, A.n)) @ xt
    if nrhs == 1:
        xt, b = xt[:, 0], b[:, 0]
    return A, S, (cp, ri, v), v64, np.asfortranarray(b), xt


def _worker(rank, world, port, kind, nx, pr, pc, out_dir, device):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("SLU_WATCHDOG_S", "120")  # the library's watchdog is opt-in
    try:
        import torch.distributed as dist  # before the engine: see gridrun.run_grid
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from superlu_dist_amd.engine import Comm, Plan
        gg = GlooGrid(rank, pr, pc)
        A, S, (cp, ri, v), v64, b, xt = system(kind, nx)
        lu = S.distribute(pr, pc, gg.myrow, gg.mycol)
        comm = Comm.host_p2p(pr, pc, rank, device, gg.p2p)
        p = Plan(lu, comm=comm)
        p.set_a_pattern(cp, ri)
        p.fill_a_d2(v64)
        info, _ = p.factor(12.0)
        x, berr, steps = p.refine_d2(b, np.zeros_like(b))
        st = p.stats()
        del p
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), x=x, berr=berr[0], steps=steps[0],
                 info=info, amalg_groups=st["amalg_groups"], t_refine_ms=st["t_refine_ms"])
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


def run_grid_d2(kind, nx, pr, pc, out_dir, device=0, timeout=240):
    """Per-rank results (x, berr, steps, ...) of the pr x pc run; the parent
    never imports torch and joins with a timeout, as gridrun.run_grid."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    world = pr * pc
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, kind, nx, pr, pc, str(out_dir), device))
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
