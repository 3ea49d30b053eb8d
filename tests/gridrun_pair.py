"""Worker of the grid case of tests/test_gpu_schur_pair.py: every rank of a
Pr x Pc grid on one GPU, over the host-staged broadcast transport of
tests/gridrun.py, factors the dense chain that pairs on one process and
returns its factors with the plan's counters (Plan.path_counts())."""
import os
import traceback

import numpy as np

from gridrun import GlooGrid, free_port


def _worker(rank, world, port, pr, pc, name, dtype, out_dir, device):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("SLU_WATCHDOG_S", "120")  # the library's watchdog is opt-in
    try:
        import torch.distributed as dist  # before the engine: see gridrun.run_grid
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from superlu_dist_amd.engine import Comm, Plan
        import test_gpu_schur_pair as t
        gg = GlooGrid(rank, pr, pc)
        A, S, an = t.case(name, dtype)
        lu = S.distribute(pr, pc, gg.myrow, gg.mycol)
        comm = Comm.host(pr, pc, rank, device, gg.bcast)
        p = Plan(lu, comm=comm)
        p.upload()
        info, tiny = p.factor(an)
        p.download()
        pc_ = p.path_counts()
        del p
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), L=lu.Lval, U=lu.Uval, info=info, tiny=tiny,
                 **{k: np.asarray(v) for k, v in pc_.items()})
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


def run_grid_pair(pr, pc, name, dtype, out_dir, device=0, timeout=240):
    """Per-rank dicts (L, U, info, tiny, the path counters); the parent never
    imports torch and joins with a timeout, as gridrun.run_grid."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    world = pr * pc
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, pr, pc, name, dtype, str(out_dir), device))
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
