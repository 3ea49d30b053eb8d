"""Child processes of tests/test_gpu_solve_block.py.

run_grid_block: every rank of a Pr x Pc (x Pz) grid on one GPU, over the
point-to-point host transport of tests/gridrun.py, factors a small stencil
and records what solve_block raises.  The refusal comes before any device
work or exchange, so no rank waits for another; the plain solve afterwards
(2D) shows the plan is still usable.

run_device_pointer: one process that imports torch first (torch brings its
own HIP runtime, see gridrun.run_grid), builds a 1x1 plan and runs
solve_block_dev on a column-major torch tensor on the device."""
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
        b = np.ones((A.n, 3), order="F")
        import ctypes as C
        from superlu_dist_amd.lib import lib
        rc = lib().slu_plan_solve_block(p.ptr, b.ctypes.data_as(C.c_void_p), A.n, 3, 0)
        msg = lib().slu_last_error().decode() if rc != 0 else ""
        unchanged = bool((b == 1.0).all())
        resid = -1.0
        if pz == 1:  # collective; every rank gets the whole x
            x = p.solve(b[:, 0])
            cp, ri, v = A.permuted(S.perm_c).arrays()
            r = -b[:, 0].copy()
            for j in range(A.n):
                r[ri[cp[j]:cp[j + 1]]] += v[cp[j]:cp[j + 1]] * x[j]
            resid = float(np.abs(r).max())
        del p
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), info=info, resid=resid, msg=msg,
                 b_unchanged=unchanged)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


def _join(procs, out_dir, timeout):
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
        raise RuntimeError("child run failed:\n" + "\n".join(bad))


def run_grid_block(pr, pc, pz, out_dir, device=0, timeout=240):
    """Per-rank dicts (info, resid, msg, b_unchanged); the parent never
    imports torch and joins with a timeout, as gridrun.run_grid."""
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


def _dev_worker(out_dir, device):
    try:
        import torch  # before the engine: see gridrun.run_grid
        from lusolve import solve_1x1
        from superlu_dist_amd.engine import Plan
        from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
        A = Csc.stencil(STENCIL_3D7, 12, 12, 12)
        S = Symbolic(A, nd_order(12, 12, 12), 60, 256)
        lu = S.distribute()
        p = Plan(lu)
        p.upload()
        assert p.factor(12.0) == (0, 0)
        p.download()
        n, nrhs, ldb = A.n, 33, A.n + 5
        b = np.asfortranarray(np.random.default_rng(11).standard_normal((n, nrhs)))
        x_host = p.solve_block(b)
        x_host2 = p.solve_block(b)
        x_ref = np.stack([solve_1x1(lu, b[:, r]) for r in range(nrhs)], axis=1)
        # column-major (ldb x (nrhs + 1)) = the rows of a C-ordered (nrhs + 1, ldb) tensor
        sent = -7.25e300
        host = np.full((nrhs + 1, ldb), sent)
        host[:nrhs, :n] = b.T
        t = torch.from_numpy(host).to(f"cuda:{device}")
        torch.cuda.synchronize()  # the caller's writes have completed
        p.solve_block_dev(t.data_ptr(), ldb, nrhs)
        passes, launches, ms = p.solve_block_info()
        back = t.cpu().numpy()
        ok = bool((back[:nrhs, n:] == sent).all() and (back[nrhs] == sent).all())
        del p
        np.savez(os.path.join(out_dir, "rank0.npz"), x_host=x_host, x_host2=x_host2, x_ref=x_ref,
                 x_dev=back[:nrhs, :n].T, sentinels_ok=ok, passes=passes, ms=ms)
    except Exception:
        with open(os.path.join(out_dir, "rank0.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


def run_device_pointer(out_dir, device=0, timeout=240):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dev_worker, args=(str(out_dir), device))]
    procs[0].start()
    _join(procs, str(out_dir), timeout)
    z = np.load(os.path.join(out_dir, "rank0.npz"))
    return {k: z[k] for k in z.files}
