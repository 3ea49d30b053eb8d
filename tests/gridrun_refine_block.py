"""Child processes of tests/test_gpu_refine_block.py.

run_grid_refine_block: every rank of a Pr x Pc (x Pz) grid on one GPU, over
the point-to-point host transport of tests/gridrun.py, factors a small
stencil filled through fill_a and records what refine_block and
refine_block_d2 raise.  The refusals come before any device work or
exchange, so no rank waits for another.

run_device_pointer: one process that imports torch first (torch brings its
own HIP runtime, see gridrun.run_grid), builds an fp64 and an fp32 (d2) 1x1
plan and refines column-major torch tensors on the device in place through
refine_block_dev, beside the host-array calls on the same data."""
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
        import ctypes as C
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
        if pz > 1:
            p.upload()
        else:
            cp, ri, v = A.permuted(S.perm_c).arrays()
            p.set_a_pattern(cp, ri)
            p.fill_a(v)
        info, _ = p.factor(12.0)
        b = np.ones((A.n, 3), order="F")
        x = np.full((A.n, 3), 0.5, order="F")
        msgs = []
        for fn in (lib().slu_plan_refine_block, lib().slu_plan_refine_block_d2):
            rc = fn(p.ptr, b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), A.n, 3, 0, None, None)
            msgs.append(lib().slu_last_error().decode() if rc != 0 else "")
        unchanged = bool((b == 1.0).all() and (x == 0.5).all())
        del p
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), info=info, msg=msgs[0], msg_d2=msgs[1],
                 unchanged=unchanged)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


def run_grid_refine_block(pr, pc, pz, out_dir, device=0, timeout=240):
    """Per-rank dicts (info, msg, msg_d2, unchanged); the parent never imports
    torch and joins with a timeout, as gridrun.run_grid."""
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


SENT = -7.25e300


def _dev_refine(torch, p, device, b, x0, d2):
    """refine_block_dev on (ld x (nrhs + 1)) column-major device arrays = the
    rows of C-ordered (nrhs + 1, ld) tensors; (x, berr, steps, b and the
    sentinels untouched)."""
    n, nrhs = b.shape
    ld = n + 5
    hb, hx = np.full((nrhs + 1, ld), SENT), np.full((nrhs + 1, ld), SENT)
    hb[:nrhs, :n] = b.T
    hx[:nrhs, :n] = x0.T
    tb, tx = torch.from_numpy(hb).to(f"cuda:{device}"), torch.from_numpy(hx).to(f"cuda:{device}")
    torch.cuda.synchronize()  # the caller's writes have completed
    berr, steps = p.refine_block_dev(tb.data_ptr(), tx.data_ptr(), ld, nrhs, d2=d2)
    bx = tx.cpu().numpy()
    ok = bool(np.array_equal(tb.cpu().numpy(), hb) and (bx[:nrhs, n:] == SENT).all() and (bx[nrhs] == SENT).all())
    return bx[:nrhs, :n].T, berr, steps, ok


def _dev_worker(out_dir, device):
    try:
        import torch  # before the engine: see gridrun.run_grid
        from gridrun_d2 import system
        from superlu_dist_amd.engine import Plan
        from superlu_dist_amd.frontend import STENCIL_3D7, Csc, Symbolic, nd_order
        import scipy.sparse as sp
        out = {}
        # fp64
        A = Csc.stencil(STENCIL_3D7, 9, 9, 9)
        S = Symbolic(A, nd_order(9, 9, 9), 60, 256)
        p = Plan(S.distribute())
        cp, ri, v = A.permuted(S.perm_c).arrays()
        p.set_a_pattern(cp, ri)
        p.fill_a(v)
        assert p.factor(12.0) == (0, 0)
        b = np.asfortranarray(sp.csc_matrix((v, ri, cp), shape=(A.n, A.n))
                              @ np.random.default_rng(11).standard_normal((A.n, 33)))
        x0 = p.solve_block(b)
        x0[:, ::2] = 0.0  # every other column has steps to take
        xh, beh, sth = p.refine_block(b, x0)
        xd, bed, std, ok = _dev_refine(torch, p, device, b, x0, False)
        out.update(x_host=xh, berr_host=beh, steps_host=sth, x_dev=xd, berr_dev=bed, steps_dev=std, ok=ok,
                   info=np.array(p.refine_block_info()))
        del p
        # fp32 factors, fp64 refinement
        A, S, (cp, ri, v), v64, b, xt = system(STENCIL_3D7, 8, nrhs=33)
        p = Plan(S.distribute())
        p.set_a_pattern(cp, ri)
        p.fill_a_d2(v64)
        assert p.factor(12.0)[0] == 0
        x0 = np.zeros_like(b)
        xh, beh, sth = p.refine_block_d2(b, x0)
        xd, bed, std, ok = _dev_refine(torch, p, device, b, x0, True)
        out.update(d2_x_host=xh, d2_berr_host=beh, d2_steps_host=sth, d2_x_dev=xd, d2_berr_dev=bed,
                   d2_steps_dev=std, d2_ok=ok)
        del p
        np.savez(os.path.join(out_dir, "rank0.npz"), **out)
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
