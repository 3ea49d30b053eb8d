"""Child processes of tests/test_gpu_solve_block_trans.py and
tests/test_gpu_refine_block_trans.py.

run_grid_block_t: every rank of a Pr x Pc (x Pz) grid on one GPU, over the
point-to-point host transport of tests/gridrun.py, factors a small stencil
and records what solve_block_t and refine_block_t raise with SLU_TRANS.  The
refusals come before any device work or exchange, so no rank waits for
another; the plain solve afterwards (2D) shows the plan is still usable.

run_device_pointer_t: one process that imports torch first (torch brings its
own HIP runtime, see gridrun.run_grid), builds a 1x1 plan of an unsymmetric
system and runs solve_block_dev and refine_block_dev with trans="T" on
column-major torch tensors on the device."""
import functools
import os
import traceback

import numpy as np

from gridrun import GlooGrid, free_port
from gridrun_block import _join

SENT = -7.25e300


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
        cp, ri, v = A.permuted(S.perm_c).arrays()
        if pz > 1:
            p.upload()
        else:
            p.set_a_pattern(cp, ri)
            p.fill_a(v)
        info, _ = p.factor(12.0)
        b = np.ones((A.n, 3), order="F")
        x = np.full((A.n, 3), 0.5, order="F")
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = lib().slu_plan_solve_block_t(p.ptr, 1, vp(b), A.n, 3, 0)
        msg_solve = lib().slu_last_error().decode() if rc != 0 else ""
        rc = lib().slu_plan_refine_block_t(p.ptr, 1, vp(b), vp(x), A.n, 3, 0, None, None)
        msg_refine = lib().slu_last_error().decode() if rc != 0 else ""
        unchanged = bool((b == 1.0).all() and (x == 0.5).all())
        resid = -1.0
        if pz == 1:  # collective; every rank gets the whole x
            y = p.solve(b[:, 0])
            r = -b[:, 0].copy()
            for j in range(A.n):
                r[ri[cp[j]:cp[j + 1]]] += v[cp[j]:cp[j + 1]] * y[j]
            resid = float(np.abs(r).max())
        del p
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), info=info, resid=resid, msg_solve=msg_solve,
                 msg_refine=msg_refine, unchanged=unchanged)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


def run_grid_block_t(pr, pc, pz, out_dir, device=0, timeout=240):
    """Per-rank dicts (info, resid, msg_solve, msg_refine, unchanged); the
    parent never imports torch and joins with a timeout, as gridrun.run_grid."""
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


def _padded(torch, device, a, ld):
    """(ld x (ncols + 1)) column-major device array of sentinels around a =
    the rows of a C-ordered (ncols + 1, ld) tensor; (tensor, host copy)."""
    n, k = a.shape
    h = np.full((k + 1, ld), SENT)
    h[:k, :n] = a.T
    return torch.from_numpy(h).to(f"cuda:{device}"), h


def _dev_worker(out_dir, device):
    try:
        import torch  # before the engine: see gridrun.run_grid
        from lusolve_t import solve_1x1_t, unsym_stencil
        from superlu_dist_amd.engine import Plan
        from superlu_dist_amd.frontend import STENCIL_3D7, Symbolic, nd_order
        import scipy.sparse as sp
        A = unsym_stencil(STENCIL_3D7, (9, 9, 9), 0)
        S = Symbolic(A, nd_order(9, 9, 9), 60, 256)
        lu = S.distribute()
        p = Plan(lu)
        cp, ri, v = A.permuted(S.perm_c).arrays()
        p.set_a_pattern(cp, ri)
        p.fill_a(v)
        assert p.factor(14.0) == (0, 0)
        p.download()
        n, nrhs, ld = A.n, 33, A.n + 5
        Bt = sp.csc_matrix((v, ri, cp), shape=(n, n)).T
        b = np.asfortranarray(Bt @ np.random.default_rng(11).standard_normal((n, nrhs)))
        x_host = p.solve_block(b, trans="T")
        x_ref = np.stack([solve_1x1_t(lu, b[:, r]) for r in range(nrhs)], axis=1)
        t, h = _padded(torch, device, b, ld)
        torch.cuda.synchronize()  # the caller's writes have completed
        p.solve_block_dev(t.data_ptr(), ld, nrhs, trans="T")
        passes, launches, ms = p.solve_block_info()
        back = t.cpu().numpy()
        ok = bool((back[:nrhs, n:] == SENT).all() and (back[nrhs] == SENT).all())
        out = dict(x_host=x_host, x_ref=x_ref, x_dev=back[:nrhs, :n].T, sentinels_ok=ok, passes=passes, ms=ms)
        # refinement: every other column has steps to take
        x0 = x_host.copy()
        x0[:, ::2] = 0.0
        xh, beh, sth = p.refine_block(b, x0, trans="T")
        tb, hb = _padded(torch, device, b, ld)
        tx, _ = _padded(torch, device, x0, ld)
        torch.cuda.synchronize()
        bed, std = p.refine_block_dev(tb.data_ptr(), tx.data_ptr(), ld, nrhs, trans="T")
        bx = tx.cpu().numpy()
        rok = bool(np.array_equal(tb.cpu().numpy(), hb) and (bx[:nrhs, n:] == SENT).all()
                   and (bx[nrhs] == SENT).all())
        out.update(r_x_host=xh, r_berr_host=beh, r_steps_host=sth, r_x_dev=bx[:nrhs, :n].T, r_berr_dev=bed,
                   r_steps_dev=std, r_ok=rok, r_info=np.array(p.refine_block_info()))
        del p
        np.savez(os.path.join(out_dir, "rank0.npz"), **out)
    except Exception:
        with open(os.path.join(out_dir, "rank0.err"), "w") as fh:
            fh.write(traceback.format_exc())
        raise


@functools.lru_cache(maxsize=None)
def run_device_pointer_t(device=0, timeout=240):
    """One child run per session, shared by the solve and the refinement test."""
    import multiprocessing as mp
    import tempfile
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as out_dir:
        procs = [ctx.Process(target=_dev_worker, args=(out_dir, device))]
        procs[0].start()
        _join(procs, out_dir, timeout)
        z = np.load(os.path.join(out_dir, "rank0.npz"))
        return {k: z[k] for k in z.files}
