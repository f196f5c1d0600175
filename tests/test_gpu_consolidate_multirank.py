"""The consolidation penalty under data parallelism with TWO real rank processes (the pattern of test_gpu_tpgm_multirank: RCCL with
two GPUs, both ranks on cuda:0 over gloo with one).  Each rank estimates the importance on its own image; the accumulated sum and the
count are all-reduced once, so both ranks hold bit-identical importance, equal to the one-process estimate over both images within
the accumulate bound.  Every rank then adds the same penalty gradient to the same all-reduced flat gradient, so the replicas stay
bit-identical and the trajectory is the one-rank global-batch run's."""
import hashlib

import numpy as np
import pytest
import torch

from test_gpu_multirank import _free_port

pytestmark = pytest.mark.gpu
STEPS = 2


def _rank_main(rank, world, port, backend, out):
    import torch.distributed as dist
    from cswin_unet_amd.continual import Consolidation
    from cswin_unet_amd.trainer import DataParallelTrainer
    from test_gpu_consolidate_step import LAM, SGD_LR, _batch9, _synthetic_importance
    from test_gpu_continual_step import OLD, _models
    n_dev = torch.cuda.device_count()
    torch.cuda.set_device(rank % n_dev)
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    net = _models(expand=False)[0]
    img, lab = _batch9(0)
    img, lab = img[rank:rank + 1].contiguous(), lab[rank:rank + 1].contiguous()
    tr = DataParallelTrainer(net, OLD, base_lr=SGD_LR, max_iterations=100, group=dist.group.WORLD, use_graph=True)
    assert tr.collectives and tr.world == 2
    cons = Consolidation(tr, "ewc", weight=LAM)
    cons.estimate([(img, lab)])
    imp = cons.flat.flat_importance.cpu().numpy()
    anchored = bool(torch.equal(cons.flat.flat_anchor, tr.engine.flat_param)) and all(p.grad is None for p in net.parameters()) and net.training
    _synthetic_importance(cons.flat)
    rows = []
    for _ in range(STEPS):
        stats = tr.train_step(img, lab)
        rows.append([float(v) for v in stats] + [float(v) for v in cons.flat.scalars])
    digest = hashlib.sha256(tr.engine.flat_param.cpu().numpy().tobytes()).hexdigest()
    out.put((rank, hashlib.sha256(imp.tobytes()).hexdigest(), imp if rank == 0 else None, anchored, rows, digest))
    dist.barrier()
    dist.destroy_process_group()


def _run_two_ranks():
    import queue
    import time
    import torch.multiprocessing as mp
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, backend, q), daemon=True) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        t0 = time.time()
        while len(res) < 2 and time.time() - t0 < 300:
            try:
                item = q.get(timeout=2)
                res[item[0]] = item[1:]
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs):          # a dead rank: do not wait for the other
                    break
    finally:
        for p in procs:
            p.join(60 if len(res) == 2 else 5)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs) and len(res) == 2, [p.exitcode for p in procs]
    return res, backend


def _one_rank():
    """The one-process run: the importance over the two one-image batches with every gradient read back, then STEPS steps on the
    global batch of both images."""
    from cswin_unet_amd.continual import Consolidation
    from test_gpu_consolidate_step import LAM, _batch9, _synthetic_importance, _trainer
    net, tr = _trainer("sgd", True)
    img, lab = _batch9(0)
    cons = Consolidation(tr, "ewc", weight=LAM)
    seen, launch = [], cons.flat.accumulate

    def recording(grad_scale=1.0):
        seen.append(tr.engine.flat_grad.cpu().numpy())
        launch(grad_scale)
    cons.flat.accumulate = recording
    cons.estimate([(img[r:r + 1].contiguous(), lab[r:r + 1].contiguous()) for r in range(2)])
    opt = tr.engine.opt
    mask = np.zeros(opt.numel, bool)
    for o, p in zip(opt.offsets, opt.params):
        mask[o:o + p.numel()] = True
    _synthetic_importance(cons.flat)
    rows = []
    for _ in range(STEPS):
        stats = tr.train_step(img, lab)
        rows.append([float(v) for v in stats] + [float(v) for v in cons.flat.scalars])
    return seen, mask, np.array(rows)


def test_two_ranks_share_one_importance_and_stay_identical():
    from test_consolidate_host import estimate_bound, importance_ref
    from test_gpu_step_tail import close
    seen, mask, one = _one_rank()
    res, backend = _run_two_ranks()
    (d0, imp, ok0, rows0, p0), (d1, _, ok1, rows1, p1) = res[0], res[1]
    assert d0 == d1, backend                                             # bit-identical importance on both ranks
    assert ok0 and ok1 and len(seen) == 2
    total = importance_ref(seen, 0, count=1)
    close(imp[mask], (total / 2)[mask], estimate_bound(total, 2, 0, 2)[mask], f"consolidate.multirank.{backend}.importance")
    assert (imp[mask] > 0).mean() > 0.5 and (imp[~mask] == 0).all()
    assert p0 == p1, backend                                             # the replicas' flat_param after the steps, bit for bit
    rows0, rows1 = np.array(rows0), np.array(rows1)
    print(backend, "one rank", one, "rank 0", rows0, "rank 1", rows1, sep="\n")
    assert np.array_equal(rows0[:, 3:], rows1[:, 3:])                    # the penalty is formed from identical buffers
    for rows in (rows0, rows1):
        assert np.allclose(rows[:, :3], one[:, :3], rtol=2e-3), (backend, rows, one)       # test_gpu_multirank's tolerance on the losses
        assert rows[0, 3] == 0 and rows[1, 3] > 0 and np.allclose(rows[1:, 3:], one[1:, 3:], rtol=2e-3)
