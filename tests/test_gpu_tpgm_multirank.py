"""TPGM under data parallelism with TWO real rank processes (the pattern of test_gpu_multirank: RCCL with two GPUs, both ranks on
cuda:0 over gloo with one): each rank runs the iterations on its own image, the gradients of the projected weights are all-reduced
before the radii move, so the radii stay bit-identical on both ranks -- and equal the host oracle fed the rank's all-reduced
gradient within the bounds of test_tpgm_host."""
import numpy as np
import pytest
import torch

from test_gpu_multirank import _free_port

pytestmark = pytest.mark.gpu


def _rank_main(rank, world, port, backend, out):
    import torch.distributed as dist
    from cswin_unet_amd.continual import TPGM
    from cswin_unet_amd.trainer import DataParallelTrainer
    from test_gpu_continual_step import LR, NEW, OLD, _batch, _distill, _models
    from test_gpu_tpgm_step import PROJ_LR, _state, move_off_the_anchor, oracle_step
    n_dev = torch.cuda.device_count()
    torch.cuda.set_device(rank % n_dev)
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    net, teacher = _models()
    img, lab = _batch()
    img, lab = img[rank:rank + 1].contiguous(), lab[rank:rank + 1].contiguous()
    tr = DataParallelTrainer(net, OLD + NEW - 1, base_lr=LR, max_iterations=100, group=dist.group.WORLD, use_graph=True, distill=_distill(teacher))
    assert tr.collectives and tr.world == 2
    tp = TPGM(tr, proj_lr=PROJ_LR)
    opt, flat = tr.engine.opt, tp.flat
    move_off_the_anchor(opt)
    norms = flat.tensor_norms().cpu().numpy()
    tp.set_constraints((0.5 * norms.astype(np.float64)).astype(np.float32))
    theta = opt.flat_param.clone()
    tp.iterate([(img, lab)], 1)
    before = _state(flat)
    tp.iterate([(img, lab)], 1)
    after = _state(flat)
    assert bool(torch.equal(opt.flat_param, theta)) and flat.step_count == 2
    # the second iteration against the oracle, from the state the first one left; flat_grad holds the SUM over the ranks
    state = (before["gamma"], before["m"], before["v"])
    held = oracle_step(opt, flat, theta, tr.engine.flat_grad, state, 2, 0.5, float(after["scalars"][1]))
    free = oracle_step(opt, flat, theta, tr.engine.flat_grad, state, 2, 0.5, None)
    worst = {}
    for name in ("gamma", "m", "v", "norm", "ratio"):
        err, bound = np.abs(after[name].astype(np.float64) - held[name][0]), held[name][1]
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[name] = float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
    (gnorm, bG), (coef, bcoef) = free["gnorm"], free["coef"]
    worst["gnorm"] = abs(float(after["scalars"][0]) - gnorm) / bG
    worst["coef"] = 0.0 if (coef == 1.0 and after["scalars"][1] == 1.0) else abs(float(after["scalars"][1]) - coef) / bcoef
    moved = float(np.abs(after["gamma"] - before["gamma"]).max())
    out.put((rank, {k: after[k].tobytes() for k in ("gamma", "m", "v", "ratio")}, worst, (int(held["live"].sum()), int(held["live"].size)), moved))
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
                r, bits, worst, live, moved = q.get(timeout=2)
                res[r] = (bits, worst, live, moved)
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


def test_two_ranks_keep_identical_radii_that_match_the_oracle():
    res, backend = _run_two_ranks()
    for name in ("gamma", "m", "v", "ratio"):
        assert res[0][0][name] == res[1][0][name], (backend, name)          # bit-identical on both ranks
    for r in (0, 1):
        _, worst, live, moved = res[r]
        print(backend, "rank", r, "live radii", live, "largest move", moved, "error / bound", worst)
        assert live[0] > 0.5 * live[1] and moved > 1e-3      # the first iteration moved every live radius by proj_lr: some left (0, norm)
        assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), (backend, r, worst)
