"""Data-parallel training step for CSWin-UNet on MI355X (counterpart of the reference's trainer.py:20-95).

Same objective and schedule as ``trainer_synapse``: loss = 0.4*CE + 0.6*Dice (trainer.py:55-57), SGD momentum 0.9 /
weight decay 1e-4 (:42), poly learning rate base_lr*(1 - it/max_it)^0.9 applied after the step (:61-63).  What changes is
the execution model, MI355X-first:

  * one process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI) instead of the reference's single-process
    nn.DataParallel (:37-38): replicas are persistent, only gradients travel.
  * the reference computes the loss on the gathered GLOBAL batch; CE is linear in the per-rank means but soft Dice is
    not, so the 1 + 3*ncls partial sums are all-reduced before the Dice ratio is formed (28 floats) -- the objective
    is the reference's, not a per-rank Dice.
  * gradients are packed by one multi-tensor launch into a flat buffer which is all-reduced in a few large buckets
    (sized for 7 point-to-point xGMI links, not for many small NVSwitch messages) and consumed by one fused SGD launch.
  * the step is captured into four hipGraphs (forward + loss sums | loss + decoder backward + packing | encoder backward
    merge2..norm + packing | encoder backward patch-embed..stage2 + packing) with the collectives between them, so ~700
    kernel launches cost four graph launches on the host, the decoder's gradient all-reduce overlaps the encoder backward,
    the deep encoder's (stage 3/4: 92 % of the encoder bytes) overlaps the shallow encoder backward, and only the last
    ~2.7 MB bucket is exposed.

The protocol (which collectives, which scalings) lives in ``DataParallelTrainer`` and is device agnostic; the device work
lives in an *engine*.  ``HipEngine`` is the product (C ABI kernels, hipGraphs).  tests/test_dp_gloo.py drives the same
protocol with a CPU engine over gloo to check 2-rank == 1-rank-global-batch semantics without a GPU.
"""
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from ._lib import call, ptr, stream
from .continual import Distill
from .ops import BoundaryObjective, CeDiceObjective, ContinualObjective, augment_batch, engine_backward, intensity_batch
from .optim import ADAM_MOMENTS, FlatAdamW, FlatSGD


def init_distributed():
    """(rank, local_rank, world, group).  torchrun / torch.distributed.run environment; world 1 needs nothing."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        torch.cuda.set_device(local % max(torch.cuda.device_count(), 1))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        # "nccl" IS RCCL on ROCm.  CSWIN_DIST_BACKEND=gloo lets several ranks share one GPU (rehearsals on a 1-GPU box:
        # RCCL refuses two ranks on one device); the protocol is the same, only the transport differs.
        backend = os.environ.get("CSWIN_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local, world, (dist.group.WORLD if world > 1 else None)


def synthetic_batch(batch, img_size, num_classes, seed, device):
    """Synthetic stand-in for a Synapse minibatch (datasets/dataset_synapse.py:62-69 after RandomGenerator):
    image (B, 1, H, W) fp32 ~ N(0,1), label (B, H, W) int64 uniform in [0, num_classes)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    img = torch.randn(batch, 1, img_size, img_size, generator=g)
    lab = torch.randint(0, num_classes, (batch, img_size, img_size), generator=g)
    return img.to(device), lab.to(device)


def poly_lr(base_lr, iter_num, max_iterations):
    return base_lr * (1.0 - iter_num / max_iterations) ** 0.9


def cosine_lr(base_lr, epoch, t_max):
    """torch.optim.lr_scheduler.CosineAnnealingLR(T_max=t_max, eta_min=0) in closed form (universal_train.py:894): the rate of
    epoch `epoch`, for a loop that runs lr_schedule="constant" and sets the rate once per epoch."""
    return base_lr * (1.0 + math.cos(math.pi * epoch / t_max)) / 2.0


def kervadec_alpha(epoch, start=0.01, step=0.01, cap=1.0):
    """The boundary loss's weight as Kervadec et al. (MIDL 2019) schedule it: `start` in epoch 0, raised by `step` per epoch, at
    most `cap`.  The ready-made args.boundary_weight of trainer_synapse."""
    return min(start + step * epoch, cap)


def scale_lr_for_batch(base_lr, batch_size):
    """train.py:104-105: base_lr *= batch_size / 24 only when batch_size != 24 and batch_size % 6 == 0 (per-GPU batch)."""
    return base_lr * batch_size / 24 if (batch_size != 24 and batch_size % 6 == 0) else base_lr


def _boundary_alpha(a, who):
    """The boundary loss's weight as a float; ValueError for anything but a finite number (True is no weight)."""
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a):
        raise ValueError(f"{who} must be a finite number, got {a!r}")
    return float(a)


ENGINE_OPTIMIZERS = ("sgd", "adamw", "adam")
DECODER_PREFIXES = ("stage_up", "upsample", "concat_linear", "norm_up", "output")


class HipEngine:
    """Device side of one training step on this rank's MI355X: C-ABI kernels, optionally replayed from hipGraphs.

    Backward runs in two phases -- decoder half, then encoder half (the U-Net's boundary tensors are the bottleneck and
    the three skips) -- each ending with the multi-tensor packing of its gradients, so that the data-parallel protocol
    can put the decoder bucket on the wire (RCCL, own stream) while the encoder half is still computing.

    distill (continual.Distill, or a dict of its fields): the objective becomes the continual-learning one of ops.continual_loss --
    the frozen teacher runs on the same image inside the forward part of the step, `sums` has 3 + 3*ncls entries and `stats` is
    [loss, focal, dice, kd, ce]; w_ce / w_dice are not used then.  The teacher is no part of the optimiser's flat buffers.

    optimizer: "sgd" (FlatSGD, the reference's trainer.py) or "adamw" (FlatAdamW, its universal_train.py: `momentum` is ignored,
    `weight_decay` is AdamW's decoupled decay, max_grad_norm clips the global gradient norm first).  Under data parallelism the
    update runs after the all-reduce, so the norm is the averaged gradient's and every rank forms the same coefficient.
    "adam" is the reference's finetune.py:183: torch.optim.Adam, whose `weight_decay` is added to the gradient (coupled L2); it
    clips like "adamw" when max_grad_norm is given.  moments ("adamw" and "adam"): "kept" is the optimiser as torch runs it, "fresh"
    takes both moments as zero at every step, which is finetune.py:237's optimiser built anew for every step.  set_auto_rates
    turns on that loop's per-step learning rates.

    boundary (None, a float alpha, or a dict of ops.BoundaryObjective's fields): the objective becomes w_ce * CE + w_dice * Dice +
    alpha * boundary (Kervadec et al., MIDL 2019) -- the labels' signed distance maps are made on the device inside the forward
    part of the step, `sums` has 2 + 3*ncls entries and `stats` is [loss, ce, dice, boundary].  alpha is a device float:
    set_boundary_weight changes it between replays of the captured step.  Not together with distill.

    consolidation (an attribute, None by default): an optim.FlatConsolidation on this engine's flat buffers, attached by
    continual.Consolidation.  apply() then adds the EWC / MAS / L2-SP penalty's gradient to flat_grad in front of the optimiser
    launch (two more launches in the eager tail of the step; the captured graphs are untouched); its strength is a device float,
    set_consolidation_weight changes it between steps.  `stats` keeps its layout: the penalty is consolidation.scalars[0]."""

    def __init__(self, model, num_classes, lr, momentum, weight_decay, w_ce, w_dice, use_graph=True, distill=None, optimizer="sgd",
                 max_grad_norm=None, betas=(0.9, 0.999), eps=1e-8, moments="kept", boundary=None):
        if optimizer not in ENGINE_OPTIMIZERS:
            raise ValueError(f"HipEngine: optimizer must be one of {ENGINE_OPTIMIZERS}, got {optimizer!r}")
        if optimizer == "sgd" and max_grad_norm is not None:
            raise ValueError('HipEngine: max_grad_norm needs optimizer="adamw" or "adam" (FlatSGD does not clip)')
        if moments not in ADAM_MOMENTS or (optimizer == "sgd" and moments != "kept"):
            raise ValueError(f'HipEngine: moments must be one of {ADAM_MOMENTS} ("fresh" with optimizer="adamw" or "adam" only), got {moments!r}')
        self.model, self.ncls, self.w_ce, self.w_dice = model, num_classes, w_ce, w_dice
        self.distill = Distill.of(distill)
        if boundary is not None:
            if self.distill is not None:
                raise ValueError("HipEngine: boundary together with distill is not implemented (the continual objective has no boundary term)")
            boundary = dict(boundary) if isinstance(boundary, dict) else dict(alpha=boundary)
            # dist_maps is the per-call cache of ops.boundary_loss: in an engine it would pin one batch's maps for every step
            unknown = set(boundary) - {"w_ce", "w_dice", "alpha", "class_weight", "boundary_class_weight"}
            if unknown:
                raise ValueError(f"HipEngine: boundary has no field {sorted(unknown)} (alpha, w_ce, w_dice, class_weight, boundary_class_weight)")
            boundary["alpha"] = _boundary_alpha(boundary.get("alpha", 0.01), "HipEngine: boundary")
        self.core = model.cswin_unet if hasattr(model, "cswin_unet") else model
        names = [n for n, p in model.named_parameters() if p.requires_grad]
        self.param_names = names                        # aligned with self.opt.params
        if optimizer != "sgd":
            self.opt = FlatAdamW(model.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                 decoupled=optimizer == "adamw", moments=moments)
        else:
            self.opt = FlatSGD(model.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)
        is_dec = [any(seg.startswith(DECODER_PREFIXES) for seg in n.split(".")[:2]) for n in names]
        self.n_enc = is_dec.index(True) if True in is_dec else len(names)
        self.split_backward = 0 < self.n_enc < len(names) and all(is_dec[self.n_enc:]) and hasattr(self.core, "forward_features")
        self.core.detach_decoder_inputs = self.split_backward
        # second cut inside the encoder, in front of merge2: parameters [n_mid, n_enc) = merge2, stage3, merge3, stage4, norm
        self.n_mid = next(i for i, n in enumerate(names) if "merge2" in n.split(".")[:2]) if self.split_backward else 0
        dev = self.opt.flat_param.device
        if boundary is not None:
            self.objective = BoundaryObjective(**{"w_ce": w_ce, "w_dice": w_dice, **boundary})
            self.objective._alpha(dev)                  # the device float exists before any capture: a fill inside a graph would be replayed
        else:
            self.objective = ContinualObjective(self.distill) if self.distill else CeDiceObjective(w_ce, w_dice)
        self.sums = torch.zeros(self.objective.n_sums(num_classes), dtype=torch.float32, device=dev)
        self.stats = torch.zeros(self.objective.n_stats, dtype=torch.float32, device=dev)     # [loss, ce, dice] of the last step; distill: [loss, focal, dice, kd, ce]
        self._teacher_logits, self._batch_pixels = None, None
        self._coef = torch.zeros(2 * num_classes, dtype=torch.float32, device=dev)
        # nn.Dropout with p > 0 (no reference config has one): the dropout kernels take their seeds from the HOST generator when the op
        # is called -- once, at capture, for a replayed graph -- and add the device-resident epoch counter (ops.dropout_epoch) to
        # them; the step advances that counter by one kernel inside graph A, so every replay draws fresh masks
        self._live_dropout = any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in model.modules())
        self.use_graph, self._graphs, self._logits = use_graph, None, None
        self._wire = {}
        self.consolidation = None                       # an optim.FlatConsolidation (continual.Consolidation attaches it): apply() adds its gradient

    # flat views the protocol all-reduces / broadcasts
    @property
    def flat_param(self):
        return self.opt.flat_param

    @property
    def flat_grad(self):
        return self.opt.flat_grad

    def set_lr(self, lr):
        self.opt.set_lr(lr)

    def set_boundary_weight(self, alpha):
        """The boundary term's weight from the next step on, captured or not (an eager fill of the objective's device float)."""
        if not isinstance(self.objective, BoundaryObjective):
            raise ValueError("HipEngine.set_boundary_weight needs an engine built with boundary=")
        self.objective.set_boundary_weight(_boundary_alpha(alpha, "HipEngine.set_boundary_weight: boundary weight"))

    def set_lr_weights(self, weights, default=0.0):
        """Per-tensor learning-rate multipliers by parameter name (continual.surgical_lr_weights' result); a tensor that is not
        named gets `default` -- 0, as the reference's create_surgical_optimizer has it.  None: all 1.  optimizer="adamw" only."""
        if not hasattr(self.opt, "set_lr_weights"):
            raise ValueError('HipEngine.set_lr_weights needs optimizer="adamw"')
        if weights is None:
            self.opt.set_lr_weights(None)
            return
        unknown = set(weights) - set(self.param_names)
        if unknown:
            raise KeyError(f"HipEngine.set_lr_weights: no trainable parameter named {sorted(unknown)[:4]}")
        self.opt.set_lr_weights([float(weights.get(n, default)) for n in self.param_names])

    def set_auto_rates(self, groups, statistic="grad", default=0.0):
        """Per-step learning rates (finetune.py:223-236): every step gives the tensors of group k the rate lr * n_k / max_j n_j,
        n the groups' statistics of that step's own gradient, formed on the device (FlatAdamW.set_auto_rates: no host read, the
        same three launches).  groups: {group: [parameter names]} (continual.finetune_groups), or "tensors" for one group per
        tensor; statistic: "grad", the norm of the group's gradient, or "ratio", that over the norm of its parameters; a tensor
        in no group gets the multiplier `default`.  None turns the rates off.  Replaces set_lr_weights, and is replaced by it.
        optimizer="adamw" or "adam" only.  Under data parallelism the update runs after the all-reduce, so every rank forms the
        same rates from the same averaged flat_grad and the replicas stay bit-identical.  opt.group_stats holds the statistics
        of the last step, one per entry of opt.group_names (the groups in the order their first tensor has among the parameters),
        opt.lr_weights the multipliers."""
        if not hasattr(self.opt, "set_auto_rates"):
            raise ValueError('HipEngine.set_auto_rates needs optimizer="adamw" or "adam"')
        if groups is None:
            self.opt.set_auto_rates(None)
            return
        if isinstance(groups, str):
            if groups != "tensors":
                raise ValueError(f'HipEngine.set_auto_rates: groups must be {{group: [parameter names]}} or "tensors", got {groups!r}')
            per_tensor = list(range(len(self.param_names)))
        else:
            named = [n for members in groups.values() for n in members]
            unknown = set(named) - set(self.param_names)
            if unknown:
                raise KeyError(f"HipEngine.set_auto_rates: no trainable parameter named {sorted(unknown)[:4]}")
            if len(named) != len(set(named)):
                raise ValueError("HipEngine.set_auto_rates: a parameter is named in more than one group")
            empty = [g for g, members in groups.items() if not members]
            if empty:
                raise ValueError(f"HipEngine.set_auto_rates: group {empty[0]!r} has no parameter")
            where = {n: g for g, members in groups.items() for n in members}
            per_tensor = [where.get(n) for n in self.param_names]
        self.opt.set_auto_rates(per_tensor, statistic, default)

    # ---- eager pieces -------------------------------------------------------------------------------------------
    def _forward_sums(self, img, lab):
        if self._live_dropout:
            from .ops import advance_dropout_epoch
            advance_dropout_epoch(img.device)           # inside graph A when captured: a new mask set per replayed step
        logits = self.model(img)
        if self.distill is not None:
            with torch.no_grad():                       # inside graph A when captured; the buffer is kept for the backward graph
                self._teacher_logits = self.distill.teacher(img).contiguous()
        self._batch_pixels = lab.numel() // lab.shape[0]
        self.objective.sums(logits.detach(), lab, self.sums, self._teacher_logits)
        return logits

    def _backward(self, outputs, grad_outputs, lo, hi, extra_inputs=()):
        """One backward phase: the gradients of parameters lo..hi-1 end in their range of opt.flat_grad (placed there by the ops,
        the rest gathered); returns the gradients of `extra_inputs`."""
        params = self.opt.params[lo:hi]
        with engine_backward(self.opt):
            grads = torch.autograd.grad(outputs, params + list(extra_inputs), grad_outputs)
        for p, g in zip(params, grads):
            p.grad = g
        self.opt.gather_grads(lo, hi)
        return list(grads[len(params):])

    def _backward_decoder(self, logits, lab, dice_grad_scale):
        """loss backward + decoder half; returns the gradients of the boundary tensors."""
        dlogits = self.objective.grad(logits.detach(), lab, self._coef, dice_grad_scale, self._teacher_logits)
        n, n_enc = len(self.opt.params), self.n_enc
        self.opt.zero_grad()
        if not self.split_backward:
            self._backward([logits], [dlogits], 0, n)
            return None
        core = self.core
        # core.dec_in: the detached leaves the decoder consumed (detach_decoder_inputs)
        return [core.xb, core.x1, core.x2, core.x3], self._backward([logits], [dlogits], n_enc, n, core.dec_in)

    def _backward_encoder_deep(self, boundary):
        """merge2 .. norm (92 % of the encoder's parameters): from the bottleneck and the stage-3 skip back to the
        detached stage-2 output.  Returns what the shallow phase needs."""
        (xb, x1, x2, x3), (dxb, dx1, dx2, dx3) = boundary
        (dmid,) = self._backward([xb, x3], [dxb, dx3], self.n_mid, self.n_enc, [self.core.enc_mid_in])
        return [x2, x1], [dx2 + dmid, dx1]

    def _backward_encoder(self, boundary, lo=0, hi=None):
        bound, dbound = boundary
        self._backward(bound, dbound, lo, self.n_enc if hi is None else hi)

    def _phase_ranges(self):
        n = len(self.opt.params)
        if not self.split_backward:
            return [self.opt.flat_range(0, n)]
        if self.n_mid:
            return [self.opt.flat_range(self.n_enc, n), self.opt.flat_range(self.n_mid, self.n_enc), self.opt.flat_range(0, self.n_mid)]
        return [self.opt.flat_range(self.n_enc, n), self.opt.flat_range(0, self.n_enc)]

    def _capture(self, img, lab, dice_grad_scale):
        # PyTorch's capture recipe: a few eager iterations on a side stream (allocator state and autograd's
        # AccumulateGrad nodes then belong to a non-default stream), then capture all parts into one memory pool
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                logits = self._forward_sums(img, lab)
                self.finalize(lab.numel())
                boundary = self._backward_decoder(logits, lab, dice_grad_scale)
                if boundary is not None:
                    self._run_encoder_phases(boundary)
        torch.cuda.current_stream().wait_stream(side)
        self._img, self._lab = img.clone(), lab.clone()
        self.opt.zero_grad()
        graphs = [torch.cuda.CUDAGraph()]
        # thread_local: RCCL's watchdog thread polls events of earlier collectives while we capture; its calls must not
        # invalidate the capture (the default "global" mode polices every thread of the process)
        mode = dict(capture_error_mode="thread_local")
        with torch.cuda.graph(graphs[0], **mode):
            logits = self._forward_sums(self._img, self._lab)
        graphs.append(torch.cuda.CUDAGraph())
        with torch.cuda.graph(graphs[1], pool=graphs[0].pool(), **mode):
            boundary = self._backward_decoder(logits, self._lab, dice_grad_scale)
        if boundary is not None:
            for phase in self._encoder_phases(boundary):
                graphs.append(torch.cuda.CUDAGraph())
                with torch.cuda.graph(graphs[-1], pool=graphs[0].pool(), **mode):
                    phase()
        self._graphs = graphs

    def _encoder_phases(self, boundary):
        """The encoder half as callables, one per all-reduce bucket boundary (deep part first: it owns 92 % of the bytes)."""
        if not self.n_mid:
            return [lambda: self._backward_encoder(boundary)]
        state = {}

        def deep():
            state["shallow"] = self._backward_encoder_deep(boundary)

        def shallow():
            self._backward_encoder(state["shallow"], 0, self.n_mid)

        return [deep, shallow]

    def _run_encoder_phases(self, boundary):
        for phase in self._encoder_phases(boundary):
            phase()

    # ---- protocol hooks -----------------------------------------------------------------------------------------
    def forward_sums(self, img, lab, dice_grad_scale):
        """Forward + local loss partial sums -> self.sums (device)."""
        if self.use_graph and self._graphs is None:
            self._capture(img, lab, dice_grad_scale)
        if self._graphs is not None:
            if img.data_ptr() != self._img.data_ptr():
                self._img.copy_(img)
                self._lab.copy_(lab)
            # a replay runs no Python: a weight written from outside the step (load_state_dict, load_from, copy_ on a parameter)
            # since the last one is noticed here by its version counter and answered with one re-pack of the bf16 shadow
            from ._lib import shadows_current
            shadows_current(self.opt)
            self._graphs[0].replay()
        else:
            self._logits = self._forward_sums(img, lab)
            self._lab_eager = lab

    def finalize(self, n_pixels_global):
        """sums (already all-reduced) -> stats and the Dice gradient coefficients.  The global image count (the distillation's
        'batchmean' divides by images) follows from the pixels per image forward_sums saw."""
        self.objective.finalize(self.sums, self.stats, self._coef, n_pixels_global, n_pixels_global // self._batch_pixels)

    def backward_phases(self, dice_grad_scale):
        """Generator: runs one backward phase per iteration and yields the [lo, hi) range of flat_grad it completed."""
        ranges = self._phase_ranges()
        if self._graphs is not None:
            for g, r in zip(self._graphs[1:], ranges):
                g.replay()
                yield r
        else:
            boundary = self._backward_decoder(self._logits, self._lab_eager, dice_grad_scale)
            yield ranges[0]
            if boundary is not None:
                for phase, r in zip(self._encoder_phases(boundary), ranges[1:]):
                    phase()
                    yield r
            self._logits = None

    def set_consolidation_weight(self, weight):
        """The strength of the attached consolidation penalty from the next step on (an eager fill of its device float)."""
        if self.consolidation is None:
            raise ValueError("HipEngine.set_consolidation_weight: no consolidation is attached (continual.Consolidation)")
        self.consolidation.set_weight(weight)

    def apply(self, grad_scale):
        """The eager tail of the step: the attached consolidation penalty's gradient is added to flat_grad first, so clipping, auto
        rates and Adam's moments see it as part of the loss."""
        if self.consolidation is not None:
            self.consolidation.penalise(grad_scale)
        self.opt.apply(grad_scale)

    # bf16 gradient wire (HIP kernels; the wire buffer of a bucket is allocated once and reused every step)
    def pack_wire(self, chunk, dtype, scale=1.0):
        if dtype != torch.bfloat16:
            raise ValueError(f"HipEngine wire dtype {dtype}: only torch.bfloat16 is implemented")
        key = (chunk.data_ptr(), chunk.numel())
        wire = self._wire.get(key)
        if wire is None:
            wire = self._wire[key] = torch.empty(chunk.numel(), dtype=torch.bfloat16, device=chunk.device)
        call("cswin_pack_bf16_scaled", ptr(chunk), ptr(wire), chunk.numel(), float(scale), stream())
        return wire

    def unpack_wire(self, wire, chunk):
        call("cswin_unpack_bf16", ptr(wire), ptr(chunk), chunk.numel(), stream())


class DataParallelTrainer:
    """The data-parallel protocol of one step (device agnostic; see module docstring)."""

    def __init__(self, model=None, num_classes=9, base_lr=0.05, max_iterations=1000, momentum=0.9, weight_decay=1e-4,
                 group=None, use_graph=True, buckets=2, w_ce=0.4, w_dice=0.6, engine=None, force_collectives=False,
                 allreduce_dtype=None, distill=None, optimizer="sgd", max_grad_norm=None, lr_schedule="poly", moments="kept",
                 boundary=None):
        if lr_schedule not in ("poly", "constant"):
            raise ValueError(f'DataParallelTrainer: lr_schedule must be "poly" or "constant", got {lr_schedule!r}')
        if engine is None and optimizer not in ("sgd", "adamw"):
            # this argument keeps its two values; the fine-tuning loop's coupled Adam comes in as an engine of its own
            raise ValueError(f'DataParallelTrainer: optimizer must be "sgd" or "adamw", got {optimizer!r} '
                             f'(torch.optim.Adam\'s coupled decay: pass engine=HipEngine(..., optimizer="adam"))')
        self.lr_schedule = lr_schedule                  # "constant": the step leaves the rate alone (an outer loop sets it, cosine_lr)
        self.group = group
        self.world = dist.get_world_size(group) if group is not None else 1
        self.base_lr, self.max_iterations, self.iter_num = base_lr, max_iterations, 0
        self.engine = engine if engine is not None else HipEngine(model, num_classes, base_lr, momentum, weight_decay,
                                                                 w_ce, w_dice, use_graph, distill, optimizer, max_grad_norm,
                                                                 moments=moments, boundary=boundary)
        self.model = model
        self.nbuckets = max(1, buckets)
        # torch.bfloat16: gradients travel as bf16 (47 MB instead of 94 MB per step, BASELINE configs[2]); the sum is formed
        # in bf16 by the collective, the fp32 master weights and momentum are untouched.  None: fp32 on the wire.
        self.allreduce_dtype = allreduce_dtype
        # run the collectives even with one rank (they are identities then): lets a 1-GPU box exercise the RCCL path
        self.collectives = self.world > 1 or (force_collectives and group is not None)
        if self.collectives:                    # identical replicas: rank 0's initial weights everywhere
            dist.broadcast(self.engine.flat_param, src=0, group=group)
            if hasattr(self.engine, "opt"):
                self.engine.opt.refresh_shadow()        # the broadcast wrote the flat buffer directly (no parameter version moves)

    @property
    def stats(self):
        return self.engine.stats

    def set_boundary_weight(self, alpha):
        """HipEngine.set_boundary_weight: every rank sets the same weight."""
        self.engine.set_boundary_weight(alpha)

    def set_consolidation_weight(self, weight):
        """HipEngine.set_consolidation_weight: every rank sets the same strength, so the replicas stay bit-identical."""
        self.engine.set_consolidation_weight(weight)

    def set_auto_rates(self, groups, statistic="grad", default=0.0):
        """HipEngine.set_auto_rates.  The update runs after the all-reduce, so every rank forms the same rates from the same
        averaged flat_grad: nothing more travels, and the replicas stay bit-identical."""
        self.engine.set_auto_rates(groups, statistic, default)

    # ---- per-phase timing of the backward / all-reduce / update part of a step (bench.py's dp_diagnostics) ----
    _timing = None

    def _mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def enable_timing(self, on=True):
        """Record a HIP event on the compute stream after the loss, after every backward phase, before and after the loop that
        makes the compute stream wait for the collectives (+ the bf16 unpack kernels) and after the update, for the steps that
        follow.  The wait-loop interval is the all-reduce time the backward did NOT hide."""
        self._timing = {"ev": [], "bucket_bytes": []} if on else None

    def collect_timing(self):
        """Mean milliseconds per recorded step: backward phases (in order), exposed all-reduce (+ unpack), update."""
        tm = self._timing
        if not tm or not tm["ev"]:
            return None
        torch.cuda.synchronize()
        rows = [[a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])] for ev in tm["ev"]]
        mean = [sum(r[i] for r in rows) / len(rows) for i in range(len(rows[0]))]
        nph = len(mean) - 3          # events: loss | after each phase (its buckets enqueued) | before the waits | after them | after the update
        return {"steps": len(rows), "backward_phase_ms": [round(v, 3) for v in mean[:nph]],
                "allreduce_exposed_ms": round(mean[nph] + mean[nph + 1], 3), "update_ms": round(mean[nph + 2], 3),
                "bucket_bytes": tm["bucket_bytes"], "wire": "bf16 (pre-divided by world)" if self.allreduce_dtype is not None else "fp32",
                "world": self.world}

    def train_step(self, img, lab):
        """One optimisation step on this rank's shard.  Returns the device tensor [loss, ce, dice] (no host sync)."""
        if lab.dtype != torch.int64:
            lab = lab.long()
        lab = lab.contiguous()
        eng, world = self.engine, self.world
        # Dice is a function of GLOBAL sums; gradients are averaged over ranks afterwards, so the local Dice gradient
        # (already built from global coefficients) is pre-multiplied by world to survive the 1/world averaging.
        eng.forward_sums(img, lab, dice_grad_scale=float(world))
        if self.collectives:
            dist.all_reduce(eng.sums, group=self.group)                 # 1 + 3*ncls floats
        eng.finalize(lab.numel() * world)
        tm = self._timing
        if tm is not None:
            tm["ev"].append([self._mark()])
        works = []
        wired = self.collectives and self.allreduce_dtype is not None
        for lo, hi in eng.backward_phases(dice_grad_scale=float(world)):
            if tm is not None:
                tm["ev"][-1].append(self._mark())
            if self.collectives:
                # this phase's gradients are final: put them on the wire now (RCCL runs on its own stream, ordered after
                # the work enqueued so far) while the next backward phase computes.  Few large buckets: xGMI is 7
                # point-to-point links, per-message latency matters more than on a switched fabric.
                g = eng.flat_grad
                step = max((hi - lo + self.nbuckets - 1) // self.nbuckets, 1 << 22)      # never below 16 MB per message
                step = (step + 63) // 64 * 64                                             # buckets start 256-B aligned
                for o in range(lo, hi, step):
                    chunk = g[o:min(o + step, hi)]
                    if tm is not None and len(tm["ev"]) == 1:
                        tm["bucket_bytes"].append(chunk.numel() * (2 if wired else 4))
                    if not wired:
                        works.append((dist.all_reduce(chunk, group=self.group, async_op=True), None, None))
                    else:
                        # bf16 wire: the bucket is packed PRE-DIVIDED by the world size, so the collective's bf16 sum is the mean
                        # itself (no mantissa bits spent on a factor that is divided out again) and apply() below scales by 1
                        pack = getattr(eng, "pack_wire", None)          # HipEngine: HIP pack kernel into a persistent wire buffer
                        wire = pack(chunk, self.allreduce_dtype, 1.0 / world) if pack else (chunk / world).to(self.allreduce_dtype)
                        works.append((dist.all_reduce(wire, group=self.group, async_op=True), chunk, wire))
        if tm is not None:
            tm["ev"][-1].append(self._mark())
        for w, chunk, wire in works:
            w.wait()
            if wire is not None:
                unpack = getattr(eng, "unpack_wire", None)
                if unpack:
                    unpack(wire, chunk)
                else:
                    chunk.copy_(wire)
        if tm is not None:
            tm["ev"][-1].append(self._mark())
        eng.apply(grad_scale=1.0 if wired else 1.0 / world)
        if tm is not None:
            tm["ev"][-1].append(self._mark())
        self.iter_num += 1
        if self.lr_schedule == "poly":
            eng.set_lr(poly_lr(self.base_lr, self.iter_num - 1, self.max_iterations))   # trainer.py:61-63
        return eng.stats

    def state_dict(self):
        """Reference checkpoint format: the model's state_dict (trainer.py:84)."""
        return self.model.state_dict()


class _Prefetcher:
    """Pinned host batches -> device on a side stream, one batch ahead of the step that consumes them.
    augment="hip": the loader yields RawSliceParams' raw batches (image, uint8 label, params); they are uploaded and finished by
    ops.augment_batch(..., output_size) on the same side stream, so the augmentation too overlaps the previous step, and the
    (image, label) pair handed out is the one the host path yields.  blur_sigma (augment="hip" only): augment_batch's; on the
    host path the loader's RandomGenerator blurs.
    intensity: None, or a datasets.IntensityAugment: after the batch is on the device (and augment_batch has run, with
    augment="hip") the prefetcher draws one record per sample from a numpy Generator of its own, seeded with intensity_seed (an
    int or a sequence of ints), and ops.intensity_batch applies them to the images on the side stream; labels are untouched.
    The draws happen in this process in batch order, so they do not depend on the loader's workers.  intensity_seed may also be
    a numpy.random.Generator, which is then used and advanced: how one stream of draws spans several prefetchers (epochs)."""

    def __init__(self, loader, device, augment="host", output_size=None, blur_sigma=None, intensity=None, intensity_seed=0):
        if augment not in ("host", "hip"):
            raise ValueError(f'_Prefetcher: augment must be "host" or "hip", got {augment!r}')
        if augment == "hip" and (output_size is None or len(output_size) != 2):
            raise ValueError(f'_Prefetcher: augment="hip" needs output_size = (h, w), got {output_size!r}')
        self.it, self.device, self.augment, self.output_size = iter(loader), device, augment, output_size
        self.blur_sigma = blur_sigma if augment == "hip" else None
        self.intensity = intensity
        if intensity is not None:
            self.intensity_rng = intensity_seed if isinstance(intensity_seed, np.random.Generator) else np.random.default_rng(intensity_seed)
        self.stream = torch.cuda.Stream(device)
        self._next()

    def _next(self):
        try:
            batch = next(self.it)
        except StopIteration:
            self.batch = None
            return
        with torch.cuda.stream(self.stream):
            img, lab = batch['image'].to(self.device, non_blocking=True), batch['label'].to(self.device, non_blocking=True)
            if self.augment == "hip":
                # the raw uploads and augment_batch's temporaries are allocated, written and read on the side stream only: they
                # never cross to the consumer's stream, only the two results do (recorded in __next__ like the host path's)
                img, lab = augment_batch(img, lab, batch['params'], self.output_size, blur_sigma=self.blur_sigma)
            if self.intensity is not None:                              # its temporaries, too, live and die on the side stream
                img = intensity_batch(img, self.intensity.draw(img.shape[0], self.intensity_rng))
            self.batch = (img, lab)

    def __iter__(self):
        return self

    def __next__(self):
        if self.batch is None:
            raise StopIteration
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        img, lab = self.batch
        img.record_stream(torch.cuda.current_stream(self.device))
        lab.record_stream(torch.cuda.current_stream(self.device))
        self._next()
        return img, lab


def _step_options(args):
    """The optional attributes of trainer_synapse's `args` that choose the step, each defaulting to trainer.py's own; checked
    before any file or device is touched."""
    from fractions import Fraction

    from .optim import RATE_STATISTICS
    o = dict(optimizer=getattr(args, "optimizer", "sgd"), weight_decay=getattr(args, "weight_decay", 1e-4), w_ce=getattr(args, "w_ce", 0.4),
             w_dice=getattr(args, "w_dice", 0.6), lr_schedule=getattr(args, "lr_schedule", "poly"), moments=getattr(args, "moments", "kept"),
             auto_rates=getattr(args, "auto_rates", None), subset=getattr(args, "subset_fraction", None),
             intensity=getattr(args, "intensity", None), boundary=getattr(args, "boundary_weight", None),
             consolidation=getattr(args, "consolidation", None), consolidation_weight=getattr(args, "consolidation_weight", None))
    cons = o["consolidation"]
    if cons is None:
        if o["consolidation_weight"] is not None:
            raise ValueError("trainer_synapse: consolidation_weight without consolidation (a continual.Consolidation state dict, or a path to one)")
    else:
        from .optim import check_consolidation
        if isinstance(cons, dict):
            if "method" not in cons or "tensors" not in cons:
                raise ValueError('trainer_synapse: consolidation must be a continual.Consolidation.state_dict() ("method", "weight", "tensors")')
            check_consolidation(cons["method"], cons.get("weight", 0.0), "trainer_synapse: consolidation")
        elif not isinstance(cons, (str, os.PathLike)):
            raise ValueError(f"trainer_synapse: consolidation must be None, a continual.Consolidation state dict or a path to one, got {type(cons).__name__}")
        if o["consolidation_weight"] is not None:
            o["consolidation_weight"] = check_consolidation("ewc", o["consolidation_weight"], "trainer_synapse: consolidation_weight")[1]
    if o["boundary"] is not None and not callable(o["boundary"]):
        o["boundary"] = _boundary_alpha(o["boundary"], "trainer_synapse: boundary_weight (None, a number or a function epoch -> weight)")
    if o["intensity"] is not None:
        from .datasets import IntensityAugment
        if o["intensity"] == "nnunet":
            o["intensity"] = IntensityAugment.nnunet()
        elif not isinstance(o["intensity"], IntensityAugment):
            raise ValueError(f'trainer_synapse: intensity must be None, "nnunet" or a datasets.IntensityAugment, got {o["intensity"]!r}')
    if o["optimizer"] not in ENGINE_OPTIMIZERS:
        raise ValueError(f"trainer_synapse: optimizer must be one of {ENGINE_OPTIMIZERS}, got {o['optimizer']!r}")
    if o["lr_schedule"] not in ("poly", "constant"):
        raise ValueError(f'trainer_synapse: lr_schedule must be "poly" or "constant", got {o["lr_schedule"]!r}')
    if o["moments"] not in ADAM_MOMENTS or (o["optimizer"] == "sgd" and o["moments"] != "kept"):
        raise ValueError(f'trainer_synapse: moments must be one of {ADAM_MOMENTS} ("fresh" with optimizer="adamw" or "adam" only), got {o["moments"]!r}')
    if o["auto_rates"] is not None:
        if o["auto_rates"] not in RATE_STATISTICS:
            raise ValueError(f"trainer_synapse: auto_rates must be None or one of {RATE_STATISTICS}, got {o['auto_rates']!r}")
        if o["optimizer"] == "sgd":
            raise ValueError('trainer_synapse: auto_rates needs optimizer="adamw" or "adam" (FlatSGD has one rate)')
    if o["subset"] is not None:
        if not 0.0 < float(o["subset"]) <= 1.0:
            raise ValueError(f"trainer_synapse: subset_fraction must lie in (0, 1], got {o['subset']!r}")
        f = Fraction(o["subset"]).limit_denominator(1000)               # 0.2 is 1/5: n // 5 slices, as finetune.py:167 counts them
        o["subset"] = (f.numerator, f.denominator)
    return o


def trainer_synapse(args, model, snapshot_path, group=None, log_every=1, checkpoint=None):
    """Counterpart of the reference's ``trainer_synapse(args, model, snapshot_path)`` (trainer.py:20-95) on the HIP engine.

    args: root_path, list_dir, img_size, num_classes, batch_size (per GPU), base_lr, max_epochs, optionally num_workers and
    augment: "host" (default) = RandomGenerator in the workers; "hip" = the workers only draw the random parameters
    (RawSliceParams) and the prefetcher applies them on the device (ops.augment_batch: float32 slices of one shape per batch);
    blur_sigma: None (default), or the sigma of the blurred copy of the dataset to train on (finetune.py:262-268 reads
    Synapse_blurred, written by apply_blur_train.py with scipy.ndimage.gaussian_filter): the stored slices are blurred as they
    are read, by RandomGenerator on the host or by ops.augment_batch on the device, whichever `augment` selects.
    Same dataset / augmentation / loss / optimiser / LR schedule / checkpoint schedule (``epoch_N.pth`` every third epoch
    of the second half and at the end, :79-90).  Differences, all execution-side: one process per GPU (pass the process
    group; each rank reads its own shard through a DistributedSampler) instead of nn.DataParallel; batches are prefetched
    to the device on a side stream; the last incomplete batch of an epoch is dropped because the step is a captured
    hipGraph with a fixed batch shape; tensorboard image logging is not reproduced.

    Further optional attributes of args choose another step, each defaulting to the above (surgical_trainer sets them all):
    optimizer ("sgd", "adamw", "adam": HipEngine's), weight_decay (1e-4), w_ce / w_dice (0.4 / 0.6), lr_schedule ("poly", or
    "constant": the rate stays base_lr), moments ("kept" / "fresh": HipEngine's), auto_rates (None, or "grad" / "ratio": per-step
    rates over continual.finetune_groups(model) with that statistic, HipEngine.set_auto_rates), subset_fraction (None, or the part
    of the slices to train on, torch.randperm(n, generator=manual_seed(seed))[:n * fraction], finetune.py:166-169).
    intensity: None (default), "nnunet" or a datasets.IntensityAugment: appearance augmentation of every batch on the device
    (ops.intensity_batch on the prefetcher's stream, after either `augment` path), drawn from one numpy Generator seeded with
    (seed, rank): ranks differ, and a seeded run draws the same records whatever num_workers is.
    boundary_weight: None (default), the weight alpha of the boundary loss (HipEngine's boundary=) as a float, or a function
    epoch -> alpha applied at the start of every epoch (kervadec_alpha is the published schedule); the log line then carries the
    boundary term.
    consolidation: None (default), or the state_dict() of a continual.Consolidation estimated on the old task (or a path to one
    saved with torch.save): the EWC / MAS / L2-SP penalty of that state, carried onto this model's parameters
    (continual.carry_consolidation_state), is attached to the engine for the whole run, and the log gains its value.
    consolidation_weight: its strength (default: the state's own).
    checkpoint: None for the schedule above, or a function epoch -> file name or None."""
    import logging
    import random
    import sys

    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler

    from .checkpoint import save_checkpoint
    from .datasets import RandomGenerator, RawSliceParams, Synapse_dataset, collate_raw_slices

    augment = getattr(args, "augment", "host")
    if augment not in ("host", "hip"):
        raise ValueError(f'trainer_synapse: augment must be "host" or "hip", got {augment!r}')
    blur_sigma = getattr(args, "blur_sigma", None)
    if blur_sigma is not None:
        from .utils import gaussian_taps
        gaussian_taps(blur_sigma)                                       # ValueError for a sigma neither path takes
    opts = _step_options(args)
    os.makedirs(snapshot_path, exist_ok=True)
    logging.basicConfig(filename=os.path.join(snapshot_path, "log.txt"), level=logging.INFO,
                        format='[%(asctime)s.%(msecs)03d] %(message)s', datefmt='%H:%M:%S')
    if not any(isinstance(h, logging.StreamHandler) and getattr(h, "stream", None) is sys.stdout for h in logging.getLogger().handlers):
        logging.getLogger().addHandler(logging.StreamHandler(sys.stdout))
    logging.info(str(args))
    rank = dist.get_rank(group) if group is not None else 0
    world = dist.get_world_size(group) if group is not None else 1
    device = next(model.parameters()).device
    db_train = Synapse_dataset(base_dir=args.root_path, list_dir=args.list_dir, split="train",
                               transform=RawSliceParams(output_size=[args.img_size, args.img_size]) if augment == "hip" else
                               RandomGenerator(output_size=[args.img_size, args.img_size], blur_sigma=blur_sigma))
    seed = getattr(args, "seed", 1234)
    if opts["subset"] is not None:
        # finetune.py:166-169: a fixed random part of the slices, drawn once from the seed
        num, den = opts["subset"]
        n_all = len(db_train)
        keep = torch.randperm(n_all, generator=torch.Generator().manual_seed(seed))[:n_all * num // den]
        db_train = torch.utils.data.Subset(db_train, keep.tolist())
    print("The length of train set is: {}".format(len(db_train)))

    n_workers = getattr(args, "num_workers", 8)

    def worker_init_fn(worker_id):
        # trainer.py:33-34 seeds `random` only, with seed + worker_id.  Under data parallelism every rank would then share
        # one augmentation coin-flip stream, so the seed is offset by rank * num_workers (rank 0 = the reference's seeds).
        random.seed(seed + rank * max(n_workers, 1) + worker_id)

    sampler = DistributedSampler(db_train, num_replicas=world, rank=rank, shuffle=True, seed=seed) if world > 1 else None
    loader = DataLoader(db_train, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler,
                        num_workers=n_workers, pin_memory=True, drop_last=True, worker_init_fn=worker_init_fn,
                        collate_fn=collate_raw_slices if augment == "hip" else None,
                        persistent_workers=False)    # like the reference: workers are re-created and re-seeded every epoch
    max_epoch = args.max_epochs
    max_iterations = max_epoch * len(loader)
    if max_iterations == 0:
        raise ValueError(f"trainer_synapse: {len(db_train)} samples give no full batch of {args.batch_size} per rank "
                         f"(the captured step has a fixed batch shape, the last incomplete batch is dropped)")
    logging.info("{} iterations per epoch. {} max iterations ".format(len(loader), max_iterations))
    model.train()
    step = dict(weight_decay=opts["weight_decay"], w_ce=opts["w_ce"], w_dice=opts["w_dice"])
    boundary = opts["boundary"]
    if boundary is not None:
        step.update(boundary=float(boundary(0)) if callable(boundary) else boundary)
    if opts["optimizer"] == "adam":                  # DataParallelTrainer's own `optimizer` keeps its two values: the engine is handed in
        engine = HipEngine(model, args.num_classes, args.base_lr, 0.9, use_graph=True, optimizer="adam", moments=opts["moments"], **step)
        step = dict(engine=engine)
    else:
        step.update(optimizer=opts["optimizer"], moments=opts["moments"])
    trainer = DataParallelTrainer(model, args.num_classes, base_lr=args.base_lr, max_iterations=max_iterations, group=group,
                                  lr_schedule=opts["lr_schedule"], **step)
    if opts["auto_rates"] is not None:
        from .continual import finetune_groups
        trainer.set_auto_rates(finetune_groups(model), opts["auto_rates"])
    cons = None
    if opts["consolidation"] is not None:
        from .continual import Consolidation
        state = opts["consolidation"]
        if not isinstance(state, dict):
            state = torch.load(state, map_location=device)
        weight = state["weight"] if opts["consolidation_weight"] is None else opts["consolidation_weight"]
        cons = Consolidation(trainer, method=state["method"], weight=weight, exclude=state.get("exclude", ()), state=state)
    iter_num = 0
    intensity_rng = np.random.default_rng([int(seed), rank]) if opts["intensity"] is not None else None     # one stream over all epochs
    for epoch_num in range(max_epoch):
        if sampler is not None:
            sampler.set_epoch(epoch_num)
        if callable(boundary):
            trainer.set_boundary_weight(float(boundary(epoch_num)))
            if rank == 0:
                logging.info('epoch %d : boundary weight : %f' % (epoch_num, trainer.engine.objective.alpha))
        for image_batch, label_batch in _Prefetcher(loader, device, augment, (args.img_size, args.img_size), blur_sigma=blur_sigma,
                                                    intensity=opts["intensity"], intensity_seed=intensity_rng):
            stats = trainer.train_step(image_batch, label_batch)
            iter_num += 1
            if log_every and iter_num % log_every == 0 and rank == 0:
                loss, loss_ce, *rest = stats.tolist()                # the only host sync of the loop
                if boundary is None:
                    logging.info('iteration %d : loss : %f, loss_ce: %f' % (iter_num, loss, loss_ce))
                else:
                    logging.info('iteration %d : loss : %f, loss_ce: %f, loss_dice: %f, loss_boundary: %f' % (iter_num, loss, loss_ce, *rest))
                if cons is not None:                                 # the penalty of this step's weights before the update; same sync point
                    logging.info('iteration %d : consolidation penalty : %f' % (iter_num, float(cons.penalty)))
                if opts["auto_rates"] is not None:                   # finetune.py:236 logs every group's rate; same sync point
                    opt = trainer.engine.opt
                    rates = dict(zip(opt.group_names, (opt.group_stats / opt.group_stats.max() * opt.lr_dev).tolist()))
                    logging.info('iteration %d : group rates : %s' % (iter_num, rates))
        if checkpoint is not None:
            name = checkpoint(epoch_num)
        else:
            save_interval = 3
            last = epoch_num >= max_epoch - 1
            name = 'epoch_' + str(epoch_num) + '.pth' if last or (epoch_num > int(max_epoch / 2) and (epoch_num + 1) % save_interval == 0) else None
        if rank == 0 and name is not None:
            save_mode_path = os.path.join(snapshot_path, name)
            save_checkpoint(model, save_mode_path)
            logging.info("save model to {}".format(save_mode_path))
    return "Training Finished!"


def surgical_trainer(args, model, snapshot_path, group=None, log_every=1):
    """Counterpart of the reference's ``surgical_trainer(args, model, snapshot_path)`` (finetune.py:146-254), its surgical
    fine-tuning on the blurred Synapse slices, for ONE (lr, weight decay) pair: args.base_lr and args.weight_decay (default 1e-4).
    The reference sweeps continual.FINETUNE_GRID from one pretrained model; that sweep is the caller's loop, a fresh copy of the
    model per pair.

    It is trainer_synapse with: loss 0.2 CE + 0.8 Dice (:205); torch.optim.Adam with coupled weight decay (:183, optimizer="adam");
    a constant rate; every step's rate of each of the 22 groups of continual.finetune_groups set to lr * n_k / max_j n_j, n the
    norm of the group's gradient (:116-144, 225-236; auto_rates="grad", formed on the device); a fifth of the slices, drawn once
    from args.seed (:166-169); a checkpoint model_lr{lr}_wd{wd}_epoch{epoch}.pth whenever epoch % args.save_interval == 0 (:250-251,
    save_interval defaults to 1).  args.boundary_weight, args.consolidation and args.consolidation_weight are passed on as they are.  args.moments ("kept" by default) chooses between Adam with running moments and the reference
    as written, which builds a new optimiser every step ("fresh").  args.auto_rates and args.subset_fraction override the
    statistic and the part.  Deviations: one forward/backward per step, whose gradient is both measured and
    applied, where the reference measures on a second batch and steps with that batch's gradient; the per-step tune_metrics.pt
    and the debug image are not written (the group rates are logged every log_every steps)."""
    import copy

    args = copy.copy(args)
    lr, wd = args.base_lr, getattr(args, "weight_decay", 1e-4)
    interval = getattr(args, "save_interval", 1)
    args.optimizer, args.weight_decay, args.w_ce, args.w_dice, args.lr_schedule = "adam", wd, 0.2, 0.8, "constant"
    args.moments = getattr(args, "moments", "kept")
    args.auto_rates = getattr(args, "auto_rates", "grad")
    args.subset_fraction = getattr(args, "subset_fraction", 0.2)
    trainer_synapse(args, model, snapshot_path, group=group, log_every=log_every,
                    checkpoint=lambda epoch: f"model_lr{lr}_wd{wd}_epoch{epoch}.pth" if epoch % interval == 0 else None)
    return "Surgical Training Finished!"
