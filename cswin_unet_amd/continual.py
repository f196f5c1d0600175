"""Host side of the continual-learning workflow (the reference's universal_train.py): a trained model is extended to the organ
classes of a new dataset without forgetting the old ones.  The objective itself is ops.continual_loss (csrc/cl_loss.hip); here
are the four small pieces around it:

    old = expand_classes(model, new_classes)            # widen `output`; BEFORE any HipEngine / FlatSGD is built on the model
    teacher = freeze_teacher(model_before_expansion)    # the frozen old model whose logits are distilled
    table = new_label_map(old, new_classes, device)     # new-dataset label k >= 1 -> old + k - 1
    weights = extreme_class_weights(counts, active)     # the focal loss's class weights

and the "surgical" mode's learning rate per parameter tensor (universal_train.py:626-690, 871-896):

    w = surgical_lr_weights(model, engine.opt, batches, distill)    # relative gradient norms of a few batches, largest = 1
    w = surgical_lr_weights(model, engine.opt, batches, distill, method="eb-criterion")     # or: 1 where mean(g^2 / (var_0(g) + 1e-8)) >= 0.95, else 0
    engine.set_lr_weights(w)                                        # FlatAdamW's per-tensor multipliers; unnamed tensors get 0

or that loop's finer-grained relative, finetune.py's surgical trainer, whose rates are renewed at every step on the device
(trainer.surgical_trainer runs the whole loop):

    engine.set_auto_rates(finetune_groups(model))                   # its 22 parameter groups: rate_k = lr * ||g_k|| / max_j ||g_j||, per step

and TPGM, the trainable projection toward the pretrained weights (universal_train.py:391-615, 898-902, 972-974):

    tpgm = TPGM(trainer)                                            # BEFORE fine-tuning: the anchor is the weights as they are now
    if tpgm_due(epoch, start_epoch, frequency): tpgm.iterate(held_out_batches, max_iters)     # learns the radii; the weights are restored
    tpgm.apply()                                                    # once, after training: the weights are projected

and the quadratic penalties that hold every weight near its old-task value in proportion to its importance (EWC, MAS, L2-SP):

    cons = Consolidation(trainer, "ewc", weight=400.0)              # attaches to the engine: every step adds the penalty's gradient
    cons.estimate(old_task_batches)                                 # the empirical Fisher of a few batches; the anchor is the weights now
    state = carry_consolidation_state(cons.state_dict(), dict(expanded_model.named_parameters()))     # across expand_classes

and the two ends of a stage that close the loop, label statistics before it and evaluation after it:

    counts = scan_labels(raw_label_slices, total_classes, table)    # (N, classes + 1) per-slice class histogram, ops.class_counts
    weights = extreme_class_weights(counts.sum(0)[:total_classes], active)
    sampler = PositiveSampling(dataset, scan_labels(raw_label_slices, 4)[:, :4] > 0, KITS23_RULE)
    ...
    results = evaluate_tasks(net, {0: synapse_volumes, 1: kits23_volumes}, REFERENCE_STAGE_CLASSES, (224, 224), resize="hip")

(universal_test.py scores a model per dataset on that dataset's own output channels, task_class_indices; checkpoint_num_classes,
strip_wrapper_prefixes and task_level read a checkpoint's task level.)

surgical_lr_weights, TPGM, Consolidation, scan_labels and evaluate_tasks run kernels; nothing else here does."""
import copy
import math
import random
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
from torch import nn

__all__ = ["expand_classes", "new_label_map", "extreme_class_weights", "freeze_teacher", "Distill", "rgn_weights", "eb_weights", "eb_metrics", "surgical_lr_weights", "finetune_groups", "FINETUNE_GROUPS", "FINETUNE_GRID", "TPGM", "tpgm_due", "Consolidation", "carry_consolidation_state",
           "task_class_indices", "task_level", "checkpoint_num_classes", "strip_wrapper_prefixes", "evaluate_tasks", "scan_labels",
           "PositiveSampling", "REFERENCE_TASKS", "REFERENCE_STAGE_CLASSES", "KITS23_RULE", "LITS17_RULE"]


def _core(model):
    return model.cswin_unet if hasattr(model, "cswin_unet") else model


def expand_classes(model, new_classes):
    """Widen the final 1x1 convolution `output` (no bias) from `old` to old + new_classes - 1 classes -- the new dataset's
    background is the old one (universal_train.py:269) -- and return `old`.  The old rows are copied bit for bit, the new rows
    drawn by kaiming_normal_ (:302-323); `num_classes` follows on the core and on the CSwinUnet wrapper.

    The convolution is REPLACED: call this before a HipEngine, a DataParallelTrainer or a FlatSGD is built on the model (they
    alias the parameters that exist then into flat buffers), and take freeze_teacher()'s copy before it."""
    if new_classes < 1:
        raise ValueError(f"expand_classes: new_classes={new_classes} (it counts the new dataset's background: >= 1)")
    core = _core(model)
    old_conv = core.output
    if not isinstance(old_conv, nn.Conv2d) or old_conv.bias is not None:
        raise TypeError("expand_classes: `output` must be the bias-free nn.Conv2d of CSWinTransformer")
    old = old_conv.out_channels
    total = old + new_classes - 1
    w_old = old_conv.weight
    new_conv = nn.Conv2d(old_conv.in_channels, total, kernel_size=old_conv.kernel_size, stride=old_conv.stride,
                         padding=old_conv.padding, bias=False).to(device=w_old.device, dtype=w_old.dtype)
    with torch.no_grad():
        new_conv.weight[:old] = w_old
        if total > old:
            nn.init.kaiming_normal_(new_conv.weight[old:])
    new_conv.weight.requires_grad_(w_old.requires_grad)
    new_conv.train(old_conv.training)
    core.output = new_conv
    core.num_classes = total
    if core is not model and hasattr(model, "num_classes"):
        model.num_classes = total
    return old


def new_label_map(old_classes, new_classes, device=None):
    """int32 table of map_new_dataset_labels (universal_train.py:243-258): 0 -> 0, k >= 1 -> old_classes + k - 1.  It has
    new_classes entries; ops.continual_loss treats a label outside it as out of range."""
    table = torch.arange(new_classes, dtype=torch.int32) + (old_classes - 1)
    table[0] = 0
    return table.to(device) if device is not None else table


def extreme_class_weights(counts, active_classes):
    """Class weights of universal_train.py:1019-1030 from per-class pixel counts: 1/sqrt(count + 1e-6) on the active classes that
    occur (0 for a count of 0), normalised so that the active weights sum to the number of active classes, background capped at
    0.5, 0 on every other class.  Returns a float32 CPU tensor of len(counts)."""
    counts = torch.as_tensor(counts, dtype=torch.float64)
    active = sorted(set(int(c) for c in active_classes))
    w = torch.zeros(counts.numel(), dtype=torch.float64)
    for c in active:
        if counts[c] > 0:
            w[c] = 1.0 / math.sqrt(float(counts[c]) + 1e-6)
    s = float(w[active].sum()) if active else 0.0
    if s > 0:
        w[active] = w[active] / s * len(active)
    w[0] = min(float(w[0]), 0.5)
    return w.float()


def freeze_teacher(model):
    """A deep copy of `model` in eval() whose parameters take no gradient: the old model of the distillation term."""
    # activations a forward pass left on the modules (the U-Net's boundary tensors) belong to an autograd graph and cannot be
    # deep-copied: the copy gets None in their place.  The model itself is not touched, and every other attribute is copied.
    memo = {}
    for m in model.modules():
        for v in vars(m).values():
            for t in (v if isinstance(v, (list, tuple)) else (v,)):
                if isinstance(t, torch.Tensor) and t.grad_fn is not None:
                    memo[id(t)] = None
    teacher = copy.deepcopy(model, memo)
    teacher.eval()
    teacher.requires_grad_(False)
    return teacher


@dataclass
class Distill:
    """The `distill` option of HipEngine / DataParallelTrainer: the frozen teacher and the parameters of ops.continual_loss."""
    teacher: nn.Module
    w_focal: float = 0.2
    w_dice: float = 0.8
    kd_weight: float = 0.5
    temperature: float = 3.0
    focal_gamma: float = 4.0
    focal_alpha: float = 1.0
    class_weight: Optional[torch.Tensor] = None
    label_map: Optional[torch.Tensor] = None

    @classmethod
    def of(cls, spec):
        return spec if isinstance(spec, cls) or spec is None else cls(**dict(spec))


def rgn_weights(names, norms_per_batch, normalise=True):
    """The RGN learning-rate weights of universal_train.py:626-690 and :876-881 from per-tensor norms.  names: the parameter names,
    aligned with the rows of every entry of norms_per_batch, each a (T, 2) array of (||g||, ||p||).  Names containing "bn" or
    "norm" (any case) are dropped; per batch a tensor's ratio is ||g|| / ||p|| when ||p|| > 1e-8, else 0; the ratios are averaged
    over the batches and divided by their maximum (a maximum <= 0 gives all zeros; normalise=False: the means as they are).
    Returns {name: weight}."""
    names = list(names)
    keep = [i for i, n in enumerate(names) if "bn" not in n.lower() and "norm" not in n.lower()]
    ratios = []
    for norms in norms_per_batch:
        norms = [[float(a), float(b)] for a, b in norms]
        if len(norms) != len(names):
            raise ValueError(f"rgn_weights: {len(norms)} rows of norms for {len(names)} names")
        ratios.append([norms[i][0] / norms[i][1] if norms[i][1] > 1e-8 else 0.0 for i in keep])
    if not ratios:
        return {}
    mean = [sum(r[k] for r in ratios) / len(ratios) for k in range(len(keep))]
    if not normalise:
        return {names[i]: mean[k] for k, i in enumerate(keep)}
    top = max(mean) if mean else 0.0
    return {names[i]: (mean[k] / top if top > 0 else 0.0) for k, i in enumerate(keep)}


def eb_weights(names, evidence_per_batch, threshold=0.95):
    """The eb-criterion learning-rate weights of universal_train.py:669-672 and :883-891 from per-tensor statistics, the counterpart
    of rgn_weights.  names: the parameter names, aligned with the entries of every element of evidence_per_batch, each a (T,)
    sequence of mean(g * g / (var(g, dim 0) + 1e-8)) (optim.FlatAdamW.tensor_evidence).  Names containing "bn" or "norm" (any case)
    are dropped; the statistic is averaged over the batches as np.array(v).mean(0) does, in float64 on the values given; the weight
    is 1.0 where the mean is >= threshold and 0.0 elsewhere, a NaN mean included (the reference's comparison is false for it).
    Nothing is normalised.  Returns {name: weight}, {} without batches; eb_metrics gives the means themselves."""
    return {n: (1.0 if m >= threshold else 0.0) for n, m in eb_metrics(names, evidence_per_batch).items()}


def eb_metrics(names, evidence_per_batch):
    """{name: batch mean of the eb-criterion statistic} for the names eb_weights keeps, in order; {} without batches."""
    names = list(names)
    keep = [i for i, n in enumerate(names) if "bn" not in n.lower() and "norm" not in n.lower()]
    rows = []
    for ev in evidence_per_batch:
        ev = [float(v) for v in ev]
        if len(ev) != len(names):
            raise ValueError(f"eb_weights: {len(ev)} statistics for {len(names)} names")
        rows.append(ev)
    if not rows:
        return {}
    return {names[i]: float(np.array([r[i] for r in rows]).mean(0)) for i in keep}


SURGICAL_METHODS = ("RGN", "eb-criterion")              # universal_train.py's --auto_tune modes


def surgical_lr_weights(model, opt, batches, distill, method="RGN", return_metrics=False):
    """The learning-rate weights of the surgical mode from the focal criterion's gradients on `batches` (an iterable of (image,
    label) device tensors), measured by the flat optimiser `opt` (optim.FlatAdamW built on `model`): per batch one forward in
    eval() mode, ops.continual_loss with the focal term alone (w_focal = 1, w_dice = 0, kd_weight = 0 and the distill's gamma,
    alpha, class weights and label map; the teacher's logits are passed, their term has weight 0), backward, opt.gather_grads()
    and, by `method`, "RGN": opt.tensor_norms() -> rgn_weights; "eb-criterion": opt.tensor_evidence() -> eb_weights.  The
    statistics stay on the device until one host read at the end; the model's training mode is restored and every .grad is None
    afterwards.  `opt` may be a HipEngine's (trainer.engine.opt): the engine's cut of the autograd graph between encoder and decoder
    is lifted while the gradients are measured.  return_metrics=True: (weights, {name: the batch mean the weight was made from}),
    that is the ratio ||g|| / ||p|| before the division by the maximum, or the eb statistic before the threshold (the reference
    logs their range)."""
    from . import ops
    if method not in SURGICAL_METHODS:
        raise ValueError(f"surgical_lr_weights: method={method!r} (one of {SURGICAL_METHODS})")
    eb = method == "eb-criterion"
    d = Distill.of(distill)
    names = dict((p.data_ptr(), n) for n, p in model.named_parameters())
    names = [names[p.data_ptr()] for p in opt.params]
    was_training = model.training
    model.eval()
    # a HipEngine built on the model cuts the autograd graph at the decoder's inputs for its phased backward: one loss.backward()
    # must reach every parameter here, so the cut is lifted for the measurement
    core = _core(model)
    cut = bool(getattr(core, "detach_decoder_inputs", False))
    if cut:
        core.detach_decoder_inputs = False
    stats = []
    try:
        for img, lab in batches:
            logits = model(img)
            with torch.no_grad():
                teacher_logits = d.teacher(img).contiguous()
            loss, _ = ops.continual_loss(logits, lab, teacher_logits, w_focal=1.0, w_dice=0.0, kd_weight=0.0, temperature=d.temperature,
                                         focal_gamma=d.focal_gamma, focal_alpha=d.focal_alpha, class_weight=d.class_weight,
                                         label_map=d.label_map)
            opt.zero_grad()
            loss.backward()
            opt.gather_grads()
            stats.append(opt.tensor_evidence() if eb else opt.tensor_norms())
            opt.zero_grad()
    finally:
        if cut:
            core.detach_decoder_inputs = True
        model.train(was_training)
    host = torch.stack(stats).cpu().tolist() if stats else []          # the one host read
    weights = eb_weights(names, host) if eb else rgn_weights(names, host)
    if not return_metrics:
        return weights
    return weights, (eb_metrics(names, host) if eb else rgn_weights(names, host, normalise=False))


# finetune.py:82-113: the 22 parameter groups of its surgical fine-tuning, each one attribute of the core network, in its order
FINETUNE_GROUPS = (("stem", "stage1_conv_embed"), ("encoder1", "stage1"), ("merge1", "merge1"), ("encoder2", "stage2"), ("merge2", "merge2"),
                   ("encoder3", "stage3"), ("merge3", "merge3"), ("encoder4", "stage4"), ("bottleneck", "norm"),
                   ("decoder4", "stage_up4"), ("upsample4", "upsample4"), ("concat4", "concat_linear4"),
                   ("decoder3", "stage_up3"), ("upsample3", "upsample3"), ("concat3", "concat_linear3"),
                   ("decoder2", "stage_up2"), ("upsample2", "upsample2"), ("concat2", "concat_linear2"),
                   ("decoder1", "stage_up1"), ("upsample1", "upsample1"), ("norm_up", "norm_up"), ("output", "output"))
FINETUNE_GRID = ((1e-3, 1e-4), (1e-4, 1e-4), (1e-5, 1e-4))         # finetune.py:152-156: the (lr, weight decay) pairs it sweeps


def finetune_groups(model):
    """{group: [parameter names]} of finetune.py's get_parameter_groups (:77-114) for `model` (the CSwinUnet wrapper or the core
    network), the 22 groups in the reference's order and the names as model.named_parameters() gives them, in that order: what
    HipEngine.set_auto_rates takes."""
    core, prefix = _core(model), "cswin_unet." if hasattr(model, "cswin_unet") else ""
    return {group: [f"{prefix}{attr}.{n}" for n, _ in getattr(core, attr).named_parameters()] for group, attr in FINETUNE_GROUPS}


def tpgm_due(epoch, start_epoch, frequency):
    """Whether the projection update runs before epoch `epoch` (universal_train.py:898-900)."""
    return epoch >= start_epoch and (epoch - start_epoch + 1) % frequency == 0


class TPGM:
    """The TPGM of universal_train.py:391-615 on a DataParallelTrainer whose engine is a HipEngine: optim.FlatTPGM on the engine's
    flat buffers, driven through the engine's own step hooks, so the captured hipGraphs are replayed as they are (they read the
    projected weights from the flat parameter buffer).  The anchor is the weights at construction.

    Two deliberate differences from universal_train.py ("TPGM"): the radii receive the gradient tpgm.py:47-56 gives
    them (the reference's temporary_parameter_replace cuts the autograd graph, so its own update loop changes nothing), and the
    iterations minimise the objective the engine was built with, through the engine's own forward.  With no iteration run,
    apply() is the reference's projection.

    names in `exclude` are never projected.  Nothing is printed or logged; ratio_stats() is the reference's get_ratio_stats."""

    def __init__(self, trainer, norm_mode="l2", proj_lr=0.01, exclude=()):
        from .optim import FlatTPGM
        eng = trainer.engine
        if not hasattr(eng, "opt") or not hasattr(eng, "param_names"):
            raise TypeError("continual.TPGM needs a trainer whose engine owns flat buffers (HipEngine)")
        self.trainer = trainer
        self.flat = FlatTPGM(eng.opt, eng.param_names, norm_mode=norm_mode, proj_lr=proj_lr, exclude=exclude)

    def iterate(self, batches, max_iters):
        """max_iters projection-update iterations (tpgm_iters(apply=False), :579-603) on `batches`, a re-iterable of (image, label)
        device tensors that is cycled when exhausted: forward and backward under the projected weights, all-reduce of the
        gradient under data parallelism, Adam on the radii, re-projection.  The weights (and the bf16 shadow) are restored
        afterwards, also when a batch raises; the optimiser's state is never touched."""
        import torch.distributed as dist
        tr, flat = self.trainer, self.flat
        eng, world = tr.engine, tr.world
        it = iter(batches)
        flat.begin()
        try:
            for _ in range(int(max_iters)):
                try:
                    img, lab = next(it)
                except StopIteration:
                    it = iter(batches)
                    img, lab = next(it)
                lab = (lab if lab.dtype == torch.int64 else lab.long()).contiguous()
                eng.forward_sums(img, lab, dice_grad_scale=float(world))
                if tr.collectives:
                    dist.all_reduce(eng.sums, group=tr.group)
                eng.finalize(lab.numel() * world)
                for _range in eng.backward_phases(dice_grad_scale=float(world)):
                    pass
                if tr.collectives:
                    dist.all_reduce(eng.flat_grad, group=tr.group)
                flat.update(1.0 / world)
                flat.reproject()
        finally:
            flat.end()

    def apply(self):
        """The final projection (tpgm_iters(apply=True), :613-615): the weights are moved into their balls, once."""
        self.flat.apply()

    def ratio_stats(self):
        return self.flat.ratio_stats()

    def set_constraints(self, gamma):
        self.flat.set_constraints(gamma)

    def state_dict(self):
        return self.flat.state_dict()

    def load_state_dict(self, sd):
        self.flat.load_state_dict(sd)


def _drop_kept_activations(model):
    """None in the place of every activation a forward pass left on the modules (the U-Net's boundary tensors; the next forward
    writes them again): they hold the pass's autograd graph, and with it the parameters' AccumulateGrad nodes, alive."""
    for m in model.modules():
        for k, v in list(vars(m).items()):
            if any(isinstance(t, torch.Tensor) and t.grad_fn is not None for t in (v if isinstance(v, (list, tuple)) else (v,))):
                setattr(m, k, None)


class Consolidation:
    """EWC, MAS or L2-SP on a DataParallelTrainer whose engine is a HipEngine: optim.FlatConsolidation on the engine's flat buffers,
    attached to the engine so that every step's eager tail adds the penalty's gradient to the flat gradient in front of the optimiser
    launch (HipEngine.apply; the captured hipGraphs are replayed as they are).  The anchor is the weights at construction, or
    `state`'s (a state_dict() of an earlier stage, carried onto this model's parameters by carry_consolidation_state).

        cons = Consolidation(trainer, "ewc", weight=400.0)              # after the old task is trained, BEFORE the new one
        cons.estimate(old_task_batches)                                 # importance <- mean of the squared gradients; anchor <- weights
        ... trainer.train_step(...)                                     # cons.penalty is the device float of the last step's penalty
        cons.consolidate(new_task_batches, decay=0.9)                   # online EWC: importance <- decay importance + new; anchor <- weights

    method "ewc": the empirical Fisher of the engine's log-likelihood loss, one squared gradient per BATCH: batches of one sample
    give the per-sample Fisher, larger batches the square of the batch-mean gradient.  "mas": |gradient of the mean squared output
    norm|, no labels used.  "l2sp": importance 1, nothing to estimate.  names in `exclude` are not penalised."""

    def __init__(self, trainer, method="ewc", weight=1.0, exclude=(), state=None):
        from .optim import FlatConsolidation, check_consolidation
        method, weight = check_consolidation(method, weight, "continual.Consolidation")
        if state is not None and state.get("method") != method:
            raise ValueError(f"continual.Consolidation: the state is {state.get('method')!r}'s, method is {method!r}")
        eng = trainer.engine
        if not hasattr(eng, "opt") or not hasattr(eng, "param_names"):
            raise TypeError("continual.Consolidation needs a trainer whose engine owns flat buffers (HipEngine)")
        self.trainer = trainer
        self.flat = FlatConsolidation(eng.opt, eng.param_names, method=method, weight=weight, exclude=exclude)
        if state is not None:
            self._load_tensors(state)
        eng.consolidation = self.flat

    def detach(self):
        """The engine steps without the penalty again; this object keeps its buffers."""
        if self.trainer.engine.consolidation is self.flat:
            self.trainer.engine.consolidation = None

    @property
    def penalty(self):
        """Device view of the last step's (or report()'s) penalty (no sync)."""
        return self.flat.scalars[0:1]

    def report(self):
        """FlatConsolidation.report(): [penalty, sum w_t F d^2, ||theta - anchor||] of the weights as they are, on the device."""
        return self.flat.report()

    def set_weight(self, weight):
        self.flat.set_weight(weight)

    def _default_loss(self):
        from . import ops
        eng = self.trainer.engine
        if self.flat.method == "mas":
            return lambda img, logits, lab: logits.square().sum() / logits.shape[0]
        d = getattr(eng, "distill", None)
        if d is None:
            return lambda img, logits, lab: ops.ce_dice_loss(logits, lab, 1.0, 0.0)[0]

        def focal(img, logits, lab):              # surgical_lr_weights' call: the base loss has no instantiation on the widened head
            with torch.no_grad():
                teacher_logits = d.teacher(img).contiguous()
            return ops.continual_loss(logits, lab, teacher_logits, w_focal=1.0, w_dice=0.0, kd_weight=0.0, temperature=d.temperature,
                                      focal_gamma=d.focal_gamma, focal_alpha=d.focal_alpha, class_weight=d.class_weight, label_map=d.label_map)[0]
        return focal

    def estimate(self, batches, loss=None, decay=0.0):
        """importance <- decay importance + (1 / n) sum over `batches` (an iterable of (image, label) device tensors) of the
        statistic of one eager gradient each; anchor <- the weights.  Per batch one forward in eval() mode, the loss, backward,
        opt.gather_grads() and one accumulate launch; the engine's cut between encoder and decoder is lifted for it.  loss: a
        function (logits, labels) -> scalar, or None for the method's own (the class docstring).  Under data parallelism every
        rank accumulates its own batches, then the sum and the count are all-reduced once.  The training mode is restored and
        every .grad is None afterwards, also when a batch raises (the importance and the anchor are then as they were); weights,
        shadow and optimiser state are never touched."""
        import torch.distributed as dist

        from .optim import check_decay
        flat, tr = self.flat, self.trainer
        if flat.method == "l2sp":
            raise ValueError('continual.Consolidation.estimate: method "l2sp" has importance 1, there is nothing to estimate')
        decay = check_decay(decay, "continual.Consolidation.estimate")
        eng = tr.engine
        model, opt = eng.model, eng.opt
        fn = self._default_loss() if loss is None else (lambda img, logits, lab: loss(logits, lab))
        was_training = model.training
        model.eval()
        core = _core(model)
        cut = bool(getattr(core, "detach_decoder_inputs", False))
        if cut:
            core.detach_decoder_inputs = False
        count, done = 0, False
        flat.begin_estimate()
        # The loop runs on a side stream, as the eager iterations in front of HipEngine's capture do: autograd binds a parameter's
        # AccumulateGrad node to the stream of the forward that first uses it, and the node lives as long as a graph that uses it.
        # Bound to the default stream it would draw that stream into a capture of the step that follows; the activations the
        # model keeps, which hold the last graph, are dropped at the end for the same reason.
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(side):
                for img, lab in batches:
                    lab = (lab if lab.dtype == torch.int64 else lab.long()).contiguous()
                    value = fn(img, model(img), lab)
                    opt.zero_grad()
                    value.backward()
                    opt.gather_grads()
                    flat.accumulate(1.0)
                    opt.zero_grad()
                    count += 1
            done = True
        finally:
            torch.cuda.current_stream().wait_stream(side)
            _drop_kept_activations(model)
            if cut:
                core.detach_decoder_inputs = True
            model.train(was_training)
            opt.zero_grad()
            if not done:
                flat.cancel_estimate()
        if tr.collectives:
            total = torch.tensor([float(count)], dtype=torch.float32, device=opt.flat_param.device)
            dist.all_reduce(flat.scratch, group=tr.group)
            dist.all_reduce(total, group=tr.group)
            count = int(total.item())
        if count == 0:
            flat.cancel_estimate()
            raise ValueError("continual.Consolidation.estimate: no batch was given")
        flat.finish(count, decay)

    def consolidate(self, batches, decay, loss=None):
        """The online form at the end of a stage: importance <- decay importance + this stage's; anchor <- the weights."""
        self.estimate(batches, loss=loss, decay=decay)

    def state_dict(self):
        """{"method", "weight", "exclude", "tensors": {name: {"anchor", "importance"}}}, the tensors in parameter shape (importance
        None for "l2sp"): keyed by name, so that it outlives the flat layout (carry_consolidation_state)."""
        flat, opt = self.flat, self.flat.opt
        tensors = {}
        for n, p, o in zip(flat.names, opt.params, opt.offsets):
            cut = slice(o, o + p.numel())
            tensors[n] = {"anchor": flat.flat_anchor[cut].view(p.shape).clone(),
                          "importance": None if flat.flat_importance is None else flat.flat_importance[cut].view(p.shape).clone()}
        return {"method": flat.method, "weight": flat.weight, "exclude": list(flat.exclude), "tensors": tensors}

    def _load_tensors(self, state):
        flat, opt = self.flat, self.flat.opt
        carried = carry_consolidation_state(state, {n: p.data for n, p in zip(flat.names, opt.params)})
        with torch.no_grad():
            for n, p, o in zip(flat.names, opt.params, opt.offsets):
                cut, entry = slice(o, o + p.numel()), carried["tensors"][n]
                flat.flat_anchor[cut].copy_(entry["anchor"].reshape(-1))
                if flat.flat_importance is not None:
                    flat.flat_importance[cut].copy_(entry["importance"].reshape(-1))

    def load_state_dict(self, state):
        """A state_dict() of this method, carried onto this model's parameters (carry_consolidation_state); the weight follows."""
        if state.get("method") != self.flat.method:
            raise ValueError(f"continual.Consolidation.load_state_dict: the state is {state.get('method')!r}'s, this object {self.flat.method!r}'s")
        self._load_tensors(state)
        self.flat.set_weight(state["weight"])


def carry_consolidation_state(state, current):
    """A Consolidation.state_dict() mapped onto the parameters `current` ({name: tensor}) of a model whose layout has changed since
    (expand_classes runs between the estimation on the old model and the next trainer): a new state with exactly current's names.
    Same shape: copied.  First dimension grown with equal trailing dimensions (the widened `output.weight`): the leading rows are
    carried, the new rows get importance 0 and the current values as anchor.  A name the state does not have: importance 0, anchor
    the current value.  Any other mismatch: ValueError naming the tensor.  No device work beyond the copies; runs on the CPU."""
    l2sp = state.get("method") == "l2sp"
    out = {}
    for name, cur in current.items():
        cur = cur.detach()
        old = state["tensors"].get(name)
        anchor = cur.clone()
        importance = None if l2sp else torch.zeros_like(cur)
        if old is not None:
            a = old["anchor"]
            grown = a.dim() >= 1 and a.dim() == cur.dim() and a.shape[0] < cur.shape[0] and a.shape[1:] == cur.shape[1:]
            if a.shape != cur.shape and not grown:
                raise ValueError(f"carry_consolidation_state: {name} has shape {tuple(a.shape)} in the state and {tuple(cur.shape)} now "
                                 f"(only a grown first dimension can be carried)")
            rows = Ellipsis if a.dim() == 0 else slice(0, a.shape[0])
            anchor[rows] = a.to(device=cur.device, dtype=cur.dtype)
            if not l2sp:
                f = old["importance"]
                if f is None or f.shape != a.shape:
                    raise ValueError(f"carry_consolidation_state: {name} has no importance of its anchor's shape in the state")
                importance[rows] = f.to(device=cur.device, dtype=cur.dtype)
        out[name] = {"anchor": anchor, "importance": importance}
    return {"method": state.get("method"), "weight": state.get("weight"), "exclude": list(state.get("exclude", ())), "tensors": out}


# ------------------------------------------------------------------------------------------------
# evaluation of a continual model (universal_test.py) and the label statistics of a stage
# ------------------------------------------------------------------------------------------------
REFERENCE_TASKS = {"synapse": 0, "kits23": 1, "lits17": 2}          # the reference's chain, in training order
REFERENCE_STAGE_CLASSES = (9, 4, 3)                                 # each dataset's class count, its background included
KITS23_RULE = [(0.3, 3), (0.5, 2), (None, 1)]                       # PositiveSamplingDataset.__getitem__, stage 1 (:223-230)
LITS17_RULE = [(0.4, 2), (None, 1)]                                 # stage 2 (:234-239); None stands for positive_ratio


def _stage_offsets(stage_classes):
    """Total class count after every stage: n0, n0 + (n1 - 1), ... (every later dataset shares the background)."""
    stage_classes = [int(n) for n in stage_classes]
    if not stage_classes or any(n < 1 for n in stage_classes):
        raise ValueError(f"stage_classes={stage_classes!r}: one class count >= 1 per dataset")
    totals = [stage_classes[0]]
    for n in stage_classes[1:]:
        totals.append(totals[-1] + n - 1)
    return stage_classes, totals


def task_class_indices(stage_classes, task):
    """The output channels of dataset `task` in a model trained on the chain stage_classes (per-dataset class counts in training
    order): task 0 has range(n0); task t >= 1 has [0] + the n_t - 1 channels its stage appended.  For (9, 4, 3) these are the
    three lists of universal_test.py:27-40: 0..8, [0, 9, 10, 11], [0, 12, 13]."""
    stage_classes, totals = _stage_offsets(stage_classes)
    if not 0 <= task < len(stage_classes):
        raise ValueError(f"task_class_indices: task {task} of a chain of {len(stage_classes)}")
    if task == 0:
        return list(range(stage_classes[0]))
    return [0] + list(range(totals[task - 1], totals[task]))


def task_level(num_classes, stage_classes):
    """How many tasks of the chain a model with num_classes outputs has learned (9 -> 1, 12 -> 2, 14 -> 3 for the reference's
    chain, universal_test.py:171-178).  ValueError for a count that no prefix of the chain gives."""
    _, totals = _stage_offsets(stage_classes)
    if int(num_classes) not in totals:
        raise ValueError(f"task_level: {num_classes} classes match no prefix of the chain {tuple(stage_classes)} (totals {totals})")
    return totals.index(int(num_classes)) + 1


def strip_wrapper_prefixes(state_dict):
    """A copy of state_dict whose keys have lost every leading "module." (DataParallel) and "base_model." (the reference's
    continual wrapper), in whichever order they were stacked (universal_test.py:206-218)."""
    out = {}
    for key, value in state_dict.items():
        while key.startswith(("module.", "base_model.")):
            key = key.split(".", 1)[1]
        out[key] = value
    return out


def checkpoint_num_classes(state_dict):
    """Class count of a checkpoint: the rows of output.weight or cswin_unet.output.weight after strip_wrapper_prefixes.  KeyError
    if neither is there (the reference goes on to guess among all keys that contain "output"; here that is an error)."""
    sd = strip_wrapper_prefixes(state_dict)
    for key in ("output.weight", "cswin_unet.output.weight"):
        if key in sd:
            return int(sd[key].shape[0])
    raise KeyError("checkpoint_num_classes: neither output.weight nor cswin_unet.output.weight in the state dict")


def evaluate_tasks(net, loaders, stage_classes, patch_size, *, num_classes=None, **evaluate_volumes_kwargs):
    """utils.evaluate_volumes per task of a continual model: loaders maps a task index of the chain stage_classes to a volume
    loader, every task is scored on its own channels (task_class_indices) against its dataset's own label ids.  The model's class
    count is num_classes, or else the num_classes attribute of the first module of net that has one.  A task whose channels reach
    beyond it is refused by name before anything runs (the reference fails with an IndexError inside the first volume).
    Returns {task: (per_volume, class_mean, mean_dice, mean_hd95)} -- evaluate_volumes' return, so with assd=True among the
    keyword arguments (which, like voxelspacing, go to evaluate_volumes as they are) a fifth element mean_assd."""
    from .utils import evaluate_volumes
    stage_classes = [int(n) for n in stage_classes]
    if num_classes is None:
        num_classes = next((m.num_classes for m in net.modules() if isinstance(getattr(m, "num_classes", None), int)), None)
    if num_classes is None:
        raise TypeError("evaluate_tasks: no module of the model has a num_classes attribute; pass num_classes=")
    num_classes = int(num_classes)
    plan = {}
    for task in loaders:
        idx = task_class_indices(stage_classes, task)
        if max(idx) >= num_classes:
            names = {v: k for k, v in REFERENCE_TASKS.items()} if tuple(stage_classes) == REFERENCE_STAGE_CLASSES else {}
            raise ValueError(f"evaluate_tasks: task {task}{' (' + names[task] + ')' if task in names else ''} reads output channels up "
                             f"to {max(idx)}, the model has {num_classes} classes: it has not learned that task")
        plan[task] = idx
    return {task: evaluate_volumes(loaders[task], net, stage_classes[task], patch_size, class_indices=idx, **evaluate_volumes_kwargs)
            for task, idx in plan.items()}


def _label_bytes(a, where):
    """An (H, W) / (n, H, W) array of integer values in 0..255 (any integer or float dtype) as uint8 (n, H, W); ValueError else."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim not in (2, 3) or a.dtype.kind not in "biuf":
        raise ValueError(f"scan_labels: {where} has shape {a.shape} and dtype {a.dtype}; (H, W) or (n, H, W) numbers are scanned")
    a = a[None] if a.ndim == 2 else a
    if a.size:
        bad = (a != np.rint(a)) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
        bad |= ~((a >= 0) & (a <= 255))                         # a NaN fails both comparisons
        if bad.any():
            k = tuple(int(i) for i in np.argwhere(bad)[0])
            raise ValueError(f"scan_labels: {where} holds {a[k]!r} at {k}: not an integer in 0..255")
    return np.ascontiguousarray(a.astype(np.uint8))


def scan_labels(label_slices, ncls, label_map=None, batch=256, device="cuda"):
    """Per-slice class histogram of a dataset's raw labels: an int64 CPU tensor (N, ncls + 1) in input order, column c < ncls the
    pixels of class c, the last column the pixels without a class (ops.class_counts).  label_slices: an iterable of (H, W) or
    (n, H, W) numpy arrays (or CPU tensors) of any integer or float dtype holding integers in 0..255, as the .npz slices do; a
    value that is not raises ValueError before anything is uploaded.  Runs of equal shape are uploaded as uint8 in batches of up
    to `batch` slices, one kernel launch each.  label_map: continual.new_label_map's table (any device) or None.

    `.sum(0)[:ncls]` is the `counts` argument of extreme_class_weights over the WHOLE dataset: the reference counts the first 21
    batches of its shuffled loader only (universal_train.py:1006-1015).  `[:, :classes] > 0` is PositiveSampling's presence
    table, taken from the raw slices and not, as the reference's constructor does, from one random augmentation of each."""
    from . import ops
    dmap = None if label_map is None else torch.as_tensor(label_map).to(device=device, dtype=torch.int32)
    out, pending, held = [], [], 0

    def flush():
        nonlocal pending, held
        if pending:
            dev = torch.from_numpy(np.concatenate(pending)).to(device)
            out.append(ops.class_counts(dev, ncls, dmap).cpu())
            pending, held = [], 0

    for i, a in enumerate(label_slices):
        a = _label_bytes(a, f"entry {i}")
        if pending and pending[0].shape[1:] != a.shape[1:]:
            flush()
        while len(a):
            take = a[:int(batch) - held]
            pending.append(take)
            held += len(take)
            a = a[len(take):]
            if held >= int(batch):
                flush()
    flush()
    return torch.cat(out) if out else torch.zeros((0, int(ncls) + 1), dtype=torch.int64)


class PositiveSampling(torch.utils.data.Dataset):
    """PositiveSamplingDataset of universal_train.py:193-241 with its draw order, on a presence table instead of a decoding pass:
    presence is the boolean (N, classes) table `scan_labels(...)[:, :classes] > 0`, rule an ordered list of (probability or None,
    class), None standing for positive_ratio (KITS23_RULE, LITS17_RULE).  __getitem__(idx): for every entry in turn one
    random.random() is drawn -- always, before the class's slice list is looked at, as in `random.random() < p and
    self.class_indices[c]` -- and on a draw below the probability with a non-empty list the item is
    base_dataset[random.choice(list)]; if no entry fires it is base_dataset[idx % len(base_dataset)]."""

    def __init__(self, base_dataset, presence, rule, positive_ratio=0.8):
        presence = torch.as_tensor(presence)
        if presence.dim() != 2 or presence.shape[0] != len(base_dataset):
            raise ValueError(f"PositiveSampling: presence {tuple(presence.shape)} for a dataset of {len(base_dataset)} samples")
        self.base_dataset, self.positive_ratio = base_dataset, positive_ratio
        self.rule = [(positive_ratio if p is None else float(p), int(c)) for p, c in rule]
        if any(not 0 <= c < presence.shape[1] for _, c in self.rule):
            raise ValueError(f"PositiveSampling: the rule names a class outside the {presence.shape[1]} columns of presence")
        self.class_indices = {c: torch.nonzero(presence[:, c] != 0).flatten().tolist() for _, c in self.rule}

    def __len__(self):
        return len(self.base_dataset)

    def __getitem__(self, idx):
        for p, c in self.rule:
            if random.random() < p and self.class_indices[c]:
                return self.base_dataset[random.choice(self.class_indices[c])]
        return self.base_dataset[idx % len(self.base_dataset)]
