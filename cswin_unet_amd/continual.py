"""Host side of the continual-learning workflow (the reference's universal_train.py): a trained model is extended to the organ
classes of a new dataset without forgetting the old ones.  The objective itself is ops.continual_loss (csrc/cl_loss.hip); here
are the four small pieces around it:

    old = expand_classes(model, new_classes)            # widen `output`; BEFORE any HipEngine / FlatSGD is built on the model
    teacher = freeze_teacher(model_before_expansion)    # the frozen old model whose logits are distilled
    table = new_label_map(old, new_classes, device)     # new-dataset label k >= 1 -> old + k - 1
    weights = extreme_class_weights(counts, active)     # the focal loss's class weights

and the "surgical" mode's learning rate per parameter tensor (universal_train.py:626-690, 871-896):

    w = surgical_lr_weights(model, engine.opt, batches, distill)    # relative gradient norms of a few batches, largest = 1
    engine.set_lr_weights(w)                                        # FlatAdamW's per-tensor multipliers; unnamed tensors get 0

and TPGM, the trainable projection toward the pretrained weights (universal_train.py:391-615, 898-902, 972-974):

    tpgm = TPGM(trainer)                                            # BEFORE fine-tuning: the anchor is the weights as they are now
    if tpgm_due(epoch, start_epoch, frequency): tpgm.iterate(held_out_batches, max_iters)     # learns the radii; the weights are restored
    tpgm.apply()                                                    # once, after training: the weights are projected

Only surgical_lr_weights and TPGM run the model; nothing else here launches a kernel."""
import copy
import math
from dataclasses import dataclass
from typing import Optional

import torch
from torch import nn

__all__ = ["expand_classes", "new_label_map", "extreme_class_weights", "freeze_teacher", "Distill", "rgn_weights", "surgical_lr_weights", "TPGM", "tpgm_due"]


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


def rgn_weights(names, norms_per_batch):
    """The RGN learning-rate weights of universal_train.py:626-690 and :876-881 from per-tensor norms.  names: the parameter names,
    aligned with the rows of every entry of norms_per_batch, each a (T, 2) array of (||g||, ||p||).  Names containing "bn" or
    "norm" (any case) are dropped; per batch a tensor's ratio is ||g|| / ||p|| when ||p|| > 1e-8, else 0; the ratios are averaged
    over the batches and divided by their maximum (a maximum <= 0 gives all zeros).  Returns {name: weight}."""
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
    top = max(mean) if mean else 0.0
    return {names[i]: (mean[k] / top if top > 0 else 0.0) for k, i in enumerate(keep)}


def surgical_lr_weights(model, opt, batches, distill):
    """rgn_weights of the focal criterion's gradients on `batches` (an iterable of (image, label) device tensors), measured by the
    flat optimiser `opt` (optim.FlatAdamW built on `model`): per batch one forward in eval() mode, ops.continual_loss with the
    focal term alone (w_focal = 1, w_dice = 0, kd_weight = 0 and the distill's gamma, alpha, class weights and label map; the
    teacher's logits are passed, their term has weight 0), backward, opt.gather_grads() and opt.tensor_norms().  The norms stay
    on the device until one host read at the end; the model's training mode is restored and every .grad is None afterwards."""
    from . import ops
    d = Distill.of(distill)
    names = dict((p.data_ptr(), n) for n, p in model.named_parameters())
    names = [names[p.data_ptr()] for p in opt.params]
    was_training = model.training
    model.eval()
    norms = []
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
            norms.append(opt.tensor_norms())
            opt.zero_grad()
    finally:
        model.train(was_training)
    host = torch.stack(norms).cpu().tolist() if norms else []          # the one host read
    return rgn_weights(names, host)


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
