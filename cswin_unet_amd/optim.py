"""The optimisers of the training loops on flat buffers: SGD(momentum, weight_decay) of the reference's trainer.py:42,60-63
(FlatSGD), clip_grad_norm_ + AdamW with a learning rate per tensor of its universal_train.py:693-725, 934-939 (FlatAdamW; with
decoupled=False and set_auto_rates the Adam with per-step group rates of its finetune.py:183, 223-239), and the trainable projection toward the pretrained weights of its :391-615 (FlatTPGM, over either of the two).

All parameters are re-pointed into ONE flat fp32 buffer (32-B aligned slots), the optimiser state and the gradients live in
more of the same layout.  A step is a multi-tensor gather of the per-parameter .grad tensors into the flat gradient buffer (the
buffer RCCL all-reduces, in buckets, under data parallelism) and one fused update kernel -- for AdamW with clipping, two norm
kernels in front of it.  The learning rate lives in device memory so that a captured hipGraph can be replayed under a schedule.
"""
from typing import NamedTuple

import numpy as np
import torch

from ._lib import call, precision, ptr, register_shadow, stream

_CHUNK = 16384      # floats per gather / update workgroup


def _next_bias_corrections(obj, what, betas):
    """obj.step_count moved on by one and (1 - beta1^t, 1 - beta2^t) of the new count, in Python floats as torch forms them.
    Refused inside a stream capture, the count untouched."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what} inside a stream capture: the host's step count, and with it the bias corrections, would be frozen into the graph")
    obj.step_count += 1
    return 1.0 - betas[0] ** obj.step_count, 1.0 - betas[1] ** obj.step_count


class _FlatBuffers:
    """The slot layout, the chunk table, the gradient gather and the bf16 shadow that the flat optimisers share."""

    def __init__(self, params, lr):
        name = type(self).__name__
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError(f"{name} got no trainable parameters")
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"{name} runs on a HIP device only")
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + 7) // 8 * 8          # 32-B slots: the bf16 shadow of every parameter is 16-B aligned as well
        self.numel = off
        rows, first = chunk_table([p.numel() for p in self.params], self.offsets)
        self.nchunks = len(rows)
        self.chunks = torch.from_numpy(rows.view(np.int64).reshape(-1, 2)).to(dev)        # built and uploaded once, for FlatTPGM as well
        self.first_chunk = torch.from_numpy(first).to(dev)
        self.flat_param = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(off, dtype=torch.float32, device=dev)
        self._alloc_state(off, dev)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat_param[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view                       # parameters now alias the flat buffer
        # bf16 working copy of the weights for the bf16 matmul mode (the Linears read it instead of rounding the fp32 master
        # weights in every GEMM); written by the update kernel, re-packed when something else writes the parameters
        self.flat_param16 = torch.empty(off, dtype=torch.bfloat16, device=dev)
        self.refresh_shadow()
        register_shadow(self, self.flat_param)
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        self.lr = float(lr)
        # gather tables: one {src, dst, n} record per <= 16 Ki-float chunk, per gathered parameter range
        self._tables = {}
        self.param_groups = [{"lr": self.lr, "params": self.params}]   # torch.optim-like view for loops that poke lr

    def _alloc_state(self, numel, dev):
        raise NotImplementedError

    # -- schedule -------------------------------------------------------------------------------------------
    def set_lr(self, lr):
        self.lr = float(lr)
        self.param_groups[0]["lr"] = self.lr
        self.lr_dev.fill_(self.lr)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    # -- step -----------------------------------------------------------------------------------------------
    def flat_range(self, first, last):
        """[lo, hi) element range of the flat buffers covered by parameters first..last-1."""
        lo = self.offsets[first]
        hi = self.offsets[last - 1] + (self.params[last - 1].numel() + 7) // 8 * 8
        return lo, hi

    def _gather_table(self, first, last):
        """(device table of {src, dst, n} rows, row count) that packs p.grad of parameters first..last-1 into flat_grad; rebuilt
        when a gradient has moved.  Gradients that already are their slot (ops.engine_backward) need no row."""
        name = type(self).__name__
        key = tuple(p.grad.data_ptr() if p.grad is not None else 0 for p in self.params[first:last])
        slot = self._tables.setdefault((first, last), {"key": None, "n": 0, "host": None, "dev": None})
        if key != slot["key"]:
            rows = []
            base = self.flat_grad.data_ptr()
            for p, o, src in zip(self.params[first:last], self.offsets[first:last], key):
                if src == 0:
                    raise RuntimeError(f"{name}.step(): a parameter has no gradient")
                if src == base + 4 * o:
                    continue                          # written in place: nothing to pack
                if not p.grad.is_contiguous():
                    raise RuntimeError(f"{name}.step(): non-contiguous gradient")
                n = p.numel()
                for c in range(0, n, _CHUNK):
                    rows.append((src + 4 * c, base + 4 * (o + c), min(_CHUNK, n - c)))
            if rows:
                capturing = torch.cuda.is_current_stream_capturing()
                if slot["host"] is None or slot["host"].shape[0] != len(rows):
                    # the row count depends on how many gradients were placed; the tables are sized in an eager warm-up
                    if capturing:
                        raise RuntimeError(f"{name}: the gather table would have to be reallocated inside a stream capture")
                    slot["host"] = torch.zeros(len(rows), 3, dtype=torch.int64).pin_memory()
                    slot["dev"] = torch.zeros(len(rows), 3, dtype=torch.int64, device=self.flat_grad.device)
                if not capturing:
                    torch.cuda.current_stream().synchronize()      # a previous async upload may still read the host buffer
                slot["host"].numpy()[:] = np.asarray(rows, dtype=np.int64)
                # async upload from pinned memory: a memcpy node when captured (the host buffer lives with the optimiser)
                slot["dev"].copy_(slot["host"], non_blocking=True)
            slot["key"], slot["n"] = key, len(rows)
        return slot["dev"], slot["n"]

    def gather_grads(self, first=0, last=None):
        """Pack p.grad of parameters first..last-1 into self.flat_grad (one launch)."""
        table, rows = self._gather_table(first, len(self.params) if last is None else last)
        if rows:
            call("cswin_multi_copy", ptr(table), rows, stream())
        return self.flat_grad

    def refresh_shadow(self):
        call("cswin_pack_bf16", ptr(self.flat_param), ptr(self.flat_param16), self.numel, stream())

    def step(self, grad_scale=1.0):
        self.gather_grads()
        self.apply(grad_scale)


class FlatSGD(_FlatBuffers):
    def __init__(self, params, lr, momentum=0.9, weight_decay=1e-4):
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        super().__init__(params, lr)

    def _alloc_state(self, numel, dev):
        self.flat_mom = torch.zeros(numel, dtype=torch.float32, device=dev)

    def apply(self, grad_scale=1.0):
        """p, m <- SGD(flat_grad * grad_scale) (one launch)."""
        call("cswin_sgd_flat", ptr(self.flat_param), ptr(self.flat_grad), ptr(self.flat_mom), self.numel, ptr(self.lr_dev),
             self.momentum, self.weight_decay, float(grad_scale), ptr(self.flat_param16) if precision() == 1 else None, stream())

    def state_dict(self):
        return {"momentum": self.flat_mom.clone(), "lr": self.lr}

    def load_state_dict(self, sd):
        self.flat_mom.copy_(sd["momentum"])
        self.set_lr(sd["lr"])


def chunk_table(numels, offsets):
    """The static table the chunked kernels walk (csrc/flat_chunks.h): (records, first_chunk).  records: one {'off': int64 element offset into the flat
    buffers, 'n': int32 <= 16384, 'tensor': int32} per chunk (16 bytes, the library's record), tensors in order and each tensor's
    chunks in order; chunks tile [offset, offset + numel) of every tensor exactly, so none crosses a slot or covers a pad word,
    and every offset is a multiple of 4 (slots start at multiples of 8, 16384 is one of 4).  first_chunk: int32 (T + 1,), the
    chunks of tensor t are first_chunk[t] .. first_chunk[t + 1] - 1."""
    rec = np.dtype([("off", "<i8"), ("n", "<i4"), ("tensor", "<i4")])
    rows, first = [], [0]
    for t, (n, o) in enumerate(zip(numels, offsets)):
        if n <= 0 or o % 8:
            raise ValueError(f"chunk_table: tensor {t} has {n} elements at offset {o} (slots start at multiples of 8 floats)")
        rows += [(o + c, min(_CHUNK, n - c), t) for c in range(0, n, _CHUNK)]
        first.append(len(rows))
    return np.array(rows, dtype=rec), np.array(first, dtype=np.int32)


_EB_COLS = 64       # columns of a tile of csrc/eb.hip at the most: one wave's lanes


def column_tiles(shapes, offsets):
    """The static table of csrc/eb.hip, which reduces along dimension 0 of every tensor: (records, first_tile).  A tensor of shape
    (d0, ...) at element offset `off` is d0 rows of inner = numel / d0 contiguous columns (a 0-dimensional tensor counts as (1,)).
    records: one {'off': int64, 'd0', 'inner', 'col0', 'ncols', 'tensor', 'width': int32} per tile (32 bytes, the library's record),
    tensors in order and each tensor's tiles in column order; a tile is all d0 rows of columns col0 .. col0 + ncols - 1, tiles take
    64 columns each until the last takes the rest, so every column is covered exactly once and no pad word is.  width is the
    smallest power of two >= ncols: the lanes that run along the columns, 256 / width row phases share dimension 0 (1 for a bias,
    16 for inner = 9).  first_tile: int32 (T + 1,), the tiles of tensor t are first_tile[t] .. first_tile[t + 1] - 1.  This is the
    table's only producer, so the kernel's preconditions are checked here."""
    rec = np.dtype([("off", "<i8"), ("d0", "<i4"), ("inner", "<i4"), ("col0", "<i4"), ("ncols", "<i4"), ("tensor", "<i4"), ("width", "<i4")])
    rows, first = [], [0]
    for t, (shape, o) in enumerate(zip(shapes, offsets)):
        shape = tuple(int(s) for s in shape) or (1,)
        numel = int(np.prod(shape, dtype=np.int64))
        if numel <= 0 or numel >= 2 ** 31 or o % 8:
            raise ValueError(f"column_tiles: tensor {t} has shape {shape} at offset {o} (1 to 2^31 - 1 elements, slots start at multiples of 8 floats)")
        d0, inner = shape[0], numel // shape[0]
        for col0 in range(0, inner, _EB_COLS):
            ncols = min(_EB_COLS, inner - col0)
            rows.append((o, d0, inner, col0, ncols, t, 1 << (ncols - 1).bit_length()))
        first.append(len(rows))
    rows = np.array(rows, dtype=rec)
    ok = ((rows["col0"] >= 0) & (rows["ncols"] >= 1) & (rows["col0"] + rows["ncols"] <= rows["inner"]) & (rows["ncols"] <= rows["width"])
          & (rows["width"] <= _EB_COLS) & (rows["width"] & (rows["width"] - 1) == 0))
    if not ok.all():
        raise ValueError(f"column_tiles: record {int(np.argmin(ok))} would read outside its tensor: {rows[int(np.argmin(ok))]}")
    return rows, np.array(first, dtype=np.int32)


RATE_STATISTICS = ("grad", "ratio")    # cswin_rate_finalize's `statistic`, by index
ADAM_MOMENTS = ("kept", "fresh")
ADAM_COUPLED, ADAM_FRESH = 1, 2        # the bits of cswin_adam_flat's flags


def group_table(groups, ntensors, statistic="grad"):
    """The static table of cswin_rate_finalize (csrc/adamw.hip): (group_first, group_tensors, group_of, names).  groups: one entry
    per tensor, a hashable group id or None for a tensor in no group; the groups are numbered in order of first appearance
    (names[k] is group k's id).  group_first: int32 (G + 1,); group_tensors: int32 CSR list, group k's tensors are
    group_tensors[group_first[k] .. group_first[k + 1] - 1] in tensor order (they need not be contiguous); group_of: int32 (T,), -1
    for a tensor in no group.  This is the table's only producer, so the kernel's preconditions are checked here, and `statistic`
    with them."""
    if statistic not in RATE_STATISTICS:
        raise ValueError(f"group_table: statistic must be one of {RATE_STATISTICS}, got {statistic!r}")
    groups = list(groups)
    if len(groups) != ntensors:
        raise ValueError(f"group_table: {len(groups)} group entries for {ntensors} parameter tensors")
    index, members = {}, []
    group_of = np.full(ntensors, -1, np.int32)
    for t, g in enumerate(groups):
        if g is None:
            continue
        if g not in index:
            index[g] = len(members)
            members.append([])
        group_of[t] = index[g]
        members[index[g]].append(t)
    if not members:
        raise ValueError("group_table: no tensor is in a group")
    first = np.cumsum([0] + [len(m) for m in members]).astype(np.int32)
    tensors = np.array([t for m in members for t in m], dtype=np.int32)
    return first, tensors, group_of, list(index)


class FlatAdamW(_FlatBuffers):
    """torch.optim.AdamW (decoupled weight decay) on the flat buffers, with torch.nn.utils.clip_grad_norm_(max_grad_norm) fused
    in front of it when max_grad_norm is given and an optional learning-rate multiplier per parameter tensor (set_lr_weights).
    apply() is three launches (two without clipping), no host sync and no allocation; the step count lives on the host, where
    the bias corrections 1 - beta^t are formed in Python floats as torch forms them.

    decoupled=False: torch.optim.Adam(weight_decay), the decay added to the gradient (finetune.py:183).  moments="fresh": m and v
    are zero at every step and never touched, which is an optimiser built anew for every step (finetune.py:237); "kept" is Adam.
    set_auto_rates: the multipliers are formed on the device from every step's own gradient (cswin_rate_finalize in the place of
    cswin_norm_finalize, so still three launches and no host sync)."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=None, decoupled=True, moments="kept"):
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0):
            raise ValueError(f"FlatAdamW: betas {betas} must lie in [0, 1)")
        if moments not in ADAM_MOMENTS:
            raise ValueError(f"FlatAdamW: moments must be one of {ADAM_MOMENTS}, got {moments!r}")
        self.decoupled, self.moments = bool(decoupled), moments
        self._auto = None                                                                 # set_auto_rates()'s table and settings
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        super().__init__(params, lr)
        dev, T = self.flat_param.device, len(self.params)
        self._partial = torch.zeros(self.nchunks, 2, dtype=torch.float32, device=dev)
        self.tensor_sumsq = torch.zeros(T, 2, dtype=torch.float32, device=dev)            # (sum g^2, sum p^2) per tensor
        self.scalars = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)          # [total_norm, clip_coef] of the last apply
        self._norms_scalars = torch.zeros(2, dtype=torch.float32, device=dev)             # tensor_norms() leaves `scalars` alone
        self._lr_mult = torch.ones(T, dtype=torch.float32, device=dev)
        self._use_mult = False
        self._eb = None                                                                   # tensor_evidence()'s table and partials, on first use
        self.step_count = 0

    def _alloc_state(self, numel, dev):
        self.flat_m = torch.zeros(numel, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(numel, dtype=torch.float32, device=dev)

    @property
    def grad_norm(self):
        """Device view of the total gradient norm the last apply() clipped by (of flat_grad * grad_scale)."""
        return self.scalars[0:1]

    def set_lr_weights(self, w):
        """Per-tensor learning-rate multipliers aligned with self.params (None: all 1).  A multiplier of exactly 0 freezes the
        tensor bit for bit; its moments still move."""
        if w is None:
            self._use_mult, self._auto = False, None
            return
        w = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
        if w.numel() != len(self.params):
            raise ValueError(f"FlatAdamW.set_lr_weights: {w.numel()} weights for {len(self.params)} parameter tensors")
        self._lr_mult.copy_(w)
        self._use_mult, self._auto = True, None

    def set_auto_rates(self, groups, statistic="grad", default=0.0):
        """Per-step rates (finetune.py:223-236): from now on every apply() gives tensor t the multiplier n_k / max_j n_j of its
        group k, formed on the device from that step's flat_grad * grad_scale.  groups: one entry per tensor of self.params, a group
        id or None; statistic "grad": n_k = the norm of the group's concatenated gradient; "ratio": that over the norm of the
        group's parameters (0 where that is <= 1e-8).  A tensor in no group gets `default`.  None turns the rates off (all
        multipliers 1).  Replaces set_lr_weights' multipliers, as those replace these.  The table is built and uploaded here, once."""
        if groups is None:
            self._use_mult, self._auto = False, None
            return
        first, tensors, group_of, names = group_table(groups, len(self.params), statistic)
        dev = self.flat_param.device
        self._auto = {"groups": list(groups), "statistic": statistic, "default": float(default), "names": names, "n": len(names),
                      "first": torch.from_numpy(first).to(dev), "tensors": torch.from_numpy(tensors).to(dev),
                      "of": torch.from_numpy(group_of).to(dev), "stat": torch.zeros(len(names), dtype=torch.float32, device=dev)}
        self._use_mult = True

    @property
    def group_stats(self):
        """Device (G,) tensor of the groups' statistics of the last apply() under set_auto_rates, the groups in order of first
        appearance (no sync)."""
        if self._auto is None:
            raise RuntimeError("FlatAdamW.group_stats: no auto rates are set (set_auto_rates)")
        return self._auto["stat"]

    @property
    def group_names(self):
        """The group ids set_auto_rates was given, entry k for row k of group_stats."""
        if self._auto is None:
            raise RuntimeError("FlatAdamW.group_names: no auto rates are set (set_auto_rates)")
        return list(self._auto["names"])

    @property
    def lr_weights(self):
        """Device (T,) view of the multipliers the last apply() used (set_lr_weights', or that step's auto rates); None: all 1."""
        return self._lr_mult if self._use_mult else None

    def _sumsq(self, with_params, tensor_sumsq, scalars, grad_scale, max_norm):
        call("cswin_chunk_sumsq", ptr(self.flat_grad), ptr(self.flat_param) if with_params else None, ptr(self.chunks), self.nchunks,
             ptr(self._partial), stream())
        call("cswin_norm_finalize", ptr(self._partial), ptr(self.first_chunk), len(self.params), float(grad_scale), float(max_norm),
             ptr(tensor_sumsq), ptr(scalars), stream())

    def apply(self, grad_scale=1.0):
        """p, m, v <- AdamW(clip(flat_grad * grad_scale)) -- Adam with decoupled=False, from zero moments with moments="fresh",
        at this step's own rates under set_auto_rates."""
        bc1, bc2 = _next_bias_corrections(self, "FlatAdamW.apply()", self.betas)
        clip, auto = self.max_grad_norm is not None, self._auto
        if auto is not None:
            ratio = auto["statistic"] == "ratio"
            call("cswin_chunk_sumsq", ptr(self.flat_grad), ptr(self.flat_param) if ratio else None, ptr(self.chunks), self.nchunks,
                 ptr(self._partial), stream())
            call("cswin_rate_finalize", ptr(self._partial), ptr(self.first_chunk), len(self.params), float(grad_scale),
                 self.max_grad_norm if clip else float("inf"), ptr(auto["first"]), ptr(auto["tensors"]), ptr(auto["of"]), auto["n"],
                 int(ratio), auto["default"], ptr(self.tensor_sumsq), ptr(self.scalars), ptr(auto["stat"]), ptr(self._lr_mult), stream())
        elif clip:
            self._sumsq(False, self.tensor_sumsq, self.scalars, grad_scale, self.max_grad_norm)
        fresh = self.moments == "fresh"
        flags = (0 if self.decoupled else ADAM_COUPLED) | (ADAM_FRESH if fresh else 0)
        if fresh:
            bc1, bc2 = 1.0 - self.betas[0], 1.0 - self.betas[1]                           # every step is a new optimiser's first
        head = (ptr(self.flat_param), ptr(self.flat_grad), None if fresh else ptr(self.flat_m), None if fresh else ptr(self.flat_v),
                ptr(self.chunks), self.nchunks, ptr(self.lr_dev), ptr(self._lr_mult) if self._use_mult else None,
                ptr(self.scalars) if clip else None, *self.betas, self.eps, self.weight_decay, float(grad_scale), bc1, bc2)
        tail = (ptr(self.flat_param16) if precision() == 1 else None, stream())
        if flags:
            call("cswin_adam_flat", *head, flags, *tail)
        else:
            call("cswin_adamw_flat", *head, *tail)

    def tensor_norms(self):
        """(T, 2) device tensor of (||g||, ||p||) per parameter tensor, of flat_grad and flat_param as they are (no sync)."""
        out = torch.empty_like(self.tensor_sumsq)
        self._sumsq(True, out, self._norms_scalars, 1.0, 1.0)
        return out.sqrt_()

    def tensor_evidence(self):
        """(T,) device tensor of the eb-criterion statistic per parameter tensor, mean(g * g / (var(g, dim 0, unbiased) + 1e-8)) of
        flat_grad as it is (universal_train.py:669-672; NaN for a tensor whose first dimension is 1, as torch.var gives): two
        launches of csrc/eb.hip, no sync, no allocation but the result.  The tile table is built and uploaded on first use."""
        if self._eb is None:
            dev = self.flat_grad.device
            rows, first = column_tiles([tuple(p.shape) for p in self.params], self.offsets)
            self._eb = (torch.from_numpy(rows.view(np.int64).reshape(-1, 4)).to(dev), len(rows), torch.from_numpy(first).to(dev),
                        torch.tensor([p.numel() for p in self.params], dtype=torch.int32, device=dev),
                        torch.zeros(len(rows), dtype=torch.float32, device=dev))
        tiles, ntiles, first_tile, numel, partial = self._eb
        out = torch.empty(len(self.params), dtype=torch.float32, device=self.flat_grad.device)
        call("cswin_eb_tiles", ptr(self.flat_grad), ptr(tiles), ntiles, ptr(partial), stream())
        call("cswin_eb_finalize", ptr(partial), ptr(first_tile), ptr(numel), len(self.params), ptr(out), stream())
        return out

    def state_dict(self):
        """The keys "decoupled", "moments" and "auto_rates" are there only when one of them departs from AdamW with kept moments and
        no auto rates: that optimiser's dict is the one it always wrote."""
        auto = self._auto
        sd = {"m": self.flat_m.clone(), "v": self.flat_v.clone(), "step": self.step_count, "lr": self.lr,
              "lr_weights": self._lr_mult.clone() if self._use_mult else None}
        if not self.decoupled or self.moments != "kept" or auto is not None:
            sd.update(decoupled=self.decoupled, moments=self.moments,
                      auto_rates=None if auto is None else {k: auto[k] for k in ("groups", "statistic", "default")})
        return sd

    def load_state_dict(self, sd):
        """A dict without the keys "decoupled", "moments" and "auto_rates" (one written before they existed) loads as it always
        did and leaves the first two as this optimiser was built."""
        moments = sd.get("moments", self.moments)
        if moments not in ADAM_MOMENTS:
            raise ValueError(f"FlatAdamW.load_state_dict: moments must be one of {ADAM_MOMENTS}, got {moments!r}")
        self.flat_m.copy_(sd["m"])
        self.flat_v.copy_(sd["v"])
        self.step_count = int(sd["step"])
        self.set_lr(sd["lr"])
        self.decoupled, self.moments = bool(sd.get("decoupled", self.decoupled)), moments
        self.set_lr_weights(sd["lr_weights"])
        if sd.get("auto_rates") is not None:
            self.set_auto_rates(**sd["auto_rates"])


TPGM_BETAS, TPGM_EPS = (0.9, 0.999), 1e-8       # torch.optim.Adam's defaults, which universal_train.py:552 takes; csrc/tpgm.hip holds the same constants
TPGM_HEAD_WORDS = ("head", "final", "classifier", "output", "segmentation_head")
TPGM_EXCLUDED, TPGM_HEAD = 1, 2                  # the bits of cswin_tpgm_finalize's per-tensor flags


def tpgm_is_head(name):
    """The "final / classification layer" rule of universal_train.py:418 and :471: a wider initial radius and a wider clamp."""
    return any(w in name.lower() for w in TPGM_HEAD_WORDS)


def tpgm_init_gamma(name, param_norm):
    """The initial projection radius of universal_train.py:415-421 from the tensor's own L2 norm."""
    return max(10.0, param_norm * 5.0) if tpgm_is_head(name) else max(3.0, param_norm * 2.0)


class RatioStats(NamedTuple):
    """(min, max, mean) of the projection ratios, the order of the reference's get_ratio_stats (universal_train.py:507-515)."""
    min: float
    max: float
    mean: float


class FlatTPGM:
    """TPGM (universal_train.py:391-615) over the flat buffers of a FlatSGD / FlatAdamW `opt`: every tensor of opt.params is kept
    inside a ball of learned radius gamma_t around its value when this object was built (the anchor).  names: the parameter names,
    aligned with opt.params (they decide the head tensors and match `exclude`).  csrc/tpgm.hip's three kernels do all the work;
    nothing here synchronises with the host except the one read that forms the initial radii and ratio_stats().

        begin()                  save theta, put the projected theta~ into opt.flat_param (and the bf16 shadow)
        update(grad_scale)       opt.flat_grad holds dL/dtheta~: clip_grad_norm_(gamma, 1) + one Adam step on gamma
        reproject()              theta~ of the new gamma, from the saved theta
        end()                    theta and the shadow back, bit for bit
        apply()                  theta <- theta~ (the final projection), in place

    Memory: two more flat buffers (anchor, saved) and a few floats per tensor."""

    def __init__(self, opt, names, norm_mode="l2", proj_lr=0.01, exclude=()):
        names = list(names)
        if len(names) != len(opt.params):
            raise ValueError(f"FlatTPGM: {len(names)} names for {len(opt.params)} parameter tensors")
        unknown = set(exclude) - set(names)
        if unknown:
            raise KeyError(f"FlatTPGM: no trainable parameter named {sorted(unknown)[:4]}")
        self.opt, self.names, self.norm_mode, self.proj_lr = opt, names, str(norm_mode), float(proj_lr)
        self.l1 = 0 if "l2" in self.norm_mode else 1                                     # universal_train.py:463
        dev, T = opt.flat_param.device, len(names)
        self.chunks, self.first_chunk, self.nchunks = opt.chunks, opt.first_chunk, opt.nchunks     # the optimiser's own table
        self._partial = torch.zeros(self.nchunks, 2, dtype=torch.float32, device=dev)
        excl = set(exclude)
        self.flags_host = [(TPGM_EXCLUDED if n in excl else 0) | (TPGM_HEAD if tpgm_is_head(n) else 0) for n in names]
        self._flags = torch.tensor(self.flags_host, dtype=torch.int32, device=dev)
        self.flat_anchor = opt.flat_param.clone()
        self.flat_saved = torch.zeros_like(opt.flat_param)
        self.gamma = torch.zeros(T, dtype=torch.float32, device=dev)
        self.ratio = torch.ones(T, dtype=torch.float32, device=dev)
        self.norm = torch.zeros(T, dtype=torch.float32, device=dev)                      # ||theta - anchor|| of the last launch
        self.gamma_m = torch.zeros(T, dtype=torch.float32, device=dev)
        self.gamma_v = torch.zeros(T, dtype=torch.float32, device=dev)
        self.scalars = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)         # [norm of dL/dgamma, clip coefficient] of the last update
        self.step_count = 0
        self._active, self._ratio_current = False, False
        # the initial radii: ||theta_t|| is the distance to an anchor of zeros, which flat_saved still is
        self._ratios(opt.flat_param, self.flat_saved, l1=0)
        pn = self.norm.cpu().tolist()                                                    # the one host read
        self.gamma.copy_(torch.tensor([tpgm_init_gamma(n, v) for n, v in zip(names, pn)], dtype=torch.float32))
        self.norm.zero_()
        self.ratio.fill_(1.0)

    # -- launches -------------------------------------------------------------------------------------------
    def _stats(self, p, anchor, g, l1=None):
        call("cswin_tpgm_chunk_stats", ptr(p), ptr(anchor), ptr(g), ptr(self.chunks), self.nchunks, self.l1 if l1 is None else l1,
             ptr(self._partial), stream())

    def _finalize(self, mode, grad_scale=1.0, bc1=1.0, bc2=1.0, l1=None):
        call("cswin_tpgm_finalize", ptr(self._partial), ptr(self.first_chunk), len(self.names), self.l1 if l1 is None else l1, ptr(self._flags),
             ptr(self.gamma), ptr(self.gamma_m), ptr(self.gamma_v), float(grad_scale), self.proj_lr, bc1, bc2, mode, ptr(self.ratio),
             ptr(self.norm), ptr(self.scalars), stream())

    def _ratios(self, p, anchor, l1=None):
        self._stats(p, anchor, None, l1)
        self._finalize(0, l1=l1)

    def _project(self, src):
        opt = self.opt
        call("cswin_tpgm_project", ptr(src), ptr(self.flat_anchor), ptr(opt.flat_param), ptr(self.ratio), ptr(self.chunks), self.nchunks,
             ptr(opt.flat_param16) if precision() == 1 else None, stream())

    # -- the projection update ------------------------------------------------------------------------------
    def begin(self):
        """Save theta once, then theta~ -> opt.flat_param (+ the shadow in the bf16 mode)."""
        if self._active:
            raise RuntimeError("FlatTPGM.begin(): already begun (end() restores the parameters)")
        self.flat_saved.copy_(self.opt.flat_param)
        self._active = True
        self._ratio_current = False
        self.reproject()

    def reproject(self):
        """theta~ of the current gamma, from the saved theta (one launch right after update(), three otherwise)."""
        if not self._active:
            raise RuntimeError("FlatTPGM.reproject() outside begin() ... end()")
        if not self._ratio_current:
            self._ratios(self.flat_saved, self.flat_anchor)
            self._ratio_current = True
        self._project(self.flat_saved)

    def update(self, grad_scale=1.0):
        """opt.flat_grad * grad_scale is dL/dtheta~: gamma <- Adam(clip_grad_norm_(dL/dgamma, 1)), against the SAVED theta (two
        launches); self.ratio holds the ratios of the new gamma afterwards."""
        if not self._active:
            raise RuntimeError("FlatTPGM.update() outside begin() ... end()")
        bc1, bc2 = _next_bias_corrections(self, "FlatTPGM.update()", TPGM_BETAS)
        self._stats(self.flat_saved, self.flat_anchor, self.opt.flat_grad)
        self._finalize(1, grad_scale, bc1, bc2)
        self._ratio_current = True

    def end(self):
        """theta and its shadow back, bit for bit."""
        if not self._active:
            return
        self.opt.flat_param.copy_(self.flat_saved)
        if precision() == 1:
            self.opt.refresh_shadow()
        self._active = False

    # -- the projection -------------------------------------------------------------------------------------
    def apply(self):
        """theta <- anchor + ratio (theta - anchor) in place (universal_train.py:613-615); a tensor inside its ball is not stored."""
        if self._active:
            raise RuntimeError("FlatTPGM.apply() between begin() and end(): the parameters hold theta~")
        self._ratios(self.opt.flat_param, self.flat_anchor)
        self._project(self.opt.flat_param)

    def tensor_norms(self):
        """(T,) device tensor of ||theta - anchor|| per tensor (sum |.| in the l1 mode), of opt.flat_param as it is -- of the saved
        theta between begin() and end().  No sync; self.ratio holds the ratios of the current gamma afterwards."""
        self._ratios(self.flat_saved if self._active else self.opt.flat_param, self.flat_anchor)
        self._ratio_current = self._active
        return self.norm.clone()

    def ratio_stats(self):
        """RatioStats (min, max, mean) of the last launch's ratios over the tensors that are not excluded, (0, 0, 0) when there is
        none: get_ratio_stats of universal_train.py:507-515.  One host read."""
        r = [v for v, f in zip(self.ratio.cpu().tolist(), self.flags_host) if not f & TPGM_EXCLUDED]
        return RatioStats(min(r), max(r), sum(r) / len(r)) if r else RatioStats(0.0, 0.0, 0.0)

    def set_constraints(self, gamma):
        """The radii, aligned with names (a sequence or tensor of T floats) or {name: value} for some of them."""
        if isinstance(gamma, dict):
            unknown = set(gamma) - set(self.names)
            if unknown:
                raise KeyError(f"FlatTPGM.set_constraints: no trainable parameter named {sorted(unknown)[:4]}")
            cur = self.gamma.cpu()
            for i, n in enumerate(self.names):
                if n in gamma:
                    cur[i] = float(gamma[n])
            gamma = cur
        gamma = torch.as_tensor(gamma, dtype=torch.float32).reshape(-1)
        if gamma.numel() != len(self.names):
            raise ValueError(f"FlatTPGM.set_constraints: {gamma.numel()} radii for {len(self.names)} parameter tensors")
        self.gamma.copy_(gamma)
        self._ratio_current = False

    def state_dict(self):
        return {"gamma": self.gamma.clone(), "m": self.gamma_m.clone(), "v": self.gamma_v.clone(), "step": self.step_count,
                "anchor": self.flat_anchor.clone(), "norm_mode": self.norm_mode, "proj_lr": self.proj_lr}

    def load_state_dict(self, sd):
        if self._active:
            raise RuntimeError("FlatTPGM.load_state_dict() between begin() and end()")
        self.gamma.copy_(sd["gamma"])
        self.gamma_m.copy_(sd["m"])
        self.gamma_v.copy_(sd["v"])
        self.flat_anchor.copy_(sd["anchor"])
        self.step_count = int(sd["step"])
        self.norm_mode, self.proj_lr = str(sd["norm_mode"]), float(sd["proj_lr"])
        self.l1 = 0 if "l2" in self.norm_mode else 1
        self._ratio_current = False


CONSOLIDATION_METHODS = ("ewc", "mas", "l2sp")
CONSOLIDATION_STATISTIC = {"ewc": 0, "mas": 1}     # cswin_importance_accumulate's `statistic`


def check_consolidation(method, weight, who="FlatConsolidation"):
    """(method, weight) as they are stored; ValueError for an unknown method or a weight that is negative or not finite."""
    if method not in CONSOLIDATION_METHODS:
        raise ValueError(f"{who}: method must be one of {CONSOLIDATION_METHODS}, got {method!r}")
    try:
        weight = float(weight)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: weight must be a finite number >= 0, got {weight!r}") from None
    if not (0.0 <= weight < float("inf")):
        raise ValueError(f"{who}: weight must be a finite number >= 0, got {weight!r}")
    return method, weight


def check_decay(decay, who="FlatConsolidation.finish"):
    decay = float(decay)
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f"{who}: decay must lie in [0, 1], got {decay!r}")
    return decay


class FlatConsolidation:
    """A quadratic penalty that holds every weight of a FlatSGD / FlatAdamW `opt` near its value when this object was built (the
    anchor) in proportion to an importance F >= 0 (csrc/consolidate.hip):

        penalty = (weight / 2) sum_t w_t sum_i F_i (theta_i - anchor_i)^2          gradient: weight w_t F_i (theta_i - anchor_i)

    method "ewc": F is the empirical Fisher, the mean over batches of the squared gradient of the log-likelihood loss (a batch of
    one sample gives the per-sample form; a larger batch the square of the batch-mean gradient); "mas": the mean of |gradient of the
    squared output norm|, which needs no labels; "l2sp": F = 1 and no importance buffer.  names: the parameter names, aligned with
    opt.params; names in `exclude` get w_t = 0 (their gradient keeps its bits).

        penalise(grad_scale)     opt.flat_grad += (weight w_t / grad_scale) F d, before opt.apply(grad_scale): clipping, auto rates
                                 and Adam's moments see it as if it were part of the loss.  Two launches, no host read.
        report()                 the same two launches with no gradient: scalars and per_tensor alone
        set_weight(weight)       an eager fill of the device float the kernels read
        begin_estimate() / accumulate(grad_scale) per batch / finish(count, decay):
                                 F = decay F + (1 / count) sum over the batches of (grad_scale g)^2 or |grad_scale g|; anchor <- theta

    scalars (device): [penalty, sum_t w_t sum F d^2, ||theta - anchor||]; per_tensor (T, 2): (sum F d^2, sum d^2).
    Memory: two more flat buffers (one for "l2sp"), a third between begin_estimate() and finish()."""

    def __init__(self, opt, names, method="ewc", weight=1.0, exclude=()):
        method, weight = check_consolidation(method, weight)
        names = list(names)
        if len(names) != len(opt.params):
            raise ValueError(f"FlatConsolidation: {len(names)} names for {len(opt.params)} parameter tensors")
        unknown = set(exclude) - set(names)
        if unknown:
            raise KeyError(f"FlatConsolidation: no trainable parameter named {sorted(unknown)[:4]}")
        dev = opt.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FlatConsolidation runs on a HIP device only")
        self.opt, self.names, self.method, self.weight, self.exclude = opt, names, method, weight, tuple(exclude)
        T = len(names)
        self.chunks, self.first_chunk, self.nchunks = opt.chunks, opt.first_chunk, opt.nchunks      # the optimiser's own table
        self._partial = torch.zeros(self.nchunks, 2, dtype=torch.float32, device=dev)
        excl = set(exclude)
        self.tensor_weight = torch.tensor([0.0 if n in excl else 1.0 for n in names], dtype=torch.float32, device=dev)
        self.lam_dev = torch.full((1,), weight, dtype=torch.float32, device=dev)
        self.per_tensor = torch.zeros(T, 2, dtype=torch.float32, device=dev)
        self.scalars = torch.zeros(3, dtype=torch.float32, device=dev)
        self.flat_anchor = opt.flat_param.clone()
        self.flat_importance = None if method == "l2sp" else torch.zeros_like(opt.flat_param)
        self._scratch = None

    # -- the penalty ----------------------------------------------------------------------------------------
    def _launch(self, g, penalty_scale):
        call("cswin_consolidate_chunks", ptr(self.opt.flat_param), ptr(self.flat_anchor), ptr(self.flat_importance), ptr(g), ptr(self.chunks),
             self.nchunks, ptr(self.lam_dev), ptr(self.tensor_weight), float(penalty_scale), ptr(self._partial), stream())
        call("cswin_consolidate_finalize", ptr(self._partial), ptr(self.first_chunk), len(self.names), ptr(self.lam_dev),
             ptr(self.tensor_weight), ptr(self.per_tensor), ptr(self.scalars), stream())

    def penalise(self, grad_scale=1.0):
        """opt.flat_grad += (weight w_t / grad_scale) F (theta - anchor); scalars and per_tensor of theta as it is."""
        grad_scale = float(grad_scale)
        if not grad_scale > 0.0:
            raise ValueError(f"FlatConsolidation.penalise: grad_scale must be positive, got {grad_scale!r}")
        self._launch(self.opt.flat_grad, 1.0 / grad_scale)

    def report(self):
        """scalars (a device view, no sync) of theta as it is; the gradient is not touched."""
        self._launch(None, 1.0)
        return self.scalars

    def set_weight(self, weight):
        _, self.weight = check_consolidation(self.method, weight, "FlatConsolidation.set_weight")
        self.lam_dev.fill_(self.weight)

    # -- the estimation -------------------------------------------------------------------------------------
    def _need_importance(self, what):
        if self.flat_importance is None:
            raise ValueError(f'FlatConsolidation.{what}: method "l2sp" has no importance to estimate')

    def begin_estimate(self):
        self._need_importance("begin_estimate")
        self._scratch = torch.zeros_like(self.opt.flat_param)

    def accumulate(self, grad_scale=1.0):
        """scratch += (grad_scale flat_grad)^2 ("ewc") or |grad_scale flat_grad| ("mas") (one launch)."""
        self._need_importance("accumulate")
        if self._scratch is None:
            raise RuntimeError("FlatConsolidation.accumulate() outside begin_estimate() ... finish()")
        call("cswin_importance_accumulate", ptr(self.opt.flat_grad), ptr(self._scratch), ptr(self.chunks), self.nchunks, float(grad_scale),
             CONSOLIDATION_STATISTIC[self.method], stream())

    @property
    def scratch(self):
        """The sum accumulate() has formed so far (data parallelism all-reduces it once before finish()); None outside an estimation."""
        return self._scratch

    def cancel_estimate(self):
        self._scratch = None

    def finish(self, count, decay=0.0):
        """importance = decay importance + scratch / count (one launch); anchor <- theta; the scratch buffer is released."""
        self._need_importance("finish")
        decay = check_decay(decay)
        if self._scratch is None:
            raise RuntimeError("FlatConsolidation.finish() without begin_estimate()")
        if not count > 0:
            raise ValueError(f"FlatConsolidation.finish: count must be positive, got {count!r}")
        call("cswin_flat_axpby", ptr(self.flat_importance), ptr(self._scratch), ptr(self.chunks), self.nchunks, decay, 1.0 / float(count), stream())
        self.flat_anchor.copy_(self.opt.flat_param)
        self._scratch = None

    # -- state ----------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"method": self.method, "weight": self.weight, "exclude": list(self.exclude), "anchor": self.flat_anchor.clone(),
                "importance": None if self.flat_importance is None else self.flat_importance.clone()}

    def load_state_dict(self, sd):
        if sd["method"] != self.method:
            raise ValueError(f"FlatConsolidation.load_state_dict: the state is {sd['method']!r}'s, this object {self.method!r}'s")
        self.flat_anchor.copy_(sd["anchor"])
        if self.flat_importance is not None:
            self.flat_importance.copy_(sd["importance"])
        self.set_weight(sd["weight"])
