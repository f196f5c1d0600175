"""The optimisers of the training loops on flat buffers: SGD(momentum, weight_decay) of the reference's trainer.py:42,60-63
(FlatSGD) and clip_grad_norm_ + AdamW with a learning rate per tensor of its universal_train.py:693-725, 934-939 (FlatAdamW).

All parameters are re-pointed into ONE flat fp32 buffer (32-B aligned slots), the optimiser state and the gradients live in
more of the same layout.  A step is a multi-tensor gather of the per-parameter .grad tensors into the flat gradient buffer (the
buffer RCCL all-reduces, in buckets, under data parallelism) and one fused update kernel -- for AdamW with clipping, two norm
kernels in front of it.  The learning rate lives in device memory so that a captured hipGraph can be replayed under a schedule.
"""
import numpy as np
import torch

from ._lib import call, precision, ptr, register_shadow, stream

_CHUNK = 16384      # floats per gather / update workgroup


class _FlatBuffers:
    """The slot layout, the gradient gather and the bf16 shadow that the flat optimisers share."""

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
    """The static table the AdamW kernels walk: (records, first_chunk).  records: one {'off': int64 element offset into the flat
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


class FlatAdamW(_FlatBuffers):
    """torch.optim.AdamW (decoupled weight decay) on the flat buffers, with torch.nn.utils.clip_grad_norm_(max_grad_norm) fused
    in front of it when max_grad_norm is given and an optional learning-rate multiplier per parameter tensor (set_lr_weights).
    apply() is three launches (two without clipping), no host sync and no allocation; the step count lives on the host, where
    the bias corrections 1 - beta^t are formed in Python floats as torch forms them."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=None):
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0):
            raise ValueError(f"FlatAdamW: betas {betas} must lie in [0, 1)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        super().__init__(params, lr)
        dev, T = self.flat_param.device, len(self.params)
        rows, first = chunk_table([p.numel() for p in self.params], self.offsets)
        self.nchunks = len(rows)
        self._chunks = torch.from_numpy(rows.view(np.int64).reshape(-1, 2)).to(dev)       # built and uploaded once
        self._first_chunk = torch.from_numpy(first).to(dev)
        self._partial = torch.zeros(self.nchunks, 2, dtype=torch.float32, device=dev)
        self.tensor_sumsq = torch.zeros(T, 2, dtype=torch.float32, device=dev)            # (sum g^2, sum p^2) per tensor
        self.scalars = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)          # [total_norm, clip_coef] of the last apply
        self._norms_scalars = torch.zeros(2, dtype=torch.float32, device=dev)             # tensor_norms() leaves `scalars` alone
        self._lr_mult = torch.ones(T, dtype=torch.float32, device=dev)
        self._use_mult = False
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
            self._use_mult = False
            return
        w = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
        if w.numel() != len(self.params):
            raise ValueError(f"FlatAdamW.set_lr_weights: {w.numel()} weights for {len(self.params)} parameter tensors")
        self._lr_mult.copy_(w)
        self._use_mult = True

    def _sumsq(self, with_params, tensor_sumsq, scalars, grad_scale, max_norm):
        call("cswin_chunk_sumsq", ptr(self.flat_grad), ptr(self.flat_param) if with_params else None, ptr(self._chunks), self.nchunks,
             ptr(self._partial), stream())
        call("cswin_norm_finalize", ptr(self._partial), ptr(self._first_chunk), len(self.params), float(grad_scale), float(max_norm),
             ptr(tensor_sumsq), ptr(scalars), stream())

    def apply(self, grad_scale=1.0):
        """p, m, v <- AdamW(clip(flat_grad * grad_scale))."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FlatAdamW.apply() inside a stream capture: the host's step count, and with it the bias corrections, "
                               "would be frozen into the graph")
        self.step_count += 1
        b1, b2 = self.betas
        clip = self.max_grad_norm is not None
        if clip:
            self._sumsq(False, self.tensor_sumsq, self.scalars, grad_scale, self.max_grad_norm)
        call("cswin_adamw_flat", ptr(self.flat_param), ptr(self.flat_grad), ptr(self.flat_m), ptr(self.flat_v), ptr(self._chunks), self.nchunks,
             ptr(self.lr_dev), ptr(self._lr_mult) if self._use_mult else None, ptr(self.scalars) if clip else None, b1, b2, self.eps,
             self.weight_decay, float(grad_scale), 1.0 - b1 ** self.step_count, 1.0 - b2 ** self.step_count,
             ptr(self.flat_param16) if precision() == 1 else None, stream())

    def tensor_norms(self):
        """(T, 2) device tensor of (||g||, ||p||) per parameter tensor, of flat_grad and flat_param as they are (no sync)."""
        out = torch.empty_like(self.tensor_sumsq)
        self._sumsq(True, out, self._norms_scalars, 1.0, 1.0)
        return out.sqrt_()

    def state_dict(self):
        return {"m": self.flat_m.clone(), "v": self.flat_v.clone(), "step": self.step_count, "lr": self.lr,
                "lr_weights": self._lr_mult.clone() if self._use_mult else None}

    def load_state_dict(self, sd):
        self.flat_m.copy_(sd["m"])
        self.flat_v.copy_(sd["v"])
        self.step_count = int(sd["step"])
        self.set_lr(sd["lr"])
        self.set_lr_weights(sd["lr_weights"])
