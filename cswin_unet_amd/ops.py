"""torch.autograd.Function wrappers over the C ABI (include/cswin_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator), the autograd tape and the
current stream.  All arithmetic of the hot path happens in libcswin_hip.so.  Every op raises
CswinHipError on a non-HIP tensor -- there is no CPU / eager fallback.
"""
import ctypes
import math
import types

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import AugmentDesc, ConvImageJob, CswinHipError, ReduceJob, WgradDesc, act_bf16, call, dev_f32, lib, precision, ptr, shadow_ptr, stream

__all__ = ["layer_norm", "linear", "linear_pair", "mlp", "stripe_attention", "cswin_block", "conv_tokens", "patch_embed_conv", "carafe_reassemble",
           "carafe_reassemble_nchw", "conv_weight_images", "head_compose", "tokens_to_nchw", "matmul_nn", "ce_dice_loss", "continual_loss", "dropout", "img2windows", "windows2img",
           "seg_metrics", "connected_components", "filter_components", "COMPONENT_TILE", "resize_slices", "argmax_zoom_back", "augment_batch", "class_counts", "gaussian_blur",
           "view_batch", "tta_argmax_zoom_back", "gaussian_blur_each", "intensity_batch", "signed_distance_maps", "boundary_loss"]


# ------------------------------------------------------------------------------------------------
# slab reductions and gradient placement of a backward pass
# ------------------------------------------------------------------------------------------------
# Every weight / LayerNorm / LePE gradient ends in a small deterministic reduction of partial slabs (cswin_reduce_job).  By
# default an op launches its own (a CSWinBlock: its six to eight in one launch) so that the gradient tensors it returns are
# complete when autograd sees them (accumulation into an existing .grad, hooks).  Inside `engine_backward(opt)` -- the HipEngine
# wraps each of its backward phases in it, and owns what happens to the gradients afterwards -- two things change:
#   * gradients of opt's leaf parameters are WRITTEN IN PLACE into the optimiser's flat gradient buffer (the reduction's output
#     pointer is the parameter's slot), so the pass that packed them afterwards (three launches, 2 x 94 MB per step) has nothing
#     left to copy;
#   * a reduction WAITS -- for a block-tail launch that carries it, or for the exit of the context: one launch per 48 jobs instead
#     of 77 launches of ~7 us per step -- if and only if everything it writes lies inside that flat buffer.  Nothing in the pass
#     reads a slot, and the buffer outlives the pass; any other output (a composed weight's gradient feeds the next backward node,
#     a frozen parameter's is dropped by autograd at once) is reduced before the op returns.
# Both rely on nobody reading opt.flat_grad before the context exits and on .grad being None when the pass starts.
MAX_REDUCE_JOBS = 48
TAIL_RIDER_JOBS = 16


class engine_backward:
    """with engine_backward(opt): ... one backward pass whose parameter gradients go straight to opt.flat_grad and whose slab
    reductions run late, at exit at the latest.  The ops talk to the innermost open pass (`_pass`); outside any, and for
    engine_backward(None), that is a pass without a buffer: every gradient is a fresh tensor and no reduction waits."""

    def __init__(self, opt=None):
        self._flat = opt.flat_grad if opt is not None else None
        self._slots = {p.data_ptr(): (o, p.numel()) for p, o in zip(opt.params, opt.offsets)} if opt is not None else {}
        self._queue = []             # (ReduceJob copy, the tensors it reads), oldest first
        self._given = set()          # offsets of the slots handed out in this pass

    def __enter__(self):
        global _pass
        self._outer, _pass = _pass, self
        return self

    def __exit__(self, *exc):
        global _pass
        _pass = self._outer
        if exc[0] is None:           # an exception drops the queue unlaunched
            self.flush()
        return False

    def grad(self, param_key, shape, device):
        """The tensor a parameter gradient is written to: None for an absent parameter (`param_key` is what _param_keys()
        recorded in forward), the parameter's slot of the flat gradient buffer if it is a leaf parameter of this pass's
        optimiser, a fresh tensor otherwise."""
        if param_key is None:
            return None
        n = math.prod(shape)
        o, numel = self._slots.get(param_key, (0, -1)) if param_key else (0, -1)
        if numel != n:
            return torch.empty(tuple(shape), dtype=torch.float32, device=device)
        if o in self._given:
            raise CswinHipError(f"engine_backward: two ops of one backward pass use the leaf parameter at offset {o} of flat_grad; "
                                f"the first gradient is already placed there and its reduction may still be waiting")
        self._given.add(o)
        return self._flat[o:o + n].view(shape)

    def _in_flat(self, address):
        return self._flat is not None and 0 <= address - self._flat.data_ptr() < 4 * self._flat.numel()

    def reduce(self, jobs, reads):
        """jobs: ReduceJob structs filled by entry points called with `deferred` (one that had nothing to reduce leaves its slot
        zeroed); reads: the workspaces they read.  A job that writes nothing but flat_grad slots joins the queue, the others run
        now, in one launch."""
        now = []
        for j in jobs:
            if j.part and all(self._in_flat(a) for a in (j.out, j.out2) if a):
                self._queue.append((ReduceJob.from_buffer_copy(j), reads))
            elif j.part:
                now.append(j)
        if now:
            _rows_sum((ReduceJob * len(now))(*now))

    def queued_outputs(self):
        """Every address a waiting reduction will write."""
        return [a for j, _ in self._queue for a in (j.out, j.out2) if a]

    def take_pending(self, maxn=TAIL_RIDER_JOBS):
        """Up to `maxn` waiting reductions (oldest first) for a launch that can carry them at the end of its grid
        (cswin_linear_bwd_tail): (pointer to the jobs or None, count, owner).  They leave the queue: the caller holds `owner`
        until that launch is enqueued; what the jobs read is released with it (the allocator reuses it in stream order)."""
        taken, self._queue = self._queue[:maxn], self._queue[maxn:]
        arr = (ReduceJob * len(taken))(*[j for j, _ in taken])
        return (_job_ptr(arr) if taken else None), len(taken), (arr, taken)

    def flush(self):
        while self._queue:
            _rows_sum(self.take_pending(MAX_REDUCE_JOBS)[2][0])


_pass = engine_backward()


def _param_keys(*ts):
    """Per parameter, what engine_backward.grad() places its gradient by: None for an absent one (no gradient), the address of
    a leaf of the autograd graph (a module parameter passed as it is), 0 for anything else -- a view or a function of a
    parameter shares or lacks its address, but its gradient is somebody's input, not final."""
    return tuple(None if t is None else t.data_ptr() if t.is_leaf else 0 for t in ts)


def _job_ptr(jobs, i=0):
    """Pointer to slot i of a ctypes array of ReduceJob."""
    return ctypes.c_void_p(ctypes.addressof(jobs) + i * ctypes.sizeof(ReduceJob))


def _rows_sum(jobs):
    """One reduction launch for a ctypes array of ReduceJob."""
    call("cswin_rows_sum_multi", _job_ptr(jobs), len(jobs), stream())


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16) // 4 + 4, dtype=torch.float32, device=device)


def _reduced(nbytes, device, launch, njobs=1):
    """A launch that leaves partial slabs: launch(workspace pointer, its bytes, pointer to `njobs` job slots) with a workspace
    of its own, then the pass reduces (or queues) what it left."""
    ws, jobs = _ws(nbytes, device), (ReduceJob * njobs)()
    launch(ptr(ws), nbytes, _job_ptr(jobs))
    _pass.reduce(jobs, (ws,))


def _int_array(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _stored16(*ts):
    """Storage bits (io_bf16 / y_bf16 of include/cswin_hip.h) read off the tensors: bit i = the i-th is stored as bf16."""
    return sum(1 << i for i, t in enumerate(ts) if t is not None and t.dtype == torch.bfloat16)


def _rows_per_sample(t):
    """Rows of the (M, C) matrix `t` per entry of a per-sample row_scale (the entry points read it only beside one)."""
    return t.numel() // (t.shape[0] * t.shape[-1])


# ------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------
def _layernorm_fwd(x, gamma, beta, eps, dtype=torch.float32):
    """(y stored as `dtype`, mean, rstd) of LayerNorm over the last dimension."""
    C = x.shape[-1]
    M = x.numel() // C
    y = torch.empty_like(x, dtype=dtype)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    call("cswin_layernorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), M, C, eps, _stored16(y), stream())
    return y, mean, rstd


def _layernorm_bwd(dy, x, mean, rstd, gamma, dx, dg, db, slab=None, *, dres=None, dx16=None):
    """dx = dres + LayerNorm backward of dy; dx16: bf16 tensor that receives the rounded twin of dx.  slab: (workspace pointer,
    bytes, job slot) of a caller that reduces later; by default the launch has its own and is reduced at once."""
    C = x.shape[-1]
    M = x.numel() // C
    if slab is None:
        return _reduced(lib().cswin_layernorm_bwd_workspace(M, C), x.device,
                        lambda *s: _layernorm_bwd(dy, x, mean, rstd, gamma, dx, dg, db, s, dres=dres, dx16=dx16))
    ws, nbytes, job = slab
    call("cswin_layernorm_bwd", ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(dx), ptr(dg), ptr(db), ws, nbytes,
         M, C, job, ptr(dx16), stream())


class _LayerNorm(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x, gamma, beta = dev_f32(x, "layer_norm input"), dev_f32(gamma), dev_f32(beta)
        y, mean, rstd = _layernorm_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.keys = _param_keys(gamma, beta)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        dx = torch.empty_like(x)
        dg, db = (_pass.grad(k, gamma.shape, gamma.device) for k in ctx.keys)
        _layernorm_bwd(dev_f32(dy), x, mean, rstd, gamma, dx, dg, db)
        return dx, dg, db, None


def layer_norm(x, gamma, beta, eps=1e-5):
    return _LayerNorm.apply(x, gamma, beta, eps)


# ------------------------------------------------------------------------------------------------
# Linear (+ fused skip-concat input, residual / DropPath epilogue)
# ------------------------------------------------------------------------------------------------
# bf16 TWINS of fp32 residual-stream gradients (bf16 mode): a block's backward hands the gradient of its input to the next
# backward as fp32 (the residual path needs it) and leaves a rounded copy here for that block's GEMMs.  An entry is consumed
# once and only by the very tensor it was made for (same TensorImpl: the entry keeps the tensor alive, so its address cannot be
# reused); autograd sums fan-outs into new tensors, which then simply have no twin.
_twins = {}


def _twin_put(t, t16):
    _twins[t.data_ptr()] = (t, t16)


def _twin_take(t):
    e = _twins.pop(t.data_ptr(), None)
    return e[1] if e is not None and e[0]._cdata == t._cdata else None


def clear_twins():
    _twins.clear()


def _wsrc(w):
    """(pointer, io_bf16 bits) of a Linear weight for cswin_linear_fwd / _bwd_data: in the bf16 mode with bf16 storage, the bf16
    shadow the optimiser keeps of it (bit 2) when there is one -- same values as the GEMM's own rounding, half the bytes --,
    else the fp32 tensor.  The Linear helpers below take a weight as this pair or as a plain fp32 tensor."""
    if act_bf16() and w.shape[0] % 4 == 0 and w.shape[1] % 4 == 0:
        sp = shadow_ptr(w)
        if sp is not None:
            return sp, 4
    return ptr(w), 0


def _linear_fwd(x, w, b, N, *, dtype=torch.float32, gelu=False, x2=None, residual=None, row_scale=None, order=None):
    """y (..., N) = [x | x2] @ w^T + b as `dtype`;  residual: y = residual + row_scale[sample] * (...);  gelu: (y, GELU(y)).
    order: the sample order of a DropPath branch (drop_path_order): the dropped samples' rows of x are not read."""
    pw, w16 = w if isinstance(w, tuple) else (ptr(w), 0)
    K1 = x.shape[-1]
    K = K1 + (x2.shape[-1] if x2 is not None else 0)
    y = torch.empty(x.shape[:-1] + (N,), dtype=dtype, device=x.device)
    y_act = torch.empty_like(y) if gelu else None
    args = (ptr(x), ptr(x2), K1 if x2 is not None else 0, pw, ptr(b), ptr(y), ptr(y_act), ptr(residual), ptr(row_scale),
            _rows_per_sample(x), x.numel() // K1, N, K, precision(), _stored16(x, y) | w16)
    if order is not None:
        call("cswin_linear_fwd_skip", *args, ptr(order), x.shape[0], stream())
    else:
        call("cswin_linear_fwd", *args, stream())
    return (y, y_act) if gelu else y


def _linear_bwd_data(dy, w, dx, *, dx2=None, gelu_pre=None, row_scale=None, add=None, order=None):
    """[dx | dx2] = add + row_scale[sample] * ((dy @ w) * gelu'(gelu_pre)); also plain c = a @ b for row-major b.
    order: as for _linear_fwd; the dropped samples' rows of dy and gelu_pre are not read, their rows of dx are zeros."""
    pw, w16 = w if isinstance(w, tuple) else (ptr(w), 0)
    N, K1 = dy.shape[-1], dx.shape[-1]
    K = K1 + (dx2.shape[-1] if dx2 is not None else 0)
    args = (ptr(dy), pw, ptr(dx), ptr(dx2), K1 if dx2 is not None else 0, ptr(gelu_pre), ptr(row_scale),
            _rows_per_sample(dy), ptr(add), dy.numel() // N, N, K, precision(), _stored16(dy, dx, None, gelu_pre) | w16)
    if order is not None:
        call("cswin_linear_bwd_data_skip", *args, ptr(order), dy.shape[0], stream())
    else:
        call("cswin_linear_bwd_data", *args, stream())


def _linear_bwd_weight(dy, x, dw, db, slab=None, *, x2=None, row_scale=None):
    """dw = (row_scale * dy)^T @ [x | x2], db = column sums of dy (or None).  slab as for _layernorm_bwd."""
    N, K1 = dy.shape[-1], x.shape[-1]
    K = K1 + (x2.shape[-1] if x2 is not None else 0)
    M = dy.numel() // N
    if slab is None:
        return _reduced(lib().cswin_linear_bwd_weight_workspace(M, N, K), dy.device,
                        lambda *s: _linear_bwd_weight(dy, x, dw, db, s, x2=x2, row_scale=row_scale))
    ws, nbytes, job = slab
    call("cswin_linear_bwd_weight", ptr(dy), ptr(x), ptr(x2), K1 if x2 is not None else 0, ptr(row_scale), _rows_per_sample(dy),
         ptr(dw), ptr(db), ws, nbytes, M, N, K, job, precision(), stream())


MAX_MASK_SAMPLES = 256     # nsamples bound of the *_masked weight-gradient and the *_skip entry points (include/cswin_hip.h)


def drop_path_order(u, keep):
    """DropPath factors and sample orders of one step from its uniform draws u (rows, B) and keep probabilities keep (rows[, 1]):
    (scales (rows, B) = (u < keep) / keep, order (rows, 1 + B) int32 = per row the kept count, the kept samples, the dropped ones)."""
    u, keep = dev_f32(u, "DropPath draws"), dev_f32(keep, "keep probabilities")
    rows, B = u.shape
    assert keep.numel() == rows and B <= MAX_MASK_SAMPLES
    scales = torch.empty_like(u)
    order = torch.empty(rows, 1 + B, dtype=torch.int32, device=u.device)
    call("cswin_drop_path_order", ptr(u), ptr(keep), ptr(scales), ptr(order), rows, B, stream())
    return scales, order


def _fill_wgrad(d, dy, x, row_scale, dw, dbias, workspace, ws_bytes):
    """One WgradDesc of cswin_linear_bwd_weight_batch / _tail.  workspace: device pointer."""
    d.dy, d.x, d.row_scale, d.dw, d.dbias = (t.data_ptr() if t is not None else None for t in (dy, x, row_scale, dw, dbias))
    d.workspace, d.ws_bytes, d.rows_per_sample = workspace, ws_bytes, _rows_per_sample(dy)
    d.N, d.K = dy.shape[-1], x.shape[-1]
    d.M, d.precision, d.io_bf16 = dy.numel() // d.N, precision(), _stored16(dy, x)


def _linear_bwd_weight_batch(wg, jobs, pending=(None, 0)):
    """A WgradDesc array in one launch; jobs receives their reductions, pending = (pointer, count) earlier ones ride along."""
    call("cswin_linear_bwd_weight_batch", ctypes.cast(wg, ctypes.c_void_p), len(wg), _job_ptr(jobs), *pending, stream())


class _Linear(Function):
    @staticmethod
    def forward(ctx, x, w, b, x2, residual, row_scale):
        x, w = dev_f32(x, "linear input"), dev_f32(w, "linear weight")
        b, x2, residual, row_scale = dev_f32(b), dev_f32(x2), dev_f32(residual), dev_f32(row_scale)
        K = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
        assert w.shape[1] == K, f"linear: weight {tuple(w.shape)} vs input features {K}"
        y = _linear_fwd(x, _wsrc(w), b, w.shape[0], x2=x2, residual=residual, row_scale=row_scale)
        ctx.save_for_backward(x, w, x2, row_scale)
        ctx.has_res, ctx.keys = residual is not None, _param_keys(w, b)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w, x2, row_scale = ctx.saved_tensors
        dy = dev_f32(dy)
        need = ctx.needs_input_grad
        dx = dx2 = dw = db = None
        if need[0] or (x2 is not None and need[3]):
            dx = torch.empty_like(x)
            dx2 = torch.empty_like(x2) if x2 is not None else None
            _linear_bwd_data(dy, _wsrc(w), dx, dx2=dx2, row_scale=row_scale)
        if need[1]:
            dw = _pass.grad(ctx.keys[0], w.shape, w.device)
            db = _pass.grad(ctx.keys[1], w.shape[:1], w.device)
            _linear_bwd_weight(dy, x, dw, db, x2=x2, row_scale=row_scale)
        return dx, dw, db, dx2, (dy if ctx.has_res else None), None


def linear(x, w, b=None, x2=None, residual=None, row_scale=None):
    """y = [x | x2] @ w^T + b;  with residual: y = residual + row_scale[sample] * (...)  (DropPath + skip add)."""
    return _Linear.apply(x, w, b, x2, residual, row_scale)


class _LinearPair(Function):
    """Two Linears of the same input (CARAFE: `down` and `out` 1x1 convs of x, cswin_unet.py:240,265).  As two separate
    autograd nodes their input gradients meet in an aten::add over (B, L, C); here the second data-gradient GEMM adds into
    the first one's result in its epilogue."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x, w1, b1, w2, b2 = (dev_f32(t) for t in (x, w1, b1, w2, b2))
        assert w1.shape[1] == w2.shape[1] == x.shape[-1]
        ctx.save_for_backward(x, w1, w2)
        ctx.keys = _param_keys(w1, b1, w2, b2)
        return tuple(_linear_fwd(x, w, b, w.shape[0]) for w, b in ((w1, b1), (w2, b2)))

    @staticmethod
    @once_differentiable
    def backward(ctx, dy1, dy2):
        x, w1, w2 = ctx.saved_tensors
        dy1, dy2 = dev_f32(dy1), dev_f32(dy2)
        K = x.shape[-1]
        M = x.numel() // K
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _linear_bwd_data(dy1, w1, dx)
            _linear_bwd_data(dy2, w2, dx, add=dx)
        grads, keep = [], []
        wg, jobs = (WgradDesc * 2)(), (ReduceJob * 2)()
        for i, (dy, w) in enumerate(((dy1, w1), (dy2, w2))):
            dw = _pass.grad(ctx.keys[2 * i], w.shape, w.device)
            db = _pass.grad(ctx.keys[2 * i + 1], w.shape[:1], w.device)
            nbytes = lib().cswin_linear_bwd_weight_workspace(M, w.shape[0], K)
            keep.append(_ws(nbytes, w.device))
            _fill_wgrad(wg[i], dy, x, None, dw, db, ptr(keep[-1]), nbytes)
            grads += [dw, db]
        _linear_bwd_weight_batch(wg, jobs)
        _pass.reduce(jobs, keep)
        return (dx,) + tuple(grads)


def linear_pair(x, w1, b1, w2, b2):
    """(x @ w1^T + b1, x @ w2^T + b2) with one fused input gradient."""
    return _LinearPair.apply(x, w1, b1, w2, b2)


# Device-resident dropout epoch: every dropout launch adds its value to the seed it was given.  The seed itself comes from the host
# generator when the op is called -- under hipGraph replay that is ONCE, at capture -- so the engine advances this counter by one
# kernel inside the captured step and every replay draws fresh masks (forward and backward of one step see the same value).
_epoch = {}


def dropout_epoch(device):
    t = _epoch.get(device)
    if t is None:
        t = _epoch[device] = torch.zeros(1, dtype=torch.int64, device=device)
    return t


def advance_dropout_epoch(device):
    """epoch += 1 on the current stream (capturable)."""
    dropout_epoch(device).add_(1)


def _draw_seeds(n):
    return tuple(int(v) for v in torch.randint(0, 2 ** 62, (n,)).tolist())      # host RNG: torch.manual_seed controls it


def _dropout(x, y, p, seed, *, residual=None, row_scale=None):
    """y (may be x) = residual + row_scale[sample] * dropout_p(x), mask of (seed + epoch); the backward: the same on dy."""
    call("cswin_dropout", ptr(x), ptr(residual), ptr(row_scale), ptr(y), x.numel(), x.numel() // x.shape[0], float(p), int(seed),
         ptr(dropout_epoch(x.device)), stream())


class _Mlp(Function):
    """fc1 -> GELU(erf) -> drop -> fc2 -> drop (cswin_unet.py:22-28) with the optional residual/DropPath epilogue of :179.
    drop_p = 0 (every reference config): two GEMMs with fused epilogues.  drop_p > 0: the two nn.Dropouts are separate
    launches of cswin_dropout (masks regenerated from their seeds in backward; they commute with the GELU' factor)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual, row_scale, drop_p, seeds):
        x, w1, b1, w2, b2 = (dev_f32(t) for t in (x, w1, b1, w2, b2))
        residual, row_scale = dev_f32(residual), dev_f32(row_scale)
        s1, s2 = _wsrc(w1), _wsrc(w2)
        pre, act = _linear_fwd(x, s1, b1, w1.shape[0], gelu=True)
        if drop_p > 0:
            _dropout(act, act, drop_p, seeds[0])
            y = _linear_fwd(act, s2, b2, w2.shape[0])
            _dropout(y, y, drop_p, seeds[1], residual=residual, row_scale=row_scale)
        else:
            y = _linear_fwd(act, s2, b2, w2.shape[0], residual=residual, row_scale=row_scale)
        ctx.save_for_backward(x, w1, w2, pre, act, row_scale)
        ctx.has_res, ctx.keys = residual is not None, _param_keys(w1, b1, w2, b2)
        ctx.drop = (float(drop_p), seeds)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w1, w2, pre, act, row_scale = ctx.saved_tensors
        dy = dev_f32(dy)
        K = x.shape[-1]
        Hd, N = w1.shape[0], w2.shape[0]
        M = x.numel() // K
        dev = x.device
        drop_p, seeds = ctx.drop
        dyl, rs_gemm = dy, row_scale                 # gradient of fc2's output, and the row factor still to be applied by the GEMMs
        if drop_p > 0:
            dyl = torch.empty_like(dy)
            _dropout(dy, dyl, drop_p, seeds[1], row_scale=row_scale)
            rs_gemm = None
        # d pre = (row_scale * dy @ w2) * gelu'(pre)   (GELU backward fused into the data-gradient epilogue)
        dpre = torch.empty_like(pre)
        _linear_bwd_data(dyl, w2, dpre, gelu_pre=pre, row_scale=rs_gemm)
        if drop_p > 0:
            _dropout(dpre, dpre, drop_p, seeds[0])
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _linear_bwd_data(dpre, w1, dx)
        # both weight gradients
        k1, kb1, k2, kb2 = ctx.keys
        dw2, db2 = _pass.grad(k2, w2.shape, dev), _pass.grad(kb2, (N,), dev)
        nbytes = max(lib().cswin_linear_bwd_weight_workspace(M, N, Hd), lib().cswin_linear_bwd_weight_workspace(M, Hd, K))
        ws, ws1 = _ws(nbytes, dev), _ws(nbytes, dev)
        jobs = (ReduceJob * 2)()
        _linear_bwd_weight(dyl, act, dw2, db2, (ptr(ws), nbytes, _job_ptr(jobs, 0)), row_scale=rs_gemm)
        dw1, db1 = _pass.grad(k1, w1.shape, dev), _pass.grad(kb1, (Hd,), dev)
        _linear_bwd_weight(dpre, x, dw1, db1, (ptr(ws1), nbytes, _job_ptr(jobs, 1)))
        _pass.reduce(jobs, (ws, ws1))
        return dx, dw1, db1, dw2, db2, (dy if ctx.has_res else None), None, None, None


def mlp(x, w1, b1, w2, b2, residual=None, row_scale=None, drop_p=0.0):
    return _Mlp.apply(x, w1, b1, w2, b2, residual, row_scale, float(drop_p), _draw_seeds(2) if drop_p > 0 else (0, 0))


class _MatmulNN(Function):
    """c (M, K) = a (M, N) @ b (N, K) -- used to compose the 1x1 `output` head with upsample1.out."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = dev_f32(a), dev_f32(b)
        c = torch.empty(a.shape[0], b.shape[1], dtype=torch.float32, device=a.device)
        _linear_bwd_data(a, b, c)
        ctx.save_for_backward(a, b)
        return c

    @staticmethod
    @once_differentiable
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = dev_f32(dc)
        da = _linear_fwd(dc, b, None, a.shape[1])       # da = dc @ b^T
        db = torch.empty_like(b)                        # db (N, K) = a^T @ dc
        _linear_bwd_weight(a, dc, db, None)
        return da, db


def matmul_nn(a, b):
    return _MatmulNN.apply(a, b)


# ------------------------------------------------------------------------------------------------
# fused stripe attention
# ------------------------------------------------------------------------------------------------
# `mode` of the attention helpers (qkv_bf16 of include/cswin_hip.h).  The first three say what is STORED as bf16 and follow from
# the tensors' dtypes; the last also selects bf16 matrix instructions, which no dtype tells: so the caller names the mode.
#   ATTN_FP32: every tensor fp32;  ATTN_QKV16: qkv and dqkv stored as bf16;  ATTN_IO16: and the forward outputs y, y0 (arithmetic
#   still fp32);  ATTN_MFMA16: storage of ATTN_IO16, operands rounded to bf16 on their way into bf16 matrix instructions
ATTN_FP32, ATTN_QKV16, ATTN_IO16, ATTN_MFMA16 = 0, 1, 3, 7


def _attn_drop_args(drop, device):
    """(p, seed, epoch pointer) tail of the attention entry points for one _attn_drop() draw."""
    return drop[0], drop[1], ptr(dropout_epoch(device)) if drop[0] > 0 else None


def _attn_fwd(qkv, lw, lb, y, y0, lse, reso, split, idx, heads, scale, drop, mode):
    """y = both branches' softmax(scale q k^T) v + LePE(v);  y0 (or None): the same without LePE, lse: row log-sum-exp."""
    B, _, C3 = qkv.shape
    call("cswin_attn_fwd", ptr(qkv), _ptr_array(lw), _ptr_array(lb), ptr(y), ptr(y0), ptr(lse), B, reso, C3 // 3, len(idx),
         _int_array(heads), _int_array(idx), split, float(scale or 0.0), *_attn_drop_args(drop, qkv.device), mode, stream())


def _attn_bwd(qkv, lw, lb, lse, y0, dy, dqkv, dlw, dlb, reso, split, idx, heads, scale, drop, mode, slab=None):
    """Backward of _attn_fwd.  slab as for _layernorm_bwd (one job per branch)."""
    B, _, C3 = qkv.shape
    ha, ia = _int_array(heads), _int_array(idx)
    if slab is None:
        nbytes = lib().cswin_attn_bwd_workspace(B, reso, C3 // 3, len(idx), ha, ia, split)
        again = lambda *s: _attn_bwd(qkv, lw, lb, lse, y0, dy, dqkv, dlw, dlb, reso, split, idx, heads, scale, drop, mode, s)
        return _reduced(nbytes, qkv.device, again, njobs=2)
    ws, nbytes, jobs = slab
    call("cswin_attn_bwd", ptr(qkv), _ptr_array(lw), _ptr_array(lb), ptr(lse), ptr(y0), ptr(dy), ptr(dqkv), _ptr_array(dlw),
         _ptr_array(dlb), ws, nbytes, B, reso, C3 // 3, len(idx), ha, ia, split, float(scale or 0.0), jobs,
         *_attn_drop_args(drop, qkv.device), mode, stream())


class _StripeAttention(Function):
    @staticmethod
    def forward(ctx, qkv, reso, split, idx, heads, scale, drop, *wb):
        # qkv may arrive STORED as bf16 (the bf16 mode's activation storage): the kernel widens on load, dqkv comes back as bf16
        q16 = qkv.dtype == torch.bfloat16 and qkv.is_cuda
        qkv = qkv.contiguous() if q16 else dev_f32(qkv, "attention qkv")
        nb = len(idx)
        ws_ = [dev_f32(t).view(t.shape[0], 9) for t in wb[:nb]]
        bs_ = [dev_f32(t) for t in wb[nb:]]
        B, L, C3 = qkv.shape
        if L != reso * reso:
            raise ValueError("flatten img_tokens has wrong size")
        y = torch.empty(B, L, C3 // 3, dtype=torch.float32, device=qkv.device)
        y0 = torch.empty_like(y) if any(ctx.needs_input_grad) else None          # P V without LePE: the backward's delta term
        lse = torch.empty(B, sum(heads), L, dtype=torch.float32, device=qkv.device)
        ctx.meta = (reso, split, tuple(idx), tuple(heads), scale, drop, ATTN_QKV16 if q16 else ATTN_FP32)
        _attn_fwd(qkv, ws_, bs_, y, y0, lse, *ctx.meta)
        ctx.save_for_backward(qkv, lse, y0, *ws_, *bs_)
        ctx.keys = _param_keys(*wb)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        qkv, lse, y0, *wb_ = ctx.saved_tensors
        nb = len(wb_) // 2
        ws_, bs_ = wb_[:nb], wb_[nb:]
        dqkv = torch.empty_like(qkv)
        dws = [_pass.grad(k, t.shape, t.device) for k, t in zip(ctx.keys[:nb], ws_)]
        dbs = [_pass.grad(k, t.shape, t.device) for k, t in zip(ctx.keys[nb:], bs_)]
        _attn_bwd(qkv, ws_, bs_, lse, y0, dev_f32(dy), dqkv, dws, dbs, *ctx.meta)
        return (dqkv, None, None, None, None, None, None) + tuple(d.view(d.shape[0], 1, 3, 3) for d in dws) + tuple(dbs)


def _attn_drop(p):
    """(p, seed) of one attention-probability dropout draw (nn.Dropout of cswin_unet.py:57,101); the seed comes from the host
    generator (torch.manual_seed controls it), the backward kernels regenerate the mask from it."""
    p = float(p)
    return (p, _draw_seeds(1)[0]) if p > 0 else (0.0, 0)


def stripe_attention(qkv, reso, split, idx, heads, lepe_w, lepe_b, scale=None, attn_drop=0.0):
    """qkv (B, L, 3C) -> (B, L, C).  idx/heads/lepe_w/lepe_b: one entry per branch.  attn_drop: dropout probability on the
    attention probabilities (training only; the caller passes 0 in eval mode)."""
    return _StripeAttention.apply(qkv, reso, split, tuple(idx), tuple(heads), scale, _attn_drop(attn_drop), *lepe_w, *lepe_b)


# ------------------------------------------------------------------------------------------------
# whole CSWinBlock as ONE autograd node
# ------------------------------------------------------------------------------------------------
class _CSWinBlock(Function):
    """x -> x + dp1(proj(attn(qkv(LN1 x)))) -> ... + dp2(fc2(gelu(fc1(LN2 .))))  (cswin_unet.py:160-181).

    Same launch helpers as the fine-grained ops; as one node the backward chains them by hand, so the two residual-fork
    gradient sums are the `dres` input of the LayerNorm backward kernel (no aten::add), and 14 autograd nodes per
    block become one."""

    @staticmethod
    def forward(ctx, x, reso, split, idx, heads, scale, eps1, eps2, rs1, rs2, orders, drop, g1, b1, wqkv, bqkv, wp, bp, g2, b2, w1, bb1,
                w2, bb2, *lepe):
        x = dev_f32(x, "block input")
        B, L, C = x.shape
        if L != reso * reso:
            raise ValueError("flatten img_tokens has wrong size")
        dev = x.device
        nb = len(idx)
        lw = [dev_f32(t).view(t.shape[0], 9) for t in lepe[:nb]]
        lb = [dev_f32(t) for t in lepe[nb:]]
        rs1, rs2 = dev_f32(rs1), dev_f32(rs2)
        # bf16 mode: every tensor of the block that only GEMMs and the attention kernel read -- both LayerNorm outputs, qkv, the
        # attention output, the MLP hidden pair and (backward) the gradients of qkv and the hidden layer -- is STORED as bf16, and
        # the GEMMs read the weights' bf16 shadow (_wsrc).  The residual stream (x, x1, y), its gradients, the LayerNorm / softmax
        # statistics, master weights and every accumulation stay fp32.
        s16 = act_bf16() and C % 4 == 0
        t16 = torch.bfloat16 if s16 else torch.float32
        E16 = lambda *shape: torch.empty(*shape, dtype=t16, device=dev)
        sq, sp, s1, s2 = (_wsrc(w) if s16 else w for w in (wqkv, wp, w1, w2))
        attn = (reso, split, tuple(idx), tuple(heads), scale, drop, ATTN_MFMA16 if s16 else ATTN_FP32)
        # fp32 with the step's sample orders (drop_path_order): the eight forward / data-gradient Linears leave the dropped samples'
        # rows out.  Their rows of qkv / pre / act then hold the bias's image and of x1 / y the residual: finite, and never used.
        o1 = o2 = None
        if orders is not None and precision() == 0 and B <= MAX_MASK_SAMPLES and C % 4 == 0 and w1.shape[0] % 4 == 0:
            o1, o2 = orders
        ctx.orders = (o1, o2)
        h1, m1, r1 = _layernorm_fwd(x, g1, b1, eps1, t16)
        qkv = _linear_fwd(h1, sq, bqkv, 3 * C, dtype=t16, order=o1)
        att, lse = E16(B, L, C), torch.empty(B, sum(heads), L, dtype=torch.float32, device=dev)
        att0 = E16(B, L, C) if any(ctx.needs_input_grad) else None       # P V without LePE: the attention backward's delta term
        _attn_fwd(qkv, lw, lb, att, att0, lse, *attn)
        x1 = _linear_fwd(att, sp, bp, C, residual=x, row_scale=rs1, order=o1)
        h2, m2, r2 = _layernorm_fwd(x1, g2, b2, eps2, t16)
        pre, act = _linear_fwd(h2, s1, bb1, w1.shape[0], dtype=t16, gelu=True, order=o2)
        y = _linear_fwd(act, s2, bb2, C, residual=x1, row_scale=rs2, order=o2)
        ctx.save_for_backward(x, m1, r1, h1, qkv, lse, att, att0, x1, m2, r2, h2, pre, act, rs1, rs2, g1, wqkv, wp, g2, w1, w2, *lw, *lb)
        ctx.attn = attn
        ctx.keys = _param_keys(g1, b1, wqkv, bqkv, wp, bp, g2, b2, w1, bb1, w2, bb2, *lepe)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x, m1, r1, h1, qkv, lse, att, att0, x1, m2, r2, h2, pre, act, rs1, rs2, g1, wqkv, wp, g2, w1, w2, *lwb) = ctx.saved_tensors
        nb = len(lwb) // 2
        lw, lb = lwb[:nb], lwb[nb:]
        dy = dev_f32(dy)
        o1, o2 = ctx.orders
        B, L, C = x.shape
        M, Hd = B * L, w1.shape[0]
        dev, h = x.device, lib()
        s16 = h1.dtype == torch.bfloat16                  # the storage the forward chose
        # the slab reductions (4 split-K weight gradients, 2 LayerNorm dgamma/dbeta, 1-2 LePE conv gradients) are deferred
        # and run as ONE launch
        wq, lq = h.cswin_linear_bwd_weight_workspace, h.cswin_layernorm_bwd_workspace
        sizes = [wq(M, C, Hd), wq(M, Hd, C), lq(M, C), wq(M, C, C), wq(M, 3 * C, C), lq(M, C)]
        sizes = [(n + 255) // 256 * 256 for n in sizes]
        ws = _ws(sum(sizes), dev)
        wsp = [ctypes.c_void_p(ws.data_ptr() + sum(sizes[:i])) for i in range(6)]
        jobs = (ReduceJob * 8)()
        sq, sp, s1, s2 = (_wsrc(w) if s16 else w for w in (wqkv, wp, w1, w2))
        dy16 = _twin_take(dy) if s16 else None          # rounded copy of dy left by the backward that produced it (see _twins)
        dyg = dy16 if dy16 is not None else dy          # what the GEMMs read
        # ---- MLP branch ----
        dpre = torch.empty_like(pre)
        _linear_bwd_data(dyg, s2, dpre, gelu_pre=pre, row_scale=rs2, order=o2)
        # the four weight gradients are off the critical path: they run as ONE batched launch once all operands exist
        wg = (WgradDesc * 4)()
        kg1, kb1, kwqkv, kbqkv, kwp, kbp, kg2, kb2, kw1, kbb1, kw2, kbb2, *klepe = ctx.keys
        G = lambda key, *shape: _pass.grad(key, shape, dev)
        dw2, db2 = G(kw2, *w2.shape), G(kbb2, C)
        _fill_wgrad(wg[0], dyg, act, rs2, dw2, db2, wsp[0], sizes[0])
        dw1, db1 = G(kw1, *w1.shape), G(kbb1, Hd)
        _fill_wgrad(wg[1], dpre, h2, None, dw1, db1, wsp[1], sizes[1])
        dh2 = torch.empty_like(x)                                      # fp32 (x is)
        _linear_bwd_data(dpre, s1, dh2, order=o2)
        dx1, dg2, dbt2 = torch.empty_like(x), G(kg2, C), G(kb2, C)
        dx1_16 = torch.empty_like(x, dtype=torch.bfloat16) if s16 else None      # the GEMMs below read the twin, the residual path dx1
        _layernorm_bwd(dh2, x1, m2, r2, g2, dx1, dg2, dbt2, (wsp[2], sizes[2], _job_ptr(jobs, 2)), dres=dy, dx16=dx1_16)
        dx1g = dx1_16 if s16 else dx1
        # ---- attention branch ----
        datt = dh2                                                     # reuse
        _linear_bwd_data(dx1g, sp, datt, row_scale=rs1, order=o1)
        dwp, dbp = G(kwp, *wp.shape), G(kbp, C)
        _fill_wgrad(wg[2], dx1g, att, rs1, dwp, dbp, wsp[3], sizes[3])
        dqkv = torch.empty_like(qkv)
        dlw = [G(k, *t.shape) for k, t in zip(klepe[:nb], lw)]
        dlb = [G(k, *t.shape) for k, t in zip(klepe[nb:], lb)]
        reso, split, idx, heads = ctx.attn[:4]
        naw = h.cswin_attn_bwd_workspace(B, reso, C, nb, _int_array(heads), _int_array(idx), split)
        aws = _ws(naw, dev)
        _attn_bwd(qkv, lw, lb, lse, att0, datt, dqkv, dlw, dlb, *ctx.attn, (ptr(aws), naw, _job_ptr(jobs, 6)))
        dwqkv, dbqkv = G(kwqkv, *wqkv.shape), G(kbqkv, 3 * C)
        _fill_wgrad(wg[3], dqkv, h1, None, dwqkv, dbqkv, wsp[4], sizes[4])
        wjobs = (ReduceJob * 4)()
        dh1 = datt                                                     # reuse again
        # the previous blocks' slab reductions ride at the end of this grid; `riders` owns them and what they read until the
        # launch is enqueued (the end of this function)
        pend, npend, riders = _pass.take_pending()
        if precision() == 0:
            # fp32: the qkv data gradient rides in the weight-gradient batch's launch as well (both only wait for dqkv)
            tail = (ptr(dqkv), ptr(wqkv), ptr(dh1), M, 3 * C, C, ctypes.cast(wg, ctypes.c_void_p), 4, _job_ptr(wjobs), pend, npend)
            masks = (rs2, rs2, rs1, rs1) if B <= MAX_MASK_SAMPLES else (None,) * 4
            if any(m is not None for m in masks):
                # DropPath: a sample with rs2 == 0 has zero rows in rs2 . dy and in dpre, one with rs1 == 0 in rs1 . dx1 and in dqkv
                # (the attention backward of datt = 0), so the factors are the sample masks of the weight gradients those feed
                skip = (ctypes.c_void_p * 4)(*[m.data_ptr() if m is not None else None for m in masks])
                if o1 is not None:
                    call("cswin_linear_bwd_tail_skip", *tail, skip, _int_array([B] * 4), ptr(o1), B, stream())
                else:
                    call("cswin_linear_bwd_tail_masked", *tail, skip, _int_array([B] * 4), stream())
            else:
                call("cswin_linear_bwd_tail", *tail, stream())
        else:
            _linear_bwd_weight_batch(wg, wjobs, (pend, npend))
            _linear_bwd_data(dqkv, sq, dh1)
        for slot, ji in enumerate((0, 1, 3, 4)):
            jobs[ji] = wjobs[slot]
        dx, dg1, dbt1 = torch.empty_like(x), G(kg1, C), G(kb1, C)
        dx16 = torch.empty_like(x, dtype=torch.bfloat16) if s16 else None
        _layernorm_bwd(dh1, x, m1, r1, g1, dx, dg1, dbt1, (wsp[5], sizes[5], _job_ptr(jobs, 5)), dres=dx1, dx16=dx16)
        if s16:
            _twin_put(dx, dx16)
        _pass.reduce(jobs, (ws, aws))
        grads = (dx, None, None, None, None, None, None, None, None, None, None, None, dg1, dbt1, dwqkv, dbqkv, dwp, dbp, dg2, dbt2, dw1, db1,
                 dw2, db2)
        return grads + tuple(d.view(d.shape[0], 1, 3, 3) for d in dlw) + tuple(dlb)


def cswin_block(x, reso, split, idx, heads, scale, norm1, qkv, proj, norm2, fc1, fc2, lepe_w, lepe_b, rs1=None, rs2=None, attn_drop=0.0,
                orders=None):
    """Fused CSWinBlock forward/backward.  norm*/qkv/proj/fc*: nn.Modules holding the parameters.  attn_drop: dropout probability
    on the attention probabilities (pass 0 outside training).  orders: None, or the rows of drop_path_order's order that belong to
    (rs1, rs2): the block's Linears then skip the dropped samples' rows (fp32)."""
    return _CSWinBlock.apply(x, reso, split, tuple(idx), tuple(heads), scale, norm1.eps, norm2.eps, rs1, rs2, orders, _attn_drop(attn_drop),
                             norm1.weight, norm1.bias, qkv.weight, qkv.bias, proj.weight, proj.bias, norm2.weight,
                             norm2.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, *lepe_w, *lepe_b)


# ------------------------------------------------------------------------------------------------
# convolutions on tokens
# ------------------------------------------------------------------------------------------------
MAX_CONV_IMAGE_JOBS = 16
_conv_images = {}        # weight address -> (weight, cpad, w_perm, w_permT, w_flipT) of the open conv_weight_images context


def _same_conv(w, stride, pad):
    """A stride-1 "same" convolution: its data gradient is a forward convolution of dy with the mirrored / transposed image."""
    return stride == 1 and 2 * pad == w.shape[2] - 1 and w.shape[0] % 4 == 0


class conv_weight_images:
    """with conv_weight_images(specs): ... -- the implicit-GEMM weight images of every convolution the body will run, written by
    ONE launch on entry instead of one launch per convolution and direction.  specs: (weight, cpad, stride, pad) per convolution
    (weight (Cout, Cin, ks, ks) on the HIP device, cpad >= Cin the channel count of its input tokens).  conv_tokens /
    patch_embed_conv called inside with one of these very weights take its images from here (and keep the backward's in their
    context, as they keep their own); any other weight gets its images the usual way.  The images are fresh tensors of this
    pass: what a backward needs is what its forward saw."""

    def __init__(self, specs):
        self._specs = [sp for sp in specs if sp[0] is not None and sp[0].is_cuda and sp[0].dtype == torch.float32 and sp[0].is_contiguous()]

    def __enter__(self):
        global _conv_images
        self._outer = _conv_images
        images, jobs = {}, []
        grad = torch.is_grad_enabled()
        for w, cpad, stride, pad in self._specs[:MAX_CONV_IMAGE_JOBS]:
            Cout, Cin, ks, _ = w.shape
            E = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=w.device)
            same = _same_conv(w, stride, pad)
            need_dx = grad and cpad == Cin                   # channel-padded input tokens are an image: no input gradient
            wp = E(Cout, ks * ks, cpad)
            wpt = E(ks * ks, Cout, cpad) if need_dx and not same else None
            wf = E(Cin, ks * ks, Cout) if need_dx and same else None
            images[w.data_ptr()] = (w, cpad, wp, wpt, wf)
            jobs.append(ConvImageJob(w.data_ptr(), wp.data_ptr(), wpt.data_ptr() if wpt is not None else None,
                                     wf.data_ptr() if wf is not None else None, Cout, Cin, ks, cpad))
        if jobs:
            arr = (ConvImageJob * len(jobs))(*jobs)
            call("cswin_conv_weight_images", ctypes.cast(arr, ctypes.c_void_p), len(jobs), stream())
        _conv_images = images
        return self

    def __exit__(self, *exc):
        global _conv_images
        _conv_images = self._outer
        return False


def _images_of(w, cpad):
    """(w_perm, w_permT, w_flipT) of the open conv_weight_images context for this very weight, or None."""
    e = _conv_images.get(w.data_ptr())
    if e is not None and e[0].shape == w.shape and e[1] == cpad:
        return e[2:]
    return None


def _permute_w(w, cpad, want_t):
    Cout, Cin, ks, _ = w.shape
    wp = torch.empty(Cout, ks * ks, cpad, dtype=torch.float32, device=w.device)
    wpt = torch.empty(ks * ks, Cout, cpad, dtype=torch.float32, device=w.device) if want_t else None
    call("cswin_conv_weight_permute", ptr(w), ptr(wp), ptr(wpt), Cout, Cin, ks, cpad, stream())
    return wp, wpt


def _conv_tok_fwd(x, w_img, b, y, H, W, ks, stride, pad):
    """y (B, OH*OW, Cout) = convolution of the tokens x (B, H*W, Cin) with the implicit-GEMM weight image w_img, + b."""
    call("cswin_conv_tok_fwd", ptr(x), ptr(w_img), ptr(b), ptr(y), x.shape[0], H, W, x.shape[-1], y.shape[-1], ks, stride, pad,
         precision(), stream())


class _ConvTokens(Function):
    @staticmethod
    def forward(ctx, x, w, b, H, W, stride, pad):
        x, w, b = dev_f32(x, "conv input"), dev_f32(w), dev_f32(b)
        B, L, Cin = x.shape
        assert L == H * W and w.shape[1] == Cin
        Cout, ks = w.shape[0], w.shape[2]
        OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        need_dx = ctx.needs_input_grad[0]
        # stride-1 "same" convolutions take their data gradient as a forward convolution of dy (see backward): no transposed image
        same = _same_conv(w, stride, pad)
        img = _images_of(w, Cin)
        wf = None
        if img is not None and (img[1] is not None or same or not need_dx):
            wp, wpt, wf = img                                # made with every other convolution's at the start of the pass
        else:
            wp, wpt = _permute_w(w, Cin, need_dx and not same)   # both weight images in one launch; the transposed one is kept
        y = torch.empty(B, OH * OW, Cout, dtype=torch.float32, device=x.device)
        _conv_tok_fwd(x, wp, b, y, H, W, ks, stride, pad)
        ctx.save_for_backward(x, w, wpt, wf if need_dx else None)
        ctx.meta = (H, W, stride, pad)
        ctx.keys = _param_keys(w, b)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w, wpt, wf = ctx.saved_tensors
        H, W, stride, pad = ctx.meta
        dy = dev_f32(dy)
        B, L, Cin = x.shape
        Cout, ks = w.shape[0], w.shape[2]
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if _same_conv(w, stride, pad):
                # dx = conv(dy, mirrored / transposed weights): both operands r-contiguous on the forward kernel, instead of
                # the generic transposed gather (CARAFE4 encoder, 16 -> 144 channels at 56 x 56: 13.41 -> 13.36 ms per step)
                if wf is None:
                    wf = torch.empty(Cin, ks * ks, Cout, dtype=torch.float32, device=x.device)
                    call("cswin_conv_weight_flipT", ptr(w), ptr(wf), Cout, Cin, ks, stream())
                _conv_tok_fwd(dy, wf, None, dx, H, W, ks, 1, pad)
            else:
                if wpt is None:
                    _, wpt = _permute_w(w, Cin, True)
                call("cswin_conv_tok_bwd_data", ptr(dy), ptr(wpt), ptr(dx), B, H, W, Cin, Cout, ks, stride, pad, precision(), stream())
        dw = _pass.grad(ctx.keys[0], w.shape, x.device)      # written in the parameter layout by the slab reduction itself
        db = _pass.grad(ctx.keys[1], (Cout,), x.device)
        _reduced(lib().cswin_conv_tok_bwd_weight_workspace(B, H, W, Cin, Cout, ks, stride, pad), x.device,
                 lambda ws, nbytes, job: call("cswin_conv_tok_bwd_weight", ptr(dy), ptr(x), ptr(dw), ptr(db), ws, nbytes, B, H, W, Cin,
                                              Cout, ks, stride, pad, 1, job, precision(), stream()))
        return dx, dw, db, None, None, None, None


def conv_tokens(x, w, b, H, W, stride, pad):
    """nn.Conv2d(w, b, stride, pad) applied to tokens x (B, H*W, Cin) -> (B, OH*OW, Cout)."""
    return _ConvTokens.apply(x, w, b, H, W, stride, pad)


class _PatchEmbedConv(Function):
    """Conv2d(in_chans, E, 7, 4, 2) on an NCHW image -> tokens (cswin_unet.py:339-340); no input gradient."""

    @staticmethod
    def forward(ctx, img, w, b, stride, pad):
        img, w, b = dev_f32(img, "image"), dev_f32(w), dev_f32(b)
        B, Cin, H, W = img.shape
        Cout, ks = w.shape[0], w.shape[2]
        cpad = (Cin + 3) // 4 * 4
        st = stream()
        x = torch.empty(B, H * W, cpad, dtype=torch.float32, device=img.device)
        call("cswin_nchw_to_tokens", ptr(img), ptr(x), B, Cin, H, W, cpad, st)
        images = _images_of(w, cpad)
        wp = images[0] if images is not None else _permute_w(w, cpad, False)[0]
        OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        y = torch.empty(B, OH * OW, Cout, dtype=torch.float32, device=img.device)
        _conv_tok_fwd(x, wp, b, y, H, W, ks, stride, pad)
        ctx.save_for_backward(x, w)
        ctx.meta = (H, W, stride, pad)
        ctx.keys = _param_keys(w, b)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        H, W, stride, pad = ctx.meta
        dy = dev_f32(dy)
        B, cpad = x.shape[0], x.shape[-1]
        Cout, Cin, ks, _ = w.shape
        dw = _pass.grad(ctx.keys[0], w.shape, x.device)
        db = _pass.grad(ctx.keys[1], (Cout,), x.device)
        # channel-padded input (3 -> 4): the slab reduction drops the padded columns as it writes the parameter layout
        _reduced(lib().cswin_conv_tok_bwd_weight_workspace(B, H, W, cpad, Cout, ks, stride, pad), x.device,
                 lambda ws, nbytes, job: call("cswin_conv_tok_bwd_weight_cpad", ptr(dy), ptr(x), ptr(dw), ptr(db), ws, nbytes, B, H, W,
                                              cpad, Cin, Cout, ks, stride, pad, job, precision(), stream()))
        return None, dw, db, None, None


def patch_embed_conv(img, w, b, stride=4, pad=2):
    return _PatchEmbedConv.apply(img, w, b, stride, pad)


# ------------------------------------------------------------------------------------------------
# CARAFE reassembly, layout adapters
# ------------------------------------------------------------------------------------------------
class _CarafeReassemble(Function):
    """C = None: out (B, S*S*L, Cz) tokens.  C: out (B, C, S*H, S*W), the first C channels as planes, written by the reassembly
    kernel and read by its backward -- for the segmentation head, whose C class maps travel in Cz = 16 channel tokens."""

    @staticmethod
    def forward(ctx, e, z, bias, H, W, S, C):
        e, z, bias = dev_f32(e, "carafe kernel logits"), dev_f32(z, "carafe features"), dev_f32(bias)
        B, L, Cz = z.shape
        assert L == H * W and e.shape == (B, L, 9 * S * S) and (C is None or 0 < C <= Cz)
        out = torch.empty((B, L * S * S, Cz) if C is None else (B, C, S * H, S * W), dtype=torch.float32, device=z.device)
        wt = torch.empty_like(e)
        if C is None:
            call("cswin_carafe_fwd", ptr(e), ptr(z), ptr(bias), ptr(out), ptr(wt), B, H, W, Cz, S, stream())
        else:
            call("cswin_carafe_fwd_nchw", ptr(e), ptr(z), ptr(bias), ptr(out), ptr(wt), B, H, W, Cz, C, S, stream())
        ctx.save_for_backward(z, wt)
        ctx.meta = (H, W, S, C)
        ctx.keys = _param_keys(bias)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        z, wt = ctx.saved_tensors
        H, W, S, C = ctx.meta
        dout = dev_f32(dout)
        B, L, Cz = z.shape
        de = torch.empty_like(wt)
        dz = torch.empty_like(z)
        db = _pass.grad(ctx.keys[0], (Cz,), z.device)
        io = (ptr(dout), ptr(z), ptr(wt), ptr(de), ptr(dz), ptr(db))
        if C is None:
            launch = lambda ws, nbytes, job: call("cswin_carafe_bwd", *io, ws, nbytes, B, H, W, Cz, S, job, stream())
        else:
            launch = lambda ws, nbytes, job: call("cswin_carafe_bwd_nchw", *io, ws, nbytes, B, H, W, Cz, C, S, job, stream())
        _reduced(lib().cswin_carafe_bwd_workspace(B, H, W, Cz, S), z.device, launch)       # the bias gradient's partial sums
        return de, dz, db, None, None, None, None


def carafe_reassemble(e, z, bias, H, W, S):
    return _CarafeReassemble.apply(e, z, bias, H, W, S, None)


def carafe_reassemble_nchw(e, z, bias, H, W, S, C):
    """carafe_reassemble(e, z, bias, H, W, S)[..., :C] as (B, C, S*H, S*W).  Where the NCHW backward kernel does not exist (it
    is the fused S = 4, Cz = 16 one) the token form and the layout adapter run instead: same values either way."""
    if lib().cswin_carafe_bwd_nchw_ok(H, W, z.shape[-1], S):
        return _CarafeReassemble.apply(e, z, bias, H, W, S, C)
    return tokens_to_nchw(carafe_reassemble(e, z, bias, H, W, S), C, S * H, S * W)


class _HeadCompose(Function):
    """(W_head W_out, W_head b_out), zero-padded to cpad rows: the weights of `output` (1x1, no bias) applied after CARAFE4's
    `out` (1x1), as ONE small launch, and one more for the three gradients."""

    @staticmethod
    def forward(ctx, w_head, w_out, b_out, cpad):
        w_head, w_out, b_out = dev_f32(w_head, "head weight"), dev_f32(w_out, "out weight"), dev_f32(b_out)
        ncls, E = w_head.shape[0], w_head.numel() // w_head.shape[0]
        C = w_out.numel() // w_out.shape[0]
        assert w_out.shape[0] == E and cpad >= ncls and (b_out is None or b_out.numel() == E)
        wf = torch.empty(cpad, C, dtype=torch.float32, device=w_head.device)
        bf = torch.empty(cpad, dtype=torch.float32, device=w_head.device)
        call("cswin_head_compose", ptr(w_head), ptr(w_out), ptr(b_out), ptr(wf), ptr(bf), ncls, E, C, cpad, stream())
        ctx.save_for_backward(w_head, w_out, b_out)
        ctx.keys = _param_keys(w_head, w_out, b_out)
        return wf, bf

    @staticmethod
    @once_differentiable
    def backward(ctx, dwf, dbf):
        w_head, w_out, b_out = ctx.saved_tensors
        ncls, E = w_head.shape[0], w_head.numel() // w_head.shape[0]
        C = w_out.numel() // w_out.shape[0]
        dev = w_head.device
        dwf = dev_f32(dwf) if dwf is not None else torch.zeros(ncls, C, dtype=torch.float32, device=dev)
        dbf = dev_f32(dbf)
        dwh = _pass.grad(ctx.keys[0], w_head.shape, dev)
        dwo = _pass.grad(ctx.keys[1], w_out.shape, dev)
        dbo = _pass.grad(ctx.keys[2], (E,), dev)
        call("cswin_head_compose_bwd", ptr(w_head), ptr(w_out), ptr(b_out), ptr(dwf), ptr(dbf), ptr(dwh), ptr(dwo), ptr(dbo),
             ncls, E, C, stream())
        return dwh, dwo, dbo, None


def head_compose(w_head, w_out, b_out, cpad):
    """w_head (ncls, E[, 1, 1]), w_out (E, C[, 1, 1]), b_out (E) or None -> (w_fused (cpad, C), b_fused (cpad))."""
    return _HeadCompose.apply(w_head, w_out, b_out, int(cpad))


class _TokensToNchw(Function):
    @staticmethod
    def forward(ctx, x, C, H, W):
        x = dev_f32(x)
        B, L, Cpad = x.shape
        assert L == H * W and C <= Cpad
        y = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
        call("cswin_tokens_to_nchw", ptr(x), ptr(y), B, C, H, W, Cpad, stream())
        ctx.meta = (C, H, W, Cpad)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        C, H, W, Cpad = ctx.meta
        dy = dev_f32(dy)
        B = dy.shape[0]
        dx = torch.empty(B, H * W, Cpad, dtype=torch.float32, device=dy.device)
        call("cswin_nchw_to_tokens", ptr(dy), ptr(dx), B, C, H, W, Cpad, stream())
        return dx, None, None, None


def tokens_to_nchw(x, C, H, W):
    """(B, H*W, Cpad) tokens -> (B, C, H, W) taking the first C channels."""
    return _TokensToNchw.apply(x, C, H, W)


def img2windows(img, H_sp, W_sp):
    """img (B, C, H, W) -> (B*nH*nW, H_sp*W_sp, C)   (cswin_unet.py:184-191); index-only."""
    img = dev_f32(img, "img2windows input")
    B, C, H, W = img.shape
    out = torch.empty(B * (H // H_sp) * (W // W_sp), H_sp * W_sp, C, dtype=torch.float32, device=img.device)
    call("cswin_img2windows", ptr(img), ptr(out), B, C, H, W, H_sp, W_sp, stream())
    return out


def windows2img(img_splits_hw, H_sp, W_sp, H, W):
    """(B', H_sp*W_sp, C) windows -> (B, H, W, C)   (cswin_unet.py:194-202); index-only."""
    x = dev_f32(img_splits_hw, "windows2img input")
    C = x.shape[-1]
    B = int(x.shape[0] / (H * W / H_sp / W_sp))
    out = torch.empty(B, H, W, C, dtype=torch.float32, device=x.device)
    call("cswin_windows2img", ptr(x), ptr(out), B, C, H, W, H_sp, W_sp, stream())
    return out


# ------------------------------------------------------------------------------------------------
# segmentation objectives: CE + Dice (csrc/loss.hip), focal CE + Dice + distillation (csrc/cl_loss.hip) and CE + Dice + boundary
# (csrc/bd_loss.hip, on the signed distance maps of csrc/sdm.hip)
#
# An objective has n_sums(ncls), n_stats, sums() (this rank's partial sums, left in device memory: they add across ranks),
# finalize() (the -- possibly all-reduced -- sums -> stats and the Dice gradient coefficients) and grad() (d loss / d logits).
# _SegLoss drives any of them under autograd, HipEngine (trainer.py) calls the same methods inside its captured graphs.  grad_scales()
# alone forms the gradient scales: gradients are averaged over ranks afterwards, so local means keep the local counts and the
# global Dice gets the world size.
# ------------------------------------------------------------------------------------------------
def _pixels(logits):
    B, ncls = logits.shape[:2]
    return B, ncls, logits.numel() // (B * ncls)


class CeDiceObjective:
    """w_ce * CE + w_dice * Dice (trainer.py:55-57); stats = [loss, ce, dice].  probs: the input holds probabilities
    (DiceLoss(softmax=False)); class_weight: (ncls,) device tensor or None, the Dice weights."""
    n_stats = 3

    def __init__(self, w_ce=0.4, w_dice=0.6, class_weight=None, probs=False):
        self.w_ce, self.w_dice, self.class_weight, self.probs = w_ce, w_dice, class_weight, probs

    @staticmethod
    def n_sums(ncls):
        return 1 + 3 * ncls

    def sums(self, logits, labels, sums, teacher=None):
        B, ncls, HW = _pixels(logits)
        nbytes = lib().cswin_loss_workspace(B, ncls, HW)
        call("cswin_loss_sums", ptr(logits), ptr(labels), ptr(sums), ptr(_ws(nbytes, logits.device)), nbytes, B, ncls, HW, int(self.probs), stream())

    def finalize(self, sums, out, coef, n_pixels, batch):
        call("cswin_loss_finalize", ptr(sums), ptr(out), ptr(coef), float(n_pixels), coef.numel() // 2, self.w_ce, self.w_dice,
             ptr(self.class_weight), stream())

    def grad_scales(self, B, HW, ncls, world):
        """(ce_scale, dice_scale) of cswin_loss_bwd."""
        w_ce, w_dice = self.w_ce, self.w_dice
        return w_ce / float(B * HW), w_dice / ncls * world

    def grad(self, logits, labels, coef, dice_grad_scale, teacher=None, gloss=None):
        B, ncls, HW = _pixels(logits)
        dlogits = torch.empty_like(logits)
        call("cswin_loss_bwd", ptr(logits), ptr(labels), ptr(coef), ptr(gloss), ptr(dlogits), *self.grad_scales(B, HW, ncls, dice_grad_scale),
             B, ncls, HW, int(self.probs), stream())
        return dlogits


class ContinualObjective:
    """(1 - kd_weight) * (w_focal * Focal + w_dice * Dice) + kd_weight * KD (universal_train.py:904-932); stats = [loss, focal,
    dice, kd, ce].  spec: a continual.Distill, or any object with its fields w_focal, w_dice, kd_weight, temperature, focal_gamma,
    focal_alpha, class_weight, label_map; they are read at every call, so a field changed between eager steps takes effect."""
    n_stats = 5

    def __init__(self, spec):
        self.spec = spec

    @staticmethod
    def n_sums(ncls):
        return 3 + 3 * ncls

    def _inputs(self, teacher):
        """((label_map, n_map, teacher, class_weight) as the entry points take them, old_classes)"""
        d = self.spec
        return (ptr(d.label_map), 0 if d.label_map is None else d.label_map.numel(), ptr(teacher), ptr(d.class_weight)), 0 if teacher is None else teacher.shape[1]

    def sums(self, logits, labels, sums, teacher=None):
        d = self.spec
        B, ncls, HW = _pixels(logits)
        nbytes = lib().cswin_cl_loss_workspace(B, ncls, HW)
        tensors, nold = self._inputs(teacher)
        call("cswin_cl_loss_sums", ptr(logits), ptr(labels), *tensors, ptr(sums), ptr(_ws(nbytes, logits.device)), nbytes, B, ncls, nold, HW, d.temperature,
             d.focal_alpha, d.focal_gamma, stream())

    def finalize(self, sums, out, coef, n_pixels, batch):
        """'batchmean' divides the distillation term by images: batch is the image count the sums cover."""
        d = self.spec
        call("cswin_cl_loss_finalize", ptr(sums), ptr(out), ptr(coef), float(n_pixels), float(batch), coef.numel() // 2, d.w_focal, d.w_dice,
             d.kd_weight, d.temperature, stream())

    def grad_scales(self, B, HW, ncls, world):
        """(focal_scale, dice_scale, kd_scale) of cswin_cl_loss_bwd."""
        d = self.spec
        w_focal, w_dice, kd_weight, temperature = d.w_focal, d.w_dice, d.kd_weight, d.temperature
        return (1.0 - kd_weight) * w_focal / float(B * HW), (1.0 - kd_weight) * w_dice / ncls * world, kd_weight * temperature / B

    def grad(self, logits, labels, coef, dice_grad_scale, teacher=None, gloss=None):
        d = self.spec
        B, ncls, HW = _pixels(logits)
        dlogits = torch.empty_like(logits)
        tensors, nold = self._inputs(teacher)
        call("cswin_cl_loss_bwd", ptr(logits), ptr(labels), *tensors, ptr(coef), ptr(gloss), ptr(dlogits), *self.grad_scales(B, HW, ncls, dice_grad_scale),
             B, ncls, nold, HW, d.temperature, d.focal_alpha, d.focal_gamma, stream())
        return dlogits


class _SegLoss(Function):
    @staticmethod
    def forward(ctx, logits, labels, teacher, objective, group):
        logits, teacher = dev_f32(logits, "logits"), dev_f32(teacher, "teacher_logits")
        labels = labels.contiguous()
        if labels.dtype != torch.int64:
            labels = labels.long()
        B, ncls, HW = _pixels(logits)
        sums, out, coef = (torch.empty(n, dtype=torch.float32, device=logits.device) for n in (objective.n_sums(ncls), objective.n_stats, 2 * ncls))
        objective.sums(logits, labels, sums, teacher)
        world = 1
        if group is not None:
            import torch.distributed as dist
            world = dist.get_world_size(group)
            if world > 1:
                dist.all_reduce(sums, group=group)      # a few floats: the reference's global-batch Dice, the global means
        objective.finalize(sums, out, coef, B * HW * world, B * world)
        ctx.save_for_backward(logits, labels, coef, teacher)
        ctx.meta = (objective, world)
        loss = out[0].clone()
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss, _gout):
        logits, labels, coef, teacher = ctx.saved_tensors
        objective, world = ctx.meta
        return objective.grad(logits, labels, coef, world, teacher, dev_f32(gloss.reshape(1))), None, None, None, None


def ce_dice_loss(logits, labels, w_ce=0.4, w_dice=0.6, group=None, inputs_are_probs=False, class_weight=None):
    """0.4*CE + 0.6*Dice (trainer.py:55-57).  Returns (loss, stats) with stats = [loss, ce, dice] (no host sync).
    With a process group the 1+3*ncls Dice/CE sums are all-reduced so Dice is the global-batch Dice.
    inputs_are_probs: the input holds probabilities (DiceLoss(softmax=False)); class_weight: (ncls,) device tensor or None."""
    if inputs_are_probs and w_ce != 0.0:
        raise ValueError("ce_dice_loss: cross entropy needs logits; with inputs_are_probs pass w_ce=0")
    return _SegLoss.apply(logits, labels, None, CeDiceObjective(float(w_ce), float(w_dice), dev_f32(class_weight), bool(inputs_are_probs)), group)


def _int32_map(label_map):
    if label_map is not None and (label_map.dtype != torch.int32 or not label_map.is_cuda or not label_map.is_contiguous()):
        raise CswinHipError(f"label_map must be a contiguous int32 tensor on the HIP device (continual.new_label_map), got {label_map.dtype} on {label_map.device}")
    return label_map


def continual_loss(logits, labels, teacher_logits, *, w_focal=0.2, w_dice=0.8, kd_weight=0.5, temperature=3.0, focal_gamma=4.0,
                   focal_alpha=1.0, class_weight=None, label_map=None, group=None):
    """(1 - kd_weight) * (w_focal * Focal + w_dice * Dice) + kd_weight * KD (universal_train.py:904-932) in one fused pass each way.
    Returns (loss, stats) with stats = [loss, focal, dice, kd, ce] (no host sync).  logits (B, ncls, ...), teacher_logits
    (B, old_classes, ...) of the frozen old model on the same images (no gradient), labels int64; label_map: int32 device table
    applied to the labels first (continual.new_label_map); class_weight: (ncls,) device tensor, the focal loss's `weight`.
    With a process group the 3 + 3*ncls sums are all-reduced: Dice, the focal mean and the per-image KD are the global batch's."""
    logits, teacher, class_weight = dev_f32(logits, "logits"), dev_f32(teacher_logits.detach(), "teacher_logits"), dev_f32(class_weight)
    label_map = _int32_map(label_map)
    B, ncls, HW = _pixels(logits)
    if teacher.shape[0] != B or teacher.numel() != B * teacher.shape[1] * HW:
        raise ValueError(f"continual_loss: teacher logits {tuple(teacher.shape)} do not match logits {tuple(logits.shape)}")
    # the kernels index these by pixel and by class: a mismatch would be an out-of-bounds device read
    if not labels.is_cuda or labels.numel() != B * HW:
        raise ValueError(f"continual_loss: labels {tuple(labels.shape)} on {labels.device} do not match logits {tuple(logits.shape)} on {logits.device}")
    if class_weight is not None and class_weight.numel() != ncls:
        raise ValueError(f"continual_loss: class_weight has {class_weight.numel()} entries for {ncls} classes")
    spec = types.SimpleNamespace(w_focal=float(w_focal), w_dice=float(w_dice), kd_weight=float(kd_weight), temperature=float(temperature),
                                 focal_gamma=float(focal_gamma), focal_alpha=float(focal_alpha), class_weight=class_weight, label_map=label_map)
    return _SegLoss.apply(logits, labels, teacher, ContinualObjective(spec), group)


def signed_distance_maps(labels, ncls):
    """The boundary loss's signed distance maps of a label batch on the device (csrc/sdm.hip): labels (B, H, W) int64 HIP tensor ->
    float32 (B, ncls, H, W), utils.signed_distance_maps_host bit for bit: +distance to the class outside its mask, -(distance to
    the outside - 1) inside, zeros for a class that is absent from a slice or fills it, Euclidean, in pixels, per 2-D slice.
    1 <= H, W <= 2047, 2 <= ncls <= 255.  No host sync; the row pass's workspace (half the bytes of the result) is freed on return."""
    if not labels.is_cuda:
        raise CswinHipError(f"signed_distance_maps labels are on {labels.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
    if labels.dim() != 3:
        raise ValueError(f"signed_distance_maps: labels {tuple(labels.shape)} must be (B, H, W)")
    labels = labels.contiguous()
    if labels.dtype != torch.int64:
        labels = labels.long()
    (B, H, W), ncls = labels.shape, int(ncls)
    nbytes = lib().cswin_sdm_workspace(B, ncls, H, W)
    if nbytes == 0:
        raise ValueError(f"signed_distance_maps: {lib().cswin_last_error().decode()}")
    phi = torch.empty(B, ncls, H, W, dtype=torch.float32, device=labels.device)
    call("cswin_signed_distance_maps", ptr(labels), ptr(phi), ptr(_ws(nbytes, labels.device)), nbytes, B, ncls, H, W, stream())
    return phi


class BoundaryObjective:
    """w_ce * CE + w_dice * Dice + alpha * boundary (Kervadec et al., MIDL 2019), boundary = the mean over pixels of
    sum_c wb_c * softmax_c * phi_c with phi the labels' signed distance maps; stats = [loss, ce, dice, boundary].  CE and Dice are
    CeDiceObjective's (class_weight: the Dice's); boundary_class_weight: (ncls,) device tensor, or None for 0 on class 0 and 1 on
    the rest.  alpha lives in a one-float device tensor that the kernels read, so set_boundary_weight reaches a captured step.
    sums() makes phi from the labels it is given (which must then be (B, H, W)) and keeps it for grad(); dist_maps: a
    (B, ncls, H, W) tensor to use instead, for a caller who caches the maps."""
    n_stats = 4

    def __init__(self, w_ce=0.4, w_dice=0.6, alpha=0.01, class_weight=None, boundary_class_weight=None, dist_maps=None):
        self.w_ce, self.w_dice, self.class_weight, self.boundary_class_weight = w_ce, w_dice, class_weight, boundary_class_weight
        self.alpha, self.alpha_dev, self.dist_maps, self._phi = float(alpha), None, dist_maps, None

    @staticmethod
    def n_sums(ncls):
        return 2 + 3 * ncls

    def set_boundary_weight(self, alpha):
        """An eager fill of the device float (as the optimisers' set_lr): the next step, replayed or not, uses it."""
        self.alpha = float(alpha)
        if self.alpha_dev is not None:
            self.alpha_dev.fill_(self.alpha)

    def _alpha(self, device):
        if self.alpha_dev is None:
            self.alpha_dev = torch.full((1,), self.alpha, dtype=torch.float32, device=device)
        return self.alpha_dev

    def sums(self, logits, labels, sums, teacher=None):
        B, ncls, HW = _pixels(logits)
        if self.dist_maps is not None:
            self._phi = self.dist_maps
        else:
            if labels.dim() != 3:
                raise ValueError(f"BoundaryObjective: labels {tuple(labels.shape)} must be (B, H, W) to form the distance maps")
            self._phi = signed_distance_maps(labels, ncls)
        nbytes = lib().cswin_bd_loss_workspace(B, ncls, HW)
        call("cswin_bd_loss_sums", ptr(logits), ptr(labels), ptr(self._phi), ptr(self.boundary_class_weight), ptr(sums),
             ptr(_ws(nbytes, logits.device)), nbytes, B, ncls, HW, stream())

    def finalize(self, sums, out, coef, n_pixels, batch):
        call("cswin_bd_loss_finalize", ptr(sums), ptr(out), ptr(coef), float(n_pixels), coef.numel() // 2, self.w_ce, self.w_dice,
             ptr(self._alpha(sums.device)), ptr(self.class_weight), stream())

    def grad_scales(self, B, HW, ncls, world):
        """(ce_scale, dice_scale, bd_scale) of cswin_bd_loss_bwd: the boundary mean keeps the local count, as CE does."""
        return self.w_ce / float(B * HW), self.w_dice / ncls * world, 1.0 / float(B * HW)

    def grad(self, logits, labels, coef, dice_grad_scale, teacher=None, gloss=None):
        B, ncls, HW = _pixels(logits)
        dlogits = torch.empty_like(logits)
        call("cswin_bd_loss_bwd", ptr(logits), ptr(labels), ptr(self._phi), ptr(self.boundary_class_weight), ptr(coef),
             ptr(self._alpha(logits.device)), ptr(gloss), ptr(dlogits), *self.grad_scales(B, HW, ncls, dice_grad_scale), B, ncls, HW, stream())
        return dlogits


def boundary_loss(logits, labels, alpha, w_ce=0.4, w_dice=0.6, class_weight=None, boundary_class_weight=None, dist_maps=None, group=None):
    """w_ce * CE + w_dice * Dice + alpha * boundary (Kervadec et al., MIDL 2019) in one fused pass each way.  Returns (loss, stats)
    with stats = [loss, ce, dice, boundary] (no host sync).  logits (B, ncls, H, W), labels (B, H, W) int64 on the device: their
    signed distance maps are made there (signed_distance_maps), or pass dist_maps (B, ncls, H, W) to reuse cached ones.
    class_weight: the Dice's (ncls,) weights; boundary_class_weight: the boundary term's, None = every class but 0.
    With a process group the 2 + 3*ncls sums are all-reduced: Dice and the two means are the global batch's."""
    logits, class_weight, wb, dist_maps = dev_f32(logits, "logits"), dev_f32(class_weight), dev_f32(boundary_class_weight), dev_f32(dist_maps, "dist_maps")
    B, ncls, HW = _pixels(logits)
    # the kernels index these by pixel and by class: a mismatch would be an out-of-bounds device read
    if not labels.is_cuda or labels.numel() != B * HW:
        raise ValueError(f"boundary_loss: labels {tuple(labels.shape)} on {labels.device} do not match logits {tuple(logits.shape)} on {logits.device}")
    if dist_maps is None and (logits.dim() != 4 or tuple(labels.shape) != (B,) + tuple(logits.shape[2:])):
        raise ValueError(f"boundary_loss: labels {tuple(labels.shape)} must be (B, H, W) of logits {tuple(logits.shape)} to form the distance maps")
    if dist_maps is not None and dist_maps.numel() != logits.numel():
        raise ValueError(f"boundary_loss: dist_maps {tuple(dist_maps.shape)} do not match logits {tuple(logits.shape)}")
    for w, what in ((class_weight, "class_weight"), (wb, "boundary_class_weight")):
        if w is not None and w.numel() != ncls:
            raise ValueError(f"boundary_loss: {what} has {w.numel()} entries for {ncls} classes")
    return _SegLoss.apply(logits, labels, None, BoundaryObjective(float(w_ce), float(w_dice), float(alpha), class_weight, wb, dist_maps), group)


# ------------------------------------------------------------------------------------------------
# evaluation metrics of a label volume
# ------------------------------------------------------------------------------------------------
def seg_metrics(pred, label, ncls, ndim=None):
    """Per-class Dice / HD95 ingredients of a prediction / label pair of class ids (csrc/metrics.hip).  pred, label: uint8 HIP
    tensors (D, H, W) or (H, W) with ids < ncls; ndim (default: the tensors' rank) picks the 6- or 4-neighbourhood of the border
    rule.  Returns device tensors (counts int64 [ncls, 4] = |P|, |G|, |P n G|, |dP| + |dG|; hist int32 [ncls, nbins] of squared
    surface distances), no host sync; utils.metrics_from_counts_hist turns them into (dice, hd95) pairs."""
    for t, what in ((pred, "seg_metrics prediction"), (label, "seg_metrics label")):
        if not t.is_cuda:
            raise CswinHipError(f"{what} is on {t.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
        if t.dtype != torch.uint8:
            raise CswinHipError(f"{what} has dtype {t.dtype}; class ids are passed as uint8")
    if pred.shape != label.shape or pred.dim() not in (2, 3):
        raise CswinHipError(f"seg_metrics: prediction {tuple(pred.shape)} and label {tuple(label.shape)} must be equal (D, H, W) or (H, W) shapes")
    ndim = pred.dim() if ndim is None else int(ndim)
    pred, label = pred.contiguous(), label.contiguous()
    D, H, W = (1,) * (3 - pred.dim()) + tuple(pred.shape)
    h = lib()
    nbins, nbytes = h.cswin_seg_metrics_nbins(D, H, W), h.cswin_seg_metrics_workspace(D, H, W, ndim, int(ncls))
    if nbins == 0 or nbytes == 0:
        raise CswinHipError(f"seg_metrics: {h.cswin_last_error().decode()}")
    counts = torch.empty(int(ncls), 4, dtype=torch.int64, device=pred.device)
    hist = torch.empty(int(ncls), nbins, dtype=torch.int32, device=pred.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    call("cswin_seg_metrics", ptr(pred), ptr(label), ptr(counts), ptr(hist), ptr(ws), nbytes, D, H, W, ndim, int(ncls), stream())
    return counts, hist


def voxel_spacing(voxelspacing, ndim):
    """A voxel spacing as a tuple of `ndim` floats in array order, (D, H, W) or (H, W): scipy's `sampling`, medpy's
    `voxelspacing`.  None is unit spacing, a number is that spacing along every axis, a sequence must have `ndim` entries.
    ValueError for a wrong length and for an entry that is not finite and positive."""
    ndim = int(ndim)
    if voxelspacing is None:
        return (1.0,) * ndim
    try:
        sp = (float(voxelspacing),) * ndim if np.ndim(voxelspacing) == 0 else tuple(float(v) for v in voxelspacing)
    except (TypeError, ValueError) as e:
        raise ValueError(f"voxelspacing {voxelspacing!r} is not a number or a sequence of numbers") from e
    if len(sp) != ndim:
        raise ValueError(f"voxelspacing {voxelspacing!r} has {len(sp)} entries for {ndim} dimensions")
    if not all(np.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"voxelspacing {voxelspacing!r}: every entry must be finite and positive")
    return sp


SURFACE_CAP_EXACT = 1 << 20          # list entries (8 MiB) up to which the default cap is the exact worst case
SURFACE_CAP_FRACTION = 8             # beyond: one entry per SURFACE_CAP_FRACTION voxels


def surface_cap(nvox):
    """Default capacity of ops.surface_distances' list for a volume of nvox voxels.  Every voxel can be a border voxel on both
    sides, so 2 nvox entries always suffice; that exact worst case is the default while it stays within SURFACE_CAP_EXACT
    entries.  Larger volumes get nvox / SURFACE_CAP_FRACTION (at least SURFACE_CAP_EXACT): an organ's surface is a small part
    of a volume, and utils.volume_metrics calls again with the exact size if it ever is not."""
    nvox = int(nvox)
    return 2 * nvox if 2 * nvox <= SURFACE_CAP_EXACT else max(SURFACE_CAP_EXACT, nvox // SURFACE_CAP_FRACTION)


def surface_distances(pred, label, ncls, voxelspacing, ndim=None, cap=None):
    """Per-class surface distances of a prediction / label pair under a voxel spacing (csrc/metrics.hip, cswin_surface_dist): the
    ingredients of HD95 and ASSD in physical units.  pred, label, ncls, ndim: as for seg_metrics.  voxelspacing: voxel_spacing's,
    `ndim` entries in array order.  Returns device tensors, no host sync: counts int64 [ncls, 4] (seg_metrics'), nq int64
    [ncls, 2] = the border voxels of the prediction / of the label per class (0 for a class missing on either side) and dist2
    float64 [cap]: squared distances in segments ordered class 1 P->G, class 1 G->P, class 2 P->G, ... at the exclusive prefix
    sums of nq, unordered inside a segment; entries past nq.sum() are uninitialised.  cap: the list's capacity (default
    surface_cap(voxels)); values that do not fit are dropped, which shows as nq.sum() > cap.  utils.volume_metrics sorts the
    segments and finishes on the host."""
    for t, what in ((pred, "surface_distances prediction"), (label, "surface_distances label")):
        if not t.is_cuda:
            raise CswinHipError(f"{what} is on {t.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
        if t.dtype != torch.uint8:
            raise CswinHipError(f"{what} has dtype {t.dtype}; class ids are passed as uint8")
    if pred.shape != label.shape or pred.dim() not in (2, 3):
        raise CswinHipError(f"surface_distances: prediction {tuple(pred.shape)} and label {tuple(label.shape)} must be equal (D, H, W) or (H, W) shapes")
    ndim = pred.dim() if ndim is None else int(ndim)
    if ndim not in (2, 3):
        raise CswinHipError(f"surface_distances: ndim must be 2 or 3, got {ndim}")
    sp = voxel_spacing(voxelspacing, ndim)
    sz, sy, sx = (1.0,) * (3 - ndim) + sp
    pred, label = pred.contiguous(), label.contiguous()
    D, H, W = (1,) * (3 - pred.dim()) + tuple(pred.shape)
    cap = surface_cap(pred.numel()) if cap is None else int(cap)
    if cap < 0:
        raise ValueError(f"surface_distances: cap={cap} is negative")
    h = lib()
    nbytes = h.cswin_surface_dist_workspace(D, H, W, ndim, int(ncls))
    if nbytes == 0:
        raise CswinHipError(f"surface_distances: {h.cswin_last_error().decode()}")
    counts = torch.empty(int(ncls), 4, dtype=torch.int64, device=pred.device)
    nq = torch.empty(int(ncls), 2, dtype=torch.int64, device=pred.device)
    dist2 = torch.empty(max(cap, 1), dtype=torch.float64, device=pred.device)[:cap]
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    call("cswin_surface_dist", ptr(pred), ptr(label), ptr(counts), ptr(nq), ptr(dist2), cap, ptr(ws), nbytes, D, H, W, ndim, int(ncls),
         sz, sy, sx, stream())
    return counts, nq, dist2


# ------------------------------------------------------------------------------------------------
# connected components of a label volume and the per-class size filter
# ------------------------------------------------------------------------------------------------
COMPONENT_TILE = (4, 16, 64)          # (z, y, x) tile of the labelling's tile pass (csrc/components_uf.h: CC_TZ, CC_TY, CC_TX)


def _component_volume(vol, ncls, what):
    if not vol.is_cuda:
        raise CswinHipError(f"{what} volume is on {vol.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
    if vol.dtype != torch.uint8:
        raise CswinHipError(f"{what} volume has dtype {vol.dtype}; class ids are passed as uint8")
    if vol.dim() not in (2, 3):
        raise CswinHipError(f"{what}: volume {tuple(vol.shape)} must be (D, H, W) or (H, W)")
    vol = vol.contiguous()
    D, H, W = (1,) * (3 - vol.dim()) + tuple(vol.shape)
    h = lib()
    nbytes = h.cswin_components_workspace(D, H, W)
    if nbytes == 0:
        raise CswinHipError(f"{what}: {h.cswin_last_error().decode()}")
    return vol, (D, H, W), int(ncls), nbytes


def _label_components(vol, dims, ncls, nbytes, want_sizes):
    labels = torch.empty(vol.shape, dtype=torch.int32, device=vol.device)
    sizes = torch.empty(vol.shape, dtype=torch.int32, device=vol.device) if want_sizes else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
    call("cswin_components_label", ptr(vol), ptr(labels), ptr(sizes), ptr(ws), nbytes, *dims, ncls, stream())
    return labels, sizes, ws


def connected_components(vol, ncls, return_sizes=False):
    """Face-connected components of every foreground class of a label volume (csrc/components.hip): what
    scipy.ndimage.label(vol == c) finds for every c in 1..ncls-1, in one call.  vol: uint8 HIP tensor (D, H, W) or (H, W); ids 0
    and >= ncls are background.  Returns int32 `labels` of vol's shape: 0 for background, else 1 + the smallest flat index of the
    voxel's component (the same bits on every run); with return_sizes also int32 `sizes`: the voxel count of a component at its
    smallest flat index, 0 elsewhere.  ncls in 2..255, each dimension in 1..2048.  No host sync."""
    vol, dims, ncls, nbytes = _component_volume(vol, ncls, "connected_components")
    labels, sizes, _ = _label_components(vol, dims, ncls, nbytes, return_sizes)
    return (labels, sizes) if return_sizes else labels


_rule_tables = {}


def filter_components(vol, ncls, rule, out=None):
    """vol with the small components of each class set to 0 (csrc/components.hip).  rule: "largest", or a mapping
    {class_id: {"min_size": int, "min_fraction": float}} (utils.component_rule_tables; ValueError for a bad one): a component of
    class c stays iff it has at least max(min_size, ceil(min_fraction * largest component of c)) voxels; classes the rule does not
    name, background and ids >= ncls pass through.  vol: uint8 HIP tensor (D, H, W) or (H, W).  out: None (a new tensor), vol
    itself (in place) or another contiguous uint8 tensor of vol's shape.  Returns out.  No host sync once the rule's two small
    tables are on the device (uploaded once per rule and device); utils.filter_components_host is the same rule in scipy."""
    from .utils import component_rule_tables
    ms, mf = component_rule_tables(rule, ncls)
    vol, dims, ncls, nbytes = _component_volume(vol, ncls, "filter_components")
    if out is None:
        out = torch.empty_like(vol)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.shape == vol.shape and out.is_contiguous()):
        raise CswinHipError(f"filter_components: out must be a contiguous uint8 HIP tensor of shape {tuple(vol.shape)}")
    key = (ms.tobytes(), mf.tobytes(), torch.device(vol.device))
    if key not in _rule_tables:
        _rule_tables[key] = (torch.from_numpy(ms.copy()).to(vol.device), torch.from_numpy(mf.copy()).to(vol.device))
    dms, dmf = _rule_tables[key]
    labels, sizes, ws = _label_components(vol, dims, ncls, nbytes, True)
    call("cswin_components_filter", ptr(vol), ptr(labels), ptr(sizes), ptr(dms), ptr(dmf), ptr(out), ptr(ws), nbytes, *dims, ncls, stream())
    return out


# ------------------------------------------------------------------------------------------------
# the resizes around the network in a volume evaluation
# ------------------------------------------------------------------------------------------------
def resize_slices(x, size):
    """scipy.ndimage.zoom(x[d], (h / H, w / W), order=3) of every slice of x (D, H, W), a float32 or float64 HIP tensor, as a
    float32 (D, h, w) tensor; size = (h, w).  The two 1-D operators are scipy's own (utils.zoom_operator, uploaded once per size
    pair and device), the device forms float32(R_h x[d] R_w^T) in float64 (csrc/resize.hip).  Integer dtypes raise ValueError:
    scipy rounds integer outputs, which stays on the host path."""
    if not x.is_cuda:
        raise CswinHipError(f"resize_slices input is on {x.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
    if not x.is_floating_point():
        raise ValueError(f"resize_slices: dtype {x.dtype}; integer volumes are resized on the host (scipy rounds integer outputs)")
    if x.dtype not in (torch.float32, torch.float64):
        raise CswinHipError(f"resize_slices input has dtype {x.dtype}; float32 or float64 is resized")
    if x.dim() != 3:
        raise CswinHipError(f"resize_slices: input {tuple(x.shape)} must be (D, H, W)")
    from .utils import zoom_operator_device
    x = x.contiguous()
    (D, H, W), (h, w) = x.shape, (int(size[0]), int(size[1]))
    wh, sh = zoom_operator_device(H, h, x.device)
    ww, sw = zoom_operator_device(W, w, x.device)
    y = torch.empty((D, h, w), dtype=torch.float32, device=x.device)
    call("cswin_resize_banded", ptr(x), ptr(y), ptr(wh), ptr(sh), wh.shape[1], ptr(ww), ptr(sw), ww.shape[1], D, H, W, h, w,
         int(x.dtype == torch.float64), stream())
    return y


def gaussian_blur(x, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter(x[d], sigma, truncate=truncate) (mode "reflect") of every slice of x (D, H, W), a float32 HIP
    tensor, as a new float32 tensor of the same shape (csrc/blur.hip).  The taps are scipy's own (utils.gaussian_taps, uploaded
    once per sigma and device); the device repeats scipy's float64 sums in scipy's order and rounds to float32 after each axis, as
    scipy does.  A non-contiguous view is copied.  sigma: finite, positive, radius int(truncate * sigma + 0.5) <= 32 (ValueError
    otherwise).  Integer dtypes raise ValueError: scipy rounds integer outputs, which stays on the host path."""
    if not x.is_cuda:
        raise CswinHipError(f"gaussian_blur input is on {x.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
    if not x.is_floating_point():
        raise ValueError(f"gaussian_blur: dtype {x.dtype}; integer slices are blurred on the host (scipy rounds integer outputs)")
    if x.dtype != torch.float32:
        raise CswinHipError(f"gaussian_blur input has dtype {x.dtype}; float32 is blurred")
    if x.dim() != 3:
        raise CswinHipError(f"gaussian_blur: input {tuple(x.shape)} must be (D, H, W)")
    from .utils import gaussian_taps_device
    taps, r = gaussian_taps_device(sigma, truncate, x.device)
    x = x.contiguous()
    D, H, W = x.shape
    y = torch.empty_like(x)
    call("cswin_gaussian_blur", ptr(x), ptr(y), ptr(taps), r, D, H, W, stream())
    return y


def _blur_each_tables(sigmas, truncate=4.0):
    """What cswin_gaussian_blur_each reads for a list of per-slice sigmas (None: the slice is copied): (table int32 (D, 2) of
    (taps offset, radius), taps float64), the taps of each distinct sigma stored once as w[-r] .. w[0] behind the single tap 1.0
    of the None slices.  Host only; ValueError for a sigma utils.gaussian_taps does not take."""
    from .utils import gaussian_taps
    entries, taps, table = {}, [np.ones(1)], np.zeros((len(sigmas), 2), np.int32)
    for d, s in enumerate(sigmas):
        if s is None:
            continue                                                    # (0, 0): radius 0 at the tap 1.0
        if float(s) not in entries:
            w, r = gaussian_taps(s, truncate)
            entries[float(s)] = (sum(len(t) for t in taps), r)
            taps.append(w[:r + 1])
        table[d] = entries[float(s)]
    return table, np.concatenate(taps)


def gaussian_blur_each(x, sigmas, truncate=4.0):
    """gaussian_blur with a sigma of its own for every slice, in one launch: x (D, H, W) float32 HIP tensor, sigmas a sequence of
    D entries, each None or a sigma gaussian_blur takes (ValueError otherwise).  Slice d of the result equals
    gaussian_blur(x[d:d + 1], sigmas[d]) -- scipy's gaussian_filter of that slice -- bit for bit, and x[d] where the entry is None
    (radius 0 with the single tap 1.0).  The slices' taps and the table of (offset, radius) go up in one pinned buffer per call;
    the tile plan is the one of the largest radius."""
    if not x.is_cuda:
        raise CswinHipError(f"gaussian_blur_each input is on {x.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
    if x.dtype != torch.float32:
        raise CswinHipError(f"gaussian_blur_each input has dtype {x.dtype}; float32 is blurred")
    if x.dim() != 3:
        raise CswinHipError(f"gaussian_blur_each: input {tuple(x.shape)} must be (D, H, W)")
    sigmas = list(sigmas)
    if len(sigmas) != x.shape[0]:
        raise ValueError(f"gaussian_blur_each: {len(sigmas)} sigmas for {x.shape[0]} slices")
    D, H, W = x.shape
    table, taps = _blur_each_tables(sigmas, truncate)
    packed = np.concatenate([table.reshape(-1).view(np.float64), taps])              # D int32 pairs, then the float64 taps
    x = x.contiguous()
    buf = _upload(packed.view(np.int64), x.device).view(torch.float64)
    y = torch.empty_like(x)
    call("cswin_gaussian_blur_each", ptr(x), ptr(y), ptr(buf[D:]), len(taps), ptr(buf), int(table[:, 1].max()), D, H, W, stream())
    return y


INTENSITY_DESC = np.dtype([("flags", "<i8"), ("seed", "<u8"), ("noise_std", "<f8"), ("brightness", "<f8"), ("contrast", "<f8"),
                           ("gamma", "<f8")])                                        # cswin_intensity_desc
IN_NOISE, IN_BRIGHTNESS, IN_CONTRAST, IN_GAMMA, IN_INVERT = 1, 2, 4, 8, 16


def _intensity_table(draws):
    """(cswin_intensity_desc records of checked INTENSITY_DRAW records, the `stages` argument that goes with them).  Host only."""
    table = np.zeros(len(draws), INTENSITY_DESC)
    table["flags"] = (IN_NOISE * draws["do_noise"] + IN_BRIGHTNESS * draws["do_brightness"] + IN_CONTRAST * draws["do_contrast"] +
                      IN_GAMMA * draws["do_gamma"] + IN_INVERT * (draws["invert"] & draws["do_gamma"]))
    for f in ("seed", "noise_std", "brightness", "contrast", "gamma"):
        table[f] = draws[f]
    return table, int(np.bitwise_or.reduce(table["flags"], initial=0)) & (IN_CONTRAST | IN_GAMMA)


def intensity_batch(images, draws):
    """utils.intensity_host of every sample of a batch, on the device: images float32 HIP tensor (B, h, w) or (B, 1, h, w), draws
    the HOST array of B datasets.INTENSITY_DRAW records (IntensityAugment.draw).  Returns a new float32 tensor of the same shape.
    The blur stage is gaussian_blur_each (only if a sample blurs), the other four run in float64 in csrc/intensity.hip: one launch
    for noise and brightness, one more if any sample has contrast, three more if any has gamma, a sample's workgroups leaving
    at once the launches that do not concern it.  A sample's result is the same bits on every run and in any batch.  Current
    stream, no synchronisation; the records go up as one pinned table and the workspace is the caching allocator's.  Every check
    (ValueError for the records, CswinHipError for the tensor) comes before the first launch."""
    if not images.is_cuda:
        raise CswinHipError(f"intensity_batch images are on {images.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
    if images.dtype != torch.float32:
        raise CswinHipError(f"intensity_batch images have dtype {images.dtype}; float32 images are augmented")
    if images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[1] != 1) or images.numel() == 0:
        raise CswinHipError(f"intensity_batch: images {tuple(images.shape)} must be (B, h, w) or (B, 1, h, w)")
    from .datasets.dataset_synapse import check_intensity_draws
    B, (h, w) = images.shape[0], images.shape[-2:]
    draws = check_intensity_draws(draws, B)
    table, stages = _intensity_table(draws)
    x = images.contiguous().view(B, h, w)
    if draws["do_blur"].any():
        x = gaussian_blur_each(x, [float(d["sigma"]) if d["do_blur"] else None for d in draws])
    y = torch.empty_like(x)
    nbytes = lib().cswin_intensity_workspace(B, h * w) if stages else 0
    if stages and not nbytes:
        raise CswinHipError(f"cswin_intensity_workspace failed: {lib().cswin_last_error().decode()}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device) if stages else None
    table = _upload(table.view(np.int64), x.device)
    call("cswin_intensity_batch", ptr(x), ptr(y), ptr(table), ptr(ws), nbytes, B, h * w, stages, stream())
    return y.view(images.shape)


_class_tables = {}


def _class_table(classes, ncls, device):
    """Device int32 table of a class list, validated on the host and uploaded once per (list, device)."""
    classes = tuple(classes)
    if not 1 <= len(classes) <= 255:
        raise CswinHipError(f"argmax_zoom_back: classes has {len(classes)} entries; 1..255 are supported (the result is a byte)")
    for k, c in enumerate(classes):
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < ncls:
            raise CswinHipError(f"argmax_zoom_back: classes[{k}] = {c!r} is not a class index in [0, {ncls})")
    key = (tuple(int(c) for c in classes), torch.device(device))
    if key not in _class_tables:
        _class_tables[key] = torch.tensor(key[0], dtype=torch.int32).to(device)
    return _class_tables[key]


def argmax_zoom_back(logits, size, classes=None):
    """scipy.ndimage.zoom(torch.argmax(logits, 1)[b], (H / h, W / w), order=0) of logits (B, ncls, h, w) fp32 as a uint8
    (B, H, W) HIP tensor; size = (H, W), ncls <= 255.  The source index of every output row / column is scipy's own
    (utils.nearest_index); with size == (h, w) it is the plain argmax.
    classes: a sequence of 1..255 class indices in [0, ncls) (CswinHipError otherwise): the argmax is torch.argmax(logits[:, classes],
    1), i.e. the result is the POSITION in the list -- how a continual model is scored on one dataset's own classes.  The list may
    be unordered or repeat a class (the earlier position wins); ncls itself is then not limited."""
    logits = dev_f32(logits, "argmax_zoom_back logits")
    if logits.dim() != 4:
        raise CswinHipError(f"argmax_zoom_back: logits {tuple(logits.shape)} must be (B, ncls, h, w)")
    from .utils import nearest_index_device
    (B, ncls, h, w), (H, W) = logits.shape, (int(size[0]), int(size[1]))
    table = None if classes is None else _class_table(classes, ncls, logits.device)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=logits.device)
    rows, cols = nearest_index_device(h, H, logits.device), nearest_index_device(w, W, logits.device)
    if table is None:
        call("cswin_argmax_zoom_back", ptr(logits), ptr(out), ptr(rows), ptr(cols), B, ncls, h, w, H, W, stream())
    else:
        call("cswin_argmax_zoom_back_classes", ptr(logits), ptr(out), ptr(rows), ptr(cols), ptr(table), table.numel(), B, ncls, h, w,
             H, W, stream())
    return out


# ------------------------------------------------------------------------------------------------
# test-time augmentation: the views before the network, their ensemble after it
# ------------------------------------------------------------------------------------------------
_view_tables = {}


def _view_table(views, what):
    """The int32 table of a tuple of view codes as the entry points read it -- on the host, before they launch (which is how a bad
    code is refused without a kernel) -- made once per tuple.  Whether a code is a view, and whether the shape allows it, is the
    library's decision; here only the count is checked, the table's length being what the library is told."""
    key = tuple(views)
    if not 1 <= len(key) <= 8:
        raise CswinHipError(f"{what}: {len(key)} views; 1..8 are supported")
    for k, c in enumerate(key):                                         # before the look-up: (True,) hashes as (1,)
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not -2 ** 31 <= c < 2 ** 31:
            raise CswinHipError(f"{what}: views[{k}] = {c!r} is not a view code (utils.tta_views makes them)")
    if key not in _view_tables:
        _view_tables[key] = (ctypes.c_int * len(key))(*(int(c) for c in key))
    return _view_tables[key]


def view_batch(x, views):
    """The views of a batch of slices: x (B, h, w) fp32 HIP tensor, views a sequence of 1..8 view codes (utils.tta_views) ->
    (V, B, h', w') fp32, y[v][b] = the numpy expression of utils.apply_view(x[b], views[v]); (h', w') = (h, w), and a transposing
    view (an odd code) needs h == w (CswinHipError otherwise, as for a code outside 0..7).  One launch (csrc/tta.hip); the values
    are copied bit for bit."""
    x = dev_f32(x, "view_batch input")
    if x.dim() != 3:
        raise CswinHipError(f"view_batch: input {tuple(x.shape)} must be (B, h, w)")
    table = _view_table(views, "view_batch")
    B, h, w = x.shape
    y = torch.empty((len(table), B, h, w), dtype=torch.float32, device=x.device)
    call("cswin_view_batch", ptr(x), ptr(y), table, len(table), B, h, w, stream())
    return y


def tta_argmax_zoom_back(logits, views, size, classes=None, return_probs=False):
    """The ensemble of a network's answers to ops.view_batch's views, its argmax and the order-0 zoom back, in one launch
    (csrc/tta.hip).  logits (V * B, ncls, h, w) fp32 as the network returns them for the (V * B, 1, h, w) input view_batch made,
    i.e. (V, B, ...) with slice [v] in the frame of view views[v]; CswinHipError if the batch is no multiple of V.  With
    P[b, k, r, s] = the mean over v of softmax(logits[v, b, classes])[k] at view v's image of (r, s) -- the mean of probabilities,
    float32 -- the result is scipy.ndimage.zoom(torch.argmax(P, 1)[b], (H / h, W / w), order=0) as a uint8 (B, H, W) HIP tensor;
    size = (H, W).  classes: argmax_zoom_back's list, the result being the position in it.  return_probs=True: (out, P) with P
    (B, nsel, h, w) fp32.  Above 16 candidates the kernel keeps its sums in P, which is then allocated either way."""
    logits = dev_f32(logits, "tta_argmax_zoom_back logits")
    if logits.dim() != 4:
        raise CswinHipError(f"tta_argmax_zoom_back: logits {tuple(logits.shape)} must be (V * B, ncls, h, w)")
    table = _view_table(views, "tta_argmax_zoom_back")
    V = len(table)
    if logits.shape[0] % V or logits.shape[0] == 0:
        raise CswinHipError(f"tta_argmax_zoom_back: a batch of {logits.shape[0]} logits is not a positive multiple of the {V} views")
    from .utils import nearest_index_device
    (VB, ncls, h, w), (H, W) = logits.shape, (int(size[0]), int(size[1]))
    B = VB // V
    ctable = None if classes is None else _class_table(classes, ncls, logits.device)
    nsel = ncls if ctable is None else ctable.numel()
    if not 1 <= nsel <= 255:
        raise CswinHipError(f"tta_argmax_zoom_back: {nsel} candidates; 1..255 are supported (the result is a byte)")
    out = torch.empty((B, H, W), dtype=torch.uint8, device=logits.device)
    probs = torch.empty((B, nsel, h, w), dtype=torch.float32, device=logits.device) if return_probs or nsel > 16 else None
    rows, cols = nearest_index_device(h, H, logits.device), nearest_index_device(w, W, logits.device)
    call("cswin_tta_argmax_zoom_back", ptr(logits), ptr(out), ptr(probs), ptr(rows), ptr(cols), table, V, ptr(ctable), nsel, B, ncls, h, w,
         H, W, stream())
    return (out, probs) if return_probs else out


# ------------------------------------------------------------------------------------------------
# label statistics of a continual-learning stage
# ------------------------------------------------------------------------------------------------
def class_counts(labels, ncls, label_map=None):
    """Per-slice class histogram (csrc/label_stats.hip).  labels: uint8 or int64 HIP tensor (N, H, W) or (H, W); label_map: None
    or an int32 HIP tensor (continual.new_label_map: raw id r < len(label_map) has class label_map[r], the convention of
    continual_loss).  Returns the int64 device tensor (N, ncls + 1): column c < ncls counts the elements of a slice with class c,
    the last column those without a class (outside the map, or outside [0, ncls)), so every row sums to H * W.  ncls in 1..256.
    One launch, no host sync, the same bits on every run."""
    if not labels.is_cuda:
        raise CswinHipError(f"class_counts labels are on {labels.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
    if labels.dtype not in (torch.uint8, torch.int64):
        raise CswinHipError(f"class_counts labels have dtype {labels.dtype}; class ids are passed as uint8 or int64")
    if labels.dim() not in (2, 3):
        raise CswinHipError(f"class_counts: labels {tuple(labels.shape)} must be (N, H, W) or (H, W)")
    if label_map is not None and (not label_map.is_cuda or label_map.dtype != torch.int32 or label_map.dim() != 1):
        raise CswinHipError("class_counts: label_map must be a one-dimensional int32 tensor on the HIP device")
    if not 1 <= int(ncls) <= 256:
        raise CswinHipError(f"class_counts: ncls={ncls} outside 1..256")
    labels = labels.contiguous()
    N = labels.shape[0] if labels.dim() == 3 else 1
    counts = torch.empty((N, int(ncls) + 1), dtype=torch.int64, device=labels.device)
    lmap = None if label_map is None else label_map.contiguous()
    call("cswin_class_counts", ptr(labels), labels.element_size(), ptr(lmap), 0 if lmap is None else lmap.numel(), ptr(counts), N,
         labels.shape[-2] * labels.shape[-1], int(ncls), stream())
    return counts


# ------------------------------------------------------------------------------------------------
# training augmentation of a batch of raw slices
# ------------------------------------------------------------------------------------------------
def _augment_table(descs, device):
    """Device copy of a list of (kind, k, axis, src, map tensor or None) as cswin_augment_desc records."""
    table = (AugmentDesc * len(descs))()
    for d, (kind, k, axis, src, amap) in zip(table, descs):
        d.kind, d.k, d.axis, d.src, d.map = kind, k, axis, src, None if amap is None else amap.data_ptr()
    return _upload(np.frombuffer(table, dtype=np.int64), device)           # 24-byte records; int64 keeps the 8-B alignment


def _upload(values, device):
    """int64 host values -> device through pinned memory: an asynchronous copy on the current stream (the caching host allocator
    hands the pinned block out again only after that copy has run)."""
    values = np.asarray(values, dtype=np.int64)
    host = torch.empty(values.shape, dtype=torch.int64, pin_memory=True)
    host.numpy()[...] = values
    return host.to(device, non_blocking=True)


def augment_batch(images, labels, params, size, blur_sigma=None):
    """datasets.RandomGenerator's arithmetic for a whole batch of raw slices, on the device (csrc/augment.hip, csrc/resize.hip).
    images: float32 HIP tensor (B, H, W); labels: uint8 HIP tensor (B, H, W); params: integer HOST tensor (B, 4) of
    (kind, k, axis, angle) per sample as datasets.RawSliceParams draws them (kind 0: nothing, 1: np.flip(np.rot90(x, k), axis),
    2: ndimage.rotate(x, angle, order=0, reshape=False)); size = (h, w).  Returns (image float32 (B, 1, h, w), label int64
    (B, h, w)): the transformed image through scipy's cubic zoom (resize_slices; skipped when the transformed shape is `size`
    already), the transformed label through its order-0 zoom.  Square slices take one gather, one resize and one label launch;
    for non-square ones the samples that keep the shape and those a quarter turn transposes are gathered and resized as two
    groups.  Runs on the current stream and does not synchronise it in the steady state: the parameters are read on the host,
    which is where they are, and the per-batch tables go up through pinned memory.  The FIRST use of a table is the exception:
    each (H, W, angle) rotation map is one scipy.ndimage.rotate on the host (~10 ms at 512 x 512) and a blocking upload from
    pageable memory, up to 40 times per shape over a run, and the nearest / zoom tables of a size pair likewise, once.  They
    are uploaded blocking on purpose: the copies are cached per device and later read from whichever stream calls, so a
    copy that were still in flight on the first caller's stream would race with a second stream's kernels.
    blur_sigma: None, or the sigma of scipy.ndimage.gaussian_filter applied to the raw images first (gaussian_blur: one more
    launch), as the reference blurs the stored slices that RandomGenerator then transforms; labels are untouched."""
    for t, what, dtype, why in ((images, "augment_batch images", torch.float32, "raw slices are float32 (other dtypes: augment=\"host\")"),
                                (labels, "augment_batch labels", torch.uint8, "class ids are passed as uint8")):
        if not t.is_cuda:
            raise CswinHipError(f"{what} is on {t.device}: the cswin_unet_amd ops run on a HIP device only (no CPU fallback)")
        if t.dtype != dtype:
            raise CswinHipError(f"{what} has dtype {t.dtype}; {why}")
    if images.dim() != 3 or images.shape != labels.shape:
        raise CswinHipError(f"augment_batch: images {tuple(images.shape)} and labels {tuple(labels.shape)} must be equal (B, H, W) shapes")
    if params.is_cuda or params.is_floating_point() or tuple(params.shape) != (images.shape[0], 4):
        raise CswinHipError(f"augment_batch: params must be an integer host tensor ({images.shape[0]}, 4), got {params.dtype} "
                            f"{tuple(params.shape)} on {params.device}")
    from .datasets.dataset_synapse import AUG_NONE, AUG_ROT90_FLIP, AUG_ROTATE
    from .utils import nearest_index_device, rotation_index_device
    images, labels, dev = images.contiguous(), labels.contiguous(), images.device
    if blur_sigma is not None:
        images = gaussian_blur(images, blur_sigma)
    (B, H, W), (h, w) = images.shape, (int(size[0]), int(size[1]))
    descs, swapped = [], []
    for b, (kind, k, axis, angle) in enumerate(params.tolist()):
        if kind not in (AUG_NONE, AUG_ROT90_FLIP, AUG_ROTATE) or not (0 <= k <= 3 and 0 <= axis <= 1):
            raise ValueError(f"augment_batch: sample {b} has parameters (kind, k, axis, angle) = {(kind, k, axis, angle)}")
        descs.append((kind, k, axis, b, rotation_index_device(H, W, angle, dev) if kind == AUG_ROTATE else None))
        swapped.append(kind == AUG_ROT90_FLIP and k % 2 == 1 and H != W)
    groups = [([b for b in range(B) if not swapped[b]], (H, W)), ([b for b in range(B) if swapped[b]], (W, H))]
    groups = [g for g in groups if g[0]]
    # one table: the B samples in order (the label launch, and the only image group of square slices), then the image groups
    rows = descs + ([descs[b] for idx, _ in groups for b in idx] if len(groups) > 1 else [])
    table = _augment_table(rows, dev)
    image, first = None, B if len(groups) > 1 else 0
    for idx, (Ho, Wo) in groups:
        y = torch.empty((len(idx), Ho, Wo), dtype=torch.float32, device=dev)
        call("cswin_augment_gather", ptr(images), ptr(y), ptr(table[3 * first:]), len(idx), B, H, W, Ho, Wo, stream())
        if (Ho, Wo) != (h, w):
            y = resize_slices(y, (h, w))
        if len(groups) == 1:
            image = y
        else:                                                           # the group's results go to its samples' rows
            image = torch.empty((B, h, w), dtype=torch.float32, device=dev) if image is None else image
            image.index_copy_(0, _upload(idx, dev), y)
        first += len(idx)
    label = torch.empty((B, h, w), dtype=torch.int64, device=dev)
    keep = (nearest_index_device(H, h, dev), nearest_index_device(W, w, dev))
    swap = (nearest_index_device(W, h, dev), nearest_index_device(H, w, dev)) if any(swapped) else keep
    call("cswin_augment_labels", ptr(labels), ptr(label), ptr(table), ptr(keep[0]), ptr(keep[1]), ptr(swap[0]), ptr(swap[1]), B, B, H, W,
         h, w, stream())
    return image.unsqueeze(1), label


# ------------------------------------------------------------------------------------------------
# dropout (+ residual add and DropPath factor)
# ------------------------------------------------------------------------------------------------
class _Dropout(Function):
    @staticmethod
    def forward(ctx, x, residual, row_scale, p, seed):
        x, residual, row_scale = dev_f32(x, "dropout input"), dev_f32(residual), dev_f32(row_scale)
        y = torch.empty_like(x)
        _dropout(x, y, p, seed, residual=residual, row_scale=row_scale)
        ctx.save_for_backward(row_scale)
        ctx.meta = (p, seed, residual is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (row_scale,) = ctx.saved_tensors
        p, seed, has_res = ctx.meta
        dy = dev_f32(dy)
        dx = torch.empty_like(dy)
        _dropout(dy, dx, p, seed, row_scale=row_scale)
        return dx, (dy if has_res else None), None, None, None


def dropout(x, p, residual=None, row_scale=None, seed=None):
    """residual + row_scale[sample] * dropout_p(x)  (nn.Dropout followed by the block's residual add, cswin_unet.py:27,135,178-179).
    The keep mask is a counter-based hash of (seed, element index); backward regenerates it."""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())        # host RNG (torch.manual_seed controls it); not capturable
    return _Dropout.apply(x, residual, row_scale, p, seed)
