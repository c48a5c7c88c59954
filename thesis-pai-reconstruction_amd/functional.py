"""torch.autograd bridges: PyTorch supplies the tape, libpai_hip.so supplies every number.

Each Function's forward/backward is a fixed sequence of C-ABI launches on the current
stream; nothing here synchronises with the host.
"""
from __future__ import annotations

import math

import torch

from . import ops


# --------------------------------------------------------------------------------------
# networks
# --------------------------------------------------------------------------------------
class _SlotRef:
    """Ownership of one activation slot of an engine between a forward and its backward.  The slot goes back to the
    engine's pool exactly once: after the (single) backward pass, or when the autograd context is dropped without
    one (a grad-enabled forward that is never backpropagated must not leak a full set of activations)."""

    def __init__(self, engine, slot):
        self.engine, self.slot = engine, slot

    def take(self):
        """The slot for the backward pass; a second backward through the same graph (retain_graph) is refused --
        the activations of the slot are overwritten in place by the first one."""
        if self.slot is None:
            raise ops.PaiError("second backward through the same forward: the engine's activation slot has already "
                               "been consumed (retain_graph is not supported)")
        slot, self.slot = self.slot, None
        return slot

    def __del__(self):
        if self.slot is not None:
            try:
                self.engine.release(self.slot)
            except Exception:      # interpreter shutdown
                pass
            self.slot = None


class UnetFunction(torch.autograd.Function):
    """Generator forward/backward through UnetEngine.  Parameter gradients are written into
    the engine's gradient arena and attached as ``p.grad`` directly (autograd receives None
    for them), so that data-parallel buckets can be reduced in place while the backward runs."""

    @staticmethod
    def forward(ctx, x, engine, training, bn_updates, dtype, *params):
        pred, slot = engine.forward(x, training, bn_updates, dtype)
        keep = any(ctx.needs_input_grad)
        if ctx.needs_input_grad[0]:
            raise ops.PaiError("gradient w.r.t. the generator input is not supported")
        if keep:
            ctx.engine, ctx.ref, ctx.params = engine, _SlotRef(engine, slot), params
        else:
            engine.release(slot)
        return pred

    @staticmethod
    def backward(ctx, gpred):
        engine, slot, params = ctx.engine, ctx.ref.take(), ctx.params
        arena = engine.arena()
        if getattr(engine, "overwrites_weight_grads", False):
            fresh = arena.begin_backward(params, overwrite_weights=True)
            engine.backward(slot, gpred, fresh)
        else:       # engines that ADD every gradient (attention U-Net): the whole arena is cleared
            arena.begin_backward(params)
            engine.backward(slot, gpred)
        arena.attach(params)
        engine.release(slot)
        return (None,) * (5 + len(params))


class DiscFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, engine, dtype, *params):
        logits, slot = engine.forward(x, y, dtype)
        if ctx.needs_input_grad[0]:
            raise ops.PaiError("gradient w.r.t. the conditioning image is not supported")
        if any(ctx.needs_input_grad):
            ctx.engine, ctx.ref, ctx.params = engine, _SlotRef(engine, slot), params
            ctx.need_dy = ctx.needs_input_grad[1]
            ctx.need_params = any(ctx.needs_input_grad[4:])
        else:
            engine.release(slot)
        return logits

    @staticmethod
    def backward(ctx, glogits):
        engine, slot, params = ctx.engine, ctx.ref.take(), ctx.params
        fresh = False
        if ctx.need_params:
            arena = engine.arena()
            fresh = arena.begin_backward(params, overwrite_weights=True)
        gy = engine.backward(slot, glogits, ctx.need_params, ctx.need_dy, fresh)
        if ctx.need_params:
            arena.attach(params)
        engine.release(slot)
        return (None, gy, None, None) + (None,) * len(params)


class DiscPairsFunction(torch.autograd.Function):
    """D(x, y_real) and D(x, y_fake) as ONE batch of 2N (the PatchGAN has no cross-sample coupling): returns the
    2N logits, real half first.  Only parameter gradients flow (the discriminator phase of the GAN step, reference
    models/wrapper.py:124-138: the generator output is detached there)."""

    @staticmethod
    def forward(ctx, x, y_real, y_fake, engine, dtype, *params):
        logits, slot = engine.forward(x, y_real, dtype, y2=y_fake)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise ops.PaiError("DiscPairsFunction carries no gradient to its image inputs; detach them")
        if any(ctx.needs_input_grad[5:]):
            ctx.engine, ctx.ref, ctx.params = engine, _SlotRef(engine, slot), params
        else:
            engine.release(slot)
        return logits

    @staticmethod
    def backward(ctx, glogits):
        engine, slot, params = ctx.engine, ctx.ref.take(), ctx.params
        arena = engine.arena()
        fresh = arena.begin_backward(params, overwrite_weights=True)
        engine.backward(slot, glogits, True, False, fresh)
        arena.attach(params)
        engine.release(slot)
        return (None,) * (5 + len(params))


class DiscPairsLossFunction(torch.autograd.Function):
    """``gan_discriminator_loss_pairs(DiscPairsFunction(x, y_real, y_fake), N)`` as ONE node (the discriminator phase of the
    GAN step, reference models/wrapper.py:124-138 with the loss of :68-95): on a head ``pai_head_loss`` takes, the logits, both
    BCE terms, the logit gradient and the head's input gradient are one launch in the forward pass, and a backward pass seeded
    with the cached unit scalar starts at the head's weight gradient.  Any other seed scales the fp32 logit gradient and runs
    the head's input gradient as a launch of its own; any other head (fp32 storage, a bias, an image beyond the kernel's LDS,
    ``PAI_HEAD_FUSED=0``) runs the launches of the two separate nodes.  Only parameter gradients flow."""

    @staticmethod
    def forward(ctx, x, y_real, y_fake, engine, dtype, *params):
        _check_f32_cuda(x, y_real, y_fake)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise ops.PaiError("DiscPairsLossFunction carries no gradient to its image inputs; detach them")
        need = any(ctx.needs_input_grad[5:])
        n = x.shape[0]
        ent = _ACC.get(x.device, "gan_d")
        out = torch.empty((), dtype=torch.float32, device=x.device)
        slot = engine.forward_loss(x, y_real, dtype, y_fake, n, 1.0, 0.0, ent[0], need) if engine.head_fused_ok(dtype) else None
        ctx.fused = slot is not None
        grad = None
        if slot is None:
            logits, slot = engine.forward(x, y_real, dtype, y2=y_fake)
            flat = logits.view(-1)
            k = (flat.numel() // logits.shape[0]) * n
            grad = torch.empty_like(flat) if need else None
            ops.bce_logits(flat[:k], 1.0, 1.0, ent[0], 1.0, grad[:k] if need else None)
            ops.bce_logits(flat[k:], 0.0, 1.0, ent[0], 1.0, grad[k:] if need else None)
        ops.scalar_take(ent[0], out)
        _ACC.taken(ent)
        if need:
            ctx.engine, ctx.ref, ctx.params = engine, _SlotRef(engine, slot), params
            if grad is not None:
                ctx.save_for_backward(grad)
        else:
            engine.release(slot)
        return out

    @staticmethod
    def backward(ctx, gout):
        engine, slot, params = ctx.engine, ctx.ref.take(), ctx.params
        arena = engine.arena()
        fresh = arena.begin_backward(params, overwrite_weights=True)
        if ctx.fused and _is_unit(gout):
            engine.backward(slot, None, True, False, fresh, head_done=True)
        else:
            grad = slot["grads"]["dl32"] if ctx.fused else ctx.saved_tensors[0]
            engine.backward(slot, _scaled(grad, gout).view(slot["logits"].shape), True, False, fresh)
        arena.attach(params)
        engine.release(slot)
        return (None,) * (5 + len(params))


class DiscGenLossFunction(torch.autograd.Function):
    """The generator's GAN loss in one node: ``BCE(D(x, pred), 1) + l1_weight * L1(pred, target)`` (reference
    models/wrapper.py:44-50).  ``pred`` feeds both terms; as two autograd nodes their gradients meet in an aten ``add``
    that torch launches itself -- the one kernel of the GAN step outside the C ABI, which a launch plan (plan.py) cannot
    contain.  Here the backward pass runs the discriminator's input gradient and adds the L1 term with ``pai_add_act``.
    Gradients flow to ``pred`` and, when they require them, to the discriminator's parameters."""

    @staticmethod
    def forward(ctx, x, pred, target, engine, dtype, l1_weight, *params):
        _check_f32_cuda(x, pred, target)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
            raise ops.PaiError("gradient w.r.t. the conditioning image / the target is not supported")
        pc, tc = pred.contiguous().float(), target.contiguous().float()
        need_pred, need_params = ctx.needs_input_grad[1], any(ctx.needs_input_grad[6:])
        need = need_pred or need_params
        gp = torch.empty_like(pc) if need_pred else None
        ent = _ACC.get(pc.device, "gan_g")
        # the head, BCE(logits, 1), its gradient and the head's input gradient as one launch where pai_head_loss takes the head
        slot = engine.forward_loss(x, pred, dtype, None, x.shape[0], 1.0, 1.0, ent[0], need) if engine.head_fused_ok(dtype) else None
        ctx.fused = slot is not None
        gl = None
        if slot is None:
            logits, slot = engine.forward(x, pred, dtype)
            gl = torch.empty_like(logits) if need else None
            ops.bce_logits(logits, 1.0, 1.0, ent[0], 1.0, gl)
        ops.l1(pc, tc, float(l1_weight), ent[0], float(l1_weight), gp)
        out = torch.empty((), dtype=torch.float32, device=pc.device)
        ops.scalar_take(ent[0], out)
        _ACC.taken(ent)
        if need:
            ctx.engine, ctx.ref, ctx.params = engine, _SlotRef(engine, slot), params
            ctx.need_pred, ctx.need_params = need_pred, need_params
            ctx.save_for_backward(*[g for g in (gl, gp) if g is not None])
        else:
            engine.release(slot)
        return out

    @staticmethod
    def backward(ctx, gout):
        engine, slot, params = ctx.engine, ctx.ref.take(), ctx.params
        saved = list(ctx.saved_tensors)
        unit = _is_unit(gout)
        head_done = ctx.fused and unit
        if head_done:
            gl = None
        elif ctx.fused:
            gl = _scaled(slot["grads"]["dl32"], gout).view(slot["logits"].shape)
        else:
            gl = _scaled(saved.pop(0), gout)
        fresh = False
        if ctx.need_params:
            arena = engine.arena()
            fresh = arena.begin_backward(params, overwrite_weights=True)
        # the unit seed: the L1 gradient is added in the store of the discriminator's input gradient where the engine can
        addend = saved[0] if ctx.need_pred and unit and engine.fused_enabled() else None
        gy = engine.backward(slot, gl, ctx.need_params, ctx.need_pred, fresh, head_done=head_done, addend=addend)
        if ctx.need_params:
            arena.attach(params)
        engine.release(slot)
        if ctx.need_pred and addend is None:
            gp = _scaled(saved.pop(0), gout)
            if gy.is_contiguous() and gy.numel() % 8 == 0:
                ops.add_act(torch.float32, gy, gp, ops.ACT_NONE, gy)
            else:
                gy = gy + gp
        return (None, gy, None, None, None, None) + (None,) * len(params)


# --------------------------------------------------------------------------------------
# losses
# --------------------------------------------------------------------------------------
def _check_f32_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise ops.PaiError("pai losses/metrics need HIP device tensors (no CPU fallback exists)")


class _MeanLoss(torch.autograd.Function):
    """loss = mean-reduced {bce-with-logits vs a constant target, l1, mse}; the gradient is
    produced by the same kernel pass and scaled by grad_out in backward."""

    @staticmethod
    def forward(ctx, kind, x, target):
        _check_f32_cuda(x)
        xc = x.contiguous().float()
        acc = torch.zeros((), dtype=torch.float64, device=x.device)
        need = ctx.needs_input_grad[1]
        grad = torch.empty_like(xc) if need else None
        if kind == "bce":
            ops.bce_logits(xc, float(target), 1.0, acc, 1.0, grad)
        else:
            tc = target.contiguous().float()
            (ops.l1 if kind == "l1" else ops.mse)(xc, tc, 1.0, acc, 1.0, grad)
        if need:
            ctx.save_for_backward(grad)
        return acc.float()

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return None, _scaled(grad, gout), None


class _Accumulators:
    """Persistent fp64 device accumulators, zero between uses: the ``*_take`` launch that reads one also re-arms it,
    so a step spends no fill launch on it.  One per (device, stream, purpose); a use that did not reach its take
    (an exception in between) leaves the buffer dirty -- it is then replaced, not trusted."""

    def __init__(self):
        self.bufs = {}

    def get(self, device, purpose, n=1):
        key = (device.index, torch.cuda.current_stream(device).cuda_stream, purpose)
        ent = self.bufs.get(key)
        if ent is None or ent[1] or ent[0].numel() != n:
            ent = [torch.zeros(n, dtype=torch.float64, device=device), False]
            self.bufs[key] = ent
        ent[1] = True          # armed: being accumulated into
        return ent

    @staticmethod
    def taken(ent):
        ent[1] = False


_ACC = _Accumulators()


_UNIT = {}


def unit_seed(device) -> torch.Tensor:
    """The cached fp32 scalar 1.0 of a device: ``LightningModule.manual_backward`` seeds scalar losses with it."""
    t = _UNIT.get(device.index)
    if t is None:
        t = torch.ones((), dtype=torch.float32, device=device)
        _UNIT[device.index] = t
    return t


def _is_unit(gout) -> bool:
    """gout IS the cached unit seed of its device (the test ``_scaled`` makes)."""
    u = _UNIT.get(gout.device.index) if gout.is_cuda else None
    return u is not None and gout.data_ptr() == u.data_ptr()


def _scaled(grad, gout):
    """grad * gout -- without the launch when gout IS the cached unit seed (a loss backpropagated directly)."""
    u = _UNIT.get(gout.device.index) if gout.is_cuda else None
    if u is not None and gout.data_ptr() == u.data_ptr():
        return grad
    return grad * gout


class _GanDiscLoss(torch.autograd.Function):
    """BCE(real logits, 1) + BCE(fake logits, 0), each mean-reduced (reference models/wrapper.py:68-95), over ONE
    tensor of 2N logits with the real half first: two loss launches accumulate into one fp64 scalar, a third turns it
    into the fp32 loss.  The gradient w.r.t. all 2N logits comes out of the same two passes."""

    @staticmethod
    def forward(ctx, labels, n_real):
        _check_f32_cuda(labels)
        x = labels.contiguous().float()
        flat = x.view(-1)
        k = (flat.numel() // x.shape[0]) * int(n_real)
        need = ctx.needs_input_grad[0]
        grad = torch.empty_like(flat) if need else None
        ent = _ACC.get(x.device, "gan_d")
        ops.bce_logits(flat[:k], 1.0, 1.0, ent[0], 1.0, grad[:k] if need else None)
        ops.bce_logits(flat[k:], 0.0, 1.0, ent[0], 1.0, grad[k:] if need else None)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ops.scalar_take(ent[0], out)
        _ACC.taken(ent)
        if need:
            ctx.save_for_backward(grad)
            ctx.shape = labels.shape
        return out

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return _scaled(grad, gout).view(ctx.shape), None


def gan_discriminator_loss_pairs(labels: torch.Tensor, n_real: int) -> torch.Tensor:
    """discriminator_loss(labels[n_real:], labels[:n_real]) of reference models/wrapper.py:68-95 for the logits of a
    batched (real | fake) discriminator pass."""
    return _GanDiscLoss.apply(labels, n_real)


class _GanGenLoss(torch.autograd.Function):
    """BCE(D(x, pred), 1) + l1_weight * L1(pred, target) (reference models/wrapper.py:44-50): both mean losses
    accumulate into one fp64 scalar (the L1 launch scaled by l1_weight), a third launch makes the fp32 value."""

    @staticmethod
    def forward(ctx, pred_label, pred, target, l1_weight):
        _check_f32_cuda(pred_label, pred, target)
        lc, pc, tc = pred_label.contiguous().float(), pred.contiguous().float(), target.contiguous().float()
        need_l, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gl = torch.empty_like(lc) if need_l else None
        gp = torch.empty_like(pc) if need_p else None
        ent = _ACC.get(pc.device, "gan_g")
        ops.bce_logits(lc, 1.0, 1.0, ent[0], 1.0, gl)
        ops.l1(pc, tc, float(l1_weight), ent[0], float(l1_weight), gp)
        out = torch.empty((), dtype=torch.float32, device=pc.device)
        ops.scalar_take(ent[0], out)
        _ACC.taken(ent)
        ctx.save_for_backward(*[g for g in (gl, gp) if g is not None])
        ctx.which = (need_l, need_p)
        return out

    @staticmethod
    def backward(ctx, gout):
        saved = list(ctx.saved_tensors)
        gl = _scaled(saved.pop(0), gout) if ctx.which[0] else None
        gp = _scaled(saved.pop(0), gout) if ctx.which[1] else None
        return gl, gp, None, None


def gan_generator_loss(pred_label, pred, target, l1_weight: float) -> torch.Tensor:
    """bce(D(x, pred), ones) + l1_weight * l1(pred, target): the ``loss_type == "gan"`` branch of reference
    models/wrapper.py:44-50."""
    return _GanGenLoss.apply(pred_label, pred, target, float(l1_weight))


def bce_with_logits_const(logits: torch.Tensor, target: float) -> torch.Tensor:
    """F.binary_cross_entropy_with_logits(logits, full_like(logits, target)) (reference
    models/wrapper.py:45-48,84-93)."""
    return _MeanLoss.apply("bce", logits, target)


def l1_loss(pred, target):
    """F.l1_loss (reference models/wrapper.py:49)."""
    return _MeanLoss.apply("l1", pred, target)


def mse_loss(pred, target):
    """F.mse_loss (reference models/wrapper.py:66)."""
    return _MeanLoss.apply("mse", pred, target)


class _Denormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _check_f32_cuda(x)
        xc = x.contiguous().float()
        out = torch.empty_like(xc)
        ops.denormalize(xc, None, out)
        ctx.save_for_backward(xc)
        return out

    @staticmethod
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        out = torch.empty_like(xc)
        ops.denormalize(xc, g.contiguous().float(), out)
        return out


def denormalize(x):
    """clamp(x*0.5+0.5, 0, 1) (reference models/utils.py:11)."""
    return _Denormalize.apply(x)


# --------------------------------------------------------------------------------------
# metrics (differentiable where the reference uses them as losses)
# --------------------------------------------------------------------------------------
def _ssim_sse(pred, target, denorm, per_image=False, full=False):
    _check_f32_cuda(pred, target)
    p = pred.contiguous().float()
    t = target.contiguous().float()
    n, c, h, w = p.shape
    out2 = torch.zeros(2, dtype=torch.float64, device=p.device)
    per = torch.zeros(n * c, dtype=torch.float64, device=p.device) if per_image else None
    fm = torch.empty(n, c, h, w, dtype=torch.float32, device=p.device) if full else None
    ops.ssim_sse(p, t, n * c, h, w, denorm, out2, per, fm)
    return p, t, out2, per, fm


class _SsimPsnr(torch.autograd.Function):
    """value = w_ssim * SSIM + w_psnr * PSNR (data_range 1) of (optionally denormalised) images."""

    @staticmethod
    def forward(ctx, pred, target, w_ssim, w_psnr, denorm):
        p, t, out2, _, _ = _ssim_sse(pred, target, denorm)
        n, c, h, w = p.shape
        ssim_v = out2[0] / (n * c)
        psnr_v = -torch.log(out2[1] / p.numel()) * (10.0 / math.log(10.0))
        ctx.save_for_backward(p, t, out2)
        ctx.cfg = (w_ssim, w_psnr, denorm)
        return (w_ssim * ssim_v + w_psnr * psnr_v).float()

    @staticmethod
    def backward(ctx, gout):
        p, t, out2 = ctx.saved_tensors
        w_ssim, w_psnr, denorm = ctx.cfg
        n, c, h, w = p.shape
        ws = torch.empty(ops.ssim_bwd_workspace_floats(n * c, h, w), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        # the kernel returns d[-(w_ssim*SSIM + w_psnr*PSNR)]/dpred
        ops.ssim_psnr_bwd(p, t, n * c, h, w, denorm, w_ssim, w_psnr, out2[1:], grad, ws)
        return grad * (-gout), None, None, None, None


def ssim(pred, target):
    """structural_similarity_index_measure(pred, target, data_range=1.0) (reference
    models/utils.py:38-39).  Inputs are already denormalised."""
    return _SsimPsnr.apply(pred, target, 1.0, 0.0, 0)


def psnr(pred, target):
    """peak_signal_noise_ratio(pred, target, data_range=1.0) (reference models/utils.py:42-43)."""
    return _SsimPsnr.apply(pred, target, 0.0, 1.0, 0)


def rmse(pred, target):
    """mean_squared_error(pred, target, squared=False) (reference models/utils.py:46-47)."""
    p, t, out2, _, _ = _ssim_sse(pred.detach(), target.detach(), 0)
    return torch.sqrt(out2[1] / p.numel()).float()


def ssim_psnr_of_normalized(pred, target, w_ssim, w_psnr):
    """w_ssim*SSIM + w_psnr*PSNR of denormalize(pred), denormalize(target) with the
    denormalisation fused into the metric kernel (differentiable w.r.t. pred)."""
    return _SsimPsnr.apply(pred, target, float(w_ssim), float(w_psnr), 1)


def metrics_of_normalized(pred, target):
    """(ssim, psnr, rmse) of the denormalised pair in ONE pass over the images, no graph
    (the per-step logging of reference models/wrapper.py:150-156,168-173)."""
    _check_f32_cuda(pred, target)
    p, t = pred.detach().contiguous().float(), target.detach().contiguous().float()
    n, c, h, w = p.shape
    ent = _ACC.get(p.device, "metrics", 2)
    ops.ssim_sse(p, t, n * c, h, w, 1, ent[0], None, None)
    out3 = torch.empty(3, dtype=torch.float32, device=p.device)
    ops.metrics_take(ent[0], n * c, p.numel(), out3)
    _ACC.taken(ent)
    return out3[0], out3[1], out3[2]


def ssim_per_image(pred, target, return_full_image=False):
    """reduction='none' SSIM (reference report.py:78-84,207-212): per-image values and,
    optionally, the un-cropped SSIM map."""
    p, t, out2, per, fm = _ssim_sse(pred.detach(), target.detach(), 0, per_image=True, full=return_full_image)
    n, c = p.shape[:2]
    vals = per.view(n, c).mean(dim=1).float()
    return (vals, fm) if return_full_image else vals


# --------------------------------------------------------------------------------------
# report evaluation: per-image metrics and the rendered images of a chunk, on the device
# --------------------------------------------------------------------------------------
_AFMHOT = {}


def afmhot_lut_u8(device=None) -> torch.Tensor:
    """The 256 colours of matplotlib's ``afmhot`` as uint8 [256, 3], converted like every image the report writes
    (models/utils.py:to_int).  Indexed with ``min(int(x * 256), 255)`` it gives the bytes of reference report.py:220-233
    for a float image x in [0, 1].  Built once on the host; ``device``: a cached copy there."""
    key = str(device) if device is not None else "host"
    if "host" not in _AFMHOT:
        import numpy as np
        from matplotlib import colormaps

        from .models.utils import to_int
        _AFMHOT["host"] = to_int(torch.tensor(colormaps["afmhot"](np.arange(256))[:, :3], dtype=torch.float32)).contiguous()
    if key not in _AFMHOT:
        _AFMHOT[key] = _AFMHOT["host"].to(device)
    return _AFMHOT[key]


class EvalImages:
    """Result of ``eval_images``: ``ssim`` / ``psnr`` / ``mse`` fp32 [N], ``sse`` fp64 [N] (squared error per image),
    ``strip_ssim`` fp32 [N, strips] or None, ``ssim_map_u8`` uint8 [N, C, H, W] or None, ``hot_u8`` uint8 [N, C, 3, H, W]
    or None."""
    __slots__ = ("ssim", "psnr", "mse", "sse", "strip_ssim", "ssim_map_u8", "hot_u8")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def eval_images(pred, target, denorm=False, strips=0, ssim_map=False, hot=False) -> EvalImages:
    """What the report computes for a chunk of images (reference report.py:78-96,188-233) in two launches, whatever N is:
    one pass over the whole images (per-plane SSIM and squared error, the SSIM map and the afmhot rendering as bytes), one
    over the ``strips`` horizontal strips of every plane.  ``denorm``: the inputs are raw network output / targets in
    [-1, 1] (models/utils.py:11 is fused).  The per-image values are the report's expressions, in fp64 over the per-plane
    sums, rounded once to fp32."""
    _check_f32_cuda(pred, target)
    p, t = pred.detach().contiguous().float(), target.detach().contiguous().float()
    if p.dim() != 4 or p.shape != t.shape:
        raise ops.PaiError(f"eval_images: two [N, C, H, W] tensors of one shape expected, got {tuple(p.shape)}, {tuple(t.shape)}")
    n, c, h, w = (int(v) for v in p.shape)
    strips = int(strips)
    if strips and h % strips:
        raise ops.PaiError(f"eval_images: H = {h} is not a multiple of {strips} strips")
    sums = torch.zeros(2 * n * c + n * c * strips, dtype=torch.float64, device=p.device)
    ssim_pl, sse_pl, strip_pl = sums[:n * c], sums[n * c:2 * n * c], sums[2 * n * c:]
    map_u8 = ops.padded_u8((n, c, h, w), p.device) if ssim_map else None
    hot_u8 = ops.padded_u8((n, c, 3, h, w), p.device) if hot else None
    ops.eval_planes(p, t, n * c, h, w, denorm, ssim_pl, sse_pl, map_u8, afmhot_lut_u8(p.device) if hot else None, hot_u8)
    if strips:      # [N, C, H, W] is [N * C * strips, H / strips, W]
        ops.eval_planes(p, t, n * c * strips, h // strips, w, denorm, strip_pl)
    sse = sse_pl.view(n, c).sum(dim=1)
    numel = c * h * w
    return EvalImages(ssim=ssim_pl.view(n, c).mean(dim=1).float(),
                      psnr=(-torch.log(sse / numel) * (10.0 / math.log(10.0))).float(),
                      mse=torch.sqrt(sse / numel).float() ** 2,
                      sse=sse,
                      strip_ssim=strip_pl.view(n, c, strips).mean(dim=1).float() if strips else None,
                      ssim_map_u8=map_u8, hot_u8=hot_u8)


# --------------------------------------------------------------------------------------
# spatial attention of the Palette levels (differentiable)
# --------------------------------------------------------------------------------------
class _SpatialAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, ch):
        n, t = qkv.shape[0], qkv[0].numel() // qkv.shape[-1]
        out = torch.empty(qkv.shape[:-1] + (heads * ch,), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((n, heads, t), dtype=torch.float32, device=qkv.device)
        ops.sattn_fwd_lse(qkv.dtype, qkv, n, t, heads, ch, out, lse)
        ctx.save_for_backward(qkv, out, lse)
        ctx.dims = (n, t, heads, ch)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        qkv, out, lse = ctx.saved_tensors
        n, t, heads, ch = ctx.dims
        if g.dtype != qkv.dtype:
            raise ops.PaiError(f"spatial_attention: gradient of {g.dtype} for an output of {qkv.dtype}")
        dqkv = torch.empty_like(qkv)
        ws = torch.empty(n * heads * t, dtype=torch.float32, device=qkv.device)
        ops.sattn_bwd(qkv.dtype, g.contiguous(), qkv, out, lse, n, t, heads, ch, dqkv, ws)
        return dqkv, None, None


def spatial_attention(qkv, heads: int):
    """QKVAttentionLegacy (reference models/guided_diffusion/unet.py:265-297) with a backward: qkv [N, T, 3 C] or NHWC
    [N, H, W, 3 C] (fp32 or bf16, contiguous, on the device; the channel order [head][q | k | v][ch] of the 1 x 1 qkv
    convolution) -> [..., C].  Neither direction stores the T x T scores: the forward keeps qkv, out and the fp32 log-sum-exp of
    every query, the backward recomputes the probabilities from them (``pai_sattn_bwd``).  No host synchronisation."""
    if not isinstance(qkv, torch.Tensor) or not qkv.is_cuda:
        raise ops.PaiError("spatial_attention needs a HIP device tensor (no CPU fallback exists)")
    if qkv.dim() not in (3, 4) or qkv.numel() == 0:
        raise ops.PaiError(f"spatial_attention: qkv of shape {tuple(qkv.shape)} ([N, T, 3 C] or [N, H, W, 3 C])")
    if not qkv.is_contiguous():
        raise ops.PaiError("spatial_attention: qkv must be contiguous")
    width = qkv.shape[-1]
    if heads < 1 or width % (3 * heads):
        raise ops.PaiError(f"spatial_attention: width {width} is not divisible by 3 * heads = {3 * heads}")
    ch = width // (3 * heads)
    bwd_ok = (32, 64, 128, 256) if qkv.dtype == torch.float32 else (32, 64, 128)
    ops.code_of(qkv.dtype)
    if ch not in bwd_ok:
        raise ops.PaiError(f"spatial_attention: ch={ch} per head is not supported in {qkv.dtype} (fp32: 32, 64, 128 or 256; "
                           f"bf16: 32, 64 or 128)")
    return _SpatialAttention.apply(qkv, int(heads), ch)


# --------------------------------------------------------------------------------------
# train-mode BatchNorm + FiLM + SiLU + Dropout of the Palette blocks (differentiable)
# --------------------------------------------------------------------------------------
class _FilmNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, emb_out, mask, keep_scale, act, running_mean, running_var, nbt, momentum, eps,
                advance_in_backward=False, rng=None):
        n, c = x.shape[0], x.shape[-1]
        rows = x[0].numel() // c
        m, dtype = n * rows, x.dtype
        f32 = dict(dtype=torch.float32, device=x.device)
        srows = ops.bn_stats_rows(m)
        stats = torch.empty(ops.bn_stats_buffer_rows(srows) * 2 * c, **f32)
        ops.bn_stats(dtype, x, m, c, stats)
        mean, rstd, scale, shift = (torch.empty(c, **f32) for _ in range(4))
        # detached aliases (as ConvBNAct saves them): autograd's version check does not see an in-place update of weight / bias
        # between forward and backward -- step the optimizer after the backward.  The running buffers are advanced in place
        # here, as nn.BatchNorm advances them in its forward; they are no inputs of the graph, hence no mark_dirty.
        gamma, beta = weight.detach(), bias.detach()
        ops.bn_finalize(stats, srows, c, m, gamma, beta, eps, momentum, 1, running_mean, running_var, nbt, mean, rstd, scale,
                        shift)
        ld = emb_out.shape[1] if emb_out is not None else 0
        out = torch.empty_like(x)
        if rng is not None:                # (seed, stream, step, thr): the keep bits are formed in the kernel, no mask exists
            ops.film_norm_fwd_rng(dtype, x, rows, n, c, mean, rstd, gamma, beta, emb_out, ld, *rng, keep_scale, act, out)
        else:
            ops.film_norm_fwd(dtype, x, rows, n, c, mean, rstd, gamma, beta, emb_out, ld, mask, keep_scale, act, out)
        # advance_in_backward: the reference runs this norm's forward a second time while it differentiates (its AttentionBlock
        # is always under gradient checkpointing), so the running buffers advance once more, on the same batch statistics, in
        # the backward pass.  The statistics are kept for that; nothing is recomputed.
        ctx.again = None
        if advance_in_backward and running_mean is not None:
            ctx.again = (running_mean, running_var, nbt, srows, m, momentum, eps)
        ctx.save_for_backward(x, mean, rstd, gamma, beta, emb_out, mask, stats if ctx.again else None)
        ctx.dims = (n, rows, c, ld, keep_scale, act)
        ctx.rng = rng
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, mean, rstd, gamma, beta, emb_out, mask, stats = ctx.saved_tensors
        n, rows, c, ld, keep_scale, act = ctx.dims
        if g.dtype != x.dtype:
            raise ops.PaiError(f"film_norm_act: gradient of {g.dtype} for an output of {x.dtype}")
        f32 = dict(dtype=torch.float32, device=x.device)
        if ctx.again is not None:
            running_mean, running_var, nbt, srows, m, momentum, eps = ctx.again
            unused = torch.empty(4, c, **f32)
            ops.bn_finalize(stats, srows, c, m, gamma, beta, eps, momentum, 1, running_mean, running_var, nbt, unused[0], unused[1],
                            unused[2], unused[3])
        dx = torch.empty_like(x)
        # the columns of demb past 2 C belong to nobody: zero, as the gradient of columns the op does not read
        demb = torch.zeros_like(emb_out) if emb_out is not None else None
        dgb = torch.zeros(2 * c, **f32)
        ws = torch.empty(ops.film_norm_ws_floats(n, rows, c), **f32)
        if ctx.rng is not None:
            ops.film_norm_bwd_rng(x.dtype, g.contiguous(), x, rows, n, c, mean, rstd, gamma, beta, emb_out, ld, *ctx.rng, keep_scale,
                                  act, dx, demb, dgb[:c], dgb[c:], ws)
        else:
            ops.film_norm_bwd(x.dtype, g.contiguous(), x, rows, n, c, mean, rstd, gamma, beta, emb_out, ld, mask, keep_scale, act,
                              dx, demb, dgb[:c], dgb[c:], ws)
        return (dx, dgb[:c], dgb[c:], demb) + (None,) * 10


def film_norm_act(x, weight, bias, emb_out=None, *, act="silu", dropout_mask=None, p=0.0, running_mean=None, running_var=None,
                  num_batches_tracked=None, momentum=0.1, eps=1e-5, advance_in_backward=False, dropout_rng=None):
    """A norm site of the guided-diffusion U-Net in training (reference models/guided_diffusion/unet.py:141-172,206-210):
    ``Dropout(act(BatchNorm(x) * (1 + scale) + shift))`` on batch statistics, with a backward.  x: [N, rows, C] or NHWC
    [N, H, W, C] (fp32 or bf16, contiguous, on the device); weight, bias: fp32 [C]; emb_out: None or [N, >= 2 C] of x's dtype with
    ``scale | shift`` in its first 2 C columns, contiguous (the output of ``emb_layers``); act: "silu" or "none";
    dropout_mask: uint8 of x's shape, 0 drops; with p > 0 and no mask one is drawn with ``torch.rand`` on the current stream.
    dropout_rng = (seed, stream, step) instead of a mask: the keep bits are formed inside the kernels by the device generator
    (csrc/philox.h; element kept iff its 16-bit lane >= round(p 65536)), the backward rebuilds them, no mask tensor exists and
    torch's generator is not touched; with p = 0 nothing is dropped.  Not together with dropout_mask.
    running_mean / running_var / num_batches_tracked are updated in place as nn.BatchNorm does when they are given; with
    ``advance_in_backward`` they advance a second time, on the same batch statistics, when the backward pass runs (the
    reference's AttentionBlock norm, whose forward runs again under gradient checkpointing).  The
    forward keeps x, mean, rstd, emb_out and the mask, not its output; the backward returns the gradients of x, weight, bias
    and emb_out (``pai_film_norm_fwd`` / ``pai_film_norm_bwd``).  No host synchronisation."""
    if dropout_rng is not None and dropout_mask is not None:
        raise ops.PaiError("film_norm_act: dropout_rng and dropout_mask exclude each other")
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ops.PaiError("film_norm_act needs a HIP device tensor (no CPU fallback exists)")
    if x.dim() not in (3, 4) or x.numel() == 0:
        raise ops.PaiError(f"film_norm_act: x of shape {tuple(x.shape)} ([N, rows, C] or [N, H, W, C])")
    if not x.is_contiguous():
        raise ops.PaiError("film_norm_act: x must be contiguous")
    ops.code_of(x.dtype)
    n, c = x.shape[0], x.shape[-1]
    if act not in ("silu", "none"):
        raise ops.PaiError(f"film_norm_act: act={act!r} ('silu' or 'none')")
    if c % 8 or not 8 <= c <= 2048:
        raise ops.PaiError(f"film_norm_act: C={c} (a multiple of 8, at most 2048)")
    for name, t in (("weight", weight), ("bias", bias)):
        if t.dtype != torch.float32 or t.shape != (c,) or not t.is_contiguous():
            raise ops.PaiError(f"film_norm_act: {name} must be a contiguous fp32 [C] tensor")
    if emb_out is not None:
        if emb_out.dim() != 2 or emb_out.shape[0] != n or emb_out.shape[1] < 2 * c or not emb_out.is_contiguous() \
                or emb_out.dtype != x.dtype:
            raise ops.PaiError(f"film_norm_act: emb_out must be a contiguous [N, >= 2 C] tensor of {x.dtype}")
    if not 0.0 <= p < 1.0:
        raise ops.PaiError(f"film_norm_act: p={p}")
    rng = None
    if dropout_rng is not None:
        if len(dropout_rng) != 3:
            raise ops.PaiError("film_norm_act: dropout_rng is (seed, stream, step)")
        if p > 0.0:
            seed, stream, step = dropout_rng
            rng = (ops._u64(seed), ops._u32(stream, "stream"), ops._u32(step, "step"), ops.dropout_thr(p))
    elif dropout_mask is None and p > 0.0:
        dropout_mask = (torch.rand(x.shape, device=x.device) >= p).to(torch.uint8)
    if dropout_mask is not None and (dropout_mask.dtype != torch.uint8 or dropout_mask.shape != x.shape
                                     or not dropout_mask.is_contiguous()):
        raise ops.PaiError("film_norm_act: dropout_mask must be a contiguous uint8 tensor of x's shape")
    keep_scale = 1.0 / (1.0 - p) if dropout_mask is not None or rng is not None else 1.0
    return _FilmNormAct.apply(x, weight, bias, emb_out, dropout_mask, keep_scale, ops.ACT_SILU if act == "silu" else ops.ACT_NONE,
                              running_mean, running_var, num_batches_tracked, float(momentum), float(eps),
                              bool(advance_in_backward), rng)


def dropout2d(x, p, rng):
    """``nn.Dropout2d(p)`` in training mode on channels-last memory with the keep flags of the device generator (csrc/philox.h):
    ``x * (keep(n, c) ? 1 / (1 - p) : 0)``, differentiable.  x: [N, C] (one pixel per sample, the token form), [N, rows, C] or
    NHWC [N, H, W, C], fp32 or bf16, contiguous, on the device, C a multiple of 8.  rng = (seed, sub, stream, step): the Philox
    tuple of the flat [N][C] mask; channel c of sample n is kept iff its 16-bit lane >= round(p 65536).  ``step`` is an integer or
    the device scalar of ``DeviceRNG.device_step`` (then a launch recorded into a plan follows the counter).  The backward
    regenerates the flags from the same tuple; no mask tensor exists and torch's generator is not touched
    (``pai_dropout2d_rng`` / ``pai_dropout2d_rng_dev``)."""
    from . import nnops
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ops.PaiError("dropout2d needs a HIP device tensor (no CPU fallback exists)")
    if x.dim() not in (2, 3, 4) or x.numel() == 0:
        raise ops.PaiError(f"dropout2d: x of shape {tuple(x.shape)} ([N, C], [N, rows, C] or [N, H, W, C])")
    if not x.is_contiguous():
        raise ops.PaiError("dropout2d: x must be contiguous")
    ops.code_of(x.dtype)
    if x.shape[-1] % 8:
        raise ops.PaiError(f"dropout2d: C={x.shape[-1]} (a multiple of 8)")
    if not 0.0 <= p < 1.0:
        raise ops.PaiError(f"dropout2d: p={p}")
    if rng is None or len(rng) != 4:
        raise ops.PaiError("dropout2d: rng is (seed, sub, stream, step)")
    seed, sub, stream, step = rng
    rng = (ops._u64(seed), ops._u32(sub, "sub"), ops._u32(stream, "stream"), step if torch.is_tensor(step) else ops._u32(step, "step"))
    n, c = x.shape[0], x.shape[-1]
    return nnops.Dropout2dRng.apply(x.view(n, 1, -1, c), rng, float(p)).view(x.shape)


# --------------------------------------------------------------------------------------
# Palette training objective: forward noising, MSE + variational bound (differentiable)
# --------------------------------------------------------------------------------------
def _nhwc_pixels(x, what):
    """The NHWC memory [N, H, W, C] behind an NCHW fp32 device tensor: the view itself where the memory already is NHWC (what
    ``UNet.forward_train`` returns, and any single-channel tensor), a copy otherwise."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ops.PaiError(f"{what} needs HIP device tensors (no CPU fallback exists)")
    if x.dim() != 4 or x.numel() == 0 or x.dtype != torch.float32:
        raise ops.PaiError(f"{what}: an fp32 [N, C, H, W] tensor is expected, got {x.dtype} {tuple(x.shape)}")
    return x.permute(0, 2, 3, 1).contiguous()          # no copy when the permuted view is contiguous already


def _nchw_view(p):
    n, h, w, c = p.shape
    return p.reshape(n, 1, h, w) if c == 1 else p.permute(0, 3, 1, 2)


def _steps_i32(t, n, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ops.PaiError(f"{what} needs HIP device tensors (no CPU fallback exists)")
    if t.numel() != n or t.dtype not in (torch.int32, torch.int64):
        raise ops.PaiError(f"{what}: t must hold one int32 / int64 step per sample")
    return t.reshape(-1).to(torch.int32).contiguous()


def palette_noise(y0, t, u, z, diffusion):
    """q(y_t | y_0) of reference models/palette.py:214-231 with the draws handed in: y0, z fp32 [N, C, H, W], t int [N], u fp32
    [N] (any shape of N elements) on the device -> (y_t, noise, gamma).  gamma = (gammas[t] - gammas_prev[t]) u + gammas_prev[t],
    noise = z * (t > 0), y_t = sqrt(gamma) y0 + sqrt(1 - gamma) noise in one launch (``pai_palette_noise``); t is clamped to the
    schedule inside the kernel and never read on the host.  y_t and noise are NCHW views of NHWC memory."""
    p0 = _nhwc_pixels(y0, "palette_noise")
    pz = _nhwc_pixels(z, "palette_noise")
    if pz.shape != p0.shape:
        raise ops.PaiError("palette_noise: y0 and z differ in shape")
    n, h, w, c = p0.shape
    if not 1 <= c <= 4:
        raise ops.PaiError(f"palette_noise: C={c} (1..4)")
    ti = _steps_i32(t, n, "palette_noise")
    if not isinstance(u, torch.Tensor) or not u.is_cuda or u.numel() != n or u.dtype != torch.float32:
        raise ops.PaiError("palette_noise: u must be an fp32 device tensor of N elements")
    g, gp = diffusion.gammas, diffusion.gammas_prev
    if not g.is_cuda or g.device != p0.device:
        raise ops.PaiError("palette_noise: the schedule buffers are not on the device of y0 (move the model there)")
    y_t, noise = torch.empty_like(p0), torch.empty_like(p0)
    gamma = torch.empty(n, dtype=torch.float32, device=p0.device)
    ops.palette_noise(p0, pz, u.reshape(-1).contiguous(), ti, g.contiguous(), gp.contiguous(), n, h * w, c, y_t, noise, gamma)
    return _nchw_view(y_t), _nchw_view(noise), gamma


def palette_noise_rng(y0, seed, step, diffusion):
    """``palette_noise`` with its three draws made inside the launch by the device generator (csrc/philox.h): t[n] = integer n
    of stream 0 in [0, timesteps), u[n] = uniform n of stream 1, z = the normals of stream 2 over the NHWC pixels, all of the
    tuple (seed, step).  y0 fp32 [N, C, H, W] -> (y_t, noise, gamma, t) with t int32 [N] on the device for ``palette_objective``;
    one launch (``pai_palette_noise_rng``), torch's generator is not touched, nothing is copied to the host."""
    p0 = _nhwc_pixels(y0, "palette_noise_rng")
    n, h, w, c = p0.shape
    if not 1 <= c <= 4:
        raise ops.PaiError(f"palette_noise_rng: C={c} (1..4)")
    g, gp = diffusion.gammas, diffusion.gammas_prev
    if not g.is_cuda or g.device != p0.device:
        raise ops.PaiError("palette_noise_rng: the schedule buffers are not on the device of y0 (move the model there)")
    y_t, noise = torch.empty_like(p0), torch.empty_like(p0)
    gamma = torch.empty(n, dtype=torch.float32, device=p0.device)
    t = torch.empty(n, dtype=torch.int32, device=p0.device)
    ops.palette_noise_rng(p0, g.contiguous(), gp.contiguous(), n, h * w, c, seed, step, t, y_t, noise, gamma)
    return _nchw_view(y_t), _nchw_view(noise), gamma, t


_PHILOX_KINDS = {"raw": ops.PHILOX_RAW, "uniform": ops.PHILOX_UNIFORM, "normal": ops.PHILOX_NORMAL, "int": ops.PHILOX_INT,
                 "keep": ops.PHILOX_KEEP}


def philox_fill(kind, shape, seed, sub=0, stream=0, step=0, param=0, device=None, out=None):
    """A tensor of the device generator's values (csrc/philox.h, ``pai_philox_fill``): element i of the flat tensor is value i of
    the tuple (seed, sub, stream, step).  kind: "raw" (the 32-bit words, as int32 bits), "uniform" (fp32 in [0, 1)), "normal"
    (fp32), "int" (int32 in [0, param)), "keep" (uint8 0 / 1, kept iff the 16-bit lane >= param = round(p 65536)).  ``out``: a
    contiguous device tensor of the kind's dtype to fill instead of a new one of ``shape`` on ``device``."""
    if kind not in _PHILOX_KINDS:
        raise ops.PaiError(f"philox_fill: kind={kind!r} (one of {sorted(_PHILOX_KINDS)})")
    code = _PHILOX_KINDS[kind]
    if out is None:
        if device is None or torch.device(device).type != "cuda":
            raise ops.PaiError("philox_fill needs a HIP device (no CPU fallback exists)")
        out = torch.empty(shape, dtype=ops.PHILOX_DTYPES[code], device=device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda:
        raise ops.PaiError("philox_fill needs a HIP device tensor (no CPU fallback exists)")
    elif not out.is_contiguous() or out.dtype != ops.PHILOX_DTYPES[code]:
        raise ops.PaiError(f"philox_fill: out must be a contiguous {ops.PHILOX_DTYPES[code]} tensor")
    if out.numel() == 0:
        raise ops.PaiError("philox_fill: an empty tensor")
    ops.philox_fill(code, out, seed, sub, stream, step, param)
    return out


class _PaletteObjective(torch.autograd.Function):
    """(loss, mse, vlb, vlb_n) from ``pai_palette_objective``; the launch that forms the loss also writes d loss / d model_out,
    which the backward multiplies by the incoming gradient."""

    @staticmethod
    def forward(ctx, model_out, noise, y0, y_t, t, table, learn_var):
        pm = _nhwc_pixels(model_out, "palette_objective")
        n, h, w, co = pm.shape
        c = co // 2 if learn_var else co
        f32 = dict(dtype=torch.float32, device=pm.device)
        out = torch.empty(3 + n, **f32)
        dout = torch.empty_like(pm)
        ws = torch.empty(ops.palette_objective_ws_floats(n, h * w), **f32)
        ops.palette_objective(pm, noise, y0, y_t, t, table, n, h * w, c, learn_var, 0.001 if learn_var else 0.0, out, dout, ws)
        ctx.save_for_backward(dout)
        loss, mse, vlb, vlb_n = out[2].clone(), out[0].clone(), out[1].clone(), out[3:].clone()
        ctx.mark_non_differentiable(mse, vlb, vlb_n)
        return loss, mse, vlb, vlb_n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout, *unused):
        (dout,) = ctx.saved_tensors
        return (_nchw_view(_scaled(dout, gout)),) + (None,) * 6


def palette_objective(model_out, noise, y0, y_t, t, diffusion, learn_var):
    """The training objective of reference models/palette.py:122-140 on the device: model_out fp32 [N, C, H, W] (or, learn_var,
    [N, 2 C, H, W] as eps | var; the NCHW view ``UNet.forward_train`` returns is read in place), noise, y0, y_t fp32
    [N, C, H, W], t int [N] -> (loss, mse, vlb, vlb_n).  mse = mean (eps - noise)^2; vlb_n = the KL term of the variational bound,
    or at t = 0 the discretised Gaussian negative log-likelihood, per sample in bits; vlb = mean vlb_n; loss = mse + 0.001 vlb with
    learn_var, else mse.  Only ``loss`` carries a gradient, and only into model_out: the eps columns get the MSE's (the bound
    sees a detached eps), the var columns the bound's.  The per-step scalars are gathered on the device from
    ``diffusion.step_table_device``; nothing is copied to the host."""
    pm = _nhwc_pixels(model_out, "palette_objective")
    n, h, w, co = pm.shape
    if learn_var and co % 2:
        raise ops.PaiError(f"palette_objective: learn_var needs an even channel count, got {co}")
    c = co // 2 if learn_var else co
    if not 1 <= c <= 4:
        raise ops.PaiError(f"palette_objective: C={c} (1..4)")
    pix = []
    for name, v in (("noise", noise), ("y0", y0), ("y_t", y_t)):
        p = _nhwc_pixels(v, "palette_objective")
        if p.shape != (n, h, w, c):
            raise ops.PaiError(f"palette_objective: {name} of shape {tuple(v.shape)} for a model output of {tuple(model_out.shape)}")
        pix.append(p)
    ti = _steps_i32(t, n, "palette_objective")
    table = diffusion.step_table_device(pm.device)
    return _PaletteObjective.apply(model_out, pix[0], pix[1], pix[2], ti, table, bool(learn_var))
