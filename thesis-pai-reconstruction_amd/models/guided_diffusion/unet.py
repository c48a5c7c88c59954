"""Guided-diffusion U-Net of Palette (reference models/guided_diffusion/unet.py:342-573, nn.py) on the MI355X kernels: the
eval-mode forward (sampling) and ``forward_train``, the differentiable train-mode pass.

Same module tree as the reference -- ``cond_embed``, ``input_blocks`` / ``middle_block`` / ``output_blocks`` of
``EmbedSequential`` holding ``ResBlock`` / ``AttentionBlock``, ``out`` -- built from stock ``nn`` modules as parameter
containers, so state-dict keys and shapes are interchangeable.  The reference's normalisation layers are BatchNorm
(nn.py:51-68); in eval mode each is a per-channel affine from its running statistics, so one kernel
(``pai_affine_act``) serves every norm + SiLU site, with the FiLM scale / shift of ``use_scale_shift_norm`` folded into
per-sample coefficients (``pai_film_coeffs``).  Convolutions and the 1 x 1 ``qkv`` / ``proj_out`` layers run on the
convolution family (``torch.cat`` in front of the decoder blocks is the two-pointer input), attention on
``pai_sattn_fwd`` (the T x T scores of a level are never stored).

The embedding path (``cond_embed`` and every ``emb_layers`` Linear) runs in fp32 in both precisions: it is [N, 512] per
call, and the ``emb_layers`` of all blocks are one GEMM over their concatenated weights.

Weight packs, folded BatchNorm coefficients and that concatenation are cached per (dtype, weight generation): a sampling
loop of 100 calls builds them once.

``forward_train`` composes the same module tree from autograd Functions (the blocks' ``run_train`` beside ``run``): every
norm site is ``functional.film_norm_act`` on batch statistics, every convolution ``nnops.ConvBNAct`` without a norm,
attention ``functional.spatial_attention``.  It caches nothing and drops the eval caches, because the running statistics it
advances do not move the buffers' version counters.  ``__call__`` / ``run`` in training mode keep raising.
"""
import weakref

import torch
import torch.nn as nn

from ... import functional as PF
from ... import nnops, ops
from ...ops import ACT_NONE, ACT_SILU, STREAM_DROPOUT, PaiError


class SiLU(nn.Module):
    """Parameter-free place holder (the reference's own SiLU module): the arithmetic is in ``pai_affine_act``."""


class EmbedSequential(nn.Sequential):
    """Children that take the embedding (``ResBlock``) get it; the others do not."""

    def run(self, h, h2, ctx, name):
        for j, layer in enumerate(self):
            if isinstance(layer, ResBlock):
                h, h2 = layer.run(h, h2, ctx), None
            elif isinstance(layer, AttentionBlock):
                h = layer.run(h, ctx)
            else:
                h = ctx.conv(layer, h, h2)        # the first convolution of the network
                h2 = None
            ctx.keep(f"{name}.{j}", h)
        ctx.keep(name, h)
        return h

    def run_train(self, h, h2, ctx, name):
        for j, layer in enumerate(self):
            if isinstance(layer, ResBlock):
                h, h2 = layer.run_train(h, h2, ctx, f"{name}.{j}"), None
            elif isinstance(layer, AttentionBlock):
                h = layer.run_train(h, ctx)
            else:
                h = ctx.conv(layer, h, h2)
                h2 = None
            ctx.keep(f"{name}.{j}", h)
        ctx.keep(name, h)
        return h


class Upsample(nn.Module):
    """Nearest 2x (the ``use_conv=False`` form is all ``resblock_updown`` uses)."""

    def __init__(self, channels, use_conv, out_channel=None):
        super().__init__()
        self.channels, self.out_channel, self.use_conv = channels, out_channel or channels, use_conv
        if use_conv:
            self.conv = nn.Conv2d(self.channels, self.out_channel, 3, padding=1)

    def run(self, x, ctx):
        x = ctx.upsample(x)
        return ctx.conv(self.conv, x) if self.use_conv else x

    run_train = run


class Downsample(nn.Module):
    """2 x 2 mean; the strided-convolution form (``use_conv=True``) is not reached by Palette's settings and not built."""

    def __init__(self, channels, use_conv, out_channel=None):
        super().__init__()
        self.channels, self.out_channel, self.use_conv = channels, out_channel or channels, use_conv
        if use_conv:
            self.op = nn.Conv2d(self.channels, self.out_channel, 3, stride=2, padding=1)
        else:
            if self.channels != self.out_channel:
                raise ValueError("Downsample without a convolution keeps the channel count")
            self.op = nn.AvgPool2d(kernel_size=2, stride=2)

    def run(self, x, ctx):
        if self.use_conv:
            raise PaiError("Downsample(use_conv=True) is not built on the HIP path (Palette uses resblock_updown)")
        return ctx.avgpool(x)

    run_train = run


class ResBlock(nn.Module):
    """norm -> SiLU -> 3x3 conv, FiLM-conditioned norm -> SiLU -> (dropout) -> 3x3 conv, plus the skip path; optionally
    resampling both branches (reference unet.py:105-214 with ``use_scale_shift_norm=True``)."""

    def __init__(self, channels, emb_channels, dropout, out_channel=None, use_conv=False, use_scale_shift_norm=True,
                 up=False, down=False):
        super().__init__()
        if not use_scale_shift_norm:
            raise ValueError("ResBlock: only the scale-shift (FiLM) conditioning Palette uses is built")
        self.channels, self.emb_channels, self.dropout = channels, emb_channels, dropout
        self.out_channel = out_channel or channels
        self.in_layers = nn.Sequential(nn.BatchNorm2d(channels), SiLU(),
                                       nn.Conv2d(channels, self.out_channel, 3, padding=1))
        self.updown = up or down
        if up:
            self.h_upd, self.x_upd = Upsample(channels, False), Upsample(channels, False)
        elif down:
            self.h_upd, self.x_upd = Downsample(channels, False), Downsample(channels, False)
        else:
            self.h_upd = self.x_upd = nn.Identity()
        self.emb_layers = nn.Sequential(SiLU(), nn.Linear(emb_channels, 2 * self.out_channel))
        last = nn.Conv2d(self.out_channel, self.out_channel, 3, padding=1)
        nn.init.zeros_(last.weight)
        nn.init.zeros_(last.bias)
        self.out_layers = nn.Sequential(nn.BatchNorm2d(self.out_channel), SiLU(), nn.Dropout(p=dropout), last)
        if self.out_channel == channels:
            self.skip_connection = nn.Identity()
        elif use_conv:
            self.skip_connection = nn.Conv2d(channels, self.out_channel, 3, padding=1)
        else:
            self.skip_connection = nn.Conv2d(channels, self.out_channel, 1)

    def run(self, x, x2, ctx):
        """x (and x2, read as cat([x, x2]) along the channels): NHWC -> NHWC."""
        a, b = ctx.bn(self.in_layers[0])
        if x2 is None:
            h, h2 = ctx.affine(x, a, b, ACT_SILU), None
        else:
            c1 = x.shape[3]
            h, h2 = ctx.affine(x, a[:c1], b[:c1], ACT_SILU), ctx.affine(x2, a[c1:], b[c1:], ACT_SILU)
        if self.updown:
            if x2 is not None:
                raise PaiError("ResBlock: a resampling block takes one input tensor")
            h, x = self.h_upd.run(h, ctx), self.x_upd.run(x, ctx)
        h = ctx.conv(self.in_layers[2], h, h2)
        A, B = ctx.film(self.out_layers[0], self)
        h = ctx.affine(h, A, B, ACT_SILU, per_sample=True)
        h = ctx.conv(self.out_layers[3], h)
        if isinstance(self.skip_connection, nn.Identity):
            s = x if x2 is None else torch.cat([x, x2], dim=3)       # data movement only
        else:
            s = ctx.conv(self.skip_connection, x, x2)
        return ctx.add(s, h)

    def run_train(self, x, x2, ctx, prefix):
        """``run`` in training: x (and x2) NHWC -> NHWC, every op an autograd Function.  The norm over cat([x, x2]) is two calls
        on the two tensors with the two halves of the BatchNorm: it is per channel."""
        bn = self.in_layers[0]
        x, xs = nnops.Fork.apply(x)                      # the residual branch and the skip path
        if x2 is None:
            h, h2, xs2 = ctx.norm(bn, x), None, None
        else:
            c1 = x.shape[3]
            x2, xs2 = nnops.Fork.apply(x2)
            h, h2 = ctx.norm(bn, x, lo=0, hi=c1), ctx.norm(bn, x2, lo=c1, hi=self.channels, count=False)
        if self.updown:
            if x2 is not None:
                raise PaiError("ResBlock: a resampling block takes one input tensor")
            h, xs = self.h_upd.run_train(h, ctx), self.x_upd.run_train(xs, ctx)
        h = ctx.conv(self.in_layers[2], h, h2)
        mask = ctx.masks.get(prefix)
        h = ctx.norm(self.out_layers[0], h, emb=ctx.emb[id(self)], p=self.dropout, mask=mask,
                     rng=None if mask is not None else ctx.rng.get(id(self)))
        h = ctx.conv(self.out_layers[3], h)
        if isinstance(self.skip_connection, nn.Identity):
            s = xs if xs2 is None else torch.cat([xs, xs2], dim=3)       # data movement only
        else:
            s = ctx.conv(self.skip_connection, xs, xs2)
        return ctx.add(s, h)


class AttentionBlock(nn.Module):
    """norm -> 1x1 qkv -> attention over the H * W positions -> 1x1 proj_out, + x (reference unet.py:217-262 with
    ``QKVAttentionLegacy``: the 3C channels of a position are [head][q | k | v][ch])."""

    def __init__(self, channels, num_heads=1, num_head_channels=-1):
        super().__init__()
        self.channels = channels
        if num_head_channels == -1:
            self.num_heads = num_heads
        else:
            if channels % num_head_channels:
                raise ValueError(f"q,k,v channels {channels} is not divisible by num_head_channels {num_head_channels}")
            self.num_heads = channels // num_head_channels
        self.norm = nn.BatchNorm1d(channels)
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.proj_out = nn.Conv1d(channels, channels, 1)
        nn.init.zeros_(self.proj_out.weight)
        nn.init.zeros_(self.proj_out.bias)

    def run(self, x, ctx):
        n, hh, ww, c = x.shape
        a, b = ctx.bn(self.norm)
        qkv = ctx.conv(self.qkv, ctx.affine(x, a, b, ACT_NONE))
        att = torch.empty_like(x)
        ops.sattn_fwd(ctx.dtype, qkv, n, hh * ww, self.num_heads, c // self.num_heads, att)
        return ctx.add(x, ctx.conv(self.proj_out, att))

    def run_train(self, x, ctx):
        """``run`` in training.  The reference block is always under gradient checkpointing, so its norm's forward runs again
        while it differentiates and the running statistics advance twice per step: ``twice`` moves them again in the backward
        pass (the statistics are kept; nothing is recomputed)."""
        x, xs = nnops.Fork.apply(x)
        qkv = ctx.conv(self.qkv, ctx.norm(self.norm, x, act="none", twice=True))
        return ctx.add(xs, ctx.conv(self.proj_out, PF.spatial_attention(qkv, self.num_heads)))


class _Run:
    """One forward pass: the kernels behind the blocks' ``run`` methods, reading the U-Net's caches."""

    def __init__(self, unet, cache, dtype, emb_all, capture):
        self.unet, self.cache, self.dtype, self.emb_all, self.capture = unet, cache, dtype, emb_all, capture
        self.n = emb_all.shape[0]

    def keep(self, name, t):
        """tests: the output of module ``name`` (its state-dict prefix) as fp32 NCHW."""
        if self.capture is not None:
            self.capture[name] = t.detach().float().permute(0, 3, 1, 2).contiguous()

    def bn(self, m):
        return self.cache["bn"][id(m)]

    def affine(self, x, A, B, act, per_sample=False):
        n, hh, ww, c = x.shape
        out = torch.empty_like(x)
        ops.affine_act(self.dtype, x, hh * ww, n, c, A, B, per_sample, act, out)
        return out

    def film(self, bn, block):
        a, b = self.bn(bn)
        c = block.out_channel
        f32 = dict(dtype=torch.float32, device=a.device)
        A, B = torch.empty(self.n, c, **f32), torch.empty(self.n, c, **f32)
        off = self.cache["emb_off"][id(block)]
        ops.film_coeffs(c, self.n, a, b, self.emb_all[:, off:], self.emb_all.shape[1], A, B)
        return A, B

    def conv(self, m, x, x2=None):
        n, hh, ww, c1 = x.shape
        c2 = 0 if x2 is None else x2.shape[3]
        wf, bias, k, cin, cout = self.cache["conv"][id(m)]
        if c1 + c2 != cin:
            raise PaiError(f"convolution built for {cin} input channels, got {c1} + {c2}")
        key = (id(m), n, hh, ww, c1, c2)
        d = self.cache["desc"].get(key)
        if d is None:
            d = ops.make_desc(self.dtype, 0, n, hh, ww, c1, c2, cout, 1, 0, 0, ACT_NONE, kernel=k)
            ops.ensure_workspace(ops.conv_workspace_bytes(d, 0), x.device)
            if cin <= 2 or cout <= 2:
                ops.ensure_scratch(ops.conv_scratch_bytes(d, 0), x.device)
            self.cache["desc"][key] = d
        out = torch.empty(n, hh, ww, cout, dtype=self.dtype, device=x.device)
        ops.conv_fwd(d, x, x2, wf, bias, y_raw=out)
        return out

    def upsample(self, x):
        n, hh, ww, c = x.shape
        out = torch.empty(n, 2 * hh, 2 * ww, c, dtype=x.dtype, device=x.device)
        ops.upsample2(self.dtype, x, n, hh, ww, c, out)
        return out

    def avgpool(self, x):
        n, hh, ww, c = x.shape
        if hh % 2 or ww % 2:
            raise PaiError(f"UNet: a {hh} x {ww} level cannot be halved (the input size must divide by 2 ** (levels - 1))")
        out = torch.empty(n, hh // 2, ww // 2, c, dtype=x.dtype, device=x.device)
        ops.avgpool2(self.dtype, x, n, hh, ww, c, out)
        return out

    def add(self, a, b):
        out = torch.empty_like(a)
        ops.add_act(self.dtype, a, b, ACT_NONE, out)
        return out


class _TrainRun:
    """One training pass: the autograd Functions behind the blocks' ``run_train`` methods.  ``emb``: id(ResBlock) -> its
    [N, 2 C] ``scale | shift`` in the storage dtype; ``masks``: ResBlock prefix -> uint8 NHWC dropout mask; ``rng``:
    id(ResBlock) -> the (seed, stream, step) of its dropout under the device generator (empty: torch draws the masks)."""

    def __init__(self, dtype, emb, masks, capture, rng=None):
        self.dtype, self.emb, self.masks, self.capture, self.rng = dtype, emb, masks, capture, rng or {}

    keep = _Run.keep

    def norm(self, bn, x, emb=None, act="silu", p=0.0, mask=None, lo=None, hi=None, count=True, twice=False, rng=None):
        """A norm site on the channels [lo, hi) of ``bn`` (all of them by default); ``count``: this call advances
        ``num_batches_tracked`` (one of the two calls of a norm over a concatenation does)."""
        w, b, mean, var = bn.weight, bn.bias, bn.running_mean, bn.running_var
        if lo is not None:
            w, b, mean, var = w[lo:hi], b[lo:hi], mean[lo:hi], var[lo:hi]
        return PF.film_norm_act(x, w, b, emb, act=act, dropout_mask=mask, p=float(p), running_mean=mean, running_var=var,
                                num_batches_tracked=bn.num_batches_tracked if count else None,
                                momentum=0.1 if bn.momentum is None else bn.momentum, eps=bn.eps, advance_in_backward=twice,
                                dropout_rng=rng)

    def conv(self, m, x, x2=None):
        w = m.weight
        if w.dim() == 3:                                  # Conv1d over the positions: a 1 x 1 convolution
            w = w.view(w.shape[0], w.shape[1], 1, 1)
        c2 = 0 if x2 is None else x2.shape[3]
        if x.shape[3] + c2 != w.shape[1]:
            raise PaiError(f"convolution built for {w.shape[1]} input channels, got {x.shape[3]} + {c2}")
        return nnops.ConvBNAct.apply(x, x2, w, m.bias, None, None, None, True, 1, ACT_NONE, 1, self.dtype, False)

    def upsample(self, x):
        return nnops.Upsample2.apply(x)

    def avgpool(self, x):
        if x.shape[1] % 2 or x.shape[2] % 2:
            raise PaiError(f"UNet: a {x.shape[1]} x {x.shape[2]} level cannot be halved (the input size must divide by "
                           f"2 ** (levels - 1))")
        return nnops.AvgPool2.apply(x)

    def add(self, a, b):
        return nnops.AddAct.apply(a, b, ACT_NONE)


class UNet(nn.Module):
    """The U-Net with attention and noise-level embedding (reference unet.py:342-573).

    :input: x, y [N x C x H x W] (read as cat([x, y])), gammas [N]   :output: [N x out_channel x H x W] (fp32)
    """

    def __init__(self, image_size, in_channel, inner_channel, out_channel, res_blocks, attn_res, dropout=0,
                 channel_mults=(1, 2, 4, 8), conv_resample=True, num_heads=1, num_head_channels=-1, num_heads_upsample=-1,
                 use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=False):
        super().__init__()
        if use_new_attention_order or not resblock_updown:
            raise ValueError("UNet: only the legacy attention order and resampling ResBlocks (Palette's settings) are built")
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
        self.image_size, self.in_channel, self.inner_channel, self.out_channel = image_size, in_channel, inner_channel, out_channel
        self.res_blocks, self.attn_res, self.dropout = res_blocks, tuple(attn_res), dropout
        self.channel_mults, self.conv_resample = tuple(channel_mults), conv_resample
        self.num_heads, self.num_head_channels, self.num_heads_upsample = num_heads, num_head_channels, num_heads_upsample
        self.compute_dtype = torch.float32
        self.debug_capture = None        # tests: dict name -> detached fp32 NCHW activation
        self._cache = None
        self._train_consts = None        # (ones, zeros) fp32 [emb_dim]: the unit coefficients of the embedding path's SiLU

        emb_dim = inner_channel * 4
        self.cond_embed = nn.Sequential(nn.Linear(inner_channel, emb_dim), SiLU(), nn.Linear(emb_dim, emb_dim))

        def res(cin, cout, **kw):
            return ResBlock(cin, emb_dim, dropout, out_channel=cout, use_scale_shift_norm=use_scale_shift_norm, **kw)

        def att(c, heads):
            return AttentionBlock(c, num_heads=heads, num_head_channels=num_head_channels)

        ch = first = int(channel_mults[0] * inner_channel)
        blocks = [EmbedSequential(nn.Conv2d(in_channel, ch, 3, padding=1))]
        skip_chans, ds = [ch], 1
        for level, mult in enumerate(channel_mults):
            width = int(mult * inner_channel)
            for _ in range(res_blocks):
                layers = [res(ch, width)]
                ch = width
                if ds in attn_res:
                    layers.append(att(ch, num_heads))
                blocks.append(EmbedSequential(*layers))
                skip_chans.append(ch)
            if level != len(channel_mults) - 1:
                blocks.append(EmbedSequential(res(ch, ch, down=True)))
                skip_chans.append(ch)
                ds *= 2
        self.input_blocks = nn.ModuleList(blocks)
        self.middle_block = EmbedSequential(res(ch, ch), att(ch, num_heads), res(ch, ch))
        blocks = []
        for level, mult in reversed(list(enumerate(channel_mults))):
            width = int(inner_channel * mult)
            for i in range(res_blocks + 1):
                layers = [res(ch + skip_chans.pop(), width)]
                ch = width
                if ds in attn_res:
                    layers.append(att(ch, num_heads_upsample))
                if level and i == res_blocks:
                    layers.append(res(ch, ch, up=True))
                    ds //= 2
                blocks.append(EmbedSequential(*layers))
        self.output_blocks = nn.ModuleList(blocks)
        last = nn.Conv2d(first, out_channel, 3, padding=1)
        nn.init.zeros_(last.weight)
        nn.init.zeros_(last.bias)
        self.out = nn.Sequential(nn.BatchNorm2d(ch), SiLU(), last)

    # ---- caches: weight packs, folded BatchNorm coefficients, the concatenated emb_layers ----------------------------
    def _generation(self):
        t = list(self.parameters()) + list(self.buffers())
        return (t[0].device, t[0].data_ptr(), sum(v._version for v in t))

    def prepared(self, dtype):
        """The cache for ``dtype`` at the current weights (built once per weight generation: an optimizer step, a
        ``load_state_dict``, an EMA swap or a move to another device start a new one)."""
        gen = self._generation()
        c = self._cache
        if c is not None and c["dtype"] == dtype and c["gen"] == gen:
            return c
        dev = gen[0]
        c = {"dtype": dtype, "gen": gen, "conv": {}, "bn": {}, "emb_off": {}, "desc": {}}
        f32 = dict(dtype=torch.float32, device=dev)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                w = m.weight.detach()
                if w.dim() == 3:                              # Conv1d over the positions: a 1 x 1 convolution
                    w = w.view(w.shape[0], w.shape[1], 1, 1)
                cout, cin, k, _ = w.shape
                wm = nnops._dense_fwd_pack(w, 1)              # fp32 [Cout][kh][kw][Cin]
                if dtype == torch.float32:
                    wf = wm
                else:
                    wf = torch.empty(wm.numel(), dtype=dtype, device=dev)
                    ops.pack_weights(dtype, wm, cout, k * k, cin, wf, None)
                c["conv"][id(m)] = (wf, m.bias.detach().float().contiguous(), k, cin, cout)
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                a, b = torch.empty(m.num_features, **f32), torch.empty(m.num_features, **f32)
                ops.bn_eval_coeffs(m.num_features, m.weight.detach(), m.bias.detach(), m.running_mean, m.running_var,
                                   float(m.eps), a, b)
                c["bn"][id(m)] = (a, b)
        blocks = [m for m in self.modules() if isinstance(m, ResBlock)]
        off = 0
        for blk in blocks:
            c["emb_off"][id(blk)] = off
            off += 2 * blk.out_channel
        c["emb_w"] = torch.cat([blk.emb_layers[1].weight.detach().float() for blk in blocks], 0).contiguous()
        c["emb_b"] = torch.cat([blk.emb_layers[1].bias.detach().float() for blk in blocks], 0).contiguous()
        c["lin"] = [(self.cond_embed[i].weight.detach().float().contiguous(),
                     self.cond_embed[i].bias.detach().float().contiguous()) for i in (0, 2)]
        c["ones"] = torch.ones(self.inner_channel * 4, **f32)
        c["zeros"] = torch.zeros(self.inner_channel * 4, **f32)
        self._cache = c
        return c

    @staticmethod
    def _linear(x, w, b):
        """fp32 [M, K] x [out, K]^T + b as a one-tap convolution over the rows."""
        m, k = x.shape
        d = ops.make_desc(torch.float32, 0, 1, 1, m, k, 0, w.shape[0], 1, 0, 0, ACT_NONE, kernel=1)
        ops.ensure_workspace(ops.conv_workspace_bytes(d, 0), x.device)
        y = torch.empty(m, w.shape[0], dtype=torch.float32, device=x.device)
        ops.conv_fwd(d, x, None, w, b, y_raw=y)
        return y

    def _embed(self, gammas, c):
        """[N, sum of 2 * out_channel]: emb_layers(cond_embed(gamma_embedding(gammas))) of every ResBlock, fp32."""
        n = gammas.shape[0]
        e = torch.empty(n, self.inner_channel, dtype=torch.float32, device=gammas.device)
        ops.gamma_embedding(gammas, n, self.inner_channel, e)
        e = self._linear(e, *c["lin"][0])
        ops.affine_act(torch.float32, e, 1, n, e.shape[1], c["ones"], c["zeros"], False, ACT_SILU, e)
        e = self._linear(e, *c["lin"][1])
        ops.affine_act(torch.float32, e, 1, n, e.shape[1], c["ones"], c["zeros"], False, ACT_SILU, e)
        return self._linear(e, c["emb_w"], c["emb_b"])

    def run(self, xy, gammas, cache=None):
        """xy: NHWC [N, H, W, in_channel] in the storage dtype, gammas fp32 [N] -> NHWC [N, H, W, out_channel] (storage dtype)."""
        if self.training:
            raise PaiError("UNet (HIP) is built for eval-mode sampling only: call eval() / freeze() first")
        if not xy.is_cuda or not gammas.is_cuda:
            raise PaiError("UNet (HIP) needs HIP device tensors; there is no CPU path")
        dtype = self.compute_dtype
        c = cache if cache is not None else self.prepared(dtype)
        if xy.dtype != dtype or xy.dim() != 4 or xy.shape[3] != self.in_channel or not xy.is_contiguous():
            raise PaiError(f"UNet.run takes a contiguous NHWC {dtype} tensor with {self.in_channel} channels")
        ctx = _Run(self, c, dtype, self._embed(gammas.reshape(-1).float().contiguous(), c), self.debug_capture)
        h, hs = xy, []
        for i, blk in enumerate(self.input_blocks):
            h = blk.run(h, None, ctx, f"input_blocks.{i}")
            hs.append(h)
        h = self.middle_block.run(h, None, ctx, "middle_block")
        for i, blk in enumerate(self.output_blocks):
            h = blk.run(h, hs.pop(), ctx, f"output_blocks.{i}")
        a, b = ctx.bn(self.out[0])
        return ctx.conv(self.out[2], ctx.affine(h, a, b, ACT_SILU))

    # ---- training ------------------------------------------------------------------------------------------------------
    def _embed_train(self, gammas, dtype):
        """``_embed`` with a tape: id(ResBlock) -> [N, 2 * out_channel] in the storage dtype.  fp32 up to the cast; the
        ``emb_layers`` of all blocks are one GEMM over the concatenated parameters (``torch.cat`` carries their gradients)."""
        n, dim = gammas.shape[0], self.inner_channel * 4
        f32 = dict(dtype=torch.float32, device=gammas.device)
        e = torch.empty(n, self.inner_channel, **f32)
        ops.gamma_embedding(gammas, n, self.inner_channel, e)
        k = self._train_consts
        if k is None or k[0].device != gammas.device:
            k = self._train_consts = (torch.ones(dim, **f32), torch.zeros(dim, **f32))
        for lin in (self.cond_embed[0], self.cond_embed[2]):
            e = nnops.SiLU.apply(nnops.Linear.apply(e, lin.weight, lin.bias), *k)
        blocks = [m for m in self.modules() if isinstance(m, ResBlock)]
        w = torch.cat([b.emb_layers[1].weight for b in blocks], 0)
        bias = torch.cat([b.emb_layers[1].bias for b in blocks], 0)
        emb_all = nnops.ToStorage.apply(nnops.Linear.apply(e, w, bias), dtype)
        parts = nnops.SplitCols.apply(emb_all, tuple(2 * b.out_channel for b in blocks))
        return {id(b): t for b, t in zip(blocks, parts)}

    def forward_train(self, x, y, gammas, dropout_masks=None, dropout_rng=None):
        """The train-mode pass: x, y fp32 [N x C x H x W] (read as cat([x, y])) and gammas fp32 [N] on the device ->
        fp32 [N x out_channel x H x W], connected by autograd to every parameter (not to the inputs).  Every BatchNorm
        normalises with batch statistics and advances its running buffers as the reference does in one forward + backward:
        once in the forward, the AttentionBlock norms once more in the backward.  ``dropout_masks``: optional dict from a
        ResBlock's prefix below this module (``"input_blocks.1.0"``) to a uint8 NHWC mask of its ``out_layers`` dropout (0
        drops); a block without an entry draws its own when ``dropout`` > 0.  ``dropout_rng = (seed, step)``: the blocks
        without an entry form their keep bits inside the norm kernels instead (the device generator of csrc/philox.h; the
        i-th ResBlock in ``modules()`` order has the stream 16 + i), so that no mask tensor exists and torch's generator is
        not touched.  No host synchronisation."""
        if not self.training:
            raise PaiError("UNet.forward_train is the training pass: call train() first (eval mode samples through forward)")
        if not (x.is_cuda and y.is_cuda and gammas.is_cuda):
            raise PaiError("UNet (HIP) needs HIP device tensors; there is no CPU path")
        if x.dim() != 4 or x.shape != y.shape or 2 * x.shape[1] != self.in_channel:
            raise PaiError(f"UNet.forward_train takes x and y of one [N, {self.in_channel // 2}, H, W] shape")
        dtype = self.compute_dtype
        # the running statistics advance through raw pointers: their version counters do not move, so the eval coefficients
        # cached by prepared() would go stale -- dropped now, and again when the backward pass starts (it advances the
        # attention norms once more)
        self._cache = None
        ref = weakref.ref(self)

        def invalidate(_grad):
            me = ref()
            if me is not None:
                me._cache = None

        g = gammas.reshape(-1).float().contiguous()
        if g.shape[0] != x.shape[0]:
            raise PaiError(f"UNet.forward_train: {g.shape[0]} gammas for a batch of {x.shape[0]}")
        rng = {}
        if dropout_rng is not None:
            seed, step = dropout_rng
            blocks = [m for m in self.modules() if isinstance(m, ResBlock)]
            rng = {id(b): (seed, STREAM_DROPOUT + i, step) for i, b in enumerate(blocks)}
        ctx = _TrainRun(dtype, self._embed_train(g, dtype), dict(dropout_masks or {}), self.debug_capture, rng)
        h, hs = nnops.to_nhwc(torch.cat([x, y], dim=1), dtype), []
        for i, blk in enumerate(self.input_blocks):
            h = blk.run_train(h, None, ctx, f"input_blocks.{i}")
            h, skip = nnops.Fork.apply(h)                # the next block and the decoder
            hs.append(skip)
        h = self.middle_block.run_train(h, None, ctx, "middle_block")
        for i, blk in enumerate(self.output_blocks):
            h = blk.run_train(h, hs.pop(), ctx, f"output_blocks.{i}")
        out = nnops.FromStorage.apply(ctx.conv(self.out[2], ctx.norm(self.out[0], h)))
        out.register_hook(invalidate)
        n, hh, ww, co = out.shape
        return out.reshape(n, 1, hh, ww) if co == 1 else out.permute(0, 3, 1, 2)

    def macs(self, height: int, width: int) -> int:
        """Multiply-accumulates of one forward pass on one ``height`` x ``width`` image: every convolution at the
        resolution it runs at, the Linear layers of the embedding path and the two products of every attention block."""
        total = sum(m.weight.numel() for m in self.modules() if isinstance(m, nn.Linear))

        def block(seq, px):
            t = 0
            for layer in seq:
                if isinstance(layer, ResBlock):
                    if isinstance(layer.h_upd, Upsample):
                        px *= 4
                    elif isinstance(layer.h_upd, Downsample):
                        px //= 4
                    t += px * sum(m.weight.numel() for m in layer.modules() if isinstance(m, nn.Conv2d))
                elif isinstance(layer, AttentionBlock):
                    t += px * (layer.qkv.weight.numel() + layer.proj_out.weight.numel()) + 2 * px * px * layer.channels
                else:
                    t += px * layer.weight.numel()
            return t, px

        px = height * width
        for seq in list(self.input_blocks) + [self.middle_block] + list(self.output_blocks):
            t, px = block(seq, px)
            total += t
        return total + px * self.out[2].weight.numel()

    def forward(self, x, y, gammas):
        if not x.is_cuda or not y.is_cuda:
            raise PaiError("UNet (HIP) needs HIP device tensors; there is no CPU path")
        dtype = self.compute_dtype
        out = self.run(nnops.to_nhwc(torch.cat([x, y], dim=1), dtype), gammas.to(x.device))
        n, hh, ww, co = out.shape
        o32 = out
        if dtype != torch.float32:
            o32 = torch.empty(out.shape, dtype=torch.float32, device=out.device)
            ops.cast(out, o32)
        return o32.reshape(n, 1, hh, ww) if co == 1 else o32.permute(0, 3, 1, 2)
