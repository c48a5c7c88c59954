"""Palette image-to-image diffusion model (reference models/palette.py:17-345): sampling on the MI355X kernels.

Same module tree and state-dict keys as the reference (``unet.*``, ``diffusion.{alphas,gammas,gammas_prev}``,
``diffusion_inf.*``), so a checkpoint trained by the reference loads.  Built here: ``forward`` (the reverse process of
``diffusion_inf``: one eval-mode U-Net call and one ``pai_palette_step`` launch per step) and ``validation_step``.
Training runs through names of its own beside the refusals: ``training_loss`` (the forward noising, ``unet.forward_train`` and
the MSE + variational-bound objective, the latter two kernels of csrc/palette.hip), ``make_optimizers`` (the reference's Adam
and LinearLR values) and ``fit_step``.  ``training_step`` / ``configure_optimizers`` still raise: the Lightning loop of
main.py is not wired to them; scripts/train_palette.py is the loop.

The sample chain stays fp32 in both precisions, as NHWC pixels; the U-Net reads ``[x | y_t]`` in the storage dtype from
one tensor whose y half the step kernel rewrites.  The six scalars of each step come from a table built once on the
host from the fp32 schedule buffers in the reference's expression order; the loop copies nothing back to the host.

``sampler_plan`` (opt-in; PAI_PALETTE_PLAN=1) replays the reverse step from a recorded launch plan instead of issuing its ~400
launches from Python at every step: see "the planned sampler" below and DESIGN.md 7c.

Reference behaviour kept on purpose: the sampler adds noise while ``t > 1`` (palette.py:250), not ``t > 0``.
"""
import os
from typing import Literal

import torch
import torch.nn as nn

from .. import functional as PF
from .. import nnops, ops
from ..lightning import LightningModule
from ..ops import PaiError
from ..rng import DeviceRNG  # noqa: F401  (the class lived here first; pai.DeviceRNG and this name stay the same class)
from .guided_diffusion.unet import UNet
from .utils import denormalize, to_int


def cosine_beta_schedule(timesteps: int, s: float = 0.008) -> torch.Tensor:
    """Cosine schedule (Nichol and Dhariwal, 2021), reference palette.py:348-357."""
    t = torch.linspace(0, timesteps, timesteps + 1)
    g = torch.cos((torch.pi / 2) * ((t / timesteps) + s) / (1 + s))
    g = g / g[0]
    return torch.clamp(1 - (g[1:] / g[:-1]), 0.0001, 0.9999)


def linear_beta_schedule(timesteps: int, start: float = 1e-6, end: float = 0.01) -> torch.Tensor:
    return torch.linspace(start, end, timesteps)


class DiffusionModel(nn.Module):
    """Noise schedule buffers and the per-step scalars of the reverse process (reference palette.py:177-306)."""

    def __init__(self, schedule_type: Literal["linear", "cosine"], timesteps: int, start: float = 1e-6, end: float = 0.01,
                 learn_var: bool = False, device="cpu"):
        super().__init__()
        self.timesteps, self.learn_var = timesteps, learn_var
        if schedule_type == "linear":
            betas = linear_beta_schedule(timesteps, start, end)
        elif schedule_type == "cosine":
            betas = cosine_beta_schedule(timesteps)
        else:
            raise ValueError(f"{schedule_type} is not supported.")
        betas = betas.to(device)
        self.register_buffer("alphas", 1 - betas)
        self.register_buffer("gammas", torch.cumprod(self.alphas, axis=0))
        self.register_buffer("gammas_prev", torch.cat([torch.ones((1,), device=self.gammas.device), self.gammas[:-1]]))
        self._table = None
        self._table_dev = None

    def _versions(self):
        return tuple(b._version for b in (self.alphas, self.gammas, self.gammas_prev))

    def _apply(self, fn, *args, **kwargs):
        # a move to another device replaces the buffers (their version counters restart) without changing their values
        out = super()._apply(fn, *args, **kwargs)
        if self._table is not None:
            self._table = (self._versions(), self._table[1])
        self._table_dev = None
        return out

    def step_table(self):
        """[timesteps][6] Python floats: sqrt(1 - gamma), 1 / sqrt(gamma), the coefficients of y0 and y_t in the posterior
        mean, log(var_lower), log(var_upper) -- fp32 arithmetic in the expression order of reference palette.py:271-306.
        Built from host copies of the buffers, once per value of the buffers."""
        if self._table is None or self._table[0] != self._versions():
            a, g, gp = (b.detach().to("cpu", torch.float32) for b in (self.alphas, self.gammas, self.gammas_prev))
            lower = torch.clamp((1 - a) * (1 - gp) / (1 - g), min=1e-20)
            cols = [torch.sqrt(1 - g), 1 / torch.sqrt(g), torch.sqrt(gp) * (1 - a) / (1 - g),
                    torch.sqrt(a) * (1 - gp) / (1 - g), torch.log(lower), torch.log(1 - a)]
            self._table = (self._versions(), [tuple(float(v) for v in row) for row in torch.stack(cols, 1)])
        return self._table[1]

    def step_table_device(self, device):
        """``step_table()`` as an fp32 [timesteps][6] tensor on ``device``: uploaded once per value of the buffers, so that the
        training objective gathers the row of every sample's t on the device."""
        d = self._table_dev
        if d is None or d[0] != self._versions() or d[1].device != torch.device(device):
            t = torch.tensor(self.step_table(), dtype=torch.float32).to(device)
            d = self._table_dev = (self._versions(), t)
        return d[1]


def sampler_plan_default() -> bool:
    """PAI_PALETTE_PLAN=1 makes the planned sampler the default of every Palette constructed afterwards (A/B of report.py
    and of validation without a command-line change)."""
    return os.environ.get("PAI_PALETTE_PLAN", "0") not in ("", "0")


class _StepPlan:
    """What one recorded reverse step owns: the static buffers its launches read and write, the plan, and everything the plan's
    frozen pointers need alive (the pass's activations, the weight cache)."""
    __slots__ = ("sig", "cache", "xy", "y", "gamma_next", "pos", "noise_stack", "warmed", "plan", "keep", "consts")


class _SamplerPlans:
    """The plans of one Palette, most recently used last, and the counters of ``sampler_plan_info``."""
    MAX_PLANS = 4           # each one pins one U-Net pass of activations

    def __init__(self):
        from collections import OrderedDict
        self.plans = OrderedDict()
        self.records = self.replays = 0
        self.disabled = None            # why calls run eagerly; ``sticky``: for good (a kernel the recorder cannot own)
        self.sticky = False
        self.launches_per_step = None

    def __deepcopy__(self, memo):       # a copied model records its own plans
        return _SamplerPlans()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self.__init__()


class Palette(LightningModule):
    """Palette image-to-image diffusion model.

    :param in_channels: Input channels.
    :param out_channels: Output channels.
    :param channel_mults: Channel multipliers for each level of the U-net.
    :param attention_res: Downsample rates at which attention blocks are added after the residual blocks.
    :param dropout: Dropout percentage (training only; sampling runs in eval mode).
    :param schedule_type: Noise schedule type of the training process. Either cosine or linear.
    :param learn_var: The U-Net also predicts the variance interpolation.
    :param inference_steps: Steps of the reverse process (build-only; the reference fixes 100).
    """

    def __init__(self, in_channels: int = 3, out_channels: int = 3, channel_mults=(1, 1, 2, 2, 4, 4), attention_res=(16, 8),
                 dropout: float = 0.1, schedule_type: Literal["linear", "cosine"] = "linear", learn_var: bool = False,
                 inference_steps: int = 100):
        super().__init__()
        self.save_hyperparameters()
        self.in_channels, self.out_channels, self.learn_var = in_channels, out_channels, learn_var
        self.noise_fn = None        # tests: fn(index, shape) -> fp32 noise; index 0 is y_T, index k the k-th reverse step
        # a DeviceRNG: every draw of training_loss / forward is formed inside the kernels (csrc/philox.h), torch's generator is
        # not touched.  None (the default): torch draws, as before.  draws= and noise_fn take precedence where given.
        self.device_rng = None
        # the planned sampler (``_forward_planned``): opt-in; PAI_PALETTE_PLAN=1 sets the default of new objects
        self.sampler_plan = sampler_plan_default()
        self._splan = _SamplerPlans()
        self.unet = UNet(image_size=256, in_channel=in_channels * 2,
                         out_channel=out_channels * 2 if learn_var else out_channels, res_blocks=2, inner_channel=128,
                         channel_mults=tuple(channel_mults), attn_res=tuple(attention_res), num_heads=4, dropout=dropout,
                         conv_resample=True)
        self.diffusion = DiffusionModel(schedule_type, 2000, 1e-6, 0.01, learn_var=learn_var)
        self.diffusion_inf = DiffusionModel("cosine", int(inference_steps), learn_var=learn_var)

    def _noise(self, index, shape, device):
        """fp32 NHWC pixels [N * H * W, C] of one standard normal draw of NCHW ``shape``."""
        if self.noise_fn is not None:
            z = self.noise_fn(index, shape).to(device=device, dtype=torch.float32).reshape(shape)
        else:
            z = torch.randn(shape, dtype=torch.float32, device=device)
        n, c, h, w = shape
        return z.reshape(n * h * w, 1) if c == 1 else z.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()

    def forward(self, x, output_process=False):
        """:input: [N x C x H x W] condition   :output: [N x C x H x W] sample (fp32); with ``output_process`` also
        [N x K x C x H x W]: y_T and the chain at every (steps // 7)-th step."""
        if not x.is_cuda:
            raise PaiError("Palette (HIP) needs a HIP device tensor; there is no CPU path")
        if self.in_channels != self.out_channels:
            raise PaiError("Palette samples y with the shape of x: in_channels and out_channels must agree")
        n, c, h, w = x.shape
        dev, dt = x.device, self.unet.compute_dtype
        inf = self.diffusion_inf
        steps, table = inf.timesteps, inf.step_table()
        if self.unet.training:
            raise PaiError("Palette.forward samples in eval mode: call eval() / freeze() first")
        if self.sampler_plan:
            mode = self._plan_mode()
            if mode is not None:
                return self._forward_planned(x, output_process, mode)
        cache = self.unet.prepared(dt)
        gammas = inf.gammas.to(dev).reshape(steps, 1).expand(steps, n).contiguous()      # row i: the U-Net's gammas of step i

        def nchw(pixels):
            return pixels.reshape(n, 1, h, w).clone() if c == 1 else pixels.reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()

        rng = self.device_rng if self.noise_fn is None else None
        if rng is not None:             # y_T: draw 0 of this sampling call, NHWC pixels as the step kernel numbers them
            y = PF.philox_fill("normal", (n * h * w, c), rng.seed, 0, ops.STREAM_SAMPLER, rng.step, device=dev)
        else:
            y = self._noise(0, (n, c, h, w), dev)
        process = [nchw(y)] if output_process else None
        xy = nnops.to_nhwc(torch.cat([x.to(torch.float32), nchw(y)], dim=1), dt)        # [N, H, W, 2C]: x | y_T
        every = max(steps // 7, 1)
        for k, i in enumerate(reversed(range(steps)), 1):
            eps = self.unet.run(xy, gammas[i], cache)
            if rng is not None:
                ops.palette_step_rng(dt, eps, y, n * h * w, c, self.learn_var, i > 1, table[i], rng.seed, k, rng.step, y, xy)
            else:
                z = self._noise(k, (n, c, h, w), dev)
                ops.palette_step(dt, eps, y, z, n * h * w, c, self.learn_var, i > 1, table[i], y, xy)
            if output_process and i % every == 0:
                process.append(nchw(y))
        out = nchw(y)
        if rng is not None:
            rng.advance()
        if output_process:
            return out, torch.stack(process, dim=1)
        return out

    # ---- the planned sampler ---------------------------------------------------------------------------------------------
    # One reverse step -- the U-Net pass, the step kernel, the advance of the step index: ~400 launches -- is recorded once
    # into a launch plan (ops.Plan, csrc/plan.h) and replayed from one C call for the other steps of the chain and for every
    # step of later calls.  What changes from step to step is on the device: the U-Net reads a fixed ``xy`` and a fixed
    # ``gamma_next``; the step kernel (pai_palette_step_dev / _rng_dev) takes its scalars, its noise and the next pass's
    # gamma from the step index ``pos``, and the generator's step from DeviceRNG's device mirror.  Per call, outside the plan:
    # x | y_T into ``xy``, the first gamma, pos = 1, and the final layout change.  Same kernels, same arithmetic, same stream
    # as the eager loop: the same bits.
    def _plan_mode(self):
        """"noise" | "rng" when this call can run from a plan, None (with the reason in ``sampler_plan_info()``) otherwise."""
        st = self._splan
        if st.sticky:
            return None
        if ops.PROFILE is not None or ops.PROFILE_HBM is not None:
            st.disabled = "per-launch event profiling is on"
        elif self.unet.debug_capture is not None:
            st.disabled = "the U-Net's debug capture is on (torch kernels inside the pass)"
        elif self.noise_fn is not None:
            st.disabled = None
            return "noise"
        elif self.device_rng is not None:
            st.disabled = None
            return "rng"
        else:
            st.disabled = ("torch draws the noise (neither device_rng nor noise_fn is set): torch.randn per step is a kernel "
                           "the plan cannot own")
        return None

    def _plan_sig(self, shape, dt, dev, mode, cache, table, gammas):
        h = ops.handle_for(dev)
        rng = self.device_rng if mode == "rng" else None
        return (tuple(shape), dt, dev.index, ops._stream(), bool(self.learn_var), int(table.shape[0]), mode, id(cache),
                tuple(t.data_ptr() if t is not None else 0 for t in (h.workspace, h.scratch)), table.data_ptr(),
                gammas.data_ptr(), None if rng is None else (rng.seed, rng.device_step(dev).data_ptr()),
                ops.is_deterministic())      # a plan replays the launches of the mode it was recorded in

    def _plan_step(self, rec, dt, n, npx, c, table, gammas, mode, dev):
        """One reverse step on the static buffers of ``rec``: what is recorded, and what runs un-recorded before that."""
        eps = self.unet.run(rec.xy, rec.gamma_next, rec.cache)
        if mode == "rng":
            rng = self.device_rng
            ops.palette_step_rng_dev(dt, eps, rec.y, npx, c, self.learn_var, table, rec.pos, gammas, n, rec.gamma_next, rng.seed,
                                     rng.device_step(dev), rec.y, rec.xy)
        else:
            ops.palette_step_dev(dt, eps, rec.y, rec.noise_stack, npx, c, self.learn_var, table, rec.pos, gammas, n, rec.gamma_next,
                                 rec.y, rec.xy)
        ops.counter_add(rec.pos, 1)

    def _plan_record(self, rec, *step_args):
        """Run one step while it is recorded.  False: the recorder saw a kernel of torch's own, the sampler stays eager."""
        from ..plan import _Recorder
        st = self._splan
        recorder = _Recorder()
        with recorder:
            recorder.begin()
            try:
                self._plan_step(rec, *step_args)
            finally:
                recorder.end()
        st.records += 1
        if recorder.foreign or len(recorder.items) != 1:
            kinds = sorted(set(recorder.foreign))
            st.disabled = ("the reverse step launches kernels outside the C ABI (" + ", ".join(kinds[:8]) +
                           (", ..." if len(kinds) > 8 else "") + "): it cannot be replayed from a plan") if kinds else \
                "the recorded step is not one plan segment"
            st.sticky = True
            st.plans.clear()
            return False
        rec.plan, rec.keep = recorder.items[0][1], recorder.keep
        st.launches_per_step = rec.plan.info()["launches"]
        return True

    def _forward_planned(self, x, output_process, mode):
        st = self._splan
        n, c, h, w = x.shape
        dev, dt = x.device, self.unet.compute_dtype
        inf = self.diffusion_inf
        steps, npx = inf.timesteps, n * h * w
        f32 = dict(dtype=torch.float32, device=dev)
        cache = self.unet.prepared(dt)
        table = inf.step_table_device(dev)
        gammas = inf.gammas.detach().to(**f32).contiguous()
        for k in [k for k, r in st.plans.items() if r.cache is not cache]:       # plans of an earlier weight generation
            del st.plans[k]
        args = ((n, c, h, w), dt, dev, mode, cache, table, gammas)
        sig = self._plan_sig(*args)
        rec = st.plans.get(sig)
        if rec is None:
            while len(st.plans) >= st.MAX_PLANS:
                st.plans.popitem(last=False)                                      # the least recently used one
            rec = st.plans[sig] = _StepPlan()
            rec.sig, rec.cache, rec.warmed, rec.plan, rec.keep = sig, cache, False, None, None
            rec.consts = (table, gammas)            # the plan's launches hold their addresses
            rec.xy = torch.empty(n, h, w, 2 * c, dtype=dt, device=dev)
            rec.y, rec.gamma_next = torch.empty(npx, c, **f32), torch.empty(n, **f32)
            rec.pos = torch.empty(1, dtype=torch.int32, device=dev)
            rec.noise_stack = torch.empty(steps + 1, npx * c, **f32) if mode == "noise" else None
        else:
            st.plans.move_to_end(sig)

        def nchw(pixels):           # always a copy: rec.y is rewritten by the next call
            if c == 1:
                return pixels.reshape(n, 1, h, w).clone()
            return pixels.reshape(n, h, w, c).permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format)

        rng = self.device_rng if mode == "rng" else None
        if rng is not None:         # y_T: draw 0 of this sampling call, the step read from the generator's device mirror
            ops.philox_fill_dev(ops.PHILOX_NORMAL, rec.y, rng.seed, 0, ops.STREAM_SAMPLER, rng.device_step(dev))
        else:                       # tests and fixtures: the 1 + steps draws of noise_fn, stacked once per call
            rec.noise_stack.copy_(torch.stack([self._noise(k, (n, c, h, w), dev).reshape(-1) for k in range(steps + 1)]))
            rec.y.copy_(rec.noise_stack[0].reshape(npx, c))
        process = [nchw(rec.y)] if output_process else None
        rec.xy.copy_(nnops.to_nhwc(torch.cat([x.to(torch.float32), nchw(rec.y)], dim=1), dt))
        rec.gamma_next.copy_(gammas[steps - 1].expand(n))
        ops.counter_set(rec.pos, 1)
        step_args = (dt, n, npx, c, table, gammas, mode, dev)
        every = max(steps // 7, 1)
        for i in reversed(range(steps)):
            if rec.plan is not None:
                rec.plan.run()
                st.replays += 1
            elif not rec.warmed or st.sticky:
                # the first step at this signature creates descriptors and may grow the workspace: it is not recorded
                self._plan_step(rec, *step_args)
                rec.warmed = True
            else:
                now = self._plan_sig(*args)
                if now != sig:                                                     # the warm-up step grew a registered buffer
                    st.plans[now] = st.plans.pop(sig)
                    sig = rec.sig = now
                self._plan_record(rec, *step_args)
            if output_process and i % every == 0:
                process.append(nchw(rec.y))
        out = nchw(rec.y)
        if rng is not None:
            rng.advance()
        if output_process:
            return out, torch.stack(process, dim=1)
        return out

    def sampler_plan_info(self) -> dict:
        """The state of the planned sampler, in the spirit of ``PlannedStep.describe()``: ``disabled`` is None while calls run
        from plans, otherwise the reason why they run eagerly."""
        st = self._splan
        return {"plans": sum(1 for r in st.plans.values() if r.plan is not None), "records": st.records, "replays": st.replays,
                "disabled": st.disabled, "launches_per_step": st.launches_per_step}

    def configure_optimizers(self):
        raise NotImplementedError("Palette under the Lightning loop is sampling only; train with make_optimizers() / fit_step() "
                                  "(scripts/train_palette.py)")

    def training_step(self, batch, batch_idx=0):
        raise NotImplementedError("Palette under the Lightning loop is sampling only; train with training_loss() / fit_step() "
                                  "(scripts/train_palette.py)")

    # ---- training (reference models/palette.py:102-140) ---------------------------------------------------------------------
    def training_loss(self, batch, draws=None):
        """The loss of one batch ``(x, y_0)`` (fp32 [N x C x H x W] on the device), connected by autograd to the U-Net's
        parameters: t ~ randint(0, timesteps), the forward noising, ``unet.forward_train(x, y_t, gamma)`` and the MSE +
        variational-bound objective.  ``draws = (t, z, u)`` (int [N], fp32 like y_0, fp32 [N]; device tensors) replaces the three
        draws -- tests, as ``noise_fn`` for the sampler.  With ``device_rng`` set (and no ``draws``) the three draws and every
        dropout site come from the device generator at (seed, step), and ``step`` advances once per call.  Logs ``mse_loss``,
        ``vlb_loss`` and ``loss``.  No host synchronisation."""
        x, y_0 = batch
        if not self.training or not self.unet.training:
            raise PaiError("Palette.training_loss runs in train mode: call train() first")
        if not (torch.is_tensor(x) and torch.is_tensor(y_0) and x.is_cuda and y_0.is_cuda):
            raise PaiError("Palette (HIP) needs HIP device tensors; there is no CPU path")
        n, dev = y_0.shape[0], y_0.device
        rng = self.device_rng if draws is None else None
        if rng is not None:
            y_t, noise, gamma, t = PF.palette_noise_rng(y_0, rng.seed, rng.step, self.diffusion)
            model_out = self.unet.forward_train(x, y_t, gamma, dropout_rng=(rng.seed, rng.step))
            rng.advance()
        else:
            if draws is None:
                t = torch.randint(0, self.diffusion.timesteps, (n,), device=dev)
                z = torch.randn(y_0.shape, dtype=torch.float32, device=dev)
                u = torch.rand(n, dtype=torch.float32, device=dev)
            else:
                t, z, u = draws
            y_t, noise, gamma = PF.palette_noise(y_0, t, u, z, self.diffusion)
            model_out = self.unet.forward_train(x, y_t, gamma)
        loss, mse, vlb, _ = PF.palette_objective(model_out, noise, y_0, y_t, t, self.diffusion, self.learn_var)
        self.log("mse_loss", mse, prog_bar=True)
        self.log("vlb_loss", vlb, prog_bar=True)
        self.log("loss", loss, prog_bar=True)
        return loss

    def make_optimizers(self):
        """The reference's ``configure_optimizers`` values: Adam(lr = 1e-4) on the U-Net, as the fused ``optim.MultiAdam``, and
        LinearLR over 10000 steps (factor 1/3 -> 1)."""
        from ..optim import MultiAdam
        opt = MultiAdam(self.unet.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
        return [opt], [torch.optim.lr_scheduler.LinearLR(opt, total_iters=10000)]

    def fit_step(self, batch, optimizer, scheduler=None, draws=None):
        """One optimisation step: zero_grad, ``training_loss``, backward, ``optimizer.step``, ``scheduler.step``.  Returns the
        loss as a device scalar; after a first (warm-up) step nothing here copies to the host or synchronises."""
        optimizer.zero_grad(set_to_none=True)
        loss = self.training_loss(batch, draws)
        loss.backward()
        nnops.join_wgrads()
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        return loss.detach()

    def _epoch_dir(self):
        tr = self.trainer
        log_dir = getattr(getattr(tr, "logger", None), "log_dir", None) if tr is not None else None
        if log_dir is None:
            return None
        d = os.path.join(log_dir, str(getattr(tr, "current_epoch", 0) + 1))
        os.makedirs(d, exist_ok=True)
        return d

    def validation_step(self, batch, batch_idx):
        """Reference models/palette.py:152-174: sample, write the images, log SSIM / PSNR / RMSE of the denormalised pair."""
        x, y_0 = batch
        y_pred = self.forward(x)
        out_dir = self._epoch_dir()
        if out_dir is not None:
            from PIL import Image
            imgs = to_int(denormalize(y_pred)).cpu().numpy()
            for ind, a in enumerate(imgs):
                Image.fromarray(a[0] if a.shape[0] == 1 else a.transpose(1, 2, 0)).save(
                    os.path.join(out_dir, f"output_{x.shape[0] * batch_idx + ind}.png"), compress_level=0)
        s, p, r = PF.metrics_of_normalized(y_pred, y_0)
        self.log("val_ssim", s, prog_bar=True)
        self.log("val_psnr", p, prog_bar=True)
        self.log("val_rmse", r, prog_bar=True)
