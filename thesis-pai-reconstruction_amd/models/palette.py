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


class DeviceRNG:
    """The state of the device generator (csrc/philox.h): a 64-bit ``seed`` and a ``step`` counter, two Python integers.  Every
    random value of a Palette step is a pure function of (seed, step, site, element index), so a run resumes reproducibly
    from ``state_dict()``.  ``step`` is the training step or the index of the sampling call: each consumer calls ``advance()``
    once per call.  Nothing here lives on the device, and nothing is read back from it."""

    def __init__(self, seed: int = 0, step: int = 0):
        self.seed, self.step = self._check(seed, 64, "seed"), self._check(step, 32, "step")

    @staticmethod
    def _check(v, bits, what):
        v = int(v)
        if not 0 <= v < 1 << bits:
            raise PaiError(f"DeviceRNG: {what}={v} is not an unsigned {bits}-bit integer")
        return v

    def advance(self, n: int = 1) -> int:
        """The step the next call uses; the counter is 32 bits wide and wraps."""
        self.step = (self.step + int(n)) & 0xFFFFFFFF
        return self.step

    def state_dict(self) -> dict:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state) -> None:
        self.seed, self.step = self._check(state["seed"], 64, "seed"), self._check(state["step"], 32, "step")

    def __repr__(self):
        return f"DeviceRNG(seed={self.seed}, step={self.step})"


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
