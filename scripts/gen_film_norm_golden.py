"""Generate tests/golden/ref_film_norm.npz by running the REAL reference ResBlock (models/guided_diffusion/unet.py:105-214) on
the CPU in training mode, forward and ``torch.autograd.grad``, in fp64.

Build container only (it needs the reference checkout):

    python scripts/gen_film_norm_golden.py

The reference is imported from its checkout with the stand-in packages of oracle/shims ahead of it on sys.path, as
scripts/gen_palette_golden.py does.  Only data is written (inputs, outputs, recorded figures); no reference source is copied.

One block: ``ResBlock(16, 32, dropout=0, use_scale_shift_norm=True)``, N = 3, 5 x 5 positions.  Hooks on ``out_layers[0]`` (the
BatchNorm; its input is the norm's input) and ``out_layers[1]`` (the SiLU; its output is the site's output) and on
``emb_layers`` (its output is emb_out = scale | shift) take the tensors of the graph; ``autograd.grad`` of the SiLU output with a
seeded ``dout`` gives the gradients of the norm's input, emb_out, gamma and beta.  Recorded, NHWC ([N, rows, C], rows = 25):
``shape`` (N, rows, C), ``x`` (the norm's input), ``emb_out`` [N, 2 C], ``gamma``, ``beta``, ``y`` (the SiLU output), ``dout``,
``dx``, ``demb``, ``dgamma``, ``dbeta`` (all fp64), ``running_mean`` / ``running_var`` after the step (from zeros / ones,
momentum 0.1) and ``eps``.  The block's parameters are seeded normal draws (gamma and beta of the norm too: the defaults 1 / 0
would hide them), and x, emb_out and dout are NOT bf16-representable: the tests round them as they need.
``bf16_dev_<k>`` for k in y, dx, demb, dgamma, dbeta: the relative L2 distance from the fp64 result of the same site run by
the reference's own modules (out_layers[0], the FiLM expression of ResBlock._forward, out_layers[1]) under bf16 autocast on the
bf16-rounded x / emb_out / dout.

TEST INFRASTRUCTURE ONLY.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("PAI_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "shims"))
sys.path.insert(0, ROOT)

from models.guided_diffusion.nn import normalization2d  # noqa: E402  (the reference's)
from models.guided_diffusion.unet import ResBlock       # noqa: E402  (the reference's)
from oracle import golden                              # noqa: E402

N, H, W, C, EMB = 3, 5, 5, 16, 32


class AsDouble:
    """fp64 run of the reference: its explicit ``.float()`` / ``.type(torch.float32)`` casts become double."""

    def __enter__(self):
        self.f, self.t = torch.Tensor.float, torch.Tensor.type
        t = self.t
        torch.Tensor.float = lambda s, *a, **k: s.double()
        torch.Tensor.type = lambda s, dtype=None, *a, **k: t(s, torch.float64 if dtype == torch.float32 else dtype, *a, **k)

    def __exit__(self, *exc):
        torch.Tensor.float, torch.Tensor.type = self.f, self.t
        return False


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).contiguous()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def generate():
    gen = torch.Generator().manual_seed(139)
    block = ResBlock(C, EMB, 0.0, use_scale_shift_norm=True).double()
    with torch.no_grad():
        for p in block.parameters():
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.5 if p.dim() == 1 else 0.15))
        block.out_layers[0].weight.add_(1.0)
    block.train()
    x_in = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64) * 1.5 + 0.5
    emb = torch.randn(N, EMB, generator=gen, dtype=torch.float64)
    dout = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    got = {}
    hooks = [block.out_layers[0].register_forward_pre_hook(lambda m, i: got.__setitem__("x", i[0])),
             block.out_layers[1].register_forward_hook(lambda m, i, o: got.__setitem__("y", o)),
             block.emb_layers.register_forward_hook(lambda m, i, o: got.__setitem__("emb_out", o))]
    with AsDouble():
        block(x_in, emb)
        bn = block.out_layers[0]
        assert got["x"].dtype == torch.float64 and got["y"].dtype == torch.float64
        dx, demb, dgamma, dbeta = torch.autograd.grad(got["y"], [got["x"], got["emb_out"], bn.weight, bn.bias], dout)
    for h in hooks:
        h.remove()
    assert int(bn.num_batches_tracked) == 1
    rec = {"shape": np.array([N, H * W, C]), "eps": np.array(bn.eps), "momentum": np.array(bn.momentum),
           "x": nhwc(got["x"]).numpy(), "emb_out": got["emb_out"].detach().numpy(), "gamma": bn.weight.detach().numpy(),
           "beta": bn.bias.detach().numpy(), "y": nhwc(got["y"]).numpy(), "dout": nhwc(dout).numpy(), "dx": nhwc(dx).numpy(),
           "demb": demb.numpy(), "dgamma": dgamma.numpy(), "dbeta": dbeta.numpy(),
           "running_mean": bn.running_mean.detach().numpy(), "running_var": bn.running_var.detach().numpy()}

    # the reference's own bf16-autocast deviation of this site: its modules on the bf16-rounded tensors, parameters fp32
    norm32, silu = normalization2d(C).train(), block.out_layers[1]
    with torch.no_grad():
        norm32.weight.copy_(bn.weight)
        norm32.bias.copy_(bn.bias)
    xb = got["x"].detach().bfloat16().requires_grad_(True)
    eb = got["emb_out"].detach().bfloat16().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        e4 = eb[..., None, None]
        scale, shift = torch.chunk(e4, 2, dim=1)
        yb = silu(norm32(xb) * (1 + scale) + shift)
    gb = torch.autograd.grad(yb, [xb, eb, norm32.weight, norm32.bias], dout.to(yb.dtype))
    for k, a, b in (("y", yb, got["y"]), ("dx", gb[0], dx), ("demb", gb[1], demb), ("dgamma", gb[2], dgamma),
                    ("dbeta", gb[3], dbeta)):
        rec[f"bf16_dev_{k}"] = np.array(rel_l2(a.detach(), b.detach()))
        print(f"{k}: |ref| max {float(b.detach().abs().max()):.3f} bf16_dev {float(rec[f'bf16_dev_{k}']):.3e}")
    golden.save(OUT, "ref_film_norm", rec)
    print("bytes", os.path.getsize(os.path.join(OUT, "ref_film_norm.npz")))


if __name__ == "__main__":
    generate()
