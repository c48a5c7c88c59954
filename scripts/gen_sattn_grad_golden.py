"""Generate tests/golden/ref_sattn_grad.npz by running the REAL reference QKVAttentionLegacy (models/guided_diffusion/unet.py:
265-297) on the CPU, forward and ``torch.autograd.grad``, in fp64.

Build container only (it needs the reference checkout):

    python scripts/gen_sattn_grad_golden.py

The reference is imported from its checkout with the stand-in packages of oracle/shims ahead of it on sys.path, as
scripts/gen_palette_golden.py does.  Only data is written (inputs, outputs, recorded figures); no reference source is copied.

Per case c = 0, 1, 2 with (N, T, heads, ch) = (1, 20, 2, 32), (2, 144, 4, 32), (1, 96, 1, 64): ``shape{c}``, and in this
project's layouts (qkv [N][T][heads * 3 * ch], out / dout [N][T][heads * ch] -- the reference's tensors transposed)
``qkv{c}`` and ``dout{c}`` (fp32, bf16-representable values, seeded, qkv of scale 2.0 as in tests/test_gpu_palette_ops.py),
``out{c}`` (the fp64 result stored as fp32: the tests recompute it exactly), ``dqkv{c}`` (fp64) and ``bf16_dev{c}``: the
relative L2 distance of the reference's own dqkv computed with bf16 tensors on the CPU (the same module, the same
autograd.grad call) from its fp64 dqkv.  The module's ``weight.float()`` becomes ``.double()`` in the fp64 run (AsDouble of
scripts/gen_palette_golden.py).  The fp64 dqkv of the second case alone is 0.85 MB: oracle/golden.py splits the fixture into
part files under the size limit of a committed file.

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

from models.guided_diffusion.unet import QKVAttentionLegacy    # noqa: E402  (the reference's)
from oracle import golden                                       # noqa: E402

CASES = [(1, 20, 2, 32), (2, 144, 4, 32), (1, 96, 1, 64)]


class AsDouble:
    """fp64 run of the reference: its explicit ``.float()`` becomes double."""

    def __enter__(self):
        self.f = torch.Tensor.float
        torch.Tensor.float = lambda s, *a, **k: s.double()

    def __exit__(self, *exc):
        torch.Tensor.float = self.f
        return False


def rnd_bf16(shape, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    t = torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))
    return t.to(torch.bfloat16).float()


def run(module, qkv, dout, dtype):
    """The reference module on [N, width, T] tensors of ``dtype``; returns (out, dqkv) in this project's layouts."""
    x = qkv.to(dtype).transpose(1, 2).contiguous().requires_grad_(True)
    y = module(x)
    (g,) = torch.autograd.grad(y, x, dout.to(dtype).transpose(1, 2).contiguous())
    return y.detach().transpose(1, 2).contiguous(), g.transpose(1, 2).contiguous()


def generate():
    rec = {}
    for c, (n, t, heads, ch) in enumerate(CASES):
        qkv = rnd_bf16((n, t, heads * 3 * ch), 1000 + c, 2.0)
        dout = rnd_bf16((n, t, heads * ch), 2000 + c)
        module = QKVAttentionLegacy(heads)
        with AsDouble():
            out, dqkv = run(module, qkv, dout, torch.float64)
        assert out.dtype == torch.float64 and dqkv.dtype == torch.float64
        _, g_bf = run(module, qkv, dout, torch.bfloat16)
        dev = float((g_bf.double() - dqkv).norm() / dqkv.norm())
        rec.update({f"shape{c}": np.array([n, t, heads, ch]), f"qkv{c}": qkv.numpy(), f"dout{c}": dout.numpy(),
                    f"out{c}": out.float().numpy(), f"dqkv{c}": dqkv.numpy(), f"bf16_dev{c}": np.array(dev)})
        print(f"case {c} {(n, t, heads, ch)}: |dqkv| max {float(dqkv.abs().max()):.3f} bf16_dev {dev:.3e}")
    golden.save(OUT, "ref_sattn_grad", rec)


if __name__ == "__main__":
    generate()
