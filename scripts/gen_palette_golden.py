"""Generate tests/golden/ref_palette_*.npz by running the REAL reference Palette on the CPU.

Build container only (it needs the reference checkout):

    python scripts/gen_palette_golden.py [a b c d]

The reference is imported from its checkout with the stand-in packages of oracle/shims ahead of it on sys.path, as
oracle/gen_golden.py does.  Only data is written (inputs, outputs, recorded figures); no reference source is copied.
Weights and inputs come from tests/_palette_util.py, which the tests share.

Per configuration: meta, the state-dict keys and shapes, the schedule buffers of both DiffusionModels, x / y_t / gammas and
the U-Net output for two gamma vectors, a few intermediate activations (every 8th channel) and ``bf16_dev``, the relative
L2 distance of the reference's own output under bf16 autocast from its fp32 output.  For the configurations that record
the sampler also: the 101 noise tensors, y_t and the model output at every step, the final image, ``chain_floor`` (the
same chain in fp64 against fp32, max abs) and ``chain_dev`` (max abs deviation of the final image when every U-Net output
of the fp64 chain is multiplied by 1 + 1e-4 r, r ~ N(0, 1) per element).

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from models.palette import Palette              # noqa: E402  (the reference's)
from oracle import golden                        # noqa: E402
import _palette_util as U                        # noqa: E402


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


class FedNoise:
    """torch.randn_like replaced by recorded (or recording) draws, in the dtype of the argument."""

    def __init__(self, noise=None, seed=0):
        self.noise, self.gen, self.k, self.rec = noise, torch.Generator().manual_seed(seed), 0, []

    def __call__(self, t):
        if self.noise is None:
            z = torch.randn(t.shape, generator=self.gen, dtype=torch.float32)
            self.rec.append(z)
        else:
            z = self.noise[self.k]
        self.k += 1
        return z.to(t.dtype)


def run_chain(model, x, noise, perturb=None, record=False):
    """The reference sampler with fed noise; optionally every U-Net output times (1 + 1e-4 r); optionally recording y_t and
    the model output of every step."""
    fed = FedNoise(noise, seed=7)
    unet_fwd = model.unet.forward
    ys, outs = [], []

    def unet(xx, yy, gg):
        o = unet_fwd(xx, yy, gg)
        if perturb is not None:
            o = o * (1 + 1e-4 * torch.randn(o.shape, generator=perturb, dtype=torch.float64).to(o.dtype))
        if record:
            ys.append(yy.detach().clone())
            outs.append(o.detach().clone())
        return o

    keep = torch.randn_like
    torch.randn_like = fed
    model.unet.forward = unet
    try:
        with torch.no_grad():
            final = model(x)
    finally:
        torch.randn_like = keep
        model.unet.forward = unet_fwd
    return final, fed, ys, outs


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


def generate(name):
    mults, att, (h, w), learn_var, seed, chain = U.CONFIGS[name]
    torch.manual_seed(0)
    model = Palette(**U.palette_kwargs(name))
    U.init_portable(model, seed)
    model.eval()
    x, y_t = U.inputs(name)
    keys, shapes = U.shape_table(model.state_dict())
    rec = {"meta_mults": np.array(mults), "meta_attention_res": np.array(att), "meta_size": np.array([h, w]),
           "meta_learn_var": np.array(int(learn_var)), "meta_seed": np.array(seed), "keys": keys, "shapes": shapes,
           "x": x.numpy(), "y_t": y_t.numpy()}
    for dm in ("diffusion", "diffusion_inf"):
        for b in ("alphas", "gammas", "gammas_prev"):
            rec[f"{dm}.{b}"] = getattr(getattr(model, dm), b).numpy()
    names = U.first_modules(model.unet)
    mods = dict(model.unet.named_modules())
    for gi, g in enumerate(U.GAMMAS):
        grabbed = {}
        hooks = [mods[n].register_forward_hook(lambda m, i, o, n=n: grabbed.__setitem__(n, o.detach().clone()))
                 for n in names] if gi == 0 else []
        with torch.no_grad():
            out = model.unet(x, y_t, torch.from_numpy(g))
            for hk in hooks:
                hk.remove()
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out_bf = model.unet(x, y_t, torch.from_numpy(g)).float()
        std = float(out[:, :1].std())
        assert 0.1 <= std <= 3, f"{name}: U-Net output std {std} outside [0.1, 3] -- the fixture would not pin the network"
        rec[f"gammas{gi}"] = g
        rec[f"out{gi}"] = out.numpy()
        rec[f"out{gi}_std"] = np.array(std)
        rec[f"bf16_dev{gi}"] = np.array(rel_l2(out_bf, out))
        for n, t in grabbed.items():
            rec["act:" + n] = t[:, ::U.CROP].numpy()
        print(name, f"gammas{gi}: std {std:.3f} |max| {float(out.abs().max()):.3f} bf16_dev {float(rec[f'bf16_dev{gi}']):.3e}")
    if chain:
        final, fed, ys, outs = run_chain(model, x, None, record=True)
        noise = torch.stack(fed.rec)
        assert noise.shape[0] == model.diffusion_inf.timesteps + 1
        rec.update(noise=noise.numpy(), chain_y=torch.stack(ys).numpy(), chain_out=torch.stack(outs).numpy(),
                   final=final.numpy())
        model.double()
        with AsDouble():
            f64, _, _, _ = run_chain(model, x.double(), noise)
            dev = 0.0
            for trial in range(3):
                fp, _, _, _ = run_chain(model, x.double(), noise, perturb=torch.Generator().manual_seed(100 + trial))
                dev = max(dev, float((fp - f64).abs().max()))
        rec["chain_floor"] = np.array(float((f64 - final.double()).abs().max()))
        rec["chain_dev"] = np.array(dev)
        print(name, f"chain: floor {float(rec['chain_floor']):.3e} dev {dev:.3e} |final| {float(final.abs().max()):.3f}")
    golden.save(OUT, f"ref_palette_{name}", rec)


if __name__ == "__main__":
    for cfg in (sys.argv[1:] or list(U.CONFIGS)):
        generate(cfg)
