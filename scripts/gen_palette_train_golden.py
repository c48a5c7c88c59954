"""Generate tests/golden/ref_palette_train_{a,b,c,d}.npz and ref_palette_train_a_drop.npz by running the REAL reference
Palette U-Net in training mode on the CPU: forward, then backward of a recorded output gradient.

Build container only (it needs the reference checkout):

    python scripts/gen_palette_train_golden.py [a b c d a_drop]

The reference is imported as scripts/gen_palette_golden.py imports it (the stand-in packages of oracle/shims ahead of it on
sys.path).  Only data is written; no reference source is copied.  Weights and inputs come from tests/_palette_util.py.

Per configuration the reference ``Palette(...).unet`` runs in ``.train()`` at dropout 0 with ``gammas = U.GAMMAS[0]`` in
fp64 (the recorded truth), in fp32 and under CPU bf16 autocast (the yardsticks), each from freshly initialised weights:

    out, dout                       fp64 output; dout ~ N(0, 1) (fp32 values) from torch.Generator().manual_seed(1)
    act:<module>                    the four intermediates of U.first_modules, every U.CROP-th channel (fp64 run)
    keys                            the parameter names below ``unet.``
    grad:<key>                      oracle.fingerprint.fingerprint of the fp64 gradient (36 doubles)
    dead                            0 / 1 per key: the fp64 gradient's norm is below 1e-9 (zero in exact arithmetic)
    dev32:<key>, dev32_out          live tensors: relative L2 distance of the reference's fp32 run from its fp64 run
    dev16:<key>, dev16_out          the same for its run under bf16 autocast (a and d; see HAS16)
    noise32:<key>, noise16:<key>    dead tensors: the L2 norm of what the fp32 / autocast run left there (rounding noise)
    bn_names, bn_sizes              every BatchNorm below ``unet.`` and its channel count
    bn_{mean,var,nbt}_{fwd,bwd}     running_mean | running_var (concatenated over bn_names) and num_batches_tracked after the
                                    forward and again after the backward (fp64 run)

``a_drop``: configuration a at dropout p = 0.25, fp64 and fp32 only.  Every ``out_layers.2`` of the reference gets p = 0 and
a forward hook that returns ``out * mask / 0.75`` with a seeded mask, recorded per ResBlock prefix as
``mask:<prefix>`` (np.packbits of the NHWC-ordered mask) and ``mask_shape:<prefix>`` ([N, H, W, C]).

In the autocast run the backward stays inside the autocast context and every AttentionBlock gets ``forward = _forward``:
the reference's checkpoint recomputation fails outside autocast and otherwise leaves those parameters without gradients.

The assertions below are facts about the reference the tests rely on; a fixture that breaks one would pin nothing.

TEST INFRASTRUCTURE ONLY.
"""
import os
import re
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
sys.path.insert(0, HERE)

from models.palette import Palette              # noqa: E402  (the reference's)
from oracle import golden                        # noqa: E402
from oracle.fingerprint import fingerprint       # noqa: E402
import _palette_util as U                        # noqa: E402
from gen_palette_golden import AsDouble, rel_l2  # noqa: E402

DEAD = re.compile(r"(in_layers\.2|out_layers\.3|skip_connection|proj_out)\.bias$|^input_blocks\.0\.0\.bias$")
ATT16 = re.compile(r"\.(norm|qkv)\.bias$")       # the AttentionBlock tensors whose bf16 autocast gradient is far off
# no bf16 yardstick for c (134 of 242 live tensors are past 0.125 under autocast) nor for b (attention at both levels: 22
# of 183 live tensors are past 0.25, more than the 10 % the yardstick tolerates): fp32-only fixtures
HAS16 = {"a": True, "b": False, "c": False, "d": True}
P_DROP = 0.25


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def build(name, dropout):
    torch.manual_seed(0)
    model = Palette(**dict(U.palette_kwargs(name), dropout=dropout))
    U.init_portable(model, U.CONFIGS[name][4])
    model.unet.train()
    return model.unet


def bn_modules(unet):
    return [(n, m) for n, m in unet.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def bn_state(unet):
    bns = bn_modules(unet)
    return (torch.cat([m.running_mean.double() for _, m in bns]).numpy().copy(),
            torch.cat([m.running_var.double() for _, m in bns]).numpy().copy(),
            np.array([int(m.num_batches_tracked) for _, m in bns], np.int64))


def run(name, mode, x, y, g, dout, dropout=0.0, masks=None, grab=None):
    """One forward + backward of a freshly initialised reference U-Net.  mode: "f64" | "f32" | "bf16"."""
    unet = build(name, dropout)
    if masks is not None:
        for prefix, blk in unet.named_modules():
            if type(blk).__name__ != "ResBlock":
                continue
            drop = blk.out_layers[2]
            assert isinstance(drop, torch.nn.Dropout) and drop.p == P_DROP
            drop.p = 0.0

            def hook(m, i, o, prefix=prefix):
                if prefix not in masks:
                    gen = torch.Generator().manual_seed(5000 + len(masks))
                    masks[prefix] = torch.rand(o.shape, generator=gen) >= P_DROP
                return o * masks[prefix].to(o.dtype) / (1 - P_DROP)

            drop.register_forward_hook(hook)
    hooks = []
    if grab is not None:
        mods = dict(unet.named_modules())

        def keep(m, i, o, n):
            grab.setdefault(n, o.detach().clone())          # (a hook that returns a tensor would replace the output)

        hooks = [mods[n].register_forward_hook(lambda m, i, o, n=n: keep(m, i, o, n)) for n in U.first_modules(unet)]
    if mode == "f64":
        unet.double()
        ctx, cast = AsDouble(), torch.float64
    elif mode == "f32":
        ctx, cast = _Null(), torch.float32
    else:
        ctx, cast = torch.autocast("cpu", dtype=torch.bfloat16), torch.float32
        for m in unet.modules():
            if type(m).__name__ == "AttentionBlock":
                m.forward = m._forward
    with ctx:
        out = unet(x.to(cast), y.to(cast), g.to(cast))
        after_fwd = bn_state(unet)
        out.backward(dout.to(out.dtype))
        after_bwd = bn_state(unet)
    for h in hooks:
        h.remove()
    grads = {k: p.grad.detach().double() for k, p in unet.named_parameters()}
    assert all(v is not None for v in grads.values())
    return unet, out.detach().double(), grads, after_fwd, after_bwd


def generate(tag):
    name, drop = (tag[:-5], True) if tag.endswith("_drop") else (tag, False)
    dropout = P_DROP if drop else 0.0
    masks = {} if drop else None
    x, y = U.inputs(name)
    g = torch.from_numpy(U.GAMMAS[0])
    probe = build(name, dropout)
    with torch.no_grad():
        shape = probe.eval()(x, y, g).shape
    dout = torch.randn(shape, generator=torch.Generator().manual_seed(1), dtype=torch.float32)

    grab = {}
    unet, out, g64, fwd, bwd = run(name, "f64", x, y, g, dout, dropout, masks, grab)
    _, out32, g32, _, _ = run(name, "f32", x, y, g, dout, dropout, masks)
    keys = list(g64)
    rec = {"keys": np.array(keys), "out": out.numpy(), "dout": dout.numpy(), "gammas": U.GAMMAS[0],
           "dev32_out": np.array(rel_l2(out32, out))}
    if not drop:
        for n, t in grab.items():
            rec["act:" + n] = t[:, ::U.CROP].double().numpy()
        assert len(grab) == 4
    bns = bn_modules(unet)
    rec["bn_names"] = np.array([n for n, _ in bns])
    rec["bn_sizes"] = np.array([m.num_features for _, m in bns], np.int64)
    for k, (a, b) in zip(("mean", "var", "nbt"), zip(fwd, bwd)):
        rec[f"bn_{k}_fwd"], rec[f"bn_{k}_bwd"] = a, b
    # the reference advances the AttentionBlock norms twice per forward + backward (checkpoint recomputation)
    for (n, m), f, b in zip(bns, fwd[2], bwd[2]):
        assert f == 1 and b == (2 if isinstance(m, torch.nn.BatchNorm1d) else 1), (n, f, b)

    norms = {k: float(v.norm()) for k, v in g64.items()}
    dead = [k for k in keys if norms[k] < 1e-9]
    live = [k for k in keys if k not in dead]
    assert dead == [k for k in keys if DEAD.search(k)], "the dead set is not the residual-stream convolution biases"
    assert min(norms[k] for k in live) >= 0.01, min(norms[k] for k in live)
    if name in ("a", "d"):
        assert (len(keys), len(dead)) == (200, 42), (len(keys), len(dead))
    if name == "c":
        assert (len(keys), len(dead)) == (306, 64), (len(keys), len(dead))
    rec["dead"] = np.array([int(k in dead) for k in keys], np.int64)
    for k in keys:
        rec["grad:" + k] = fingerprint(g64[k])
    for k in live:
        rec["dev32:" + k] = np.array(rel_l2(g32[k], g64[k]))
    for k in dead:
        rec["noise32:" + k] = np.array(float(g32[k].norm()))
    worst32 = max(float(rec["dev32:" + k]) for k in live)
    assert worst32 <= 2e-4, worst32
    assert float(rec["dev32_out"]) <= 1e-5, float(rec["dev32_out"])
    msg = f"{tag}: {len(keys)} tensors, {len(dead)} dead; fp32 dev: out {float(rec['dev32_out']):.2e} worst grad {worst32:.2e} " \
          f"noise {max(float(rec['noise32:' + k]) for k in dead):.2e}"

    has16 = HAS16[name] and not drop
    if has16:
        _, out16, g16, _, _ = run(name, "bf16", x, y, g, dout)
        dev16 = {k: rel_l2(g16[k], g64[k]) for k in live}
        far = [k for k in live if dev16[k] > 0.25]
        assert all(ATT16.search(k) for k in far) and len(far) <= 0.1 * len(live), (tag, len(far), len(live), far)
        rec["dev16_out"] = np.array(rel_l2(out16, out))
        assert float(rec["dev16_out"]) <= 0.05, float(rec["dev16_out"])
        for k in live:
            rec["dev16:" + k] = np.array(dev16[k])
        for k in dead:
            rec["noise16:" + k] = np.array(float(g16[k].norm()))
        msg += f"; bf16 dev: out {float(rec['dev16_out']):.2e} median {float(np.median(list(dev16.values()))):.2e} " \
               f"{len(far)} past 0.25 (max {max(dev16.values()):.2e}) noise {max(float(rec['noise16:' + k]) for k in dead):.2e}"
    rec["has16"] = np.array(int(has16))
    if drop:
        assert len(masks) == sum(type(m).__name__ == "ResBlock" for m in unet.modules())
        for prefix, m in masks.items():
            nhwc = m.permute(0, 2, 3, 1).contiguous()
            rec["mask:" + prefix] = np.packbits(nhwc.numpy().reshape(-1))
            rec["mask_shape:" + prefix] = np.array(nhwc.shape, np.int64)
    print(msg)
    golden.save(OUT, f"ref_palette_train_{tag}", rec)


if __name__ == "__main__":
    for cfg in (sys.argv[1:] or ["a", "b", "c", "d", "a_drop"]):
        generate(cfg)
