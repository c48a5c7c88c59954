"""CPU: the host side of the train-mode Palette U-Net pass (``UNet.forward_train``): the two C entry points it adds and their
refusals, the entry point's own refusals, and the fixtures recorded from the reference in training mode
(tests/golden/ref_palette_train_*.npz, scripts/gen_palette_train_golden.py) -- their dead / live classification of the
parameter gradients and the caps the GPU tests' bounds rest on, checked on the recorded numbers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _palette_util as U
from oracle import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pai_avgpool2_bwd", "pai_silu_bwd")
TAGS = ("a", "b", "c", "d", "a_drop")
DEAD = re.compile(r"(in_layers\.2|out_layers\.3|skip_connection|proj_out)\.bias$|^input_blocks\.0\.0\.bias$")
ATT16 = re.compile(r"\.(norm|qkv)\.bias$")


@pytest.fixture(scope="module")
def recs(golden_dir):
    return {t: golden.load(golden_dir, f"ref_palette_train_{t}") for t in TAGS}


def test_abi_141_entries(pai):
    src = open(os.path.join(ROOT, "include", "pai_hip.h")).read()
    decl = set(re.findall(r"\b(pai_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = pai.lib.load()
    for name in NEW:
        assert name in decl and name in pai.lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pai_version() == 141


def test_refusals_come_before_any_launch(pai):
    """Every refusal returns an error with its message in pai_last_error and never touches a pointer (there is no GPU here)."""
    lib = pai.lib.load()
    fake = ctypes.c_void_p(0x100000)          # aligned, never dereferenced
    odd = ctypes.c_void_p(0x100004)
    F32, BF16 = pai.lib.F32, pai.lib.BF16

    def pool(dtype=F32, dout=fake, N=2, H=4, W=6, C=8, dx=fake):
        return lib.pai_avgpool2_bwd(dtype, dout, N, H, W, C, dx, None)

    def silu(dtype=F32, g=fake, u=fake, numel=7, du=fake):
        return lib.pai_silu_bwd(dtype, g, u, numel, du, None)

    for call, kw, word in ((pool, dict(H=5), b"H=5"), (pool, dict(W=3), b"W=3"), (pool, dict(H=0), b"H=0"),
                           (pool, dict(C=12), b"multiple of 8"), (pool, dict(C=0), b"C=0"), (pool, dict(N=0), b"N=0"),
                           (pool, dict(dout=None), b"null"), (pool, dict(dx=None), b"null"), (pool, dict(dtype=2), b"dtype=2"),
                           (pool, dict(dtype=BF16, dx=odd), b"aligned"),
                           (pool, dict(N=1 << 20, H=1 << 12, W=1 << 12, C=1 << 12), b"too large"),
                           (silu, dict(g=None), b"null"), (silu, dict(u=None), b"null"), (silu, dict(du=None), b"null"),
                           (silu, dict(dtype=2), b"dtype=2"), (silu, dict(dtype=-1), b"dtype=-1"), (silu, dict(numel=0), b"numel=0"),
                           (silu, dict(u=odd), b"aligned"), (silu, dict(numel=1 << 43), b"too large")):
        assert call(**kw) != 0, kw
        assert word in lib.pai_last_error(), (kw, lib.pai_last_error())


def test_forward_train_exists_and_refuses(pai):
    m = pai.Palette(**U.palette_kwargs("a"))
    assert callable(getattr(m.unet, "forward_train"))
    x = torch.zeros(2, 1, 16, 16)
    g = torch.ones(2)
    m.train()
    with pytest.raises(pai.PaiError, match="device"):
        m.unet.forward_train(x, x, g)                     # host tensors
    m.eval()
    with pytest.raises(pai.PaiError, match="train"):
        m.unet.forward_train(x, x, g)                     # eval mode
    m.train()
    with pytest.raises(pai.PaiError, match="eval"):      # the eval-only entry points keep refusing training mode
        m.unet.run(x, g)
    with pytest.raises(NotImplementedError, match="sampling only"):
        m.training_step((x, x), 0)


def test_autograd_ops_refuse_host_tensors(pai):
    from thesis_pai_reconstruction_amd import nnops
    with pytest.raises(pai.PaiError):
        nnops.AvgPool2.apply(torch.zeros(1, 2, 2, 8))
    with pytest.raises(pai.PaiError):
        nnops.SiLU.apply(torch.zeros(2, 8), torch.ones(8), torch.zeros(8))


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_classification_and_caps(pai, recs, tag):
    """What the GPU tests rely on, on the recorded numbers: the dead tensors are exactly the convolution biases that feed the
    residual stream (every later norm removes a per-channel constant), every live tensor has a fingerprint and an fp32
    yardstick of at most 2e-4, and where a bf16 yardstick is recorded (a and d; b and c are fp32-only) the tensors past 0.25
    are AttentionBlock norm.bias / qkv.bias only and at most 10 % of the live ones."""
    rec = recs[tag]
    name = tag.split("_")[0]
    keys = [str(k) for k in rec["keys"]]
    m = pai.Palette(**U.palette_kwargs(name))
    assert keys == [k for k, _ in m.unet.named_parameters()]
    dead = [k for k, d in zip(keys, rec["dead"]) if d]
    live = [k for k in keys if k not in dead]
    assert dead == [k for k in keys if DEAD.search(k)]
    assert {"a": (200, 42), "b": (230, 47), "c": (306, 64), "d": (200, 42)}[name] == (len(keys), len(dead))
    for k in keys:
        assert rec["grad:" + k].shape == (36,)
    assert max(float(rec["grad:" + k][0]) for k in dead) < 1e-9
    assert min(float(rec["grad:" + k][0]) for k in live) >= 0.01
    assert max(float(rec["dev32:" + k]) for k in live) <= 2e-4
    assert all(0 < float(rec["noise32:" + k]) < 0.05 for k in dead)
    assert float(rec["dev32_out"]) <= 1e-5
    has16 = bool(rec["has16"])
    assert has16 == (tag in ("a", "d"))
    if has16:
        dev16 = {k: float(rec["dev16:" + k]) for k in live}
        far = [k for k in live if dev16[k] > 0.25]
        assert far and all(ATT16.search(k) for k in far) and len(far) <= 0.1 * len(live)
        assert 0.02 <= float(rec["dev16_out"]) <= 0.05
        assert all(("noise16:" + k) in rec for k in dead)
    # running statistics: one advance in the forward; the AttentionBlock norms once more in the backward
    mods = dict(m.unet.named_modules())
    names = [str(n) for n in rec["bn_names"]]
    assert names == [n for n, v in mods.items() if isinstance(v, torch.nn.modules.batchnorm._BatchNorm)]
    assert [int(s) for s in rec["bn_sizes"]] == [mods[n].num_features for n in names]
    total = int(rec["bn_sizes"].sum())
    for k in ("mean", "var"):
        assert rec[f"bn_{k}_fwd"].shape == (total,) and rec[f"bn_{k}_bwd"].shape == (total,)
    att = np.array([isinstance(mods[n], torch.nn.BatchNorm1d) for n in names])
    assert att.sum() == sum(type(v).__name__ == "AttentionBlock" for v in mods.values()) > 0
    assert np.all(rec["bn_nbt_fwd"] == 1) and np.all(rec["bn_nbt_bwd"] == 1 + att)
    off = np.concatenate([[0], np.cumsum(rec["bn_sizes"])])
    for i, n in enumerate(names):
        moved = np.abs(rec["bn_mean_bwd"][off[i]:off[i + 1]] - rec["bn_mean_fwd"][off[i]:off[i + 1]]).max()
        assert (moved > 1e-6) == bool(att[i]), n
    h, w = U.CONFIGS[name][2]
    co = 2 if U.CONFIGS[name][3] else 1
    assert rec["out"].shape == rec["dout"].shape == (U.N, co, h, w) and rec["out"].dtype == np.float64
    if tag == "a_drop":
        blocks = [n for n, v in mods.items() if type(v).__name__ == "ResBlock"]
        for n in blocks:
            shape = tuple(int(v) for v in rec["mask_shape:" + n])
            bits = np.unpackbits(rec["mask:" + n])[:int(np.prod(shape))]
            assert shape[0] == U.N and shape[3] == mods[n].out_channel and 0.70 < bits.mean() < 0.80, n
    else:
        assert sorted(k[4:] for k in rec if k.startswith("act:")) == sorted(U.first_modules(m.unet))
