"""Shared by the Palette tests and scripts/gen_palette_golden.py: the fixture configurations, the portable weight
initialiser and the synthetic inputs.

Why an initialiser of its own: a freshly constructed guided-diffusion U-Net zeroes the second convolution of every
ResBlock, every ``proj_out`` and the final convolution, so it predicts exactly zero and a fixture made from it would pass
with most of the network broken.  ``portable_state`` fills every ``unet.`` tensor from one numpy stream (so the reference
on the host and the HIP model get the same numbers without sharing torch's generator) at a scale at which the predicted
noise has the magnitude of ``y_t``.
"""
import numpy as np
import torch

# name -> (channel_mults, attention_res, (H, W), learn_var, seed, records the sampler chain)
CONFIGS = {
    "a": ((1, 2), (2,), (16, 16), False, 11, True),
    "b": ((1, 2), (1, 2), (16, 16), True, 12, True),
    "c": ((1, 1, 2), (2, 4), (32, 32), False, 43, False),
    "d": ((1, 2), (2,), (24, 16), False, 14, False),
}
N = 2
GAMMAS = (np.array([0.98, 0.91], np.float32), np.array([1.3e-3, 0.8e-3], np.float32))
CROP = 8            # recorded intermediate activations keep every CROP-th channel


def palette_kwargs(name):
    mults, att, _, learn_var, _, _ = CONFIGS[name]
    return dict(in_channels=1, out_channels=1, channel_mults=mults, attention_res=att, dropout=0.0, schedule_type="linear",
                learn_var=learn_var)


def portable_state(shapes, seed):
    """{key: float32 array} for every ``unet.`` key of ``shapes`` ({key: shape}); one ``default_rng(seed)`` stream over the
    sorted keys.  BatchNorm: running_var = 1 + 0.2 u, running_mean = 0.05 n, weight = 1 + 0.1 n, bias = 0.1 n; every other
    tensor 0.02 n; then ``unet.out.2.weight`` x 16.  ``num_batches_tracked`` stays 0 and draws nothing."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in sorted(shapes):
        if not k.startswith("unet."):
            continue
        shp = tuple(shapes[k])
        prefix, leaf = k.rsplit(".", 1)
        is_bn = (prefix + ".running_mean") in shapes
        if leaf == "num_batches_tracked":
            out[k] = np.zeros(shp, np.int64)
        elif leaf == "running_var":
            out[k] = (1 + 0.2 * rng.random(shp)).astype(np.float32)
        elif leaf == "running_mean":
            out[k] = (0.05 * rng.standard_normal(shp)).astype(np.float32)
        elif is_bn and leaf == "weight":
            out[k] = (1 + 0.1 * rng.standard_normal(shp)).astype(np.float32)
        elif is_bn and leaf == "bias":
            out[k] = (0.1 * rng.standard_normal(shp)).astype(np.float32)
        else:
            out[k] = (0.02 * rng.standard_normal(shp)).astype(np.float32)
    out["unet.out.2.weight"] = out["unet.out.2.weight"] * np.float32(16)
    return out


def init_portable(model, seed):
    """Load ``portable_state`` into a Palette (the reference's or the HIP one); the schedule buffers stay as built."""
    sd = model.state_dict()
    new = portable_state({k: tuple(v.shape) for k, v in sd.items()}, seed)
    with torch.no_grad():
        for k, v in new.items():
            sd[k].copy_(torch.from_numpy(v).reshape(sd[k].shape))
    return model


def inputs(name):
    """x ~ U[-1, 1), y_t ~ N(0, 1): fp32 [N, 1, H, W] from the configuration's seed."""
    _, _, (h, w), _, seed, _ = CONFIGS[name]
    rng = np.random.default_rng(1000 + seed)
    x = (rng.random((N, 1, h, w)) * 2 - 1).astype(np.float32)
    y = rng.standard_normal((N, 1, h, w)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y)


def first_modules(unet):
    """State-dict prefixes of the recorded intermediates: the first convolution, the first ResBlock, the first
    AttentionBlock and the middle block."""
    att = next(n for n, m in unet.named_modules() if type(m).__name__ == "AttentionBlock")
    return ["input_blocks.0", "input_blocks.1.0", att, "middle_block"]


def shape_table(state_dict):
    """(keys, shapes [n, 4] padded with -1) of a state dict, for the fixture."""
    keys = list(state_dict)
    shapes = np.full((len(keys), 4), -1, np.int64)
    for i, k in enumerate(keys):
        s = tuple(state_dict[k].shape)
        shapes[i, :len(s)] = s
    return np.array(keys), shapes
