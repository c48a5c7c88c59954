"""GPU: the Palette sampler (fp32 mode) against the reference's recorded chains (configurations a and b of
tests/golden/ref_palette_*.npz: the 101 noise tensors, y_t and the model output at every step, the final image).

The first steps multiply the predicted noise by 1 / sqrt(gamma) (800 at t = 99) before the clamp, so the U-Net and the step
kernel are pinned separately (teacher-forced, from the recorded y_t), and the whole chain against the reference's own
sensitivity: ``chain_dev`` is how far the final image of the fp64 chain moves when every U-Net output is perturbed by
1e-4 relative noise, ``chain_floor`` the distance of the fp32 chain from the fp64 one."""
import numpy as np
import pytest
import torch

import _palette_util as U
from _gpu_util import dev, max_err
from oracle import golden

pytestmark = pytest.mark.gpu

CHAINS = [n for n, c in U.CONFIGS.items() if c[5]]


@pytest.fixture(scope="module")
def recs(golden_dir):
    return {name: golden.load(golden_dir, f"ref_palette_{name}") for name in CHAINS}


@pytest.fixture(scope="module")
def models(pai):
    out = {}
    for name in CHAINS:
        m = U.init_portable(pai.Palette(**U.palette_kwargs(name)), U.CONFIGS[name][4]).to(dev())
        m.freeze()
        out[name] = m
    return out


@pytest.mark.parametrize("name", CHAINS)
def test_teacher_forced_steps(pai, recs, models, name):
    """From the recorded y_t of step t: the U-Net output within 1e-4 of its largest value, and y_{t-1} within
    1e-5 + 1 / sqrt(gamma_t) * 1e-4 * max |eps| -- what the step formula makes, before the clamp, of a U-Net error that the
    line before admits."""
    from thesis_pai_reconstruction_amd import nnops, ops
    rec, m = recs[name], models[name]
    x = torch.from_numpy(rec["x"]).to(dev())
    n, c, h, w = x.shape
    table, gammas = m.diffusion_inf.step_table(), m.diffusion_inf.gammas
    for t in (99, 98, 50, 2, 1, 0):
        k = 99 - t
        y_t = torch.from_numpy(rec["chain_y"][k]).to(dev())
        want_out = torch.from_numpy(rec["chain_out"][k])
        want_next = torch.from_numpy(rec["chain_y"][k + 1] if k < 99 else rec["final"])
        xy = nnops.to_nhwc(torch.cat([x, y_t], 1), torch.float32)
        eps = m.unet.run(xy, gammas[t].expand(n).contiguous())
        got_out = eps.permute(0, 3, 1, 2).cpu()
        e = max_err(got_out, want_out)
        y = y_t.reshape(n * h * w, c).clone()
        noise = torch.from_numpy(rec["noise"][k + 1]).to(dev()).reshape(n * h * w, c)
        ops.palette_step(torch.float32, eps, y, noise, n * h * w, c, m.learn_var, t > 1, table[t], y, xy)
        err = float((y.reshape(n, c, h, w).cpu().double() - want_next.double()).abs().max())
        bound = 1e-5 + table[t][1] * 1e-4 * float(want_out[:, :c].abs().max())
        print(f"palette {name} t={t}: U-Net max err / max {e:.3e}; y_(t-1) max err {err:.3e} (bound {bound:.3e})")
        assert e <= 1e-4
        assert err <= bound
        assert torch.equal(xy[..., c:].reshape(-1), y.reshape(-1))        # the y half of the next U-Net input


@pytest.mark.parametrize("name", CHAINS)
def test_whole_chain(pai, recs, models, name):
    rec, m = recs[name], models[name]
    noise = torch.from_numpy(rec["noise"])
    m.noise_fn = lambda k, shape: noise[k]
    try:
        got = m(torch.from_numpy(rec["x"]).to(dev())).cpu()
    finally:
        m.noise_fn = None
    err = float((got.double() - torch.from_numpy(rec["final"]).double()).abs().max())
    bound = 2 * float(rec["chain_dev"]) + float(rec["chain_floor"])
    print(f"palette {name} chain: final image max err {err:.3e} (bound {bound:.3e})")
    assert got.shape == rec["final"].shape
    assert err <= bound


def test_output_process_seed_and_no_host_sync(pai, recs, models):
    """``output_process`` returns y_T and the chain at every 14th step; the same seed gives the same bits; the 100-step
    loop never waits for the device (torch's sync debug mode raises on any synchronising call)."""
    m = models["a"]
    x = torch.from_numpy(recs["a"]["x"]).to(dev())
    torch.manual_seed(5)
    y1, proc = m(x, output_process=True)
    assert tuple(proc.shape) == (2, 9, 1, 16, 16) and torch.equal(proc[:, -1], y1)
    torch.manual_seed(5)
    y2 = m(x)
    assert torch.equal(y1, y2)
    torch.manual_seed(6)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y3 = m(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(y3).all()) and not torch.equal(y3, y1)
    short = pai.Palette(**U.palette_kwargs("a"), inference_steps=4).to(dev())
    short.freeze()
    _, proc = short(x, output_process=True)          # fewer than 7 steps: every step is kept
    assert tuple(proc.shape) == (2, 5, 1, 16, 16)
