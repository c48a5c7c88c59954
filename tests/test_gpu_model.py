"""GPU parity of the whole hot path through the plugin surface (Pix2Pix / UnetWrapper /
Discriminator) against (a) the golden fixtures recorded from the REAL reference and (b) the
CPU oracle run live on the same seeded inputs.

fp32 compute mode must match within 1e-4 relative (north_star); bf16 mode is held to a looser
bound plus SSIM/PSNR agreement.  Size-independent properties are checked at the BASELINE
configuration (256x256, batch 64, bf16)."""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle.fingerprint import fingerprint, fingerprint_close
from oracle.gen_golden import synth_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _bias_before_bn(k, keys):
    return k.endswith(".1.bias") and (k[:-len(".1.bias")] + ".2.weight") in keys


def build(pai, mults, loss_type, seed, dtype=torch.float32, dropout=0.0):
    m = pai.Pix2Pix(in_channels=1, out_channels=1, channel_mults=tuple(mults), dropout=dropout, loss_type=loss_type)
    g = oracle.init_state_portable(oracle.make_unet_state(1, 1, tuple(mults)), seed, perturb_bn=True)
    m.unet.load_state_dict(g, strict=True)
    d = None
    if loss_type == "gan":
        d = oracle.init_state_portable(oracle.make_disc_state(1), seed + 1)
        m.discriminator.load_state_dict(d, strict=True)
    m.to(DEV)
    m.set_precision("32" if dtype == torch.float32 else "bf16-mixed")
    m.train()
    return m, g, d


def _fp_ok(got, want_fp, rtol, what):
    ok, worst = fingerprint_close(fingerprint(got), want_fp, rtol)
    assert ok, f"{what}: worst err/tol {worst:.3g}"


@pytest.mark.parametrize("name", ["ref_forward_tiny", "ref_forward_full"])
def test_forward_matches_reference_fixture(pai, golden_dir, name):
    z = _load(golden_dir, name)
    seed, n, size = int(z["meta.seed"]), int(z["meta.n"]), int(z["meta.size"])
    m, _, _ = build(pai, [int(v) for v in z["meta.mults"]], "gan", seed)
    x, t = synth_batch(seed + 100, n, size)
    x, t = x.to(DEV), t.to(DEV)
    with torch.no_grad():
        pred = m.unet(x)
        lf = m.discriminator(x, pred)
        lr = m.discriminator(x, t)
    want = torch.from_numpy(z["pred_full"])
    assert float((pred.cpu() - want).abs().max()) < 1e-4 * float(want.abs().max())
    for got, key in ((lf, "logits_fake_full"), (lr, "logits_real_full")):
        w = torch.from_numpy(z[key])
        assert float((got.cpu() - w).norm() / w.norm()) < 1e-4


@pytest.mark.parametrize("reuse", [True, False], ids=["one_forward", "two_forwards"])
@pytest.mark.parametrize("name", ["ref_gan_tiny", "ref_gan_full"])
def test_gan_training_step_matches_reference_fixture(pai, golden_dir, name, reuse):
    z = _load(golden_dir, name)
    seed, n, size, steps = int(z["meta.seed"]), int(z["meta.n"]), int(z["meta.size"]), int(z["meta.steps"])
    m, g, d = build(pai, [int(v) for v in z["meta.mults"]], "gan", seed)
    m.reuse_generator_forward = reuse
    x, t = synth_batch(seed + 100, n, size)
    batch = (x.to(DEV), t.to(DEV))
    gkeys = set(g.keys())
    # Gradient bound.  Forward values, losses and metrics are held to 1e-4 everywhere.  Gradients
    # are held to 1e-4 on the tiny fixture, whose seed keeps every activation of every layer a
    # safe distance from the ReLU / LeakyReLU kink (oracle/gen_golden.py: ActivationMargin).  At
    # full size (tens of millions of activations) some pre-activations are always within fp32
    # rounding noise of 0, their derivative (0|1, 0.2|1) legitimately differs between any two fp32
    # implementations, and each such flip moves a gradient tensor by ~1/sqrt(numel): bound 2e-3.
    gtol = 1e-4 if name == "ref_gan_tiny" else 2e-3
    for s in range(steps):
        m.logged = {}
        m.training_step(batch, s)
        torch.cuda.synchronize()
        for k, v in m.logged.items():
            want = float(z[f"step{s}.log.{k}"])
            assert abs(float(v) - want) <= 1e-4 * max(1.0, abs(want)), (s, k, float(v), want)
        # Step 0 is the parity bar.  Later steps start from parameters that already differ by the
        # sign-SGD noise described below (~1e-3 relative), which moves ~1e-3 of the activations of
        # a small layer across the ReLU kink: tens of flips in a 32K-element tensor, i.e. a few
        # per cent on the BN gradients of the bottleneck layers.  Losses and metrics stay within
        # 1e-4 (checked above); gradients of later steps only get a gross-error bound.
        gs = gtol if s == 0 else 0.15 * s
        for k, p in m.unet.named_parameters():
            if _bias_before_bn(k, gkeys):
                continue   # analytically zero gradient: pure cancellation noise in the reference
            _fp_ok(p.grad, z[f"step{s}.ggrad.{k}"], gs, f"step{s} ggrad {k}")
        for k, p in m.discriminator.named_parameters():
            _fp_ok(p.grad, z[f"step{s}.dgrad.{k}"], gs, f"step{s} dgrad {k}")
        # Updated parameters / buffers.  Adam's first steps are sign-SGD (|update| = lr = 2e-4 for
        # every element whatever |g|), and a conv bias in front of a BatchNorm has an analytically
        # zero gradient, i.e. it is driven by cancellation noise and drags running_mean with it:
        # beyond the first step these are only reproducible to ~lr relative to the tensor's scale.
        stol = (1e-4 if name == "ref_gan_tiny" else 1e-3) if s == 0 else 4e-3 * s
        for k, v in m.unet.state_dict().items():
            if _bias_before_bn(k, gkeys):
                continue
            _fp_ok(v, z[f"step{s}.gstate.{k}"], stol * (4 if "running_mean" in k else 1), f"step{s} gstate {k}")
        for k, v in m.discriminator.state_dict().items():
            _fp_ok(v, z[f"step{s}.dstate.{k}"], stol, f"step{s} dstate {k}")
    for k, v in m.unet.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 2 * steps
    m.eval()
    m.logged = {}
    with torch.no_grad():
        m.validation_step(batch, 0)
        pred = m(batch[0])
    for k, v in m.logged.items():
        want = float(z[f"val.log.{k}"])
        assert abs(float(v) - want) <= 1e-3 * max(1.0, abs(want)), (k, float(v), want)
    _fp_ok(pred, z["val.pred"], 2e-3, "eval-mode prediction")   # after `steps` steps of drift


@pytest.mark.parametrize("name", ["ref_ssim_tiny", "ref_psnr_tiny", "ref_ssim_psnr_tiny", "ref_mse_tiny"])
def test_other_loss_types_match_reference_fixture(pai, golden_dir, name):
    z = _load(golden_dir, name)
    seed, n, size, steps = int(z["meta.seed"]), int(z["meta.n"]), int(z["meta.size"]), int(z["meta.steps"])
    loss_type = str(z["meta.loss_type"])
    m, g, _ = build(pai, [int(v) for v in z["meta.mults"]], loss_type, seed)
    assert m.discriminator is None
    x, t = synth_batch(seed + 100, n, size)
    batch = (x.to(DEV), t.to(DEV))
    gkeys = set(g.keys())
    for s in range(steps):
        m.logged = {}
        m.training_step(batch, s)
        for k, v in m.logged.items():
            want = float(z[f"step{s}.log.{k}"])
            assert abs(float(v) - want) <= 1e-4 * max(1.0, abs(want)), (s, k, float(v), want)
        for k, p in m.unet.named_parameters():
            if _bias_before_bn(k, gkeys):
                continue
            _fp_ok(p.grad, z[f"step{s}.ggrad.{k}"], 2e-4 * (1 + 2 * s), f"step{s} ggrad {k}")
    for k, v in m.unet.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == steps


def _activation_margin(g, d, x, t):
    """min |pre-activation| / rms over the small activation tensors of one oracle GAN step
    (same criterion as oracle/gen_golden.py: ActivationMargin)."""
    import torch.nn.functional as F
    worst = float("inf")

    def upd(u):
        nonlocal worst
        if u.numel() < 200_000:
            worst = min(worst, float(u.abs().min() / u.pow(2).mean().sqrt()))

    with torch.no_grad():
        gg = {k: v.clone() for k, v in g.items()}
        pred, acts = oracle.unet_forward(gg, x, training=True, return_feats=True)
        for u in acts.values():
            upd(u)
        for y in (pred, t):
            h = torch.cat([x, y], 1)
            for i in range(4):
                h = F.conv2d(h, d[f"discriminator.{i}.block.0.weight"], d[f"discriminator.{i}.block.0.bias"],
                             stride=2, padding=1)
                upd(h)
                h = F.leaky_relu(h, 0.2)
    return worst


def test_ragged_batch_against_live_oracle(pai):
    """Odd batch size / non-square image, compared with the oracle run on the host CPU."""
    mults = (1, 2, 2, 4, 4)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.random((3, 1, 64, 96), dtype=np.float32) * 2 - 1)
    t = torch.from_numpy(rng.random((3, 1, 64, 96), dtype=np.float32) * 2 - 1)
    for seed in range(77, 140):
        m, g, d = build(pai, mults, "gan", seed)
        if _activation_margin(g, d, x, t) > 2e-6:   # keep clear of the ReLU kink, see gtol note above
            break
    og, od = oracle.AdamState(), oracle.AdamState()
    want_logs, want_grads = oracle.gan_training_step(g, d, og, od, x, t, return_grads=True)
    m.logged = {}
    m.training_step((x.to(DEV), t.to(DEV)), 0)
    for k, v in want_logs.items():
        assert abs(float(m.logged[k]) - float(v)) <= 1e-4 * max(1.0, abs(float(v))), k
    for k, p in m.unet.named_parameters():
        if _bias_before_bn(k, set(g.keys())):
            continue
        w = want_grads["g"][k]
        assert float((p.grad.cpu() - w).norm() / w.norm()) < 2e-4, k
    for k, p in m.discriminator.named_parameters():
        w = want_grads["d"][k]
        assert float((p.grad.cpu() - w).norm() / w.norm()) < 2e-4, k
    for k, v in m.unet.state_dict().items():
        if not _bias_before_bn(k, set(g.keys())):
            assert float((v.cpu().double() - g[k].double()).norm()) <= 1e-4 * max(float(g[k].double().norm()), 1e-3), k


@pytest.mark.parametrize("hw", [(64, 96), (96, 64)], ids=["64x96", "96x64"])
def test_bf16_mode_tracks_fp32_path_on_a_rectangle(pai, hw):
    """The batch of test_ragged_batch_against_live_oracle (3 x 1 x 64 x 96) and its transpose on the bf16 matrix-core path
    against the fp32 path of the same weights, under the bounds of test_bf16_mode_tracks_fp32_oracle for the square image:
    prediction within 3e-2 relative L2, every logged loss / metric of one GAN step within 2 %.  In bf16 the non-square
    image reaches the patch, tile and thin kernels; the fp32 path (gg_simt) is held to the oracle by the test above."""
    mults = (1, 2, 2, 4, 4)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.random((3, 1, 64, 96), dtype=np.float32) * 2 - 1)
    t = torch.from_numpy(rng.random((3, 1, 64, 96), dtype=np.float32) * 2 - 1)
    if hw == (96, 64):
        x, t = x.transpose(2, 3).contiguous(), t.transpose(2, 3).contiguous()
    assert tuple(x.shape[2:]) == hw
    m16, _, _ = build(pai, mults, "gan", 77, dtype=torch.bfloat16)
    m32, _, _ = build(pai, mults, "gan", 77)
    batch = (x.to(DEV), t.to(DEV))
    with torch.no_grad():
        p16, p32 = m16.unet(batch[0]), m32.unet(batch[0])
    rel = float((p16 - p32).norm() / p32.norm())
    print(f"{hw}: prediction relative L2 {rel:.3e}")
    assert rel < 3e-2
    for m in (m16, m32):
        m.logged = {}
        m.training_step(batch, 0)
    torch.cuda.synchronize()
    assert set(m16.logged) == set(m32.logged) and m32.logged
    for k, v in m32.logged.items():
        got, want = float(m16.logged[k]), float(v)
        print(f"{hw}: {k} bf16 {got:.6g} fp32 {want:.6g}")
        assert abs(got - want) <= 2e-2 * max(1.0, abs(want)), (k, got, want)
    for k, p in m16.unet.named_parameters():
        assert torch.isfinite(p).all(), k


def test_bf16_mode_tracks_fp32_oracle(pai, golden_dir):
    """bf16 storage / MFMA path: losses and metrics within 2% of the reference fixture,
    per-image SSIM ordering of the prediction preserved."""
    z = _load(golden_dir, "ref_gan_full")
    seed, n, size = int(z["meta.seed"]), int(z["meta.n"]), int(z["meta.size"])
    m, g, d = build(pai, [int(v) for v in z["meta.mults"]], "gan", seed, dtype=torch.bfloat16)
    m32, _, _ = build(pai, [int(v) for v in z["meta.mults"]], "gan", seed)
    x, t = synth_batch(seed + 100, n, size)
    batch = (x.to(DEV), t.to(DEV))
    with torch.no_grad():
        p16, p32 = m.unet(batch[0]), m32.unet(batch[0])
    assert float((p16 - p32).norm() / p32.norm()) < 3e-2
    from thesis_pai_reconstruction_amd import functional as PF
    s16 = PF.ssim_per_image(PF.denormalize(p16), PF.denormalize(batch[1]))
    s32 = PF.ssim_per_image(PF.denormalize(p32), PF.denormalize(batch[1]))
    assert float((s16 - s32).abs().max()) < 5e-3
    # north_star: "SSIM/PSNR bit-identical ordering".  Rank the images by quality against targets of graded
    # difficulty (the fp32 prediction plus noise of increasing strength, so that neighbouring scores are several
    # times further apart than the bf16 deviation bounded above): both metrics must order the batch identically
    # whether the prediction came from the bf16 matrix-core path or the fp32 parity path.
    gen = torch.Generator(device="cpu").manual_seed(5)
    order = torch.randperm(n, generator=gen)
    tgt = torch.empty_like(p32)
    for rank_, i in enumerate(order.tolist()):
        noise = torch.randn(p32[i].shape, generator=gen).to(DEV)
        tgt[i] = (p32[i] + (0.05 + 0.15 * rank_) * noise).clamp(-1, 1)
    q16 = PF.ssim_per_image(PF.denormalize(p16), PF.denormalize(tgt))
    q32 = PF.ssim_per_image(PF.denormalize(p32), PF.denormalize(tgt))
    assert float(q32.sort().values.diff().min()) > 4 * 5e-3           # the ranking is not decided by bf16 noise
    assert torch.equal(q16.argsort(), q32.argsort()) and q32.argsort(descending=True).tolist() == order.tolist()
    mse16 = ((PF.denormalize(p16) - PF.denormalize(tgt)) ** 2).flatten(1).mean(1)
    mse32 = ((PF.denormalize(p32) - PF.denormalize(tgt)) ** 2).flatten(1).mean(1)
    assert torch.equal((-mse16.log()).argsort(), (-mse32.log()).argsort())       # per-image PSNR ordering
    for s in range(2):
        m.logged = {}
        m.training_step(batch, s)
        for k, v in m.logged.items():
            want = float(z[f"step{s}.log.{k}"])
            assert abs(float(v) - want) <= 3e-2 * max(1.0, abs(want)), (s, k, float(v), want)
    for k, p in m.unet.named_parameters():
        assert torch.isfinite(p).all(), k


def test_baseline_config_properties(pai):
    """BASELINE.json configs[1]: 256x256, batch 64, bf16.  Size-independent properties:
    (1) the PatchGAN has no cross-sample coupling -> changing the other samples of a batch leaves a
        sample's logits bit-identical, and D on a half batch equals the matching half of D on the full
        batch up to bf16 rounding (the K split, i.e. the summation order, may depend on the batch size);
    (2) training-mode BatchNorm output of every BN layer has ~zero mean / unit variance per channel
        (checked on the normalised tensors the engine keeps);
    (3) accumulating the weight gradient twice doubles it; (4) a few GAN steps stay finite and the
        reconstruction term improves."""
    m = pai.Pix2Pix(1, 1, (1, 2, 4, 8, 8, 8, 8, 8), 0.0, "gan")
    torch.manual_seed(0)
    m.to(DEV)
    m.set_precision("bf16-mixed")
    m.train()
    rng = np.random.default_rng(1234)
    x = torch.from_numpy(rng.random((64, 1, 256, 256), dtype=np.float32) * 2 - 1).to(DEV)
    t = torch.from_numpy(rng.random((64, 1, 256, 256), dtype=np.float32) * 2 - 1).to(DEV)
    with torch.no_grad():
        full = m.discriminator(x, t)
        half = m.discriminator(x[:32].contiguous(), t[:32].contiguous())
        t2 = t.clone()
        t2[32:] = -t2[32:]
        other = m.discriminator(x, t2)
    # same launch configuration, different neighbours: bit-identical
    assert torch.equal(full[:32], other[:32]) and not torch.equal(full[32:], other[32:])
    # a different batch size may pick another K split (summation order): equal up to bf16 rounding
    assert torch.allclose(full[:32], half, rtol=2e-2, atol=2e-2)
    assert full.shape == (64, 1, 15, 15)

    eng = m.unet.engine
    pred, slot = eng.forward(x, True, 1, torch.bfloat16)
    torch.cuda.synchronize()
    L = eng.L
    for i in range(1, L - 1):
        C = eng.enc_c[i]
        a = slot["z"][i].float().view(-1, C)
        st = slot["ebn"][i]
        u = a * st.scale + st.shift
        bn = eng.enc_bn[i]
        xh = (u - bn.bias) / bn.weight
        assert float(xh.mean(0).abs().max()) < 2e-2, i
        if a.shape[0] >= 1024:
            assert float((xh.var(0, unbiased=False) - 1).abs().max()) < 5e-2, i
    eng.release(slot)
    assert pred.shape == (64, 1, 256, 256) and bool(torch.isfinite(pred).all())
    assert float(pred.abs().max()) <= 1.0

    first = None
    for s in range(4):
        m.logged = {}
        m.training_step((x, t), s)
        vals = {k: float(v) for k, v in m.logged.items()}
        assert all(np.isfinite(v) for v in vals.values()), vals
        first = first or vals
    assert vals["train_rmse"] < first["train_rmse"]
    assert int(m.unet.encoders[1].encode[2].num_batches_tracked) == 1 + 2 * 4  # manual forward + 2 per GAN step


def test_arena_adam_equals_stock_adam(pai):
    """The fused flat-arena optimizer step (pai_adam) and torch.optim.Adam produce the same
    parameters; state_dict round-trips through the standard per-parameter layout."""
    from thesis_pai_reconstruction_amd.optim import ArenaAdam
    mults, seed = (1, 2, 2, 4), 32
    x, t = synth_batch(seed + 100, 4, 32)
    batch = (x.to(DEV), t.to(DEV))
    ma, _, _ = build(pai, mults, "gan", seed)
    mb, _, _ = build(pai, mults, "gan", seed)
    assert all(isinstance(o, ArenaAdam) for o in ma.optimizers())
    mb._pai_optimizers = [torch.optim.Adam(mb.unet.parameters(), lr=2e-4, betas=(0.5, 0.999), eps=1e-7),
                          torch.optim.Adam(mb.discriminator.parameters(), lr=2e-4, betas=(0.5, 0.999), eps=1e-7)]
    for s in range(2):
        ma.training_step(batch, s)
        mb.training_step(batch, s)
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        if sa[k].is_floating_point():
            # element-wise agreement is limited by Adam's sign-SGD start (an element whose gradient is
            # ~eps moves by up to lr depending on summation order): compare in the L2 sense
            err = float((sa[k].double() - sb[k].double()).norm())
            assert err <= 1e-4 * max(float(sb[k].double().norm()), 1e-3), (k, err)
    osd = ma.optimizers()[0].state_dict()
    assert len(osd["state"]) == len(list(ma.unet.parameters()))
    st0 = osd["state"][0]
    assert float(st0["step"]) == 2 and st0["exp_avg"].shape == next(iter(ma.unet.parameters())).shape
    # the arena really is one flat buffer the parameters alias
    arena = ma.unet.engine.arena()
    assert arena.params_adopted()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_streaming_adam_equals_the_step_at_the_end(pai, monkeypatch, dtype):
    """ArenaAdam.arm_streaming: ranges of the arena are updated from the engine's gradient-ready hook while the backward
    pass is still running (from the second step on: the first fused step moves the parameters into the arena).  Same
    arithmetic as one step() at the end -- checked BIT FOR BIT: the twin model takes the ordinary step, but on the
    streamed model's gradients (two backward passes differ by fp32-atomics noise, and Adam's first steps turn a sign
    decided by that noise into +-lr; with the same gradients nothing is left to tolerate).  The hook is released after
    every step; an optimizer whose hook belongs to someone else (a gradient reducer) is left alone."""
    mults, seed = (1, 2, 2, 4), 35
    x, t = synth_batch(seed + 100, 4, 32)
    batch = (x.to(DEV), t.to(DEV))
    ma, _, _ = build(pai, mults, "gan", seed, dtype=dtype)
    mb, _, _ = build(pai, mults, "gan", seed, dtype=dtype)
    armed, twin_steps = [], []
    for o in ma.optimizers():
        orig = o.arm_streaming
        o.arm_streaming = (lambda orig=orig: armed.append(orig()) or armed[-1])
    for oa, ob in zip(ma.optimizers(), mb.optimizers()):
        def step(*a, oa=oa, ob=ob, orig=ob.step, **k):
            # the streamed model's gradients of this step are still in its arena (zeroed by its next backward pass)
            ob._engine.arena().flat.copy_(oa._engine.arena().flat)
            twin_steps.append(1)
            return orig(*a, **k)
        ob.step = step
    from importlib import import_module
    ops = import_module(pai.__name__ + ".ops")
    fused = []
    orig_adam_pack = ops.adam_pack
    monkeypatch.setattr(ops, "adam_pack", lambda *a, **k: fused.append(1) or orig_adam_pack(*a, **k))

    def packs_of(m):
        eg, ed = m.unet.engine, m.discriminator.engine
        return eg.enc_packs + eg.dec_packs + ed.packs

    for s in range(3):
        monkeypatch.setenv("PAI_NO_STREAM_ADAM", "0")
        ma.training_step(batch, s)
        assert ma.unet.engine.grad_ready_hook is None and ma.discriminator.engine.grad_ready_hook is None
        if s >= 1 and dtype == torch.bfloat16:
            # the streamed update wrote the bf16 filter packs of the dense layers itself (pai_adam_pack): only the thin
            # layers (1- and 2-channel ends of both networks) are left to re-pack
            stale = [pk._stale(dtype) for pk in packs_of(ma)]
            assert fused and sum(stale) <= 4 < len(stale), stale
        monkeypatch.setenv("PAI_NO_STREAM_ADAM", "1")
        mb.training_step(batch, s)
        torch.cuda.synchronize()
        sa, sb = ma.state_dict(), mb.state_dict()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (s, k)
        for oa, ob in zip(ma.optimizers(), mb.optimizers()):
            aa, ab = oa._engine.arena(), ob._engine.arena()
            assert torch.equal(aa.mflat, ab.mflat) and torch.equal(aa.vflat, ab.vflat) and torch.equal(aa.pflat, ab.pflat), s
        # ... and they are the packs a re-pack of the twin's (identical) master weights gives
        for k, (pa, pb) in enumerate(zip(packs_of(ma), packs_of(mb))):
            wfa, wda = pa.get(dtype)
            wfb, wdb = pb.get(dtype)
            assert torch.equal(wfa, wfb), (s, k)
            assert (wda is None) == (wdb is None) and (wda is None or torch.equal(wda, wdb)), (s, k)
    assert armed == [False, False, True, True, True, True]        # (D, G) per step; step 0 adopts the parameters
    assert len(twin_steps) == 6
    for oa, ob in zip(ma.optimizers(), mb.optimizers()):
        assert oa.total_steps == ob.total_steps == 3
        for (ka, va), (kb, vb) in zip(oa.state_dict()["state"].items(), ob.state_dict()["state"].items()):
            assert float(va["step"]) == float(vb["step"]) == 3
            assert torch.equal(va["exp_avg"], vb["exp_avg"]) and torch.equal(va["exp_avg_sq"], vb["exp_avg_sq"]), ka
    # a foreign hook owner: arming refuses and step() takes the ordinary path
    og = ma.optimizers()[0]
    ma.unet.engine.grad_ready_hook = lambda arena, end: None
    assert og.arm_streaming() is False
    ma.unet.engine.grad_ready_hook = None

def test_weight_gradients_issued_in_threes_equal_those_issued_one_by_one(pai, monkeypatch):
    """engine.py holds the weight gradients of the bottleneck layers (<= 1024 output pixels) back and issues three behind one
    fork of the side stream (PAI_WGRAD_BATCH, default 3).  Only the ORDER OF ISSUE changes: the gradient arena of a backward
    pass is the same -- bit for bit on the dense layers' weights (slab sums in split order), to rounding noise where fp32
    atomics add (bias gradients, thin layers)."""
    mults, seed = (1, 2, 2, 4), 41
    # every layer below the head has 4 x 16 x 16 output pixels or fewer and is a held one; the head has 4 x 32 x 32 = 4096,
    # above PAI_WGRAD_BATCH_PIX, and is issued at once (the held head: test_held_head_... below)
    x, t = synth_batch(seed + 100, 4, 32)
    batch = (x.to(DEV), t.to(DEV))
    monkeypatch.setenv("PAI_NO_STREAM_ADAM", "1")   # gradients stay in the arena until step()
    grads = []
    for n in ("1", "3", "2"):
        monkeypatch.setenv("PAI_WGRAD_BATCH", n)
        m, _, _ = build(pai, mults, "gan", seed, dtype=torch.bfloat16)
        og = m.optimizers()[0]
        seen = []
        orig = og.step
        og.step = lambda *a, orig=orig, og=og, **k: seen.append(og._engine.arena().flat.clone()) or orig(*a, **k)
        m.training_step(batch, 0)
        torch.cuda.synchronize()
        assert len(seen) == 1
        grads.append((seen[0], m.unet.engine))
    g1, eng = grads[0]
    arena = eng.arena()
    for g, _ in grads[1:]:
        assert torch.isfinite(g).all()
        scale = float(g1.abs().max())
        assert float((g - g1).abs().max()) <= 1e-5 * scale
        for conv in eng.enc_conv[1:] + eng.dec_conv[:-1]:
            a, n = arena.offsets[id(conv.weight)]
            assert torch.equal(g[a:a + n], g1[a:a + n]), conv


@pytest.mark.parametrize("n,size,loss_type", [(1, 32, "gan"), (4, 16, "mse")], ids=["1x32x32_gan", "4x16x16_mse"])
def test_held_head_weight_gradient_precedes_scratch_event_and_tail_fork(pai, monkeypatch, n, size, loss_type):
    """A head of at most PAI_WGRAD_BATCH_PIX (1024) output pixels is a HELD weight gradient: wgrad() only queues it.  Its
    thin kernel and encoder 0's (on the tail stream) both use the tail of the registered scratch buffer, so the order of
    issue has to be: head launch on the side stream -> scratch event recorded on that stream -> fork_tail() with the event
    marked, which makes the tail stream wait for it.  First step of a fresh model: the side stream does not exist yet when
    wgrad() returns.  (A PatchGAN needs 32 x 32 inputs, so the 16 x 16 batch trains against the MSE loss.)
    Then the gradients of that step against a run without any overlap (PAI_NO_OVERLAP=1): dense weights bit for bit, thin
    layers and biases (fp32 atomics) to 1e-5 of the largest gradient, as in the batching test above."""
    from thesis_pai_reconstruction_amd import engine as E, ops
    mults, seed = (1, 2), 43
    x, t = synth_batch(seed + 100, n, size)
    batch = (x.to(DEV), t.to(DEV))
    monkeypatch.setenv("PAI_NO_STREAM_ADAM", "1")   # gradients stay in the arena until step()
    log = []
    orig_wgrad, orig_record, orig_tail = ops.conv_wgrad, ops.Event.record, E._SideStream.fork_tail

    def spy_wgrad(d, *a, **k):
        if d.transposed and d.Cout == 1:
            log.append(("head", None, ops._stream()))
        return orig_wgrad(d, *a, **k)

    def spy_record(self, stream=None):
        log.append(("record", self, ops._raw(stream) if stream is not None else ops._stream()))
        return orig_record(self, stream)

    def spy_tail(self):
        log.append(("fork_tail", self, self._scratch_marked))
        return orig_tail(self)

    monkeypatch.setattr(ops, "conv_wgrad", spy_wgrad)
    monkeypatch.setattr(ops.Event, "record", spy_record)
    monkeypatch.setattr(E._SideStream, "fork_tail", spy_tail)

    def one_step():
        m, _, _ = build(pai, mults, loss_type, seed, dtype=torch.bfloat16)
        og = m.optimizers()
        og = og[0] if isinstance(og, (list, tuple)) else og
        seen = []
        orig = og.step
        og.step = lambda *a, orig=orig, og=og, **k: seen.append(og._engine.arena().flat.clone()) or orig(*a, **k)
        del log[:]
        m.training_step(batch, 0)
        torch.cuda.synchronize()
        assert len(seen) == 1 and torch.isfinite(seen[0]).all()
        return seen[0], m.unet.engine

    g, eng = one_step()
    side = eng._side
    assert side.on and side.stream is not None
    heads = [i for i, e in enumerate(log) if e[0] == "head"]
    recs = [i for i, e in enumerate(log) if e[0] == "record" and e[1] is side.scratch_ev]      # none while there is no event
    tails = [i for i, e in enumerate(log) if e[0] == "fork_tail" and e[1] is side]
    assert len(heads) == 1 and len(tails) == 1, log
    assert log[heads[0]][2] == side.stream.cuda_stream, "the head's weight gradient runs on the side stream"
    assert recs and heads[0] < recs[0] < tails[0], ("head launch -> scratch event -> fork_tail", [e[0] for e in log])
    assert log[recs[0]][2] == log[heads[0]][2], "the event is recorded on the stream of the head's launch"
    assert log[tails[0]][2] is True, "_scratch_marked when fork_tail() runs"

    monkeypatch.setenv("PAI_NO_OVERLAP", "1")
    g1, eng1 = one_step()
    assert not eng1._side.on and not [e for e in log if e[0] == "record" and e[1] is eng1._side.scratch_ev]
    scale = float(g1.abs().max())
    assert float((g - g1).abs().max()) <= 1e-5 * scale
    arena = eng1.arena()
    for conv in eng1.enc_conv[1:] + eng1.dec_conv[:-1]:
        a, cnt = arena.offsets[id(conv.weight)]
        assert torch.equal(g[a:a + cnt], g1[a:a + cnt]), conv


def test_dropout2d_step_matches_reference_fixture(pai, golden_dir):
    """Dropout2d(0.5) in the widest decoder blocks (the reference's class default, models/pix2pix.py:108,
    176-179): two generator forwards per GAN step, each with its own masks.  The masks the reference drew are
    recovered by the oracle (same torch generator, same draw order -- tests/test_oracle_golden.py pins that) and
    injected into the HIP engine; everything else must match the recorded step."""
    z = _load(golden_dir, "ref_gan_dropout_tiny")
    seed, n, size, steps = int(z["meta.seed"]), int(z["meta.n"]), int(z["meta.size"]), int(z["meta.steps"])
    mults, p = [int(v) for v in z["meta.mults"]], float(z["meta.dropout"])
    m, g, d = build(pai, mults, "gan", seed, dropout=p)
    assert not m.unet.supports_forward_reuse and sum(r > 0 for r in m.unet.engine.dec_drop) == 2
    x, t = synth_batch(seed + 100, n, size)
    batch = (x.to(DEV), t.to(DEV))
    og, od = oracle.AdamState(), oracle.AdamState()
    gkeys = set(g.keys())
    for s in range(steps):
        torch.manual_seed(1000 + s)
        mask_log = []
        oracle.gan_training_step(g, d, og, od, x, t, dropout=p, mask_log=mask_log)
        queue = list(mask_log)

        def replay(j, N, C, rate, device):
            jj, mk = queue.pop(0)
            assert jj == j and rate == p and mk.shape[:2] == (N, C)
            return mk.reshape(N, C).to(device)

        m.unet.engine.dropout_mask_fn = replay
        m.logged = {}
        m.training_step(batch, s)
        torch.cuda.synchronize()
        assert not queue
        for k, v in m.logged.items():
            want = float(z[f"step{s}.log.{k}"])
            assert abs(float(v) - want) <= 1e-4 * max(1.0, abs(want)), (s, k, float(v), want)
        for k, pp in m.unet.named_parameters():
            if _bias_before_bn(k, gkeys):
                continue
            tol = (2e-4 if pp.numel() > 1 else 2e-2) if s == 0 else 0.15 * s
            _fp_ok(pp.grad, z[f"step{s}.ggrad.{k}"], tol, f"step{s} ggrad {k}")
    # eval mode: Dropout2d is the identity
    m.unet.engine.dropout_mask_fn = None
    m.eval()
    m.logged = {}
    with torch.no_grad():
        m.validation_step(batch, 0)
    for k, v in m.logged.items():
        want = float(z[f"val.log.{k}"])
        assert abs(float(v) - want) <= 2e-3 * max(1.0, abs(want)), (k, float(v), want)
    # the engine's own draw: channels of a sample are either dropped or scaled by 1 / (1 - p)
    m.train()
    with torch.no_grad():
        m.unet(batch[0])


@pytest.mark.parametrize("family", ["pix2pix", "resnext_unet"])
def test_ema_update_is_a_fused_pass_with_torch_ema_arithmetic(pai, family):
    """callbacks.EMACallback on the device (reference callbacks/ema.py:24-52 -> torch_ema): pai_lerp_multi over memory
    segments -- the parameters of a HIP engine are one segment once its optimizer has adopted them into the arena -- with
    torch_ema's own arithmetic (shadow -= (1 - d) * (shadow - p), warm-up decay), bit for bit; swap-in / restore around
    validation keeps the engines' packs current (the eval forward really runs on the shadow weights)."""
    from thesis_pai_reconstruction_amd.callbacks import EMACallback
    seed = 77
    x, t = synth_batch(seed + 100, 4, 32)
    batch = (x.to(DEV), t.to(DEV))
    if family == "pix2pix":
        m, _, _ = build(pai, (1, 2, 2, 4), "gan", seed)
    else:
        m = pai.ResUnetGAN(1, 1, "next", (1, 2, 2), 0.0, "gan").to(DEV)
        m.set_precision("32")
        m.train()
    cb = EMACallback(decay=0.9)
    cb.on_fit_start(None, m)
    ref = [p.detach().cpu().clone() for p in cb.params]
    for n in range(1, 5):
        m.training_step(batch, n - 1)
        cb.on_train_batch_end(None, m)
        w = 1.0 - min(0.9, (1 + n) / (10 + n))
        for r, p in zip(ref, cb.params):
            tmp = r - p.detach().cpu()
            tmp.mul_(w)
            r.sub_(tmp)
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(cb.shadow, ref)):
        assert torch.equal(s.cpu(), r), k
    nseg, npar = len(cb._segments), len(cb.params)
    # the two engines' arenas (pix2pix), or the generator's separately allocated tensors + the discriminator's arena
    assert nseg <= (4 if family == "pix2pix" else npar) and nseg < npar, (nseg, npar)
    live = [p.detach().clone() for p in cb.params]
    m.eval()
    with torch.no_grad():
        out_live = m(batch[0]).clone()
        cb.on_validation_start(None, m)
        for p, r in zip(cb.params, ref):
            assert torch.equal(p.detach().cpu(), r)
        out_ema = m(batch[0]).clone()
        cb.on_validation_end(None, m)
        out_back = m(batch[0]).clone()
    for p, l in zip(cb.params, live):
        assert torch.equal(p.detach(), l)
    assert torch.equal(out_back, out_live) and not torch.equal(out_ema, out_live)


def test_device_side_step_count_equals_host_side(pai):
    """ArenaAdam.enable_device_step (pai_adam_dev: the step count in device memory, for callers that capture step() into
    a hipGraph of their own) against the ordinary host-side count: same parameters and moments after three steps."""
    mults, seed = (1, 2, 2, 4), 41
    x, t = synth_batch(seed + 100, 4, 32)
    batch = (x.to(DEV), t.to(DEV))
    ma, _, _ = build(pai, mults, "gan", seed)
    mb, _, _ = build(pai, mults, "gan", seed)
    os.environ["PAI_NO_STREAM_ADAM"] = "1"        # the streamed update needs the host-side count
    try:
        for m in (ma, mb):
            m.training_step(batch, 0)                 # the first fused step adopts the parameters into the arenas
        from _gpu_util import sync_training_state
        sync_training_state(ma, mb)
        for opt in mb.optimizers():
            opt.enable_device_step()
        for s in range(1, 4):
            ma.training_step(batch, s)
            mb.training_step(batch, s)
    finally:
        os.environ.pop("PAI_NO_STREAM_ADAM", None)
    torch.cuda.synchronize()
    for oa, ob in zip(ma.optimizers(), mb.optimizers()):
        assert int(ob._dev_step) == 4 and ob.total_steps == oa.total_steps == 4
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        if sa[k].is_floating_point():
            err = float((sa[k].double() - sb[k].double()).norm())
            assert err <= 1e-4 * max(float(sb[k].double().norm()), 1e-3), (k, err)
