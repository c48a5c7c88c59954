"""The PatchGAN head with its loss in one launch (pai_head_loss) and the fp32 + addend store of block 0's input gradient
(pai_conv_dgrad_f32add) against the launches they replace: conv_fwd -> bce_logits (per half) -> cast -> conv_dgrad_act, and
conv_dgrad(only_c2) -> cast -> add_act.  Same expressions in the same order: logits, the bf16 logit gradient, the head's
input gradient and the fp32 image gradient have EQUAL BITS (compared as integers: a NaN payload counts); the loss scalar
is summed per image instead of per half (fp64), i.e. differs by at most one ulp of the fp32 value it is rounded to, and is
the same from launch to launch (exact additions: the order of the atomics does not matter).

The node-level cases run one seeded bf16 Discriminator twice, PAI_HEAD_FUSED=0 (the separate launches) and 1.  Gradients
behind the thin weight-gradient kernels (fp32 atomics: their summation order differs from run to run) are held to the 4e-2
relative error tests/test_gpu_discblock.py uses for the bf16 weight / bias gradients of a discriminator block; the gradient
w.r.t. the generated image passes deterministic kernels only and is held to equal bits."""
import numpy as np
import pytest
import torch

import oracle
from oracle.gen_golden import synth_batch
from _gpu_util import rel_err, rnd, sync_training_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
WGRAD_TOL = 4e-2        # tests/test_gpu_discblock.py: bf16 weight / bias gradients of a discriminator block


def _disc(pai, seed=5):
    from thesis_pai_reconstruction_amd.models.wrapper import Discriminator
    d = Discriminator(1)
    d.load_state_dict(oracle.init_state_portable(oracle.make_disc_state(1), seed))
    d.to(DEV)
    d.compute_dtype = BF
    return d


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def _one_ulp(a: float, b: float) -> bool:
    a32, b32 = np.float32(a), np.float32(b)
    return bool(a32 == b32 or np.nextafter(a32, b32) == b32)


def _separate(ops, eng, S, n_first, t_first, t_rest):
    """The launches pai_head_loss replaces, on the slot's a[3]: logits, fp64 loss sum, bf16 dl, du[3]."""
    P = S["P"]
    d = P["desc"][4]
    wf, wd = eng.packs[4].get(BF)
    logits = torch.empty_like(S["logits"])
    ops.conv_fwd(d, S["a"][3], None, wf, None, y_f32=logits)
    flat = logits.view(-1)
    k = (flat.numel() // logits.shape[0]) * min(n_first, logits.shape[0])
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    grad = torch.empty_like(flat)
    if k > 0:
        ops.bce_logits(flat[:k], t_first, 1.0, acc, 1.0, grad[:k])
    if k < flat.numel():
        ops.bce_logits(flat[k:], t_rest, 1.0, acc, 1.0, grad[k:])
    dl = torch.empty(flat.numel(), dtype=BF, device=DEV)
    ops.cast(grad, dl)
    du = torch.empty_like(S["a"][3])
    ops.conv_dgrad_act(d, dl, wd, du, None, S["a"][3], ops.ACT_LRELU)
    return logits, acc, dl, grad, du


def _fused(ops, eng, S, n_first, t_first, t_rest):
    d = S["P"]["desc"][4]
    wf, wd = eng.packs[4].get(BF)
    logits = torch.empty_like(S["logits"])
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    dl = torch.empty(logits.numel(), dtype=BF, device=DEV)
    dl32 = torch.empty(logits.numel(), dtype=torch.float32, device=DEV)
    du = torch.empty_like(S["a"][3])
    ops.head_loss(d, S["a"][3], wf, wd, n_first, t_first, t_rest, 1.0, acc, 1.0, logits, dl, dl32, du, ops.ACT_LRELU)
    return logits, acc, dl, dl32, du


def _compare(ops, eng, S, n_first, t_first, t_rest, tag):
    assert ops.head_loss_ok(S["P"]["desc"][4]), tag
    lo, acco, dlo, go, duo = _separate(ops, eng, S, n_first, t_first, t_rest)
    ln, accn, dln, gn, dun = _fused(ops, eng, S, n_first, t_first, t_rest)
    torch.cuda.synchronize()
    assert torch.equal(_bits(lo), _bits(ln)), (tag, "logits")
    assert torch.equal(_bits(dlo), _bits(dln)), (tag, "dl")
    assert torch.equal(_bits(go), _bits(gn)), (tag, "fp32 dl")
    assert torch.equal(_bits(duo), _bits(dun)), (tag, "du")
    a, b = float(acco.float()), float(accn.float())
    print(f"{tag}: loss separate {a!r} fused {b!r}")
    assert (np.isnan(a) and np.isnan(b)) or _one_ulp(a, b), (tag, a, b)


# (N, H, W of the images, second batch, n_first): head pixels 2x2 (one logit, every tap row / column partly outside),
# 3x4 (OW != OH, no power of two), 16x16 (the benchmark's), unequal halves at batch 3, one target for the whole batch
# (n_first = 2N), and N = 8 at 4x4 pixels: the only geometry with the workgroups of an image eight apart.
CASES = [(2, 32, 32, True, 2), (2, 48, 64, True, 2), (2, 256, 256, False, 1), (3, 48, 64, False, 1), (3, 32, 32, False, 2),
         (2, 48, 64, False, 4), (8, 64, 64, False, 5)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_%s_first%d" % (c[0], c[1], c[2], "pairs" if c[3] else "one", c[4]))
def test_head_loss_kernel_matches_separate_launches(pai, case):
    from thesis_pai_reconstruction_amd import ops
    n, h, w, pairs, n_first = case
    disc = _disc(pai)
    eng = disc.engine
    x, y, y2 = (rnd((n, 1, h, w), 40 + i).clamp(-1, 1).to(DEV) for i in range(3))
    _, S = eng.forward(x, y, BF, y2=y2 if pairs else None)
    t_first, t_rest = (1.0, 0.0) if n_first < S["P"]["N"] else (1.0, 1.0)
    _compare(ops, eng, S, n_first, t_first, t_rest, str(case))
    eng.release(S)


def test_head_loss_sum_does_not_depend_on_atomic_order(pai):
    """One fp64 atomic per image arrives in any order.  The loss of a step must still be the same number on every launch:
    the per-image totals of fp32 terms put the exact sum ON an fp32 rounding boundary once in a few dozen steps, where an
    order-dependent last bit of the fp64 sum would flip the logged loss (tests/test_gpu_plan.py holds d_loss of two runs from
    one state to equality).  32 images, 30 launches: the fp64 accumulator has the same bits every time."""
    from thesis_pai_reconstruction_amd import ops
    disc = _disc(pai)
    eng = disc.engine
    x, y = (rnd((32, 1, 64, 64), 45 + i).clamp(-1, 1).to(DEV) for i in range(2))
    _, S = eng.forward(x, y, BF)
    seen = set()
    for _ in range(30):
        _, acc, _, _, _ = _fused(ops, eng, S, 16, 1.0, 0.0)
        seen.add(int(acc.view(torch.int64).cpu()[0]))
    assert len(seen) == 1, seen
    eng.release(S)


def test_head_loss_kernel_nonfinite_pixels(pai):
    """+inf, -inf and NaN in the head's input: the same bits as the separate launches, NaN payloads included."""
    from thesis_pai_reconstruction_amd import ops
    disc = _disc(pai)
    eng = disc.engine
    x, y = (rnd((2, 1, 128, 128), 50 + i).clamp(-1, 1).to(DEV) for i in range(2))
    _, S = eng.forward(x, y, BF)
    a3 = S["a"][3].view(2, 8, 8, -1)
    a3[0, 1, 1, 3] = float("inf")
    a3[0, 6, 5, 100] = float("-inf")
    a3[1, 4, 4, 7] = float("nan")
    _compare(ops, eng, S, 1, 1.0, 0.0, "nonfinite")
    eng.release(S)


@pytest.mark.parametrize("size", [32, 64])
def test_thin_up_f32_addend_matches_three_launches(pai, size):
    from thesis_pai_reconstruction_amd import ops
    disc = _disc(pai)
    eng = disc.engine
    n = 2
    x, y = (rnd((n, 1, size, size), 55 + i).clamp(-1, 1).to(DEV) for i in range(2))
    _, S = eng.forward(x, y, BF)      # plans, workspaces and the current packs
    d = S["P"]["desc"][0]
    eng.release(S)
    assert ops.conv_dgrad_f32add_ok(d)
    _, wd = eng.packs[0].get(BF)
    du0 = rnd((n * (size // 2) * (size // 2) * 64,), 60, 0.05).to(DEV).to(BF)
    gp = rnd((n * size * size,), 61).to(DEV)
    dy = torch.empty(n * size * size, dtype=BF, device=DEV)
    ops.conv_dgrad(d, du0, wd, None, dy, only_c2=True)
    want = torch.empty(n * size * size, dtype=torch.float32, device=DEV)
    ops.cast(dy, want)
    ops.add_act(torch.float32, want, gp, ops.ACT_NONE, want)
    got = torch.empty_like(want)
    ops.conv_dgrad_f32add(d, du0, wd, gp, got)
    torch.cuda.synchronize()
    assert float(dy.float().abs().max()) > 0
    assert torch.equal(_bits(want), _bits(got))


def _grads(disc):
    return [p.grad.detach().clone() for p, _ in disc.engine.ordered_params()]


def _run_pairs(PF, disc, x, t, p, seed_scale):
    disc.zero_grad(set_to_none=True)
    loss = disc.pairs_loss(x, t, p)
    if seed_scale == 1.0:
        loss.backward(gradient=PF.unit_seed(loss.device))
    else:
        (seed_scale * loss).backward()
    torch.cuda.synchronize()
    return float(loss), _grads(disc)


def _run_gen(PF, disc, x, p, t, seed_scale):
    disc.zero_grad(set_to_none=True)
    pr = p.clone().requires_grad_(True)
    loss = disc.generator_loss(x, pr, t, 50.0)
    if seed_scale == 1.0:
        loss.backward(gradient=PF.unit_seed(loss.device))
    else:
        (seed_scale * loss).backward()
    torch.cuda.synchronize()
    return float(loss), _grads(disc), pr.grad.detach().clone()


@pytest.mark.parametrize("size", [(32, 32), (48, 64)], ids=lambda s: "%dx%d" % s)
def test_nodes_fused_against_separate(pai, monkeypatch, size):
    from thesis_pai_reconstruction_amd import functional as PF
    from thesis_pai_reconstruction_amd import ops
    disc = _disc(pai)
    x, t, p = (rnd((2, 1) + size, 70 + i).clamp(-1, 1).to(DEV) for i in range(3))
    calls = []
    real = ops.head_loss
    monkeypatch.setattr(ops, "head_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    monkeypatch.setenv("PAI_HEAD_FUSED", "0")
    want = PF.gan_discriminator_loss_pairs(disc.forward_pairs(x, t, p), 2)
    ld0, gd0 = _run_pairs(PF, disc, x, t, p, 1.0)
    lg0, gg0, gp0 = _run_gen(PF, disc, x, p, t, 1.0)
    assert not calls and float(want) == ld0      # the switch: the separate launches, the value of the two separate nodes
    monkeypatch.setenv("PAI_HEAD_FUSED", "1")
    ld1, gd1 = _run_pairs(PF, disc, x, t, p, 1.0)
    lg1, gg1, gp1 = _run_gen(PF, disc, x, p, t, 1.0)
    assert len(calls) == 2
    print(f"d_loss {ld0!r} / {ld1!r}, g loss {lg0!r} / {lg1!r}")
    assert _one_ulp(ld0, ld1) and _one_ulp(lg0, lg1)
    # the image gradient: du[3] -> three deterministic input gradients -> thin_up_k (+ the L1 term in its store)
    assert torch.equal(_bits(gp0), _bits(gp1))
    for a, b in zip(gd0 + gg0, gd1 + gg1):
        assert rel_err(b, a) < WGRAD_TOL

    # any other seed: the fp32 logit gradient is scaled, the head's input gradient is a launch of its own
    ld2, gd2 = _run_pairs(PF, disc, x, t, p, 2.0)
    lg2, gg2, gp2 = _run_gen(PF, disc, x, p, t, 2.0)
    assert len(calls) == 4 and _one_ulp(ld2, ld1) and _one_ulp(lg2, lg1)
    for a, b in zip(gd1 + gg1 + [gp1], gd2 + gg2 + [gp2]):
        assert rel_err(b, 2.0 * a) < WGRAD_TOL


def test_fp32_discriminator_keeps_the_separate_launches(pai, monkeypatch):
    """fp32 storage is outside the predicate: both nodes fall back without a word, same values as the separate nodes."""
    from thesis_pai_reconstruction_amd import functional as PF
    from thesis_pai_reconstruction_amd import ops
    disc = _disc(pai)
    disc.compute_dtype = torch.float32
    monkeypatch.setattr(ops, "head_loss", lambda *a, **k: pytest.fail("pai_head_loss on fp32 storage"))
    x, t, p = (rnd((2, 1, 32, 32), 80 + i).clamp(-1, 1).to(DEV) for i in range(3))
    want = float(PF.gan_discriminator_loss_pairs(disc.forward_pairs(x, t, p), 2))
    got, grads = _run_pairs(PF, disc, x, t, p, 1.0)
    assert got == want and all(bool(torch.isfinite(g).all()) for g in grads)
    lg, _, gp = _run_gen(PF, disc, x, p, t, 1.0)
    assert np.isfinite(lg) and bool(torch.isfinite(gp).all())


def test_planned_step_replays_with_the_fused_nodes(pai, monkeypatch):
    """tests/test_gpu_plan.py's protocol at batch 2, 64 x 64: d_loss equal, loss within 1e-4 of the eager step from the same
    state; the recorded steps went through pai_head_loss (twice per step: discriminator and generator phase)."""
    from thesis_pai_reconstruction_amd import ops
    from thesis_pai_reconstruction_amd.plan import PlannedStep
    monkeypatch.setenv("PAI_HEAD_FUSED", "1")
    calls = []
    real = ops.head_loss
    monkeypatch.setattr(ops, "head_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def build():
        m = pai.Pix2Pix(1, 1, (1, 2, 4, 8), 0.0, "gan")
        m.unet.load_state_dict(oracle.init_state_portable(oracle.make_unet_state(1, 1, (1, 2, 4, 8)), 3, perturb_bn=True))
        m.discriminator.load_state_dict(oracle.init_state_portable(oracle.make_disc_state(1), 4))
        m.to(DEV)
        m.set_precision("bf16-mixed")
        m.train()
        return m
    eager, planned = build(), build()
    ps = PlannedStep(planned, warmup=3)
    steps = 8
    for s in range(steps):
        b = tuple(t.to(DEV) for t in synth_batch(100 + s, 2, 64))
        eager.logged, planned.logged = {}, {}
        before = len(calls)
        eager.training_step(b, s)
        assert len(calls) == before + 2
        ps(b, s)
        torch.cuda.synchronize()
        assert ps.disabled is None, ps.disabled
        for k in ("d_loss", "loss"):
            a, g = float(eager.logged[k]), float(planned.logged[k])
            print(s, k, a, g)
            assert (abs(a - g) <= 1e-4 * max(1.0, abs(a))) if k == "loss" else a == g, (s, k, a, g)
        sync_training_state(eager, planned)
    assert ps.replays >= 2, ps.describe()
    # a replayed step issues no Python-side call: eager 2 per step, planned 2 per warm-up / recorded step
    assert len(calls) == 2 * steps + 2 * (steps - ps.replays)
