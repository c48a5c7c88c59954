"""CPU: the fp64 references of tests/_step_ref.py against PyTorch's own double-precision ops, autograd and torch.optim.Adam,
to 1e-12, at a few of the shapes tests/test_gpu_step_ops.py uses -- a wrong reference cannot then be "fixed" by bending a
bound over there.  Also the CPU measurements the bounds of that file rest on: the error of torch's own fp32
binary_cross_entropy_with_logits / sigmoid against fp64 (printed, and compared with the constants recorded in _step_ref), an
fp32 emulation of adam1 against the Adam bounds, and an fp32 emulation of the InstanceNorm statistics in the kernel's
summation order against the a-priori rstd bound of the offset case and the constant-plane bound."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _step_ref as R
from _gpu_util import max_err, rnd

D = torch.float64
ACTS = [R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU]


def _close(got, want, what, tol=1e-12):
    e = max_err(got, want)
    assert e < tol, (what, e)


def _torch_act(v, act):
    return F.relu(v) if act == R.ACT_RELU else (F.leaky_relu(v, R.SLOPE) if act == R.ACT_LRELU else v)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("betas", R.ADAM_BETAS, ids=str)
def test_adam_ref_is_torch_optim_adam_in_fp64(step, betas):
    """With exact coefficients the reference is torch.optim.Adam (fp64, no weight decay / amsgrad) at step ``step``, on the
    slices of every GPU case (g = 0 with v0 = 0, g = 1e-20, g = 1e18, p0 = 0, |p0| ~ 1e3)."""
    p0, g, m0, v0 = (t.to(D) for t in R.adam_inputs(6000, 7))
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=R.ADAM_LR, betas=betas, eps=R.ADAM_EPS, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = g.clone()
    opt.step()
    ref = R.adam(p0, g, m0, v0, R.adam_exact_coeffs(R.ADAM_LR, betas[0], betas[1], step), R.ADAM_EPS)
    assert int(opt.state[p]["step"]) == step
    _close(ref["m"], opt.state[p]["exp_avg"], "m")
    _close(ref["v"], opt.state[p]["exp_avg_sq"], "v")
    # the update on its own, where p0 = 0 does not hide it; and p where p0 dominates
    _close(p0 - ref["p"], p0 - p.detach(), "delta", 1e-11)
    _close(ref["delta"], p0 - p.detach(), "delta as returned", 1e-11)
    _close(ref["p"], p.detach(), "p")
    assert bool(torch.isfinite(ref["p"]).all()) and bool((ref["v"] >= 0).all())
    assert bool((ref["m_abs"] + 1e-300 >= ref["m"].abs()).all()) and bool((ref["v_abs"] == ref["v"].abs()).all())


def test_adam_kernel_coefficients():
    """The fp32 constants the kernels are launched with: fp32 arguments, omb = float32(1 - double(beta_f32)), the two step
    coefficients rounded once from double."""
    c = R.adam_coeffs(2e-4, 0.5, 0.999, 1)
    assert c["b1"] == 0.5 and c["omb1"] == 0.5 and c["b2"] == float(np.float32(0.999))
    assert c["omb2"] == float(np.float32(1.0 - float(np.float32(0.999)))) and c["omb2"] != float(np.float32(0.001))
    assert c["lr_over_bc1"] == float(np.float32(float(np.float32(2e-4)) / 0.5))
    for step in R.ADAM_STEPS:
        c, e = R.adam_coeffs(2e-4, 0.9, 0.999, step), R.adam_exact_coeffs(2e-4, 0.9, 0.999, step)
        for k in ("lr_over_bc1", "inv_sqrt_bc2", "omb1", "omb2"):
            assert abs(c[k] / e[k] - 1) < 1e-4, (step, k)       # fp32(0.999) is 2e-8 off 0.999: 2e-5 of 1 - beta2
    # a late step is not step 1: the bias corrections have gone
    assert R.adam_coeffs(2e-4, 0.9, 0.999, 100000)["inv_sqrt_bc2"] == 1.0
    assert R.adam_coeffs(2e-4, 0.9, 0.999, 1)["lr_over_bc1"] > 9.9 * R.adam_coeffs(2e-4, 0.9, 0.999, 1000)["lr_over_bc1"]


@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("betas", R.ADAM_BETAS, ids=str)
def test_adam_fp32_emulation_is_inside_the_bounds(step, betas):
    """adam1 operation by operation in numpy fp32 against the fp64 reference with the same fp32 coefficients: inside the
    three bounds the GPU test uses, so the reference and the bounds are consistent before any kernel is asked.  Printed:
    the largest error / bound, and the largest error of the update per |delta| on the p0 = 0 slice."""
    c = R.adam_coeffs(R.ADAM_LR, betas[0], betas[1], step)
    p0, g, m0, v0 = R.adam_inputs(60000, 3)
    ref = R.adam(p0, g, m0, v0, c, float(np.float32(R.ADAM_EPS)))
    p, m, v = R.adam_f32_emulation(p0, g, m0, v0, c, np.float32(R.ADAM_EPS))
    lim_m, lim_v, lim_p = R.adam_bounds(ref, c)
    rm, rv, rp = (float(((a.double() - ref[k]).abs() / l).max()) for a, k, l in ((m, "m", lim_m), (v, "v", lim_v), (p, "p", lim_p)))
    k = 10000
    upd = float(((p[:k].double() - ref["p"][:k]).abs() / ref["delta"][:k].abs().clamp_min(1e-300)).max())
    print(f"adam fp32 emulation step {step} betas {betas}: err / bound m {rm:.3g}, v {rv:.3g}, p {rp:.3g}; "
          f"update error per |delta| (p0 = 0) {upd:.3g}")
    assert rm <= 1 and rv <= 1 and rp <= 1
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all())


def test_adam_overflowing_square_in_kind():
    """g = 1e21: torch.optim.Adam in fp32 (the formula the kernel restates) has v = +inf and leaves p where it was; the fp32
    emulation of adam1 does the same, and ``fp32_range`` makes the fp64 reference say so.  g = 1e18 does not overflow."""
    betas, step = (0.9, 0.999), 2
    p0, g, m0, v0 = R.adam_overflow_inputs(4099, 9)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=R.ADAM_LR, betas=betas, eps=R.ADAM_EPS, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = g.clone()
    opt.step()
    c = R.adam_coeffs(R.ADAM_LR, betas[0], betas[1], step)
    ref = R.adam(p0, g, m0, v0, c, float(np.float32(R.ADAM_EPS)), fp32_range=True)
    over = torch.isinf(ref["v"])
    assert bool(over[0::2].all()) and not bool(over[1::2].any())
    pe, me, ve = R.adam_f32_emulation(p0, g, m0, v0, c, np.float32(R.ADAM_EPS))
    for what, pp, vv, mm in (("torch fp32", p.detach(), opt.state[p]["exp_avg_sq"], opt.state[p]["exp_avg"]), ("emulation", pe, ve, me)):
        assert torch.equal(torch.isinf(vv) & (vv > 0), over), what
        assert torch.equal(pp[over], p0[over]) and torch.equal(ref["p"][over], p0[over].double()), what
        assert bool(torch.isfinite(mm).all()) and bool(torch.isfinite(pp).all()), what
    plain = R.adam(*R.adam_inputs(6000, 7), c, float(np.float32(R.ADAM_EPS)), fp32_range=True)
    assert bool(torch.isfinite(plain["v"]).all()) and float(plain["v"].max()) > 1e32       # g = 1e18: v ~ 1e33, finite


# ---- losses -------------------------------------------------------------------------------------------------------------------
def test_loss_refs():
    x, t = rnd((4099,), 1).to(D), rnd((4099,), 2).to(D)
    t[:50] = x[:50]
    xr = x.clone().requires_grad_(True)
    F.l1_loss(xr, t, reduction="sum").backward()
    r = R.l1(x, t)
    _close(r["sum"], F.l1_loss(x, t, reduction="sum"), "l1")
    assert torch.equal(r["grad"], xr.grad) and float(r["grad"][:50].abs().max()) == 0.0
    # -0 against +0: an exact zero difference
    assert float(R.l1(torch.tensor([-0.0]), torch.tensor([0.0]))["grad"][0]) == 0.0
    xr = x.clone().requires_grad_(True)
    F.mse_loss(xr, t, reduction="sum").backward()
    r = R.mse(x, t)
    _close(r["sum"], F.mse_loss(x, t, reduction="sum"), "mse")
    _close(r["grad"], xr.grad, "mse grad")


@pytest.mark.parametrize("target", R.BCE_TARGETS)
def test_bce_ref(target):
    x = R.bce_logits(5000).to(D)
    assert set(torch.tensor(R.BCE_SPECIALS, dtype=torch.float32).double().tolist()) <= set(x.tolist())
    xr = x.clone().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(xr, torch.full_like(x, float(np.float32(target))), reduction="none")
    want.sum().backward()
    l, g = R.bce_terms(x, target)
    assert float(((l - want.detach()).abs() / (1 + x.abs())).max()) < 1e-15
    assert float((g - xr.grad).abs().max()) < 1e-15
    assert bool(torch.isfinite(l).all()) and bool(torch.isfinite(g).all())
    # the tails keep their relative accuracy: sigmoid(-100) = e^-100, loss(+100, t = 1) = log1p(e^-100) = e^-100
    l1_, g0 = R.bce_terms(torch.tensor([100.0]), 1.0)[0], R.bce_terms(torch.tensor([-100.0]), 0.0)[1]
    assert abs(float(l1_) / math.exp(-100.0) - 1) < 1e-12 and abs(float(g0) / math.exp(-100.0) - 1) < 1e-12


def test_torch_fp32_bce_error_is_what_the_gpu_bounds_assume():
    """The measurement behind BCE_TORCH_ERR / BCE_GRAD_TORCH_ERR of tests/_step_ref.py (the BCE bounds of
    tests/test_gpu_step_ops.py are four times these): the error of PyTorch-CPU's own fp32 BCE-with-logits per unit of
    1 + |x| and of sigmoid(x) - t, against fp64, over the logits of the largest GPU case, printed.  One-sided: what the GPU
    bound needs is that the recorded constants do not undercut the reference's own error by more than a margin (10 %)."""
    e_l, e_g = R.torch_fp32_bce_error(R.BCE_NUMELS[-1])
    print(f"torch fp32 CPU BCE with logits: max err / (1 + |x|) {e_l:.4g} (recorded {R.BCE_TORCH_ERR:.4g}); "
          f"sigmoid(x) - t: {e_g:.4g} (recorded {R.BCE_GRAD_TORCH_ERR:.4g})")
    # a two-sided 10 % window: the recorded constants can be neither too small for this machine's torch nor inflated
    assert 0.9 * R.BCE_TORCH_ERR <= e_l <= 1.1 * R.BCE_TORCH_ERR and 0.9 * R.BCE_GRAD_TORCH_ERR <= e_g <= 1.1 * R.BCE_GRAD_TORCH_ERR
    assert 4 * R.BCE_TORCH_ERR < 1e-5 and 4 * R.BCE_GRAD_TORCH_ERR < 1e-5      # the caps are not the binding part


def test_metrics_and_denormalize_refs():
    import oracle
    a, b = torch.rand(2, 1, 16, 16, dtype=D), torch.rand(2, 1, 16, 16, dtype=D)
    sse = float(((a - b) ** 2).sum())
    m = R.metrics_take(1.25, sse, 2, a.numel())
    assert m[0] == 0.625
    assert abs(m[1] - float(oracle.psnr(a, b))) < 1e-12 and abs(m[2] - float(oracle.rmse(a, b))) < 1e-14
    same = R.metrics_take(2.0, 0.0, 2, a.numel())
    assert same[1] == float(oracle.psnr(a, a)) == math.inf and same[2] == 0.0
    # denormalize: the oracle keeps a NaN and clamps the infinities; its backward is 0 outside, 0.5 on the closed boundaries
    x = R.denorm_specials().clone().requires_grad_(True)
    y = oracle.denormalize(x)
    y.backward(torch.ones_like(x))
    y = y.detach()
    assert math.isnan(float(y[8])) and float(y[6]) == 1.0 and float(y[7]) == 0.0
    u = x.detach() * 0.5 + 0.5
    assert torch.equal(x.grad, torch.where((u >= 0) & (u <= 1), 0.5, 0.0))
    # x = -1 and x = +1 give u = 0 and u = 1: the closed boundaries pass the gradient; one ulp below -1 does not; one ulp above
    # +1 rounds to u = 1 and does; NaN and the infinities do not
    assert x.grad[[0, 3, 5]].tolist() == [0.5] * 3 and x.grad[[2, 6, 7, 8]].tolist() == [0.0] * 4


# ---- MaxPool / Upsample / activations ---------------------------------------------------------------------------------------------
def test_maxpool_ref_conventions():
    """What the reference (torch's max_pool2d and its autograd) does at ties and NaNs: the first maximum of a window in
    row-major order wins, a NaN beats everything, the LAST NaN of a window wins."""
    nan, inf = float("nan"), float("inf")
    wins = [[2, 2, 1, 2], [0, 0, 0, 0], [-inf, -inf, -inf, -inf], [-0.0, 0.0, 0.0, -0.0], [1, nan, 5, 0], [nan, 7, nan, 1]]
    first = [0, 0, 0, 0, 1, 2]
    x = torch.tensor(wins, dtype=torch.float32).view(6, 2, 2, 1)       # [N][H][W][C]
    out, bwd = R.maxpool2(x)
    dx = bwd(torch.full((6, 1, 1, 1), 3.0)).view(6, 4)
    for i, k in enumerate(first):
        want = torch.zeros(4)
        want[k] = 3.0
        assert torch.equal(dx[i], want), (i, dx[i])
    assert math.copysign(1.0, float(out[3])) == -1.0 and float(out[2]) == -inf and math.isnan(float(out[4]))
    up = R.upsample2(torch.arange(12.0).view(1, 2, 3, 2))
    assert torch.equal(up, F.interpolate(torch.arange(12.0).view(1, 2, 3, 2).permute(0, 3, 1, 2), scale_factor=2,
                                         mode="nearest").permute(0, 2, 3, 1))
    d = rnd((2, 4, 6, 3), 5).to(D)
    xr = torch.zeros(2, 3, 2, 3, dtype=D, requires_grad=True)
    F.interpolate(xr, scale_factor=2, mode="nearest").backward(d.permute(0, 3, 1, 2))
    s, ab = R.upsample2_bwd(d)
    _close(s, xr.grad.permute(0, 2, 3, 1), "upsample2_bwd")
    assert bool((ab + 1e-300 >= s.abs()).all())


@pytest.mark.parametrize("act", ACTS)
def test_activation_refs_and_the_kink(act):
    v = torch.cat([rnd((500,), 3).to(D), torch.tensor([0.0, -0.0, 1e-300, -1e-300], dtype=D)])
    vr = v.clone().requires_grad_(True)
    y = _torch_act(vr, act)
    y.backward(torch.ones_like(v))
    assert torch.equal(R.act_fwd(v, act), y.detach())
    # torch's convention at +0 / -0: the slope of the negative side (0 for ReLU, 0.2 for LeakyReLU)
    assert torch.equal(R.act_grad(v, act), vr.grad)
    assert R.act_grad(torch.tensor([0.0, -0.0]), act).tolist() == {R.ACT_NONE: [1, 1], R.ACT_LRELU: [R.SLOPE] * 2,
                                                                   R.ACT_RELU: [0, 0]}[act]
    # through the stored, activated value the sign (and so the derivative) is the same
    assert torch.equal(R.act_grad(y.detach(), act), vr.grad)
    a, b, g1, g2 = (rnd((504,), s).to(D) for s in (4, 5, 6, 7))
    assert torch.equal(R.add_act(a, b, act), _torch_act(a + b, act))
    du, ab = R.act_bwd(g1, act, g2, R.ACT_RELU, v)
    _close(du, g1 * vr.grad + g2 * (v > 0), "act_bwd")
    assert bool((ab + 1e-300 >= du.abs()).all())


# ---- InstanceNorm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("HW,C", [(1, 8), (7, 24), (33, 72)])
def test_instnorm_refs(HW, C, act):
    x, g = rnd((3, HW, C), 1).to(D) * 2 + 0.5, rnd((3, HW, C), 2).to(D)
    xr = x.clone().requires_grad_(True)
    # [N][C][HW]; layer_norm over the pixels IS the instance norm (biased variance), and also takes HW = 1
    y = _torch_act(F.layer_norm(xr.permute(0, 2, 1), (HW,), eps=1e-5), act)
    y.backward(g.permute(0, 2, 1))
    ref = R.instnorm_fwd(x, 1e-5, act)
    _close(ref["y"], y.detach().permute(0, 2, 1), "y")
    _close(ref["mean"], x.mean(1), "mean")
    _close(ref["rstd"], 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5), "rstd")
    dx = R.instnorm_bwd(g, x, act, ref["mean"], ref["rstd"])
    if HW > 1:
        _close(dx, xr.grad, "dx", 1e-10)
    else:
        assert float(dx.abs().max()) == 0.0 and float(xr.grad.abs().max()) < 1e-9
    alt = R.instnorm_fwd(x, 1e-5, R.ACT_NONE, mean=2 * ref["mean"], rstd=ref["rstd"])
    _close(alt["y"], (x - 2 * ref["mean"][:, None]) * ref["rstd"][:, None], "y from stored statistics")


@pytest.mark.parametrize("HW", [31, 63, 4096])
def test_instnorm_one_pass_emulation_is_inside_the_offset_bound(HW):
    """The a-priori rstd bound of the offset case (mean = 10 sigma; derived in test_instnorm_offset of the GPU file) against an
    fp32 emulation of the kernel's summation order: the plain one-pass formula E[x^2] - E[x]^2 stays inside it, and so
    does the shifted form the kernel uses (sums of x - pivot: pixel 0, then the mean of that sweep), which is far more
    accurate.  Printed: error / bound."""
    rng = np.random.default_rng(5)
    x = torch.from_numpy((10.0 + rng.standard_normal((3, HW, 24))).astype(np.float32))
    ref = R.instnorm_fwd(x, 1e-5, R.ACT_NONE)
    lim = R.instnorm_offset_rstd_bound(ref["mean"], ref["var"], HW)
    for shifted in (False, True):
        m, rs = R.instnorm_one_pass_f32(x, 1e-5, shifted)
        rel = (rs.double() - ref["rstd"]).abs() / ref["rstd"]
        print(f"instnorm emulation HW {HW} shifted {shifted}: rstd max rel err {float(rel.max()):.3g}, "
              f"max err / bound {float((rel / lim).max()):.3g}")
        assert bool((rel <= lim).all())
        assert bool(((m.double() - ref["mean"]).abs() <= 1e-5 * ref["mean_abs"]).all())


def test_instnorm_constant_plane_emulation():
    """A constant plane c: the plain one-pass sums lose it at HW = 4096 (the fp32 lane sums of 128 equal terms drift: mean off
    by 18 ulp, |y| = 5e-4, four times the bound 2^-23 |c| / sqrt(eps) of one rounding of the mean); the shifted sums are
    all zero: mean = c exactly, var = 0, y = 0."""
    for c in (0.0, 3.3):
        for HW in (7, 63, 4096):
            x = torch.full((1, HW, 8), c, dtype=torch.float32)
            m, rs = R.instnorm_one_pass_f32(x, 1e-5, True)
            assert torch.equal(m, x[:, 0]) and abs(float(rs[0, 0]) - 1e-5 ** -0.5) < 1e-3
    x = torch.full((1, 4096, 8), 3.3, dtype=torch.float32)
    m, rs = R.instnorm_one_pass_f32(x, 1e-5, False)
    y = float(((x[0, 0, 0] - m[0, 0]) * rs[0, 0]).abs())
    print(f"plain one-pass, plane of 3.3, HW 4096: mean {float(m[0, 0]):.8g}, rstd {float(rs[0, 0]):.4g}, |y| {y:.3g}, "
          f"bound {2.0 ** -23 * 3.3 / math.sqrt(1e-5):.3g}")
    assert y > 2.0 ** -23 * 3.3 / math.sqrt(1e-5)


@pytest.mark.parametrize("HW", [63, 4096])
def test_instnorm_outlier_pivot_emulation(HW):
    """Pixel 0 100 sigma off the rest (the data of test_instnorm_outlier_pivot in the GPU file): with pixel 0 as the only pivot
    the kernel's summation order misses the ordinary bars at HW = 4096 (mean: 1e-5 mean |x|; rstd: 1e-5 relative); with the
    second sweep around the first sweep's mean, the form the kernel uses, it holds both.  Printed: error / bar."""
    rng = np.random.default_rng(6)
    x = torch.from_numpy((0.5 + rng.standard_normal((3, HW, 24))).astype(np.float32))
    x[:, 0, :] = 100.5
    ref = R.instnorm_fwd(x, 1e-5, R.ACT_NONE)
    worst = {}
    for stages in (1, 2):
        m, rs = R.instnorm_one_pass_f32(x, 1e-5, True, stages)
        em = float(((m.double() - ref["mean"]).abs() / (1e-5 * ref["mean_abs"])).max())
        er = float(((rs.double() - ref["rstd"]).abs() / (1e-5 * ref["rstd"])).max())
        print(f"instnorm outlier pivot HW {HW}, {stages} sweep(s): mean err / bar {em:.3g}, rstd err / bar {er:.3g}")
        worst[stages] = max(em, er)
    assert worst[2] <= 1
    if HW == 4096:
        assert worst[1] > 1


# ---- generic BatchNorm backward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act1,act2", [(R.ACT_NONE, None), (R.ACT_LRELU, R.ACT_RELU), (R.ACT_RELU, None)])
def test_bn_bwd_refs(act1, act2):
    """du, the per-block partial sums, and dz against autograd of F.batch_norm (training statistics) with one or two
    consumers of the activated output."""
    M, C, eps = 129, 8, 1e-5
    z, g1, g2 = rnd((M, C), 1).to(D) * 1.5 + 0.3, rnd((M, C), 2).to(D), rnd((M, C), 3).to(D)
    gamma, beta = 1 + 0.1 * rnd((C,), 4).to(D), 0.1 * rnd((C,), 5).to(D)
    zr, gr, br = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    pre = F.batch_norm(zr, None, None, gr, br, True, 0.0, eps)
    loss = (_torch_act(pre, act1) * g1).sum()
    if act2 is not None:
        loss = loss + (_torch_act(pre, act2) * g2).sum()
    loss.backward()
    mean, rstd = z.mean(0), 1 / torch.sqrt(z.var(0, unbiased=False) + eps)
    scale, shift = gamma * rstd, beta - mean * gamma * rstd
    _close(R.bn_pre(z, scale, shift), pre.detach(), "pre")
    du = R.bn_du(g1, act1, g2 if act2 is not None else None, act2, R.bn_pre(z, scale, shift))
    rows, rpb = 3, 43
    part, ab = R.bn_bwd_partials(du, z, mean, rstd, rows + 1, rpb)       # one block behind the last row
    assert float(part[rows].abs().max()) == 0.0 and float(ab[rows].abs().max()) == 0.0
    _close(part[1, 0], du[43:86].sum(0), "slab 1")
    sums = part.sum(0)
    _close(sums[0], br.grad, "dbeta")
    _close(sums[1], gr.grad, "dgamma")
    _close(R.bn_bwd_apply(du, z, mean, rstd, gamma, sums), zr.grad, "dz", 1e-10)
    assert bool((ab + 1e-300 >= part.abs()).all())
    # without a sign source du is the plain sum of the gradients
    assert torch.equal(R.bn_du(g1, 0, g2, 0, None), g1 + g2) and torch.equal(R.bn_du(g1, 0, None, 0, None), g1)


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def test_helper_refs():
    v = R.cast_specials()
    b = v.to(torch.bfloat16)
    # ties to even both ways, overflow to inf, NaN stays NaN, -0 keeps its sign, the smallest subnormal goes to 0
    assert b[:6].view(torch.int16).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x3F80, -0x4080, -0x407E]
    assert math.isnan(float(b[6])) and math.isinf(float(b[9])) and math.isinf(float(b[10])) and math.isfinite(float(b[11]))
    assert float(b[12]) == 0.0 and math.copysign(1.0, float(b[18])) == -1.0
    assert R.same_bits(b.float().to(torch.bfloat16), b) and not R.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert R.same_bits(torch.tensor([float("nan")]), torch.tensor([float("nan")]))
    # EMA: three roundings, as torch_ema's in-place sequence
    sh, p = rnd((1000,), 1), rnd((1000,), 2)
    want = sh.clone()
    tmp = want - p
    tmp.mul_(1 - 0.999)
    want.sub_(tmp)
    assert torch.equal(R.ema(sh, p, 1 - 0.999), want)
    assert torch.equal(R.ema(sh, p, 0.0), sh) and torch.equal(R.ema(sh, p, 1.0), sh - (sh - p))
    w = rnd((5, 3, 7), 3)
    wf, wd = R.pack_weights(w, torch.bfloat16)
    assert wd.shape == (7, 3, 5) and float(wd[6, 2, 4]) == float(w[4, 2, 6].to(torch.bfloat16)) and torch.equal(wf, w.bfloat16())
    x, mask = rnd((3, 5, 8), 4), torch.tensor([0.0, 2.0]).repeat(3, 4)
    x[0, 0, 0] = float("nan")
    out = R.dropout2d(x, mask)
    assert math.isnan(float(out[0, 0, 0])) and float(out[1, 2, 2]) == 0.0 and torch.equal(out[:, :, 1::2], 2 * x[:, :, 1::2])
