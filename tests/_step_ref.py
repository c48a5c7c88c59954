"""fp64 host references of the kernels every training step runs around the convolutions: Adam (csrc/misc.hip), the
mean-reduced losses, denormalize and the metric glue (csrc/loss.hip), MaxPool / Upsample / add_act (csrc/resnet.hip),
act_bwd and the generic BatchNorm backward (csrc/bn.hip), InstanceNorm (csrc/inorm.hip) and the small multi-tensor helpers
of csrc/misc.hip, written from the formulas of include/pai_hip.h.  Plain functions of host tensors, no device code:
tests/test_step_refs_host.py ties them to PyTorch's own double-precision ops, autograd and torch.optim.Adam,
tests/test_gpu_step_ops.py holds the kernels against them.  Every function converts what it is given to fp64 first, so
handing it the fp32 / bf16-rounded (or the kernel-stored) values makes the reference start from exactly the numbers the
kernel saw; the kernels' own fp32 constants (Adam's coefficients, the 0.2 of LeakyReLU) enter as those fp32 values."""
import math

import numpy as np
import torch

D64 = torch.float64
U = 2.0 ** -24                 # unit roundoff of fp32
TINY = 2.0 ** -149             # the smallest fp32 subnormal: the absolute error floor of one rounding near zero
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
SLOPE = float(np.float32(0.2))


def _f(t):
    return None if t is None else t.to(D64)


def same_bits(got, ref):
    """Equal bit patterns, except that any NaN matches any NaN (a payload is not part of any contract here)."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    iv = {4: torch.int32, 2: torch.int16, 1: torch.int8, 8: torch.int64}[got.element_size()]
    both_nan = torch.isnan(got) & torch.isnan(ref) if got.is_floating_point() else torch.zeros_like(got, dtype=torch.bool)
    return bool(((got.contiguous().reshape(-1).view(iv) == ref.contiguous().reshape(-1).view(iv)) | both_nan.reshape(-1)).all())


# ---- activations ------------------------------------------------------------------------------------------------------------
def act_fwd(v, act):
    v = _f(v)
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LRELU:
        return torch.where(v > 0, v, SLOPE * v)
    return v


def act_grad(a, act):
    """Derivative through the sign of the stored (activated or raw) value; at the kink (+0, -0) the slope of the negative
    side, as torch's relu / leaky_relu backward (``x > 0 ? g : g * slope``)."""
    a = _f(a)
    if act == ACT_RELU:
        return (a > 0).to(D64)
    if act == ACT_LRELU:
        return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))
    return torch.ones_like(a)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
def adam_coeffs(lr, beta1, beta2, step):
    """The kernel's own fp32 constants, as pai::adam_coeffs and the launchers form them: the arguments arrive as fp32;
    omb = float32(1 - double(beta_f32)); lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) in double, rounded to fp32."""
    lr, b1, b2 = (float(np.float32(v)) for v in (lr, beta1, beta2))
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    return {"b1": b1, "b2": b2, "omb1": float(np.float32(1.0 - b1)), "omb2": float(np.float32(1.0 - b2)),
            "lr_over_bc1": float(np.float32(lr / bc1)), "inv_sqrt_bc2": float(np.float32(1.0 / math.sqrt(bc2)))}


def adam_exact_coeffs(lr, beta1, beta2, step):
    """The same coefficients without any fp32 rounding (what torch.optim.Adam in fp64 uses)."""
    return {"b1": beta1, "b2": beta2, "omb1": 1.0 - beta1, "omb2": 1.0 - beta2,
            "lr_over_bc1": lr / (1.0 - beta1 ** step), "inv_sqrt_bc2": 1.0 / math.sqrt(1.0 - beta2 ** step)}


def adam(p0, g, m0, v0, c, eps, fp32_range=False):
    """m = b1 m0 + omb1 g;  v = b2 v0 + omb2 g^2;  den = sqrt(v) inv_sqrt_bc2 + eps;  delta = lr_over_bc1 m / den;
    p = p0 - delta.  ``m_abs`` / ``v_abs``: the sums of the absolute terms of m and v.  ``fp32_range``: a v beyond the fp32
    range is +inf, as in the kernel and in torch's fp32 formula (then den = inf, delta = 0, p = p0): the reference "in
    kind" of an overflowing g^2 (the data of adam_overflow_inputs are a factor 3 past the limit, far from its rounding)."""
    p0, g, m0, v0 = _f(p0), _f(g), _f(m0), _f(v0)
    m = c["b1"] * m0 + c["omb1"] * g
    v = c["b2"] * v0 + c["omb2"] * g * g
    if fp32_range:
        v = torch.where(v > FLT_MAX, torch.full_like(v, math.inf), v)
    den = torch.sqrt(v) * c["inv_sqrt_bc2"] + float(eps)
    delta = c["lr_over_bc1"] * m / den
    return {"p": p0 - delta, "m": m, "v": v, "den": den, "delta": delta,
            "m_abs": (c["b1"] * m0).abs() + (c["omb1"] * g).abs(), "v_abs": (c["b2"] * v0).abs() + c["omb2"] * g * g}


def adam_bounds(ref, c):
    """The three bounds of tests/test_gpu_step_ops.py (derived in its docstring): absolute-term form for the moments, and
    for p one rounding of p - delta, the relative error of delta, and the cancellation inside m carried through delta.
    4 TINY: the subnormal floor of the (at most four) roundings behind each value."""
    lim_m = 1e-5 * ref["m_abs"] + 4 * TINY
    lim_v = 1e-5 * ref["v_abs"] + 4 * TINY
    lim_p = U * ref["p"].abs() + 1e-5 * ref["delta"].abs() + c["lr_over_bc1"] * lim_m / ref["den"] + 4 * TINY
    return lim_m, lim_v, lim_p


def f32_fma(a, b, c):
    """fp32 fused multiply-add on numpy float32 arrays: the product of two fp32 numbers is exact in fp64, the sum is rounded
    to fp64 and then to fp32 (the second rounding can differ from a true fma only at an fp64 tie: never in these data)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam_f32_emulation(p0, g, m0, v0, c, eps):
    """adam1 of csrc/misc.hip operation by operation in numpy fp32 (contraction off, the two fmas spelled out)."""
    f = np.float32
    p0, g, m0, v0 = (t.numpy().astype(f) for t in (p0, g, m0, v0))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        m = f32_fma(np.full_like(m0, f(c["b1"])), m0, f(c["omb1"]) * g)
        v = f32_fma(np.full_like(v0, f(c["b2"])), v0, f(c["omb2"]) * g * g)
        den = f32_fma(np.sqrt(v), np.full_like(v, f(c["inv_sqrt_bc2"])), np.full_like(v, f(eps)))
        p = p0 - f(c["lr_over_bc1"]) * m / den
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


ADAM_STEPS = [1, 2, 1000, 100000]
ADAM_BETAS = [(0.5, 0.999), (0.9, 0.999)]
ADAM_LR, ADAM_EPS = 2e-4, 1e-7


def adam_inputs(n, seed):
    """(p0, g, m0, v0) fp32 of n elements with the slices every case carries (each a sixth of the tensor, the rest plain):
    p0 = 0 (p = -delta: the update is tested at 1e-5 of itself); |p0| ~ 1e3; g = 0 with v0 = 0 (the denominator is eps
    alone); g = +-1e-20 with m0 = v0 = 0 (g^2 underflows into the subnormals); g = +-1e18 (g^2 = 1e36: the top of the fp32
    range, v ~ 1e33).  A tensor shorter than 6 elements is plain data."""
    rng = np.random.default_rng(seed)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    p0, g = f(rng.standard_normal(n)), f(rng.standard_normal(n) * 0.1)
    m0, v0 = f(rng.standard_normal(n) * 0.05), f(rng.random(n) * 0.01)
    k = n // 6
    if k:
        sign = f(np.where(rng.random(n) < 0.5, -1.0, 1.0))
        p0[:k] = 0.0
        p0[k:2 * k] = (1e3 * (1 + f(rng.random(n)))[k:2 * k]) * sign[k:2 * k]
        g[2 * k:3 * k] = 0.0
        v0[2 * k:3 * k] = 0.0
        g[3 * k:4 * k] = 1e-20 * sign[3 * k:4 * k]
        m0[3 * k:4 * k] = 0.0
        v0[3 * k:4 * k] = 0.0
        g[4 * k:5 * k] = 1e18 * sign[4 * k:5 * k]
    return p0, g, m0, v0


FLT_MAX = float(np.finfo(np.float32).max)


def adam_overflow_inputs(n, seed):
    """(p0, g, m0, v0) with g = +-1e21 in the even elements: omb2 g^2 = 1e39 is beyond the fp32 range (3.4e38) in either order
    of the product -- (omb2 g) g = 1e18 x 1e21 in the kernel and in ATen's addcmul, omb2 (g g) -- so v = +inf, the
    denominator is inf and the update is exactly 0, while m ~ 1e20 stays finite.  (g = 1e18, the slice of adam_inputs, gives
    g^2 = 1e36 and v ~ 1e33: the top of the range, not beyond it.)  The odd elements are plain data."""
    p0, g, m0, v0 = (t.clone() for t in adam_inputs(n, seed))
    rng = np.random.default_rng(seed + 1)
    sign = torch.from_numpy(np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32))
    g[0::2] = 1e21 * sign[0::2]
    return p0, g, m0, v0


# ---- losses -------------------------------------------------------------------------------------------------------------------
def l1(x, t):
    """sum |x - t|, its absolute terms (the same), and sign(x - t) (0 at an exact zero difference, -0 against +0 included)."""
    d = _f(x) - _f(t)
    return {"sum": d.abs().sum(), "abs": d.abs().sum(), "grad": torch.sign(d)}


def mse(x, t):
    d = _f(x) - _f(t)
    return {"sum": (d * d).sum(), "abs": (d * d).sum(), "grad": 2.0 * d}


def bce_terms(x, target):
    """Per element max(x, 0) - x t + log1p(exp(-|x|)) and d/dx = sigmoid(x) - t, t the fp32 target the kernel is handed.
    sigmoid through exp(-|x|) on either side: no overflow, full relative accuracy in both tails."""
    x, t = _f(x), float(np.float32(target))
    e = torch.exp(-x.abs())
    sig = torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return torch.clamp_min(x, 0.0) - x * t + torch.log1p(e), sig - t


BCE_SPECIALS = [0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4]
BCE_NUMELS = [1, 900, 2048 * 2048 + 3]
BCE_TARGETS = [0.0, 1.0, 0.9]
# torch_fp32_bce_error(BCE_NUMELS[-1]) as measured on the CPU (tests/test_step_refs_host.py repeats and prints it): the BCE
# bounds of tests/test_gpu_step_ops.py are four times these, under their caps (1e-5 per unit of 1 + |x|; 1e-5 absolute)
BCE_TORCH_ERR = 1.011e-7         # max |loss term fp32 - fp64| / (1 + |x|)
BCE_GRAD_TORCH_ERR = 8.886e-8    # max |(sigmoid(x) - t) fp32 - fp64|


def bce_logits(numel, seed=41):
    """The first ``numel`` of: the special logits (0, +-1e-8, +-20, +-88, +-89, +-100, +-1e4), then normal data of scale 2
    with the specials repeated every 997 elements."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy((rng.standard_normal(max(numel, len(BCE_SPECIALS))) * 2.0).astype(np.float32))
    sp = torch.tensor(BCE_SPECIALS, dtype=torch.float32)
    x[:len(sp)] = sp
    if x.numel() > 1000:
        idx = torch.arange(1000, x.numel(), 997)
        x[idx] = sp[torch.arange(idx.numel()) % len(sp)]
    return x[:numel].clone()


def torch_fp32_bce_error(numel):
    """CPU measurement of the reference, not of any kernel: the error of PyTorch-CPU's own fp32
    binary_cross_entropy_with_logits(reduction="none") per unit of 1 + |x|, and of sigmoid(x) - t, against fp64, over
    bce_logits(numel) and the three targets."""
    x = bce_logits(numel)
    e_l = e_g = 0.0
    for t in BCE_TARGETS:
        tt = torch.full_like(x, t)
        l32 = torch.nn.functional.binary_cross_entropy_with_logits(x, tt, reduction="none")
        g32 = torch.sigmoid(x) - tt
        l64, g64 = bce_terms(x, t)
        e_l = max(e_l, float(((l32.double() - l64).abs() / (1 + x.double().abs())).max()))
        e_g = max(e_g, float((g32.double() - g64).abs().max()))
    return e_l, e_g


def metrics_take(sum_ssim, sse, n_images, numel):
    """{mean SSIM, PSNR (data range 1), RMSE} in fp64."""
    mse_ = sse / numel
    psnr = math.inf if mse_ == 0 else -math.log(mse_) * (10.0 / math.log(10.0))
    return [sum_ssim / n_images, psnr, math.sqrt(mse_)]


def denorm_specials():
    """-1, +1, one ulp on either side of each, +-inf, NaN, 0, -0, and values far outside, in fp32."""
    one = np.float32(1.0)
    v = [-one, np.nextafter(-one, np.float32(0)), np.nextafter(-one, np.float32(-2)), one, np.nextafter(one, np.float32(0)),
         np.nextafter(one, np.float32(2)), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), np.float32(0.0),
         np.float32(-0.0), np.float32(3.0), np.float32(-3.0), np.float32(1e30), np.float32(-1e30), np.float32(1e-40)]
    return torch.from_numpy(np.asarray(v, dtype=np.float32))


# ---- MaxPool / Upsample ---------------------------------------------------------------------------------------------------------
def maxpool2(x_nhwc):
    """[N][H][W][C] fp32 -> (out [N][H/2][W/2][C], a function mapping dout to dx) through torch's own max_pool2d and its
    autograd: the first maximum of a window wins, a NaN beats everything and the last NaN of a window wins."""
    x = x_nhwc.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(x, 2)

    def bwd(dout_nhwc):
        (dx,) = torch.autograd.grad(y, x, dout_nhwc.permute(0, 3, 1, 2).contiguous(), retain_graph=True)
        return dx.permute(0, 2, 3, 1).contiguous()
    return y.detach().permute(0, 2, 3, 1).contiguous(), bwd


def upsample2(x_nhwc):
    return x_nhwc.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()


def upsample2_bwd(dout_nhwc):
    """The fp64 sum of the four terms of every 2 x 2 window, and the sum of their absolute values."""
    d = _f(dout_nhwc)
    N, H2, W2, C = d.shape
    w = d.view(N, H2 // 2, 2, W2 // 2, 2, C)
    return w.sum((2, 4)), w.abs().sum((2, 4))


def add_act(a, b, act):
    return act_fwd(_f(a) + _f(b), act)


def act_bwd(g1, act1, g2, act2, a):
    du = _f(g1) * act_grad(a, act1)
    ab = du.abs()
    if g2 is not None:
        du = du + _f(g2) * act_grad(a, act2)
        ab = ab + (_f(g2) * act_grad(a, act2)).abs()
    return du, ab


# ---- InstanceNorm ---------------------------------------------------------------------------------------------------------------
def instnorm_fwd(x, eps, act, mean=None, rstd=None):
    """x [N][HW][C]: mean / biased variance over HW; y = act((x - mean) rstd), from the given mean / rstd [N][C] when they
    are handed in.  ``mean_abs``: the mean of |x| (the absolute terms of the mean)."""
    x = _f(x)
    mu = x.mean(1)
    var = ((x - mu[:, None]) ** 2).mean(1)
    rs = 1.0 / torch.sqrt(var + float(eps))
    m_y, r_y = (mu if mean is None else _f(mean)), (rs if rstd is None else _f(rstd))
    y = act_fwd((x - m_y[:, None]) * r_y[:, None], act)
    return {"mean": mu, "var": var, "rstd": rs, "y": y, "mean_abs": x.abs().mean(1)}


def instnorm_bwd(g, x, act, mean, rstd):
    """du = g act'(xhat), xhat = (x - mean) rstd from the mean / rstd handed in;
    dx = rstd (du - mean_HW(du) - xhat mean_HW(du xhat))."""
    g, x, mu, rs = _f(g), _f(x), _f(mean)[:, None], _f(rstd)[:, None]
    xh = (x - mu) * rs
    du = g * act_grad(xh, act)
    return rs * (du - du.mean(1, keepdim=True) - xh * (du * xh).mean(1, keepdim=True))


def instnorm_one_pass_f32(x, eps, shifted=True, stages=2):
    """The statistics of instnorm_fwd_k in the kernel's own order and precision, on the host: d = x - pivot in fp32; 32 pixel
    lanes, each an fp32 running sum of d and an fp32 fma chain of d^2 over the pixels p = lane, lane + 32, ...; the 32 lane
    sums added in fp64 in lane order and rounded to fp32; m = t1 / HW and var = max(t2 / HW - m^2, 0) in fp64; mean = pivot + m
    and rstd rounded to fp32.  The kernel sweeps twice (``stages`` = 2): pivot = pixel 0, then pivot = the fp32 mean of the
    first sweep.  ``stages`` = 1: pixel 0 alone; ``shifted`` False: pivot 0, the plain E[x^2] - E[x]^2 the kernel used
    before.  x [N][HW][C] fp32."""
    xn = x.numpy().astype(np.float32)
    N, HW, C = xn.shape
    piv = xn[:, 0] if shifted else np.zeros((N, C), np.float32)
    for _ in range(stages if shifted else 1):
        t1, t2 = np.zeros((N, C), np.float64), np.zeros((N, C), np.float64)
        for lane in range(min(32, HW)):
            s1, s2 = np.zeros((N, C), np.float32), np.zeros((N, C), np.float32)
            for p in range(lane, HW, 32):
                d = xn[:, p] - piv
                s1 = s1 + d
                s2 = f32_fma(d, d, s2)
            t1 += s1.astype(np.float64)
            t2 += s2.astype(np.float64)
        t1, t2 = t1.astype(np.float32).astype(np.float64), t2.astype(np.float32).astype(np.float64)
        m = t1 / HW
        var = np.maximum(t2 / HW - m * m, 0.0)
        mean = (piv.astype(np.float64) + m).astype(np.float32)
        piv = mean
    return torch.from_numpy(mean), torch.from_numpy((1.0 / np.sqrt(var + float(eps))).astype(np.float32))


def instnorm_offset_rstd_bound(mean, var, HW):
    """A-priori relative bound of the one-pass rstd (derived in test_instnorm_offset of tests/test_gpu_step_ops.py):
    1e-5 + 1.5 (ceil(HW / 32) + 1) u (mean^2 + var) / var."""
    n = (HW + 31) // 32
    return 1e-5 + 1.5 * (n + 1) * U * (_f(mean) ** 2 + _f(var)) / _f(var)


# ---- generic BatchNorm backward -------------------------------------------------------------------------------------------------
def bn_du(g1, act1, g2, act2, sign_src):
    """du = g1 act1'(s) + g2 act2'(s): s the stored activation, or the pre-activation z scale + shift rebuilt by the caller
    (``bn_pre``); without s: g1 (+ g2)."""
    if sign_src is None:
        return _f(g1) if g2 is None else _f(g1) + _f(g2)
    return act_bwd(g1, act1, g2, act2, sign_src)[0]


def bn_pre(z, scale, shift):
    return _f(z) * _f(scale) + _f(shift)


def bn_bwd_partials(du, z, mean, rstd, rows, rows_per_block):
    """[rows][2][C]: (sum du, sum du xhat) of each block's slab of ``rows_per_block`` rows of du / z [M][C] (blocks behind
    the last row: zeros), xhat = (z - mean) rstd, and the sums of the absolute terms."""
    du, z = _f(du), _f(z)
    M, C = z.shape
    xh = (z - _f(mean)) * _f(rstd)
    out, ab = torch.zeros(rows, 2, C, dtype=D64), torch.zeros(rows, 2, C, dtype=D64)
    for b in range(rows):
        r0, r1 = b * rows_per_block, min(M, (b + 1) * rows_per_block)
        if r0 >= r1:
            continue
        d, h = du[r0:r1], xh[r0:r1]
        out[b, 0], out[b, 1] = d.sum(0), (d * h).sum(0)
        ab[b, 0], ab[b, 1] = d.abs().sum(0), (d * h).abs().sum(0)
    return out, ab


def bn_bwd_apply(du, z, mean, rstd, gamma, sums):
    """dz = gamma rstd (du - sums[0] / M - xhat sums[1] / M), sums [2][C] as handed in (gamma None: 1)."""
    du, z = _f(du), _f(z)
    M = z.shape[0]
    xh = (z - _f(mean)) * _f(rstd)
    s = _f(sums).view(2, -1)
    gm = 1.0 if gamma is None else _f(gamma)
    return gm * _f(rstd) * (du - s[0] / M - xh * s[1] / M)


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def cast_specials():
    """fp32 values whose bf16 rounding is a tie (to even, both ways), just off a tie, NaN, +-inf, the largest finite fp32
    (rounds to inf in bf16), 3.4e38 (likewise), the largest value that stays finite, subnormals of both formats, +-0."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x7FC00000, 0x7F800000, 0xFF800000,
            0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80000001, 0x00000000,
            0x80000000, 0x7FA00000]
    v = torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())
    return torch.cat([v, torch.tensor([3.4e38, -3.4e38, 1.0, -1.5, 65504.0], dtype=torch.float32)])


def ema(shadow, param, w):
    """torch_ema's three roundings in fp32: tmp = shadow - param; tmp *= w; shadow -= tmp (w as fp32)."""
    tmp = shadow.float() - param.float()
    tmp = tmp * torch.tensor(w, dtype=torch.float32)
    return shadow.float() - tmp


def pack_weights(w, dtype):
    """w [Cout][taps][Cin] fp32 -> (forward pack: the same order in ``dtype``, input-gradient pack [Cin][taps][Cout])."""
    return w.to(dtype).contiguous(), w.permute(2, 1, 0).contiguous().to(dtype)


def dropout2d(x_nhwc, mask):
    """x [N][HW][C] of any float dtype, mask [N][C] fp32: the fp32 product rounded once to the storage type."""
    return (x_nhwc.float() * mask.float()[:, None, :]).to(x_nhwc.dtype)
