"""fp64 host references of the BatchNorm forward chain of csrc/bn.hip -- pai_bn_finalize, pai_bn_eval_coeffs, pai_bn_apply and
pai_bn2_add_act -- written from the formulas of include/pai_hip.h, plus an fp32 emulation of bn_finalize_k's arithmetic.  Plain
functions of host tensors, no device code: tests/test_bn_refs_host.py ties them to PyTorch's double-precision F.batch_norm /
F.relu / F.leaky_relu, tests/test_gpu_bn_fwd.py holds the kernels against them.

Every reference starts from exactly what the kernel is handed: finalize from the fp32 partial rows [R][2][C] as given (it is
DEFINED on the partials, not on a tensor behind them), apply and the residual tail from the fp32 scale / shift arrays and the
(bf16-rounded) tensors.  The kernel's own fp32 constants enter as those fp32 values widened to double: eps, momentum, and
1.f - momentum formed in fp32.  The clamp var = max(var, 0) is reproduced.  Activations propagate a NaN as aten does
(relu = clamp_min keeps it; -inf gives 0)."""
import numpy as np
import torch

D64 = torch.float64
U = 2.0 ** -24
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
SLOPE = float(np.float32(0.2))


def _f(t):
    return None if t is None else t.to(D64)


def f32c(v):
    """A Python float as the fp32 value the C ABI receives, widened to double."""
    return float(np.float32(v))


def one_minus_f32(momentum):
    """1.f - momentum as the kernels form it: in fp32."""
    return float(np.float32(1.0) - np.float32(momentum))


def act(v, a):
    """aten semantics in fp64: relu(NaN) = NaN, relu(-inf) = 0, relu(+-0) = 0; leaky_relu(v) = v > 0 ? v : 0.2f v."""
    v = _f(v)
    if a == ACT_RELU:
        return torch.where(v <= 0, torch.zeros_like(v), v)          # NaN <= 0 is false: the NaN stays
    if a == ACT_LRELU:
        return torch.where(v > 0, v, SLOPE * v)                      # NaN > 0 is false: 0.2 NaN = NaN
    return v


def finalize(partials, count, gamma, beta, eps, momentum, n_updates, rm0, rv0):
    """partials fp32 [R][2][C] (row r: sums, then sums of squares).  mean = S / count, var = max(Q / count - mean^2, 0) (biased),
    rstd = 1 / sqrt(var + eps), scale = gamma rstd, shift = beta - mean scale (gamma / beta None: 1 / 0); the running
    statistics advance n_updates times by r = (1.f - momentum) r + momentum stat with the unbiased variance
    var count / (count - 1) (count 1: var).  Also the absolute terms the bounds need."""
    p = _f(partials)
    C = p.shape[2]
    eps, mom, omm = f32c(eps), f32c(momentum), one_minus_f32(momentum)
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    mean = s / count
    ex2 = q / count
    var = torch.clamp_min(ex2 - mean * mean, 0.0)
    var = torch.where(torch.isnan(ex2 - mean * mean), ex2 - mean * mean, var)       # the kernel's `var < 0 ? 0 : var` keeps a NaN
    rstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones(C, dtype=D64) if gamma is None else _f(gamma)
    b = torch.zeros(C, dtype=D64) if beta is None else _f(beta)
    scale = g * rstd
    shift = b - mean * scale
    unbiased = var * count / (count - 1.0) if count > 1 else var
    out = {"mean": mean, "var": var, "rstd": rstd, "scale": scale, "shift": shift, "unbiased": unbiased,
           "shift_abs": b.abs() + (mean * scale).abs(), "amplification": ex2 / (var + eps),
           "mean_reorder": p.shape[0] * 2.0 ** -53 * p[:, 0].abs().sum(0) / count}
    if rm0 is not None:
        rm, rv = _f(rm0).clone(), _f(rv0).clone()
        for _ in range(int(n_updates)):
            rm = omm * rm + mom * mean
            rv = omm * rv + mom * unbiased
        out.update(rm=rm, rv=rv, rm_abs=_f(rm0).abs() + mean.abs(), rv_abs=_f(rv0).abs() + unbiased.abs())
    return out


def finalize_bounds(ref, n_updates):
    """The bars of tests/test_gpu_bn_fwd.py (derived in its docstring), per output."""
    lim = {"mean": 2 * U * ref["mean"].abs(), "rstd": 2 * U * ref["rstd"].abs(), "scale": 4 * U * ref["scale"].abs(),
           "shift": 6 * U * ref["shift_abs"]}
    if "rm" in ref:
        lim["rm"] = 3 * n_updates * U * ref["rm_abs"]
        lim["rv"] = 3 * n_updates * U * ref["rv_abs"]
    return lim


def eval_coeffs(gamma, beta, rm, rv, eps):
    rm, rv = _f(rm), _f(rv)
    C = rm.numel()
    rstd = 1.0 / torch.sqrt(rv + f32c(eps))
    g = torch.ones(C, dtype=D64) if gamma is None else _f(gamma)
    b = torch.zeros(C, dtype=D64) if beta is None else _f(beta)
    scale = g * rstd
    return {"scale": scale, "shift": b - rm * scale, "shift_abs": b.abs() + (rm * scale).abs()}


def apply(z, scale, shift, a):
    """act(z scale + shift) over [M][C]; ``terms``: |z scale| + |shift|."""
    z, sc, sh = _f(z), _f(scale), _f(shift)
    return {"out": act(z * sc + sh, a), "terms": (z * sc).abs() + sh.abs()}


def bn2_add_act(za, sa, ha, zb, sb, hb, act_a, a):
    """act(act_a(za sa + ha) + (zb sb + hb)), sb / hb None: + zb.  ``terms_a`` / ``terms_b``: the absolute terms of the two
    multiply-adds (identity skip: |zb|, which carries no rounding)."""
    za, zb = _f(za), _f(zb)
    x = act(za * _f(sa) + _f(ha), act_a)
    y = zb if sb is None else zb * _f(sb) + _f(hb)
    return {"out": act(x + y, a), "terms_a": (za * _f(sa)).abs() + _f(ha).abs(),
            "terms_b": zb.abs() if sb is None else (zb * _f(sb)).abs() + _f(hb).abs()}


# ---- partial rows ------------------------------------------------------------------------------------------------------------
def make_partials(R, C, count, seed, kind="normal"):
    """fp32 partial rows [R][2][C] that sum to the statistics of m R fp64 samples per channel, each weighted count / (m R), m = 4
    per row (32 where R <= 16, so that the sample variance of few rows stays near its channel's):
    the biased variance of the samples is what var comes to, so it is non-negative up to the fp32 rounding of the rows.
      normal    channel means in [-1, 1], standard deviations in [0.5, 1.5]
      offset    mean 10, std 0.1 (Q / count = 100, var = 0.01: amplification 1e4)
      constant  every sample the same c, 0.2 <= |c| <= 0.6 (no power of two: the sums and the sums of squares round
                independently): var is the rounding of the rows, on either side of 0 -- the clamp
    ``kind`` "mixed": channel c takes kind c % 3 of the three."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-1.0, 1.0, C)
    sd = rng.uniform(0.5, 1.5, C)
    m = 4 if R > 16 else 32
    x = rng.standard_normal((R, m, C))
    k = {"normal": np.zeros(C, int), "offset": np.ones(C, int), "constant": np.full(C, 2), "mixed": np.arange(C) % 3}[kind]
    mu = np.where(k == 1, 10.0, mu)
    sd = np.where(k == 1, 0.1, sd)
    x = mu + sd * x
    const = rng.uniform(0.2, 0.6, C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)
    x = np.where(k == 2, const, x)
    w = count / (float(m) * R)
    p = np.stack([w * x.sum(1), w * (x * x).sum(1)], 1).astype(np.float32)
    return torch.from_numpy(p)


# ---- fp32 emulation of bn_finalize_k -------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def finalize_f32_emulation(partials, count, gamma, beta, eps, momentum, n_updates, rm0, rv0, contract):
    """bn_finalize_k operation by operation in numpy: the fp64 sums row by row from the LAST row to the first (the reference
    sums pairwise from the first: a different order), then each fp32 rounding of the kernel -- (float)mean, rstd, g * rstd,
    b - mean * sc, (float)unbiased, and per update (1.f - m) * r + m * stat.  ``contract``: the multiply-adds fused as hipcc
    does by default (shift = fma(-mean, sc, b); r = fma(1.f - m, r, round(m * stat))), or every product rounded."""
    f = np.float32
    p = partials.numpy().astype(np.float64)
    R, _, C = p.shape
    s, q = np.zeros(C), np.zeros(C)
    for r in range(R - 1, -1, -1):
        s = s + p[r, 0]
        q = q + p[r, 1]
    mean = s / count
    var = np.maximum(q / count - mean * mean, 0.0)
    eps32, mom, omm = f(eps), f(momentum), f(1.0) - f(momentum)
    rstd = (1.0 / np.sqrt(var + float(eps32))).astype(f)
    g = np.ones(C, f) if gamma is None else gamma.numpy().astype(f)
    b = np.zeros(C, f) if beta is None else beta.numpy().astype(f)
    sc = g * rstd
    m32 = mean.astype(f)
    sh = _fma32(-m32, sc, b) if contract else b - m32 * sc
    out = {"mean": m32, "rstd": rstd, "scale": sc, "shift": sh}
    if rm0 is not None:
        unb = (var * count / (count - 1.0) if count > 1 else var).astype(f)
        rm, rv = rm0.numpy().astype(f), rv0.numpy().astype(f)
        for _ in range(int(n_updates)):
            if contract:
                rm = _fma32(np.full(C, omm, f), rm, mom * m32)
                rv = _fma32(np.full(C, omm, f), rv, mom * unb)
            else:
                rm = omm * rm + mom * m32
                rv = omm * rv + mom * unb
        out.update(rm=rm, rv=rv)
    return {k: torch.from_numpy(np.asarray(v, dtype=f)) for k, v in out.items()}
