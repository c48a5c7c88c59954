"""fp64 host references of the TransUNet token kernels (csrc/vit.hip) and of the two helpers of csrc/misc.hip they call,
written from the formulas of include/pai_hip.h (the TransUNet block).  Plain functions of host tensors, no device code:
tests/test_vit_refs_host.py ties them to PyTorch's own double-precision ops and autograd, tests/test_gpu_vit_ops.py holds
the kernels against them.  Every function converts what it is given to fp64 first, so handing it the bf16-rounded (or the
kernel-stored) values makes the reference start from exactly the numbers the kernel saw."""
import math

import torch

D64 = torch.float64


def _f(t):
    return None if t is None else t.to(D64)


# ---- LayerNorm --------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, res, gamma, beta, eps, post, P, s_stored=None, mean=None, rstd=None):
    """s = x + res (res None: s = x); mean / rstd over the last axis of s "as stored" when ``s_stored`` is given (biased
    variance, eps inside the root); y = (s - mean) * rstd * gamma + beta + post[row % P], from the given ``mean`` / ``rstd``
    when they are handed in.  ``mean_abs``: the sum of the absolute terms of the row mean."""
    s = _f(x) if res is None else _f(x) + _f(res)
    sl = s if s_stored is None else _f(s_stored)
    M, D = sl.shape
    mu = sl.mean(1)
    var = ((sl - mu[:, None]) ** 2).mean(1)
    rs = 1.0 / torch.sqrt(var + float(eps))
    m_y, r_y = (mu if mean is None else _f(mean)), (rs if rstd is None else _f(rstd))
    y = (sl - m_y[:, None]) * r_y[:, None] * _f(gamma) + _f(beta)
    if post is not None:
        y = y + _f(post).view(P, D)[torch.arange(M) % P]
    return {"sum": s, "mean": mu, "rstd": rs, "y": y, "mean_abs": sl.abs().mean(1)}


def layernorm_bwd(dy, xs, gamma, mean, rstd):
    """dx = rstd (g - mean_D(g) - xhat mean_D(g xhat)), g = dy gamma, xhat = (xs - mean) rstd; dbeta = sum_rows dy,
    dgamma = sum_rows dy xhat, and the sums of their absolute terms."""
    dy, xs, mu, rs = _f(dy), _f(xs), _f(mean)[:, None], _f(rstd)[:, None]
    xh = (xs - mu) * rs
    g = dy * _f(gamma)
    a, b = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    return {"dx": rs * (g - a - xh * b), "dbeta": dy.sum(0), "dbeta_abs": dy.abs().sum(0),
            "dgamma": (dy * xh).sum(0), "dgamma_abs": (dy * xh).abs().sum(0)}


# ---- GELU (erf form) ---------------------------------------------------------------------------------------------------
def _cdf(z):
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0))      # erfc: no cancellation in the negative tail


def gelu(z):
    z = _f(z)
    return z * _cdf(z)


def gelu_bwd(dy, z):
    z = _f(z)
    return _f(dy) * (_cdf(z) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))


GELU_NUMELS = [1, 7, 8192 * 256 + 77]
# torch_fp32_gelu_error(GELU_NUMELS[-1]) as measured on the CPU (tests/test_vit_refs_host.py repeats and prints it): the fp32
# GELU / GELU' bounds of tests/test_gpu_vit_ops.py are four times these, under their caps
GELU_TORCH_ERR = 1.221e-6
GELU_BWD_TORCH_ERR = 2.863e-7
GELU_SPECIALS = [-4.0, 4.0, 0.0, -0.0, 1e-4, -1e-4, 10.0, -10.0, 40.0, -40.0]


def gelu_args(numel):
    """The first ``numel`` of: -4, 4, +0, -0, +-1e-4, +-10, +-40, then a dense sweep of [-6, 6] (fp32)."""
    z = torch.tensor(GELU_SPECIALS, dtype=torch.float32)
    if numel > len(z):
        z = torch.cat([z, torch.linspace(-6.0, 6.0, numel - len(z), dtype=torch.float32)])
    return z[:numel].clone()


def gelu_dy(numel):
    """Upstream gradients of both signs with 0.5 <= |dy| <= 2 (an error is then comparable per unit of dy)."""
    i = torch.arange(numel, dtype=torch.float64)
    return ((0.5 + 1.5 * ((i * 0.6180339887498949) % 1.0)) * (1.0 - 2.0 * (i % 2))).float()


def torch_fp32_gelu_error(numel):
    """CPU measurement of the reference, not of any kernel: max |F.gelu fp32 - fp64| and max |its gradient - fp64| / |dy|
    of PyTorch-CPU's own fp32 op over gelu_args(numel) / gelu_dy(numel)."""
    z, dy = gelu_args(numel), gelu_dy(numel)
    zr = z.clone().requires_grad_(True)
    y = torch.nn.functional.gelu(zr)
    y.backward(dy)
    e_fwd = float((y.detach().double() - gelu(z)).abs().max())
    e_bwd = float(((zr.grad.double() - gelu_bwd(dy, z)).abs() / dy.double().abs()).max())
    return e_fwd, e_bwd


# ---- attention core -----------------------------------------------------------------------------------------------------
def _heads(t, S, B, heads, hd):
    """[S*B][heads*hd] (row = s*B + b) -> [B][heads][S][hd]."""
    return t.view(S, B, heads, hd).permute(1, 2, 0, 3)


def _rows(t, S, B, heads, hd):
    """[B][heads][S][hd] -> [S*B][heads*hd]."""
    return t.permute(2, 0, 1, 3).reshape(S * B, heads * hd)


def split_qkv(qkv, S, B, heads, hd):
    E = heads * hd
    x = _f(qkv).view(S * B, 3, E)
    return tuple(_heads(x[:, i], S, B, heads, hd) for i in range(3))


def mha_fwd(qkv, S, B, heads, hd, mask=None):
    """qkv [S*B][3E]: probs [B*heads][S][S] = softmax(q k^T / sqrt(hd)), out [S*B][E] = (probs * mask) v.  ``e_s``: the
    a-priori bound hd 2^-24 scale max_ij sum_d |q_id k_jd| of an fp32 score in any summation order; ``mass``: the largest
    row sum of probs * mask."""
    q, k, v = split_qkv(qkv, S, B, heads, hd)
    scale = 1.0 / math.sqrt(hd)
    p = torch.softmax(torch.einsum("bhid,bhjd->bhij", q, k) * scale, dim=-1)
    pm = p if mask is None else p * _f(mask).view(B, heads, S, S)
    out = torch.einsum("bhij,bhjd->bhid", pm, v)
    e_s = hd * 2.0 ** -24 * scale * float(torch.einsum("bhid,bhjd->bhij", q.abs(), k.abs()).max())
    return {"probs": p.reshape(B * heads, S, S), "out": _rows(out, S, B, heads, hd), "e_s": e_s,
            "mass": float(pm.sum(-1).max()), "vmax": float(v.abs().max())}


def mha_bwd(dout, qkv, probs, S, B, heads, hd, mask=None):
    """From the probabilities handed in: dP = (dO v^T) * mask, dS = P (dP - sum_j P dP), dQ = scale dS k, dK = scale dS^T q,
    dV = (P * mask)^T dO, packed like qkv [S*B][3E]; ``abs``: the sums of the absolute terms of every element, same packing.
    ``cancel``: what the subtraction dP - sum_j P dP can lose -- C_ij = P_ij (Abar_ij + sum_j' P_ij' Abar_ij') with
    Abar_ij = mask_ij sum_d |dO_id v_jd| (the absolute terms of dP_ij), carried through the dQ / dK products like ``abs``
    (scale sum_j C_ij |K_jd|, scale sum_i C_ij |Q_id|; zero for dV)."""
    q, k, v = split_qkv(qkv, S, B, heads, hd)
    do = _heads(_f(dout), S, B, heads, hd)
    p = _f(probs).view(B, heads, S, S)
    m = torch.ones_like(p) if mask is None else _f(mask).view(B, heads, S, S)
    scale = 1.0 / math.sqrt(hd)
    dp = torch.einsum("bhid,bhjd->bhij", do, v) * m
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    pm = p * m
    parts = [scale * torch.einsum("bhij,bhjd->bhid", ds, k), scale * torch.einsum("bhij,bhid->bhjd", ds, q),
             torch.einsum("bhij,bhid->bhjd", pm, do)]
    absum = [scale * torch.einsum("bhij,bhjd->bhid", ds.abs(), k.abs()),
             scale * torch.einsum("bhij,bhid->bhjd", ds.abs(), q.abs()),
             torch.einsum("bhij,bhid->bhjd", pm.abs(), do.abs())]
    ab = torch.einsum("bhid,bhjd->bhij", do.abs(), v.abs()) * m.abs()
    c = p * (ab + (p * ab).sum(-1, keepdim=True))
    cancel = [scale * torch.einsum("bhij,bhjd->bhid", c, k.abs()), scale * torch.einsum("bhij,bhid->bhjd", c, q.abs()),
              torch.zeros_like(parts[2])]
    pack = lambda ts: torch.cat([_rows(t, S, B, heads, hd) for t in ts], dim=1)
    return {"dqkv": pack(parts), "abs": pack(absum), "cancel": pack(cancel)}


# ---- even-pixel subsample --------------------------------------------------------------------------------------------
def subsample2(x):
    """[N][H][W][C] -> [N][H/2][W/2][C] (any dtype: a copy of bits)."""
    return x[:, ::2, ::2, :].contiguous()


def subsample2_bwd(dout, H, W):
    N, _, _, C = dout.shape
    dx = torch.zeros(N, H, W, C, dtype=dout.dtype)
    dx[:, ::2, ::2, :] = dout
    return dx


# ---- sums ---------------------------------------------------------------------------------------------------------------
def bn_stats(z, rows_per_slab):
    """[slabs][2][C]: (sum, sum of squares) of slabs of ``rows_per_slab`` rows of z [M][C], and the absolute terms."""
    z = _f(z)
    M, C = z.shape
    slabs = (M + rows_per_slab - 1) // rows_per_slab
    out, ab = torch.zeros(slabs, 2, C, dtype=D64), torch.zeros(slabs, 2, C, dtype=D64)
    for s in range(slabs):
        c = z[s * rows_per_slab:(s + 1) * rows_per_slab]
        out[s, 0], out[s, 1] = c.sum(0), (c * c).sum(0)
        ab[s, 0], ab[s, 1] = c.abs().sum(0), out[s, 1]
    return {"stats": out, "abs": ab}


def colsum(x):
    x = _f(x)
    return {"sum": x.sum(0), "abs": x.abs().sum(0)}
