"""fp64 host reference of the train-mode FiLM norm (csrc/film_norm.hip: pai_film_norm_fwd / pai_film_norm_bwd), the input data
of its tests and the CPU measurement the fp32 SiLU bounds rest on.  tests/test_film_norm_ref_host.py ties the formulas to
torch's double autograd and to the reference's own ResBlock (tests/golden/ref_film_norm.npz); tests/test_gpu_film_norm.py
compares the kernels against them element by element.

    xhat = (x - mean_c) rstd_c,  v = gamma_c xhat + beta_c,  u = v (1 + s_nc) + t_nc,  y = m k act(u)
    du = g m k act'(u),  S0_nc = sum_p du,  S1_nc = sum_p du xhat,  dt = S0,  ds = gamma S1 + beta S0,
    dbeta_c = sum_n (1 + s_nc) S0_nc,  dgamma_c = sum_n (1 + s_nc) S1_nc,
    dx = gamma rstd (du (1 + s) - dbeta / M - xhat dgamma / M)

Every sum comes with the fp64 sum of the absolute values of its terms, dx with the magnitude
T = |gamma rstd| (|du (1 + s)| + A0 / M + |xhat| A1 / M), A0 = sum |du (1 + s)|, A1 = sum |du (1 + s) xhat| over the channel.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np
import torch

EPS = float(np.float32(1e-5))
P_DROP = 0.25
KEEP = float(np.float32(1.0 / (1.0 - P_DROP)))       # the fp32 value the kernel is handed
PAD = 16                                              # unused columns behind scale | shift in a row of emb (NaN)

# torch_fp32_silu_error(largest case) as measured on the CPU (tests/test_film_norm_ref_host.py repeats and prints it): the fp32
# SiLU / SiLU' bounds of tests/test_gpu_film_norm.py are four times these, under their caps
SILU_TORCH_ERR = 9.128e-7
SILU_BWD_TORCH_ERR = 6.436e-7


def ragged_rows(slabs_of):
    """The smallest row count past the slab rule's plateau at which at least two of the last slabs own no row; ``slabs_of`` is
    ops.film_norm_slabs (host code).  Slab i owns rows [i rps, (i + 1) rps), rps = ceil(rows / slabs)."""
    top = slabs_of(1 << 30)
    rows = next(r for r in range(1, 1 << 20) if slabs_of(r) == top)
    while True:
        rows += 1
        slabs = slabs_of(rows)
        rps = -(-rows // slabs)
        if slabs - -(-rows // rps) >= 2:
            return rows


def cases(slabs_of):
    """(N, rows, C) of tests/test_gpu_film_norm.py; the fifth is the ragged case and the largest."""
    return [(2, 1, 8), (3, 37, 8), (2, 5, 264), (1, 300, 2048), (2, ragged_rows(slabs_of), 64), (2, 1000, 256)]


def _f(t):
    return t.double()


# ---- activation ---------------------------------------------------------------------------------------------------------
def act_fwd(u, act):
    return u * torch.sigmoid(u) if act == "silu" else u


def act_grad(u, act):
    if act != "silu":
        return torch.ones_like(u)
    return torch.sigmoid(u) * (1.0 + u * torch.sigmoid(-u))      # 1 - sig(u) = sig(-u): no cancellation


# ---- the op -----------------------------------------------------------------------------------------------------------------
def batch_stats(x, eps=EPS):
    """mean and rstd per channel over all N * rows positions of x [N, rows, C] (biased variance), fp64."""
    x = _f(x)
    mean = x.mean(dim=(0, 1))
    var = ((x - mean) ** 2).mean(dim=(0, 1))
    return mean, 1.0 / torch.sqrt(var + eps)


def _film(emb, N, C):
    if emb is None:
        return torch.zeros(N, 1, C, dtype=torch.float64), torch.zeros(N, 1, C, dtype=torch.float64)
    e = _f(emb)
    return e[:, None, :C], e[:, None, C:2 * C]


def forward(x, mean, rstd, gamma, beta, emb=None, mask=None, keep=1.0, act="silu"):
    """x [N, rows, C]; mean, rstd, gamma, beta [C]; emb None or [N, >= 2 C] (scale | shift | unused); mask None or 0 / 1
    [N, rows, C].  Returns xhat, u, mk and y."""
    x = _f(x)
    N, _, C = x.shape
    s, t = _film(emb, N, C)
    xhat = (x - _f(mean)) * _f(rstd)
    u = (_f(gamma) * xhat + _f(beta)) * (1.0 + s) + t
    mk = torch.ones_like(x) if mask is None else (_f(mask) != 0).double() * float(keep)
    return {"xhat": xhat, "u": u, "mk": mk, "y": mk * act_fwd(u, act)}


def backward(g, x, mean, rstd, gamma, beta, emb=None, mask=None, keep=1.0, act="silu"):
    f = forward(x, mean, rstd, gamma, beta, emb, mask, keep, act)
    xhat, u, mk = f["xhat"], f["u"], f["mk"]
    N, rows, C = xhat.shape
    M = N * rows
    s, _ = _film(emb, N, C)
    gm, bt, rs = _f(gamma), _f(beta), _f(rstd)
    du = _f(g) * mk * act_grad(u, act)
    S0, S1 = du.sum(1), (du * xhat).sum(1)                         # [N, C]
    S0a, S1a = du.abs().sum(1), (du * xhat).abs().sum(1)
    sc = 1.0 + s[:, 0]                                             # [N, C]
    dbeta, dgamma = (sc * S0).sum(0), (sc * S1).sum(0)
    A0, A1 = (sc.abs() * S0a).sum(0), (sc.abs() * S1a).sum(0)     # = sum |du (1 + s)|, sum |du (1 + s) xhat| per channel
    dus = du * (1.0 + s)
    dx = gm * rs * (dus - dbeta / M - xhat * dgamma / M)
    T = (gm * rs).abs() * (dus.abs() + A0 / M + xhat.abs() * A1 / M)
    out = {"du": du, "gmk": (_f(g) * mk).abs(), "S0": S0, "S1": S1, "S0_abs": S0a, "S1_abs": S1a, "dbeta": dbeta,
           "dgamma": dgamma, "dbeta_abs": A0, "dgamma_abs": A1, "dx": dx, "dx_T": T, "u": u, "xhat": xhat, "y": f["y"], "mk": mk}
    if emb is not None:
        out["demb"] = torch.cat([gm * S1 + bt * S0, S0], dim=1)                                    # [N, 2 C]: ds | dt
        out["demb_abs"] = torch.cat([gm.abs() * S1a + bt.abs() * S0a, S0a], dim=1)
    return out


# ---- input data -------------------------------------------------------------------------------------------------------------
def case_data(N, rows, C, seed=0):
    """fp32 host tensors of one case (the tests round x, g and emb through the storage dtype).  Channel means up to 3 standard
    deviations from 0; channel 0 constant within the batch (variance 0); u spread over about [-12, 12], channels 1 / 2 planted
    at u = +-100 (gamma 0.5, beta +-100, no FiLM there) and channel 3 at u = 0 (gamma = beta = s = t = 0); the PAD columns behind
    scale | shift in emb are NaN; the mask keeps an element with probability 1 - P_DROP."""
    gen = torch.Generator().manual_seed(1000 * seed + 17 * C + rows % 1000 + N)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    ru = lambda *shape: torch.rand(*shape, generator=gen)
    std = 0.5 + 1.5 * ru(C)
    off = 6.0 * ru(C) - 3.0
    off[4] = 3.0
    x = rn(N, rows, C) * std + off * std
    x[..., 0] = 0.75
    gamma = (0.5 + ru(C)) * torch.where(ru(C) < 0.5, -1.0, 1.0)
    beta = rn(C)
    s, t = 0.3 * rn(N, C), 2.0 * rn(N, C)
    gamma[1], beta[1], gamma[2], beta[2], gamma[3], beta[3] = 0.5, 100.0, 0.5, -100.0, 0.0, 0.0
    s[:, 1:4] = 0.0
    t[:, 1:4] = 0.0
    emb = torch.cat([s, t, torch.full((N, PAD), float("nan"))], dim=1)
    g = rn(N, rows, C)
    mask = (ru(N, rows, C) >= P_DROP).to(torch.uint8)
    return {"x": x, "gamma": gamma, "beta": beta, "emb": emb, "g": g, "mask": mask}


# ---- the measurement behind the fp32 SiLU bounds ------------------------------------------------------------------------------
def silu_args(case):
    """u (fp64, as the reference forms it from the case's tensors) and the upstream gradient (fp32) of the FiLM + SiLU + mask
    variant of ``case``."""
    N, rows, C = case
    d = case_data(N, rows, C)
    mean, rstd = batch_stats(d["x"])
    f = forward(d["x"], mean.float(), rstd.float(), d["gamma"], d["beta"], d["emb"], d["mask"], KEEP)
    return f["u"].reshape(-1), d["g"].reshape(-1)


def torch_fp32_silu_error(case):
    """CPU measurement of the reference, not of any kernel, built as torch_fp32_gelu_error of tests/_vit_ref.py: max |F.silu
    fp32 - fp64| and max |its gradient - fp64| / |dy| of PyTorch-CPU's own fp32 op, both functions on the SAME fp32 arguments:
    the fp32 roundings of silu_args(case)."""
    u, dy = silu_args(case)
    dy = torch.where(dy.abs() < 0.25, torch.full_like(dy, 0.25), dy)        # an error per unit |dy| needs |dy| away from 0
    ur = u.float().requires_grad_(True)
    y = torch.nn.functional.silu(ur)
    y.backward(dy)
    u32 = ur.detach().double()
    e_fwd = float((y.detach().double() - act_fwd(u32, "silu")).abs().max())
    e_bwd = float(((ur.grad.double() - dy.double() * act_grad(u32, "silu")).abs() / dy.double().abs()).max())
    return e_fwd, e_bwd


def silu_lim(u):
    """fp32 SiLU bar per element: four times the measured torch error, never above 1e-6 (1 + |u|)."""
    return torch.clamp(1e-6 * (1.0 + _f(u).abs()), max=4 * SILU_TORCH_ERR)


def y_rounding(u, mk, act):
    """What the SiLU bar has no term for, because its measurement starts from fp32 arguments and ends at act(u): here u is a
    computed quantity that the kernel holds as an fp32 number (half an ulp: 2^-24 |u|, which act' carries into act(u)), and
    act(u) is multiplied by m k and stored as an fp32 number (2^-24 |y|).  m k 2^-24 (|u| |act'(u)| + |act(u)|) per element:
    1.6e-5 at the planted u = 100 under the mask (k u = 133), 1.9e-6 at |u| = 12, nothing where the mask drops."""
    u = _f(u)
    return _f(mk) * 2.0 ** -24 * (u.abs() * act_grad(u, act).abs() + act_fwd(u, act).abs())


SILU_BWD_BOUND = 4 * SILU_BWD_TORCH_ERR          # per unit |g|
