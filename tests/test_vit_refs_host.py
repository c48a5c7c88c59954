"""CPU: the fp64 references of tests/_vit_ref.py against PyTorch's own double-precision ops and autograd, to 1e-12, at a
few of the shapes tests/test_gpu_vit_ops.py uses -- a wrong reference cannot then be "fixed" by bending a bound over
there.  Also the CPU measurement the fp32 GELU / GELU' bounds of that file rest on: the error of torch's own fp32 F.gelu
and of its gradient against fp64 (printed, and compared with the constants recorded in _vit_ref)."""
import math

import pytest
import torch
import torch.nn.functional as F

import _vit_ref as R
from _gpu_util import max_err, rnd

D = torch.float64


def _close(got, want, what, tol=1e-12):
    e = max_err(got, want)
    assert e < tol, (what, e)


@pytest.mark.parametrize("M,Dm,P", [(1, 1, 1), (7, 1000, 1), (12, 96, 4), (3, 257, 3)])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "res+post"])
def test_layernorm_refs(M, Dm, P, fused):
    x, r = rnd((M, Dm), 1).to(D) * 1.5 + 0.2, rnd((M, Dm), 2).to(D)
    gamma, beta, post = 1 + 0.1 * rnd((Dm,), 3).to(D), 0.1 * rnd((Dm,), 4).to(D), rnd((P, Dm), 5).to(D)
    dy = rnd((M, Dm), 6).to(D)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    s = xr + r if fused else xr
    want = F.layer_norm(s, (Dm,), gr, br, 1e-5)
    if fused:
        want = (want.view(M // P, P, Dm) + post).view(M, Dm)
    want.backward(dy)
    ref = R.layernorm_fwd(x, r if fused else None, gamma, beta, 1e-5, post if fused else None, P)
    _close(ref["y"], want.detach(), "y")
    sd = s.detach()
    _close(ref["sum"], sd, "sum")
    _close(ref["mean"], sd.mean(1), "mean")
    _close(ref["rstd"], 1 / torch.sqrt(sd.var(1, unbiased=False) + 1e-5), "rstd")
    _close(ref["mean_abs"], sd.abs().mean(1), "mean_abs")
    # handed a stored sum / mean / rstd, the reference starts from those
    alt = R.layernorm_fwd(x, r if fused else None, gamma, beta, 1e-5, None, P, s_stored=2 * sd, mean=2 * sd.mean(1),
                          rstd=ref["rstd"])
    _close(alt["y"], 2 * (sd - sd.mean(1, keepdim=True)) * ref["rstd"][:, None] * gamma + beta, "y from stored values")
    bw = R.layernorm_bwd(dy, ref["sum"], gamma, ref["mean"], ref["rstd"])
    if Dm > 1:       # D = 1: y = beta, every gradient is cancellation noise around 0
        _close(bw["dx"], xr.grad, "dx")
        _close(bw["dgamma"], gr.grad, "dgamma")
    else:
        assert float(bw["dx"].abs().max()) < 1e-9 and float(xr.grad.abs().max()) < 1e-9
    _close(bw["dbeta"], br.grad, "dbeta")
    xh = (sd - ref["mean"][:, None]) * ref["rstd"][:, None]
    _close(bw["dbeta_abs"], dy.abs().sum(0), "dbeta_abs")
    _close(bw["dgamma_abs"] + 1e-300, (dy * xh).abs().sum(0) + 1e-300, "dgamma_abs")


def test_gelu_refs():
    z = torch.cat([R.gelu_args(4000).to(D), torch.tensor([-20.0, -8.0, 8.0, 20.0], dtype=D)])
    dy = torch.cat([R.gelu_dy(4000).to(D), torch.ones(4, dtype=D)])
    zr = z.clone().requires_grad_(True)
    y = F.gelu(zr)
    y.backward(dy)
    # torch's fp64 op is 0.5 z (1 + erf(z / sqrt 2)): 1e-16 absolute of z in the negative tail, where the reference (erfc)
    # keeps full relative accuracy -- compared absolutely, per unit of (1 + |z|)
    assert float(((R.gelu(z) - y.detach()).abs() / (1 + z.abs())).max()) < 1e-15
    assert float(((R.gelu_bwd(dy, z) - zr.grad).abs() / (1 + z.abs())).max()) < 1e-15
    assert float(R.gelu(torch.tensor([-40.0]))) == 0.0 and float(R.gelu(torch.tensor([40.0]))) == 40.0
    assert abs(float(R.gelu(torch.tensor([-10.0]))) / (-10 * 0.5 * math.erfc(10 / math.sqrt(2))) - 1) < 1e-12


def test_torch_fp32_gelu_error_is_what_the_gpu_bounds_assume():
    """The measurement behind GELU_TORCH_ERR / GELU_BWD_TORCH_ERR of tests/_vit_ref.py (the fp32 bounds of
    tests/test_gpu_vit_ops.py are four times these): max |F.gelu fp32 - fp64| and max |gradient - fp64| / |dy| of
    PyTorch-CPU's own op over the arguments of the largest GPU case, printed.  One-sided: what the GPU bound needs is that
    the recorded constants do not undercut the reference's own error by more than a margin (10 %); a torch build whose fp32
    op is more accurate leaves this green."""
    e_fwd, e_bwd = R.torch_fp32_gelu_error(R.GELU_NUMELS[-1])
    print(f"torch fp32 CPU gelu: max err {e_fwd:.4g} (recorded {R.GELU_TORCH_ERR:.4g}); "
          f"gradient per |dy|: {e_bwd:.4g} (recorded {R.GELU_BWD_TORCH_ERR:.4g})")
    assert e_fwd <= 1.1 * R.GELU_TORCH_ERR and e_bwd <= 1.1 * R.GELU_BWD_TORCH_ERR


@pytest.mark.parametrize("S,B,heads,hd", [(7, 3, 2, 64), (1, 2, 2, 32), (5, 2, 2, 24), (3, 1, 1, 1), (17, 2, 2, 160)])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_mha_refs(S, B, heads, hd, masked):
    E = heads * hd
    qkv, dout = rnd((S * B, 3 * E), 9).to(D) * 0.7, rnd((S * B, E), 10).to(D)
    mask = None
    if masked:      # the 0 / (1 / 0.7) dropout mask of tests/test_gpu_vit_ops.py, from a generator of its own
        g = torch.Generator().manual_seed(5)
        mask = (torch.bernoulli(torch.full((B * heads, S, S), 0.7), generator=g) / 0.7).to(D)
    qr = qkv.clone().requires_grad_(True)
    qq, kk, vv = (c.reshape(S, B * heads, hd).transpose(0, 1) for c in qr.view(S, B, 3 * E).chunk(3, dim=-1))
    if masked:      # the header: out = (softmax(q k^T / sqrt(hd)) * mask) v
        p = torch.softmax(qq @ kk.transpose(1, 2) / math.sqrt(hd), dim=-1)
        want = ((p * mask) @ vv).transpose(0, 1).reshape(S * B, E)
    else:
        want = F.scaled_dot_product_attention(qq, kk, vv).transpose(0, 1).reshape(S * B, E)
        p = torch.softmax(qq @ kk.transpose(1, 2) / math.sqrt(hd), dim=-1)
    want.backward(dout)
    ref = R.mha_fwd(qkv, S, B, heads, hd, mask)
    _close(ref["out"], want.detach(), "out")
    _close(ref["probs"], p.detach(), "probs")
    pm = p.detach() if mask is None else p.detach() * mask
    assert abs(ref["mass"] - float(pm.sum(-1).max())) < 1e-12
    assert abs(ref["vmax"] - float(vv.detach().abs().max())) < 1e-15
    e_s = hd * 2.0 ** -24 / math.sqrt(hd) * float((qq.detach().abs() @ kk.detach().abs().transpose(1, 2)).max())
    assert abs(ref["e_s"] / e_s - 1) < 1e-12
    bw = R.mha_bwd(dout, qkv, ref["probs"], S, B, heads, hd, mask)
    if S > 1:
        _close(bw["dqkv"], qr.grad, "dqkv")
    else:           # one key: dQ = dK = 0 exactly, dV = mask * dO
        _close(bw["dqkv"][:, 2 * E:], qr.grad[:, 2 * E:], "dV")
        assert float(bw["dqkv"][:, :2 * E].abs().max()) == 0.0 and float(qr.grad[:, :2 * E].abs().max()) < 1e-15
    assert bool((bw["abs"] + 1e-300 >= bw["dqkv"].abs()).all())
    # the absolute sums are the same products with every factor made non-negative
    flip = R.mha_bwd(dout.abs(), qkv.abs(), ref["probs"], S, B, heads, hd, mask)
    _close(bw["abs"][:, 2 * E:], flip["dqkv"][:, 2 * E:], "dV abs")
    # cancel: P_ij (Abar_ij + sum_j' P_ij' Abar_ij') through the dQ / dK products, written here with matmuls per (b, h)
    pd, m1 = p.detach(), (torch.ones_like(p.detach()) if mask is None else mask)
    do_h = dout.view(S, B * heads, hd).transpose(0, 1)
    ab = (do_h.abs() @ vv.detach().abs().transpose(1, 2)) * m1
    c = pd * (ab + (pd * ab).sum(-1, keepdim=True))
    rows = lambda t: t.transpose(0, 1).reshape(S * B, E)
    _close(bw["cancel"][:, :E], rows(c @ kk.detach().abs()) / math.sqrt(hd), "cancel dQ")
    _close(bw["cancel"][:, E:2 * E], rows(c.transpose(1, 2) @ qq.detach().abs()) / math.sqrt(hd), "cancel dK")
    assert float(bw["cancel"][:, 2 * E:].abs().max()) == 0.0


def test_subsample_refs():
    x = rnd((3, 6, 10, 3), 3).to(D)
    xr = x.clone().requires_grad_(True)
    y = xr[:, ::2, ::2, :]
    g = rnd((3, 3, 5, 3), 4).to(D)
    y.backward(g)
    assert torch.equal(R.subsample2(x), y.detach().contiguous())
    assert torch.equal(R.subsample2_bwd(g, 6, 10), xr.grad)


def test_sum_refs():
    z = rnd((150, 5), 7).to(D) * 1.5 + 0.3
    st = R.bn_stats(z, 64)
    assert st["stats"].shape == (3, 2, 5)
    _close(st["stats"].sum(0)[0], z.sum(0), "sum")
    _close(st["stats"].sum(0)[1], (z * z).sum(0), "sum of squares")
    _close(st["stats"][2, 0], z[128:].sum(0), "last slab")
    _close(st["abs"].sum(0)[0], z.abs().sum(0), "abs")
    _close(R.colsum(z)["sum"], z.sum(0), "colsum")
    _close(R.colsum(z)["abs"], z.abs().sum(0), "colsum abs")
