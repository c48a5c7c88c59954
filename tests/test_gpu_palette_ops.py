"""GPU: every kernel of csrc/palette.hip against an fp64 host computation of the WHOLE tensor, written here from the formulas
of include/pai_hip.h (reference models/guided_diffusion/unet.py:265-297, nn.py:140-157, models/palette.py:233-306).

Bounds.  fp32: the project's 1e-4 of max |out| for the attention, 1e-5 / 1e-6 for the elementwise kernels (a handful of fp32
roundings on O(1) values).  bf16 attention: 2^-7 max |v| -- the probabilities and the output are each rounded once to bf16
(2^-9 relative, the output a convex combination of v rows); both can line up, and the bound allows a factor 2 over that.
bf16 elementwise: one output rounding, 2^-8 |y| + 1e-6."""
import math

import numpy as np
import pytest
import torch

from _gpu_util import dev, q, rnd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from thesis_pai_reconstruction_amd import ops
    return ops


# ---- attention ---------------------------------------------------------------------------------------------------------
def attn_ref(qkv, heads, ch):
    """qkv [N, T, heads * 3 * ch] (fp32 host) -> fp64 [N, T, heads * ch]: softmax((q s)(k s)^T) v, s = ch ** -0.25."""
    n, t, _ = qkv.shape
    x = qkv.double().view(n, t, heads, 3, ch)
    qq, kk, vv = x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2]
    s = float(ch) ** -0.25
    w = torch.einsum("nthc,nshc->nhts", qq * s, kk * s)
    w = torch.softmax(w, dim=-1)
    return torch.einsum("nhts,nshc->nthc", w, vv).reshape(n, t, heads * ch)


def run_attn(qkv, heads, ch, dtype):
    ops = _ops()
    n, t, _ = qkv.shape
    d_qkv = qkv.to(dev()).to(dtype).contiguous()
    out = torch.full((n, t, heads * ch), float("nan"), dtype=dtype, device=dev())
    ops.sattn_fwd(dtype, d_qkv, n, t, heads, ch, out)
    torch.cuda.synchronize()
    return out.float().cpu()


def check_attn(qkv, heads, ch, dtype, tag):
    want = attn_ref(qkv, heads, ch)
    got = run_attn(qkv, heads, ch, dtype)
    err = float((got.double() - want).abs().max())
    n, t, _ = qkv.shape
    vmax = float(qkv.view(n, t, heads, 3, ch)[:, :, :, 2].abs().max())
    bound = 1e-4 * float(want.abs().max()) if dtype == torch.float32 else 2.0 ** -7 * vmax
    print(f"sattn {tag} {dtype}: max err {err:.3e} bound {bound:.3e} (max|out| {float(want.abs().max()):.3f}, max|v| {vmax:.3f})")
    assert torch.isfinite(got).all()
    assert err <= bound


ATTN_CASES = [(16, 4, 32), (144, 4, 32), (144, 1, 64), (320, 4, 64), (96, 4, 256), (1, 4, 32)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,heads,ch", ATTN_CASES)
def test_sattn_against_fp64(T, heads, ch, dtype):
    qkv = q(rnd((2, T, heads * 3 * ch), seed=T + ch, scale=2.0), dtype)
    check_attn(qkv, heads, ch, dtype, f"T={T} heads={heads} ch={ch}")


def test_sattn_lane_maps_with_integer_data():
    """Exact small-integer q, k, v with an asymmetric v (v[key][c] depends on key and c differently): the scores are far
    apart, so each query copies one v row and a swapped row / column of either MFMA product shows as a wrong integer."""
    T, heads, ch = 64, 1, 32
    qkv = torch.zeros(1, T, 3 * ch)
    for i in range(T):
        qkv[0, i, i % ch] = 8.0                       # query i points at channel i % 32 ...
        qkv[0, i, ch + (5 * i + 3) % ch] = 8.0        # ... key j carries channel (5 j + 3) % 32, doubled for j >= 32
        if i >= 32:
            qkv[0, i, ch + (5 * i + 3) % ch] = 16.0
        qkv[0, i, 2 * ch:] = torch.arange(ch, dtype=torch.float32) + 3.0 * i
    want = attn_ref(qkv, heads, ch)
    got = run_attn(qkv, heads, ch, torch.bfloat16)
    # The winning key of every query has a score 64 / sqrt(32) = 11.3 above the runner-up, so the exact answer is the winner's
    # v row (integers below 256: exact in bf16) plus at most e^-11.3 * 96 = 1.2e-3, which the output rounding removes.  A
    # wrong row or column is off by a whole number.
    err = float((got.double() - want).abs().max())
    print(f"sattn integer data: max err {err:.3e}")
    assert err <= 0.01


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["last", "first"])
def test_sattn_dominant_key(where, dtype):
    """One key, in the last (or the first) key tile, scores about 30 above everything else for one query row: every earlier
    (later) tile's contribution has to be rescaled away, for that row only."""
    T, heads, ch = 320, 4, 64
    qkv = rnd((2, T, heads * 3 * ch), seed=77, scale=2.0)
    v = qkv.view(2, T, heads, 3, ch)
    iq, jk = 133, (317 if where == "last" else 3)
    for n in range(2):
        for h in range(heads):
            qv = v[n, iq, h, 0]
            others = (v[n, :, h, 1] @ qv) * ch ** -0.5
            others[jk] = -1e30
            target = float(others.max()) + 30.0
            v[n, jk, h, 1] = qv * (target * math.sqrt(ch) / float(qv @ qv))
    qkv = q(qkv, dtype)
    w = attn_ref(qkv, heads, ch)
    vv = qkv.view(2, T, heads, 3, ch)
    # the construction holds after rounding: query iq is (almost) a copy of v[jk]
    assert float((w.view(2, T, heads, ch)[:, iq] - vv[:, jk, :, 2].double()).abs().max()) < 1e-3
    check_attn(qkv, heads, ch, dtype, f"dominant key in the {where} tile")


def test_sattn_refuses_other_head_widths():
    ops = _ops()
    x = torch.zeros(1, 8, 3 * 48, device=dev())
    with pytest.raises(ops.PaiError, match="ch=48"):
        ops.sattn_fwd(torch.float32, x, 1, 8, 1, 48, torch.zeros(1, 8, 48, device=dev()))


# ---- out = act(x * A + B) --------------------------------------------------------------------------------------------
def silu64(v):
    return v / (1 + torch.exp(-v))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,rows,c,per_sample,silu", [(3, 35, 136, True, True), (3, 35, 136, False, True),
                                                      (3, 35, 136, True, False), (3, 35, 136, False, False),
                                                      (2, 4096, 128, True, True)])
def test_affine_act(n, rows, c, per_sample, silu, dtype):
    ops = _ops()
    x = q(rnd((n, rows, c), seed=rows + c, scale=2.0), dtype)
    A = rnd((n, c) if per_sample else (c,), seed=5) * 0.5 + 1.0
    B = rnd((n, c) if per_sample else (c,), seed=6)
    v = x.double() * (A.double().view(n, 1, c) if per_sample else A.double()) + \
        (B.double().view(n, 1, c) if per_sample else B.double())
    want = silu64(v) if silu else v
    out = torch.full((n, rows, c), float("nan"), dtype=dtype, device=dev())
    ops.affine_act(dtype, x.to(dev()).to(dtype), rows, n, c, A.to(dev()), B.to(dev()), per_sample,
                   ops.ACT_SILU if silu else ops.ACT_NONE, out)
    got = out.float().cpu().double()
    err = (got - want).abs()
    if dtype == torch.float32:
        rel = float(err.max() / want.abs().max())
        print(f"affine_act fp32 {(n, rows, c)} per_sample={per_sample} silu={silu}: max err / max|y| {rel:.3e}")
        assert rel <= 1e-5
    else:
        slack = float((err - (2.0 ** -8 * want.abs() + 1e-6)).max())
        print(f"affine_act bf16 {(n, rows, c)} per_sample={per_sample} silu={silu}: max err {float(err.max()):.3e} slack {slack:.3e}")
        assert slack <= 0


def test_silu_is_refused_elsewhere():
    """PAI_ACT_SILU belongs to pai_affine_act alone."""
    ops = _ops()
    a = torch.zeros(64, device=dev())
    with pytest.raises(ops.PaiError):
        ops.add_act(torch.float32, a, a, ops.ACT_SILU, torch.empty_like(a))
    with pytest.raises(ops.PaiError, match="act=7"):
        ops.affine_act(torch.float32, a.view(1, 8, 8), 8, 1, 8, a[:8], a[:8], False, 7, torch.empty(1, 8, 8, device=dev()))


# ---- 2 x 2 mean ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_avgpool2(dtype):
    ops = _ops()
    n, h, w, c = 2, 6, 10, 24
    x = q(rnd((n, h, w, c), seed=3), dtype)
    want = x.double().view(n, h // 2, 2, w // 2, 2, c).mean(dim=(2, 4))
    out = torch.full((n, h // 2, w // 2, c), float("nan"), dtype=dtype, device=dev())
    ops.avgpool2(dtype, x.to(dev()).to(dtype), n, h, w, c, out)
    err = (out.float().cpu().double() - want).abs()
    print(f"avgpool2 {dtype}: max err {float(err.max()):.3e}")
    if dtype == torch.float32:
        assert float(err.max()) <= 1e-6
    else:
        assert float((err - (2.0 ** -8 * want.abs() + 1e-6)).max()) <= 0


# ---- FiLM coefficients, noise-level embedding ---------------------------------------------------------------------
def test_film_coeffs():
    ops = _ops()
    n, c, ld, off = 3, 40, 200, 64           # scale | shift are columns [off, off + 2c) of rows of ld elements
    a, b = rnd((c,), seed=1) * 0.3 + 1.0, rnd((c,), seed=2)
    emb = rnd((n, ld), seed=3) * 0.5
    A, B = (torch.full((n, c), float("nan"), device=dev()) for _ in range(2))
    d_emb = emb.to(dev())
    ops.film_coeffs(c, n, a.to(dev()), b.to(dev()), d_emb[:, off:], ld, A, B)
    sc, sh = emb[:, off:off + c].double(), emb[:, off + c:off + 2 * c].double()
    wa, wb = a.double() * (1 + sc), b.double() * (1 + sc) + sh
    ea, eb = float((A.cpu().double() - wa).abs().max()), float((B.cpu().double() - wb).abs().max())
    print(f"film_coeffs: max err A {ea:.3e} B {eb:.3e}")
    assert ea <= 1e-6 and eb <= 1e-6


@pytest.mark.parametrize("dim", [128, 7])
def test_gamma_embedding(dim):
    ops = _ops()
    g = torch.tensor([1e-6, 1.0, 0.37, 1.3e-3], dtype=torch.float32)
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    args = g.double()[:, None] * f[None]
    want = torch.cat([torch.cos(args), torch.sin(args)], -1)
    if dim % 2:
        want = torch.cat([want, torch.zeros(len(g), 1, dtype=torch.float64)], -1)
    out = torch.full((len(g), dim), float("nan"), device=dev())
    ops.gamma_embedding(g.to(dev()), len(g), dim, out)
    err = float((out.cpu().double() - want).abs().max())
    print(f"gamma_embedding dim={dim}: max err {err:.3e}")
    assert err <= 1e-6


# ---- one reverse step --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_table(pai):
    return pai.Palette(1, 1, (1, 2), (2,), 0.0, "linear", False).diffusion_inf.step_table()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("t", [99, 50, 1, 0])
@pytest.mark.parametrize("add_noise", [0, 1])
@pytest.mark.parametrize("learn_var", [0, 1])
def test_palette_step(step_table, learn_var, add_noise, t, dtype):
    ops = _ops()
    px, c = 700, 3
    s1, rs, c0, c1, llo, lhi = (np.float64(v) for v in step_table[t])
    y = rnd((px, c), seed=t + 1)
    noise = rnd((px, c), seed=t + 2)
    rng = np.random.default_rng(t)
    y0_target = torch.from_numpy(rng.uniform(-2.0, 2.0, (px, c)))          # half of y0 beyond the clamp, on either side
    eps = q(((y.double() - y0_target / rs) / s1).float(), dtype)
    # The variance channel interpolates between the two log variances, so its domain is [-1, 1] (v in [0, 1]); about a tenth
    # of the values sit on either end.  Outside it the log variance is extrapolated: at t = 0, where log(var_lower) is
    # log(1e-20), v = 1.5 gives a standard deviation of about 100, |y_{t-1}| of several hundred, and an fp32 output cannot
    # hold 1e-5 absolute there (its ulp is 3e-5).
    var = q(rnd((px, c), seed=t + 3) * 0.6, dtype).clamp(-1.0, 1.0)
    mo =torch.cat([eps, var], 1) if learn_var else eps
    y0 = rs * (y.double() - s1 * eps.double())
    assert 0.2 < float((y0.abs() > 1).double().mean()) < 0.8
    y0 = y0.clamp(-1, 1)
    mean = c0 * y0 + c1 * y.double()
    lv = llo
    if learn_var:
        vi = (var.double() + 1) / 2
        lv = vi * lhi + (1 - vi) * llo
    want = mean + (torch.exp(0.5 * torch.as_tensor(lv)) * noise.double() if add_noise else 0.0)
    y_next = torch.full((px, c), float("nan"), device=dev())
    xy = torch.full((px, 2 * c), 7.0, dtype=dtype, device=dev())
    ops.palette_step(dtype, mo.to(dev()).to(dtype).contiguous(), y.to(dev()), noise.to(dev()), px, c, learn_var, add_noise,
                     step_table[t], y_next, xy)
    got = y_next.cpu().double()
    err = float((got - want).abs().max())
    print(f"palette_step t={t} learn_var={learn_var} add_noise={add_noise} {dtype}: max err {err:.3e}")
    assert err <= 1e-5
    xyc = xy.float().cpu().double()
    assert bool((xyc[:, :c] == 7.0).all())                                  # the x half is not touched
    assert float(((xyc[:, c:] - want).abs() - ((2.0 ** -8 if dtype == torch.bfloat16 else 0.0) * want.abs() + 1e-5)).max()) <= 0
