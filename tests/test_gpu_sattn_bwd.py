"""GPU: the differentiable spatial attention of the Palette levels -- pai_sattn_fwd_lse, pai_sattn_bwd (delta, the dK / dV
kernel with the key on the lane, the dQ kernel with the query on the lane; fp32: the vector-ALU kernels) and
functional.spatial_attention -- element by element against the fp64 formulas of tests/_sattn_ref.py, which
tests/test_sattn_ref_host.py ties to the reference's own autograd.

The backward is DEFINED on the tensors it is handed: every reference starts from exactly the stored qkv, out, lse and dout
(bf16: the bf16-rounded values; lse: the fp32 cast of the fp64 value).  Every output buffer is NaN before the call and
carries 64 NaN guard elements behind it that must still be NaN afterwards.

Bounds -- the project's existing bars (docstring of tests/test_gpu_vit_ops.py) with the one term the recomputation of P adds;
u = 2^-24, e_s = ch u scale2 max_ij sum_d |q_id k_jd| (an fp32 dot product in any order, here in the exponent of P), A = the
fp64 sum of the absolute terms of the element, C = what dP - delta can lose (tests/_sattn_ref.py):
  lse                 |lse - ref| <= 2 e_s + 1e-5 max(1, |ref|)
  out of fwd_lse      the bits of pai_sattn_fwd
  delta (ws)          1e-5 * sum_c |dO_ic O_ic|
  dqkv fp32           (1e-5 + e_s + 1e-6) A + u (2 ch + 2) C
  dqkv bf16           2^-8 (A + |ref|) + (1e-5 + e_s) A + 1e-6 max |ref|
  integer lane maps   2^-8 |ref| + 0.01 (test_mha_lane_maps)
  spatial_attention   against the fixture's fp64 dqkv: fp32 max error <= 1e-4 max |ref|; bf16 relative L2 <= twice the reference's
                      own bf16 deviation recorded in the fixture (the Palette bar)

What has and has not been run on an MI355X: DESIGN.md section 7c.

Which case fails which fault:
  a swapped row / column of a fragment (S, dP, dV^T, dK^T, dQ^T)   test_lane_maps (whole and half numbers)
  exp(s) * exp(-lse) instead of exp(s - lse)                          test_large_score (exp(100) overflows fp32)
  a padded query / key that contributes                               T = 1, 16, 130, 144: ragged tiles, P = 0 past T
  an unwritten element, a write past the end                          the NaN fill and the guards of every call
  a sum across workgroups in arrival order                            test_backward_is_reproducible
"""
import math
from functools import lru_cache

import pytest
import torch

import _sattn_ref as R
from _gpu_util import dev, q, rnd
from oracle import golden

pytestmark = pytest.mark.gpu

GUARD = 64
U = 2.0 ** -24
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
CASES = [(1, 4, 32), (16, 4, 32), (144, 4, 32), (144, 1, 64), (320, 4, 64), (130, 2, 128)]
F32_ONLY = [(96, 4, 256)]
FWD_CASES = [(16, 4, 32), (144, 4, 32), (144, 1, 64), (320, 4, 64), (96, 4, 256), (1, 4, 32)]   # ATTN_CASES of the forward's tests
N = 2


def _ops():
    from thesis_pai_reconstruction_amd import ops
    return ops


def _poisoned(n, dtype=torch.float32):
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev())


def _written(buf, n, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:]).all()), f"{what}: the guard behind the buffer was written"
    got = buf[:n].float().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: an element was not written (or is not finite)"
    return got


def _d(t, dtype):
    return t.to(dev()).to(dtype).contiguous()


def fwd_lse(qkv, heads, ch, dtype):
    """One pai_sattn_fwd_lse call on the host tensor qkv (already rounded to dtype): out (device, dtype), lse (host fp32)."""
    n, t, _ = qkv.shape
    out, lse = _poisoned(n * t * heads * ch, dtype), _poisoned(n * heads * t)
    _ops().sattn_fwd_lse(dtype, _d(qkv, dtype), n, t, heads, ch, out[:n * t * heads * ch], lse[:n * heads * t])
    _written(out, n * t * heads * ch, "out")
    return out[:n * t * heads * ch].view(n, t, heads * ch), _written(lse, n * heads * t, "lse").view(n, heads, t)


def bwd(dout, qkv, out, lse, heads, ch, dtype):
    """One pai_sattn_bwd call on host tensors: dqkv and ws as host fp32."""
    n, t, w = qkv.shape
    dqkv, ws = _poisoned(n * t * w, dtype), _poisoned(n * heads * t)
    _ops().sattn_bwd(dtype, _d(dout, dtype), _d(qkv, dtype), _d(out, dtype), _d(lse, torch.float32), n, t, heads, ch,
                     dqkv[:n * t * w], ws[:n * heads * t])
    return _written(dqkv, n * t * w, "dqkv").view(n, t, w), _written(ws, n * heads * t, "ws").view(n, heads, t)


def e_s(qkv, heads, ch):
    return ch * U / math.sqrt(ch) * R.score_abs_max(qkv, heads, ch)


def stored(qkv, dout, heads, ch, dtype):
    """The tensors a backward call is handed, as the forward would have stored them: out rounded to dtype, lse to fp32."""
    out, lse = R.forward(qkv, heads, ch)
    return q(out.float(), dtype), lse.float()


def check_bwd(qkv, dout, heads, ch, dtype, tag):
    """Backward from exactly the stored tensors against the fp64 formulas; returns (got dqkv, ref dict)."""
    out, lse = stored(qkv, dout, heads, ch, dtype)
    ref = R.backward(dout, qkv, out, lse, heads, ch)
    got, ws = bwd(dout, qkv, out, lse, heads, ch, dtype)
    es = e_s(qkv, heads, ch)
    a, c, g = ref["abs"], ref["cancel"], ref["dqkv"]
    if dtype == torch.float32:
        lim = (1e-5 + es + 1e-6) * a + U * (2 * ch + 2) * c
    else:
        lim = 2.0 ** -8 * (a + g.abs()) + (1e-5 + es) * a + 1e-6 * float(g.abs().max())
    err = (got.double() - g).abs()
    werr = (ws.double() - ref["delta"]).abs()
    wlim = 1e-5 * ref["delta_abs"]
    n, t, _ = qkv.shape
    e4, l4 = err.view(n, t, heads, 3, ch), lim.view(n, t, heads, 3, ch)
    parts = " ".join(f"{name} {float(e4[:, :, :, k].max()):.3e} ({float((e4[:, :, :, k] / l4[:, :, :, k].clamp_min(1e-300)).max()):.3f})"
                     for k, name in enumerate(("dQ", "dK", "dV")))
    print(f"sattn_bwd {tag} {IDS[DTYPES.index(dtype)]}: max err (err / bound) {parts}; delta {float(werr.max()):.3e} "
          f"({float((werr / wlim.clamp_min(1e-300)).max()):.3f}); e_s {es:.2e}")
    assert bool((werr <= wlim).all()), "delta"
    assert bool((err <= lim).all()), "dqkv"
    return got, ref


@lru_cache(maxsize=None)
def random_case(T, heads, ch, bf16):
    dtype = torch.bfloat16 if bf16 else torch.float32
    return (q(rnd((N, T, heads * 3 * ch), seed=T + ch, scale=2.0), dtype), q(rnd((N, T, heads * ch), seed=T + ch + 1), dtype))


# ---- 1. fwd_lse -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T,heads,ch", sorted(set(CASES + F32_ONLY + FWD_CASES)), ids=lambda v: str(v))
def test_fwd_lse(T, heads, ch, dtype):
    """out has the bits of pai_sattn_fwd (ch = 256 included, both dtypes); lse is m + ln(l) within the bound of an fp32 score."""
    qkv, _ = random_case(T, heads, ch, dtype == torch.bfloat16)
    out, lse = fwd_lse(qkv, heads, ch, dtype)
    plain = torch.full_like(out, float("nan"))
    _ops().sattn_fwd(dtype, _d(qkv, dtype), N, T, heads, ch, plain)
    torch.cuda.synchronize()
    assert torch.equal(out, plain)
    _, ref = R.forward(qkv, heads, ch)
    err = (lse.double() - ref).abs()
    lim = 2 * e_s(qkv, heads, ch) + 1e-5 * ref.abs().clamp_min(1.0)
    print(f"sattn_fwd_lse {(T, heads, ch)} {IDS[DTYPES.index(dtype)]}: max lse err {float(err.max()):.3e} "
          f"(err / bound {float((err / lim).max()):.3f})")
    assert bool((err <= lim).all())


# ---- 2. backward against the fp64 formulas ----------------------------------------------------------------------------------
BWD_PARAMS = [pytest.param(*c, d, id=f"{c}-{i}") for c in CASES for d, i in zip(DTYPES, IDS)]
BWD_PARAMS += [pytest.param(*c, torch.float32, id=f"{c}-f32") for c in F32_ONLY]


@pytest.mark.parametrize("T,heads,ch,dtype", BWD_PARAMS)
def test_backward_against_fp64(T, heads, ch, dtype):
    """One ragged tile (T = 1, 16), two and three key blocks with a ragged last one (130, 144, 320), a query block with a single
    live row (T = 130: rows 128, 129 are alone in the second workgroup; T = 1), every head width; ch = 256 in fp32 only (bf16
    refuses it: test_refusals)."""
    qkv, dout = random_case(T, heads, ch, dtype == torch.bfloat16)
    check_bwd(qkv, dout, heads, ch, dtype, f"{(T, heads, ch)}")


# ---- 3. lane maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,heads,ch", [(64, 1, 32), (160, 2, 64)], ids=lambda v: str(v))
@pytest.mark.parametrize("paired", [False, True], ids=["onehot", "paired"])
def test_lane_maps(paired, T, heads, ch):
    """Exact integer data (tests/_sattn_ref.py::lane_map_data; margins asserted on the host by tests/test_sattn_ref_host.py) for
    the five MFMA products of each backward kernel: a swapped row / column of any fragment is off by 0.5 or more."""
    bf = torch.bfloat16
    qkv, dout = R.lane_map_data(1, T, heads, ch, paired)
    assert torch.equal(q(qkv, bf), qkv) and torch.equal(q(dout, bf), dout)
    out_x, lse_x = R.forward(qkv, heads, ch)
    out_d, lse = fwd_lse(qkv, heads, ch, bf)
    assert float((out_d.float().cpu().double() - out_x).abs().max()) <= 0.01
    assert float((lse.double() - lse_x).abs().max()) <= 2 * e_s(qkv, heads, ch) + 1e-5 * float(lse_x.abs().max())
    # the backward is handed the whole numbers the construction stands for: the exact out is within e^-32 |v| of them, and that
    # remainder is a bf16 value where v = 0 (1e-11), which the fp64 delta would see and no fp32 sum can
    assert float((out_x - out_x.round()).abs().max()) < 1e-6 and float(out_x.abs().max()) <= 256
    out, lse_s = q(out_x.round().float(), bf), lse_x.float()
    assert torch.equal(out.double(), out_x.round())
    ref = R.backward(dout, qkv, out, lse_s, heads, ch)
    got, ws = bwd(dout, qkv, out, lse_s, heads, ch, bf)
    g = ref["dqkv"]
    err = (got.double() - g).abs()
    print(f"sattn_bwd lane maps {'paired' if paired else 'onehot'} {(T, heads, ch)}: max err {float(err.max()):.3e}, "
          f"max |ref| {float(g.abs().max()):.1f}")
    assert torch.equal(ws.double(), ref["delta"]), "delta of integer data is exact"
    assert bool((err <= 2.0 ** -8 * g.abs() + 0.01).all())
    # the construction has teeth
    p = ref["p"]
    assert float((p.max(-1).values - (0.5 if paired else 1.0)).abs().max()) < 1e-5      # lse is the fp32 cast here
    g4 = g.view(1, T, heads, 3, ch)
    assert float(g4[:, :, :, 2].abs().max()) >= 1
    if paired:
        assert float(g4[:, :, :, 0].abs().max()) >= 1 and float(g4[:, :, :, 1].abs().max()) >= 1
        assert int((g4[:, :, :, 0].abs().sum(-1) > 0.5).sum()) >= T * heads // 2


# ---- 4. / 5. a dominant key, a large score ------------------------------------------------------------------------------------
def _dominant(T, heads, ch, jk, dtype, lift, absolute):
    """The construction of test_sattn_dominant_key: for query iq of every (n, h), key jk scores `lift` above every other key
    (absolute: scores `lift`)."""
    qkv = rnd((N, T, heads * 3 * ch), seed=77, scale=2.0)
    v = qkv.view(N, T, heads, 3, ch)
    iq = 133 if T > 133 else T // 2
    for n in range(N):
        for h in range(heads):
            qv = v[n, iq, h, 0]
            others = (v[n, :, h, 1] @ qv) * ch ** -0.5
            others[jk] = -1e30
            target = lift if absolute else float(others.max()) + lift
            v[n, jk, h, 1] = qv * (target * math.sqrt(ch) / float(qv @ qv))
    return q(qkv, dtype), q(rnd((N, T, heads * ch), seed=78), dtype), iq


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("where", ["last", "first"])
def test_dominant_key(where, dtype):
    """One key, in the last (or the first) key tile, scores about 30 above everything else for one query row.  The bounds of
    test_backward_against_fp64; in fp32 the C term is what covers the dominated row (dS there is a difference of two fp32
    numbers of size |dP|)."""
    T, heads, ch = 320, 4, 64
    jk = 317 if where == "last" else 3
    qkv, dout, iq = _dominant(T, heads, ch, jk, dtype, 30.0, False)
    _, ref = check_bwd(qkv, dout, heads, ch, dtype, f"dominant key in the {where} tile")
    assert float(ref["p"][:, :, iq, jk].min()) > 1 - 1e-5, "the construction holds after rounding"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_large_score(dtype):
    """The dominant score at 100: exp(100) overflows fp32, so exp(s) * exp(-lse) is inf * 0 here; the exponent formed as one
    difference stays at 0.  Forward (lse = 100) and backward both finite, the backward inside its bound."""
    T, heads, ch = 144, 2, 64
    qkv, dout, iq = _dominant(T, heads, ch, 140, dtype, 100.0, True)
    sc = R.scores(qkv, heads, ch)
    assert float(sc[:, :, iq, 140].min()) > 95
    out, lse = fwd_lse(qkv, heads, ch, dtype)     # _written asserts that every element is finite
    _, ref = R.forward(qkv, heads, ch)
    assert bool(((lse.double() - ref).abs() <= 2 * e_s(qkv, heads, ch) + 1e-5 * ref.abs().clamp_min(1.0)).all())
    check_bwd(qkv, dout, heads, ch, dtype, "score 100")


# ---- 6. reproducibility -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_backward_is_reproducible(dtype):
    T, heads, ch = 320, 4, 64
    qkv, dout = random_case(T, heads, ch, dtype == torch.bfloat16)
    out, lse = stored(qkv, dout, heads, ch, dtype)
    a, _ = bwd(dout, qkv, out, lse, heads, ch, dtype)
    b, _ = bwd(dout, qkv, out, lse, heads, ch, dtype)
    assert torch.equal(a, b)


# ---- 7. functional.spatial_attention ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fix(golden_dir):
    return golden.load(golden_dir, "ref_sattn_grad")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [0, 1, 2])
def test_spatial_attention(pai, fix, c, dtype):
    """The autograd function: out bits of ops.sattn_fwd, qkv.grad bits of a direct ops.sattn_bwd on the saved tensors, the
    gradient against the reference's own fp64 autograd (fixture), no host synchronisation in either direction, and the NHWC
    form."""
    from thesis_pai_reconstruction_amd import functional as PF
    ops = _ops()
    n, t, heads, ch = (int(v) for v in fix[f"shape{c}"])
    qkv = _d(torch.from_numpy(fix[f"qkv{c}"]), dtype).requires_grad_(True)
    dout = _d(torch.from_numpy(fix[f"dout{c}"]), dtype)
    want = torch.from_numpy(fix[f"dqkv{c}"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = PF.spatial_attention(qkv, heads)
        out.backward(dout)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out.shape == (n, t, heads * ch) and out.dtype == dtype and qkv.grad.shape == qkv.shape
    plain = torch.empty_like(out)
    ops.sattn_fwd(dtype, qkv.detach(), n, t, heads, ch, plain)
    assert torch.equal(out.detach(), plain)
    o2, lse = torch.empty_like(plain), torch.empty(n, heads, t, device=dev())
    ops.sattn_fwd_lse(dtype, qkv.detach(), n, t, heads, ch, o2, lse)
    dq, ws = torch.empty_like(qkv), torch.empty(n * heads * t, device=dev())
    ops.sattn_bwd(dtype, dout, qkv.detach(), o2, lse, n, t, heads, ch, dq, ws)
    torch.cuda.synchronize()
    assert torch.equal(qkv.grad, dq)
    got = qkv.grad.float().cpu().double()
    if dtype == torch.float32:
        err, lim = float((got - want).abs().max()), 1e-4 * float(want.abs().max())
        print(f"spatial_attention f32 case {c}: max err {err:.3e} bound {lim:.3e}")
    else:
        err, lim = float((got - want).norm() / want.norm()), 2 * float(fix[f"bf16_dev{c}"])
        print(f"spatial_attention bf16 case {c}: rel L2 {err:.3e} bound {lim:.3e}")
    assert err <= lim
    # NHWC: the same bits
    hh = 4 if t % 4 == 0 else 1
    x4 = qkv.detach().view(n, hh, t // hh, heads * 3 * ch).clone().requires_grad_(True)
    o4 = PF.spatial_attention(x4, heads)
    o4.backward(dout.view(n, hh, t // hh, heads * ch))
    torch.cuda.synchronize()
    assert o4.shape == (n, hh, t // hh, heads * ch)
    assert torch.equal(o4.detach().view_as(out), out.detach()) and torch.equal(x4.grad.view_as(qkv), qkv.grad)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(pai):
    from thesis_pai_reconstruction_amd import functional as PF
    ops = _ops()
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev())
    with pytest.raises(ops.PaiError, match="ch=48"):
        ops.sattn_fwd_lse(torch.float32, z(1, 8, 144), 1, 8, 1, 48, z(1, 8, 48), z(8))
    with pytest.raises(ops.PaiError, match="ch=48"):
        ops.sattn_bwd(torch.float32, z(1, 8, 48), z(1, 8, 144), z(1, 8, 48), z(8), 1, 8, 1, 48, z(1, 8, 144), z(8))
    with pytest.raises(ops.PaiError, match="ch=48"):
        PF.spatial_attention(z(1, 8, 144), 1)
    bf = torch.bfloat16
    guard = torch.full((1, 8, 768), float("nan"), dtype=bf, device=dev())
    with pytest.raises(ops.PaiError, match="ch=256 has no bf16 backward"):
        ops.sattn_bwd(bf, z(1, 8, 256, dtype=bf), z(1, 8, 768, dtype=bf), z(1, 8, 256, dtype=bf), z(8), 1, 8, 1, 256, guard, z(8))
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard).all()), "refused before any launch"
    with pytest.raises(ops.PaiError, match="ch=256"):
        PF.spatial_attention(z(1, 8, 768, dtype=bf), 1)
    with pytest.raises(ops.PaiError, match="device"):
        PF.spatial_attention(torch.zeros(1, 8, 96), 1)
    with pytest.raises(ops.PaiError, match="contiguous"):
        PF.spatial_attention(z(1, 96, 8).transpose(1, 2), 1)
    with pytest.raises(ops.PaiError, match="divisible"):
        PF.spatial_attention(z(1, 8, 100), 1)
    with pytest.raises(ops.PaiError, match="null"):
        ops.sattn_bwd(torch.float32, z(1, 8, 32), z(1, 8, 96), z(1, 8, 32), None, 1, 8, 1, 32, z(1, 8, 96), z(8))
    with pytest.raises(ops.PaiError, match="aligned"):
        ops.sattn_bwd(torch.float32, z(1, 8, 32), z(1, 8, 96), z(1, 8, 32), z(9)[1:], 1, 8, 1, 32, z(1, 8, 96), z(8))
    with pytest.raises(ops.PaiError, match="65535"):
        ops.sattn_bwd(torch.float32, z(8), z(8), z(8), z(8), 65536, 1, 1, 32, z(8), z(8))
