"""GPU: every kernel of csrc/vit.hip (LayerNorm, GELU, the attention core on its vector-ALU and its matrix-core path,
subsample2, bn_stats) and the two helpers of csrc/misc.hip they call (colsum, reduce_rows), each on its own through its
ops.* wrapper, element by element against the fp64 host references of tests/_vit_ref.py (tied to PyTorch's double-precision
ops and autograd by tests/test_vit_refs_host.py), at the launch edges tests/test_gpu_transunet.py does not reach.

Every reference starts from exactly the tensors handed to the kernel (in bf16: the bf16-rounded values; the backward
kernels get the fp32 casts of the reference mean / rstd / probs, and their references use those casts).  The LayerNorm of a
residual sum is DEFINED on the sum as stored: its reference takes the sum_out the kernel wrote, which is checked
elementwise on its own (the docstring of tests/test_gpu_gate.py explains why).  Every output buffer is NaN before the call
and carries 64 NaN guard elements behind it that must still be NaN afterwards.

Bounds -- the project's existing bars, none fitted to what a kernel produced (u = 2^-24):
  fp32 elementwise outputs     |got - ref| <= 1e-5 max |ref|
  bf16 stored outputs          |got - ref| <= 2^-8 |ref| + 1e-6 max |ref|    (one rounding of an fp32 value + fp32 noise at 0)
  fp32 sums, per element       |got - ref| <= 1e-5 * (fp64 sum of the absolute terms of that element): LayerNorm mean,
                               dgamma / dbeta, bn_stats, colsum, reduce_rows
  rstd                         1e-5 relative
  probs (fp32, both paths)     |p - ref| <= ref (2 e_s + 1e-6) + 1e-9, e_s = hd u scale max_ij sum_d |q_id k_jd|: the a-priori
                               bound of an fp32 dot product in any order, once in exp(s - max) and once in the row sum;
                               row sums within 1e-5 of 1
  attention output             fp32: 1e-4 max |ref|;  bf16 vector path: the bf16 stored-output bound (P stays fp32);
                               bf16 matrix-core path: 2^-7 * mass * max |v|, mass = the largest row sum of P * mask (P and
                               the output are each rounded once to bf16, half an ulp = at most 2^-8 relative each; 2^-7
                               when both line up -- the argument of the Palette attention)
  attention gradients          with A = the fp64 sum of the absolute terms of the element (dQ: scale sum_j |dS_ij| |K_jd|,
                               dK: scale sum_i |dS_ij| |Q_id|, dV: sum_i |Pm_ij| |dO_id|):
                               fp32: 1e-5 A (test_mha_dominant_key: + u (hd + S + 2) C for the cancellation in
                               dP - sum_j P dP, which the relative bound has no term for -- derived in its docstring);
                               bf16 vector path: 2^-8 |ref| + 1e-6 max |ref| + 1e-5 A;
                               bf16 matrix-core path: 2^-8 (A + |ref|) + 1e-6 max |ref|  (dS and P^T rounded to bf16 before
                               their products: at most 2^-8 of every term; the result rounded once more: 2^-8 |ref|)
  GELU / GELU' fp32            erff / expf accuracy cannot be derived: the bar is four times the error of PyTorch-CPU's own
                               fp32 F.gelu / its gradient against fp64 on the arguments of the largest case (a CPU
                               measurement of the reference, repeated and printed by tests/test_vit_refs_host.py):
                               measured 1.221e-6 (GELU) and 2.863e-7 per unit |dy| (GELU'), so 4.884e-6 and 1.145e-6,
                               and never above 1e-6 (1 + |z|) resp. 1e-6 |dy| (1 + |z|), which is the binding part for
                               GELU at |z| < 3.88 and for GELU' at |z| < 0.145;  bf16: the bf16 stored-output bound
  subsample2 and its adjoint   the same bits (torch.equal)
  integer lane-map data        every intermediate is exact by construction, the exact answer is a whole (or half) number and a
                               swapped row / column is off by at least 0.5: 0.01 absolute (+ 2^-8 |ref| for the one output
                               rounding of a gradient), the bound of test_sattn_lane_maps_with_integer_data

Maxima measured on an MI355X (pytest -s; largest error and largest error / bound over all cases; every bound held).  The
fp32 backward of test_mha_dominant_key is younger than this run: its figures come from an fp32 emulation of the formulas on
the host only (error / bound 0.01; error / (1e-5 A) as its docstring says) and are not yet measured on the device.
  layernorm_fwd   sum_out 1.56e-2 (0.996, bf16), mean 8.7e-7 (0.004), rstd 1.3e-5 absolute at D = 1 (0.012), y f32 7.7e-7
                  (0.019), y bf16 1.56e-2 (0.994)
  layernorm_bwd   dx 7.8e-3 (0.993, bf16; f32 0.012), dbeta 6.3e-6 (0.010), dgamma 7.5e-6 (0.017)
  gelu / gelu'    f32: 4.47e-7 (0.092 of the bound) / 3.46e-7 (0.161); bf16: 7.8e-3 (0.963) / 7.8e-3 (0.996)
  probs           matrix-core 1.9e-7 (0.020), vector f32 3.9e-7 (0.101), vector bf16 1.9e-7 (0.064); row sums within 1.9e-7 of 1
  attention out   matrix-core 1.15e-2 (0.527), vector bf16 6.7e-3 (0.995), f32 8.3e-7 (0.006)
  dQ / dK / dV    matrix-core 5.9e-2 / 2.2e-2 / 2.1e-2 (0.761 / 0.752 / 0.828), vector bf16 (0.990 / 0.989 / 0.988),
                  f32 3.2e-7 / 2.2e-7 / 2.1e-7 (0.066 / 0.069 / 0.021)
  bn_stats 2.4e-4 (0.069), colsum increment 1.6e-2 (0.025), reduce_rows 1.7e-6 (0.006); subsample2: equal bits
The ratios near 1 are bf16 stored outputs: 2^-8 |ref| IS half an ulp of a value just above a power of two, so a correctly
rounded result reaches the bound and one extra rounding anywhere exceeds it.

Not covered: the branch of launch_colsum that shrinks `chunks` when blocks * chunks > 4096 (row blocks of at least 256 rows
times 256-column chunks, e.g. 512 blocks x 9 chunks or 65 x 64): more than 4096 x 256 x 256 elements, a tensor of several
hundred MB.

Which case fails which fault (read the kernels with this list):
  a dropped max-subtraction                     test_mha_large_score (one score of 100: expf overflows, probs become NaN), both
                                                paths, and ragged S = 7 next to the -inf padding keys of the matrix-core tile
  a transposed mha_tr_frag                      test_mha_lane_maps[onehot-*]: every query copies one row of an asymmetric v
                                                (forward), of an asymmetric dO (dV); [paired-*]: dQ = dS K and dK = dS^T Q
  an empty LayerNorm slab that does not write   test_layernorm_bwd[*-1030-40]: slabs 61..63 own no row, `partials` is NaN
  a one-pass variance                           test_layernorm_fwd_offset_rows (mean = 30 sigma, the rstd bound)
  a bn_stats lane count for the wrong width     test_bn_stats with C = 300 and C = 513 (last chunks of 44 and 1 columns)
  a write past numel                            the guard of every test; GELU and subsample2_bwd past the 8192 x 256 grid
"""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

import _vit_ref as R
from _gpu_util import dev, q, rnd

pytestmark = pytest.mark.gpu

GUARD = 64
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
EPS = float(np.float32(1e-5))
GELU_BOUND = 4 * R.GELU_TORCH_ERR            # 4.884e-6, capped per element by 1e-6 (1 + |z|)
GELU_BWD_BOUND = 4 * R.GELU_BWD_TORCH_ERR    # 1.145e-6 per unit |dy|, capped per element by 1e-6 (1 + |z|)


def _ops():
    from thesis_pai_reconstruction_amd import ops
    return ops


# ---- device helpers (as tests/test_gpu_gate.py) ---------------------------------------------------------------------------
def _d(t, dtype=torch.float32):
    return None if t is None else t.to(dev()).to(dtype).contiguous()


def _poisoned(n, dtype=torch.float32):
    """An output buffer of n elements followed by GUARD guard elements, all NaN."""
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev())


def _guard_ok(full, n, what):
    assert bool(torch.isnan(full[n:]).all()), f"{what}: wrote past its {n} elements"


def _written(full, n, what):
    """Nothing beyond the n elements was touched, every one of them was written; returns them on the host (fp32)."""
    _guard_ok(full, n, what)
    got = full[:n].float().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: elements left unwritten (or not finite)"
    return got


def _within(got, ref, lim, what):
    """|got - ref| <= lim elementwise; prints the largest error and the largest error / bound."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    lim = lim.double().reshape(-1) if torch.is_tensor(lim) else torch.full_like(ref, float(lim))
    err = (got - ref).abs()
    ratio = float((err / lim.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max err {float(err.max()):.3g}, max err / bound {ratio:.3g}")
    bad = err > lim
    assert not bool(bad.any()), (what, int(bad.sum()), float((err - lim).max()))


def _stored_lim(ref):
    ref = ref.double()
    return 2.0 ** -8 * ref.abs() + 1e-6 * float(ref.abs().max())


def _elem_ok(got, ref, dtype, what):
    ref = ref.double()
    _within(got, ref, 1e-5 * float(ref.abs().max()) if dtype == torch.float32 else _stored_lim(ref), what)


def _t(dtype):
    return IDS[DTYPES.index(dtype)]


def _sum_ok(got, ref, abs_terms, what):
    _within(got, ref, 1e-5 * abs_terms.double(), what)


# ---- LayerNorm forward ------------------------------------------------------------------------------------------------
LN_CASES = [(1, 1, 1), (7, 1000, 1), (12, 96, 4), (3, 257, 3), (2, 12288, 2)]


def _ln_fwd(x, r, gamma, beta, post, P, dtype, y_from_stored_stats=False):
    """One pai_layernorm_fwd call on host inputs (already rounded through dtype), all checks; r / post None: plain."""
    ops = _ops()
    M, D = x.shape
    s_buf = _poisoned(M * D, dtype) if r is not None else None
    y_buf, mean_buf, rstd_buf = _poisoned(M * D, dtype), _poisoned(M), _poisoned(M)
    ops.layernorm_fwd(dtype, _d(x, dtype), _d(r, dtype), M, D, _d(gamma), _d(beta), EPS, _d(post), P,
                      None if r is None else s_buf[:M * D], y_buf[:M * D], mean_buf[:M], rstd_buf[:M])
    torch.cuda.synchronize()
    got_s = None
    t = f"layernorm_fwd {_t(dtype)}"
    if r is not None:
        got_s = _written(s_buf, M * D, "sum_out").view(M, D)
        _elem_ok(got_s, x.double() + r.double(), dtype, f"{t} sum_out")
    got_mean, got_rstd = _written(mean_buf, M, "mean"), _written(rstd_buf, M, "rstd")
    ref = R.layernorm_fwd(x, r, gamma, beta, EPS, post, P, s_stored=got_s)
    _sum_ok(got_mean, ref["mean"], ref["mean_abs"], f"{t} mean")
    _within(got_rstd, ref["rstd"], 1e-5 * ref["rstd"], f"{t} rstd")
    if y_from_stored_stats:
        ref = R.layernorm_fwd(x, r, gamma, beta, EPS, post, P, s_stored=got_s, mean=got_mean, rstd=got_rstd)
    _elem_ok(_written(y_buf, M * D, "y"), ref["y"], dtype, f"{t} y")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "res+post"])
@pytest.mark.parametrize("M,D,P", LN_CASES, ids=lambda v: str(v))
def test_layernorm_fwd(pai, M, D, P, fused, dtype):
    """D = 1 (variance 0, rstd = eps^-1/2), D below / not a multiple of / far above the 256 threads, D = 12288 (the documented
    limit: 49 184 B of LDS), post periods 1 .. 4."""
    x, r = q(rnd((M, D), 1) * 1.5 + 0.2, dtype), q(rnd((M, D), 2), dtype)
    gamma, beta, post = 1 + 0.1 * rnd((D,), 3), 0.1 * rnd((D,), 4), rnd((P, D), 5)
    _ln_fwd(x, r if fused else None, gamma, beta, post if fused else None, P, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_fwd_offset_rows(pai, dtype):
    """Row mean = 30 standard deviations: E[x^2] - mean^2 in fp32 loses the variance to 1e-4 relative and fails the rstd bound;
    the two-pass kernel holds it.  y is referenced from the mean / rstd the kernel stored (each checked on its own): at
    |x| = 30 sigma an admissible 1e-5 relative error of the mean alone would move y by 3e-4."""
    M, D = 4, 1000
    x = q(30.0 + rnd((M, D), 11), dtype)
    assert float((x.double().mean(1) / x.double().std(1)).min()) > 25
    _ln_fwd(x, None, 1 + 0.1 * rnd((D,), 3), 0.1 * rnd((D,), 4), None, 1, dtype, y_from_stored_stats=True)


def test_layernorm_refusals(pai):
    ops = _ops()
    D = 12289
    x, g = torch.zeros(D, device=dev()), torch.ones(D, device=dev())
    m = torch.zeros(1, device=dev())
    with pytest.raises(ops.PaiError, match="12288"):
        ops.layernorm_fwd(torch.float32, x, None, 1, D, g, g, EPS, None, 1, None, torch.empty_like(x), m, m.clone())
    with pytest.raises(ops.PaiError, match="12288"):
        ops.layernorm_bwd(torch.float32, x, x, 1, D, g, m, m, torch.empty_like(x))
    with pytest.raises(ops.PaiError, match="sum_out"):
        ops.layernorm_fwd(torch.float32, x[:8], x[8:16], 1, 8, g[:8], g[:8], EPS, None, 1, None, torch.empty(8, device=dev()),
                          m, m.clone())


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------
LNB_CASES = [(M, D) for M, D, _ in LN_CASES] + [(1030, 40), (100, 300)]


def _ln_bwd(M, D, dtype, with_params):
    ops = _ops()
    xs, dy = q(rnd((M, D), 21) * 1.5 + 0.2, dtype), q(rnd((M, D), 22), dtype)
    gamma = 1 + 0.1 * rnd((D,), 23)
    st = R.layernorm_fwd(xs, None, gamma, gamma, EPS, None, 1)
    mean, rstd = st["mean"].float(), st["rstd"].float()          # what the kernel is handed, and what its reference uses
    ref = R.layernorm_bwd(dy, xs, gamma, mean, rstd)
    slabs = ops.layernorm_partial_rows(M)
    assert slabs == min(64, max(1, (M + 15) // 16))
    dx = _poisoned(M * D, dtype)
    dgb, part = _poisoned(2 * D), _poisoned(slabs * 2 * D)
    if with_params:
        ops.layernorm_bwd(dtype, _d(dy, dtype), _d(xs, dtype), M, D, _d(gamma), _d(mean), _d(rstd), dx[:M * D], dgb[:2 * D],
                          part[:slabs * 2 * D])
    else:
        ops.layernorm_bwd(dtype, _d(dy, dtype), _d(xs, dtype), M, D, _d(gamma), _d(mean), _d(rstd), dx[:M * D])
    torch.cuda.synchronize()
    t = f"layernorm_bwd {_t(dtype)}"
    _elem_ok(_written(dx, M * D, "dx"), ref["dx"], dtype, f"{t} dx")
    if not with_params:
        assert bool(torch.isnan(dgb).all()) and bool(torch.isnan(part).all())
        return
    got = _written(dgb, 2 * D, "dgamma_dbeta").view(2, D)
    _sum_ok(got[0], ref["dbeta"], ref["dbeta_abs"], f"{t} dbeta")
    _sum_ok(got[1], ref["dgamma"], ref["dgamma_abs"], f"{t} dgamma")
    p = _written(part, slabs * 2 * D, "partials").view(slabs, 2, D)
    rps = (M + slabs - 1) // slabs
    used = (M + rps - 1) // rps
    if used < slabs:
        assert bool((p[used:] == 0).all()), "slabs that own no row must write zeros"
    _sum_ok(p.double().sum(0)[0], ref["dbeta"], ref["dbeta_abs"], f"{t} partials row 0")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,D", LNB_CASES, ids=lambda v: str(v))
def test_layernorm_bwd(pai, M, D, dtype):
    """(1030, 40): 64 slabs of 17 rows, the last three own no row -- the NaN-filled `partials` must not reach dgamma / dbeta.
    (100, 300): 7 slabs, two column blocks.  (2, 12288): the LDS limit, 48 column blocks."""
    if (M, D) == (1030, 40):
        assert _ops().layernorm_partial_rows(M) == 64 and 61 * 17 >= M
    _ln_bwd(M, D, dtype, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_bwd_without_parameter_gradients(pai, dtype):
    _ln_bwd(12, 96, dtype, False)


# ---- GELU ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _gelu_case(numel, dtype):
    z, dy = q(R.gelu_args(numel), dtype), q(R.gelu_dy(numel), dtype)
    return z, dy, R.gelu(z), R.gelu_bwd(dy, z)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("numel", R.GELU_NUMELS)
def test_gelu(pai, numel, dtype):
    """+-0, +-1e-4, +-4, +-10, +-40 and a dense sweep of [-6, 6]; the largest case wraps the 8192 x 256 grid-stride loop."""
    ops = _ops()
    z, dy, want, want_g = _gelu_case(numel, dtype)
    assert numel <= 8192 * 256 or numel == R.GELU_NUMELS[-1]
    out, dz = _poisoned(numel, dtype), _poisoned(numel, dtype)
    zd = _d(z, dtype)
    ops.gelu(dtype, zd, out[:numel])
    ops.gelu_bwd(dtype, _d(dy, dtype), zd, dz[:numel])
    torch.cuda.synchronize()
    got, got_g = _written(out, numel, "gelu"), _written(dz, numel, "gelu_bwd")
    if dtype == torch.float32:
        cap = 1e-6 * (1 + z.double().abs())
        _within(got, want, torch.clamp(cap, max=GELU_BOUND), "gelu f32")
        _within(got_g, want_g, dy.double().abs() * torch.clamp(cap, max=GELU_BWD_BOUND), "gelu_bwd f32")
    else:
        _within(got, want, _stored_lim(want), "gelu bf16")
        _within(got_g, want_g, _stored_lim(want_g), "gelu_bwd bf16")


# ---- attention core ----------------------------------------------------------------------------------------------------
MFMA_CASES = [(32, 3, 2, 32), (31, 2, 3, 96), (17, 2, 2, 160), (7, 3, 2, 64), (1, 2, 2, 32), (32, 1, 1, 512)]
VEC_ONLY_CASES = [(300, 1, 2, 24), (5, 2, 2, 320), (3, 1, 1, 1)]
VEC_BF16_EDGE = [(33, 2, 1, 32), (8, 2, 2, 48)]       # just outside the matrix-core conditions (S <= 32, hd % 32 == 0)
T_NAME = {torch.float32: "float", torch.bfloat16: "unsigned short"}


def _names(path, dtype):
    if path == "mfma":
        return "mha_fwd_mfma_k", "mha_bwd_mfma_k"
    t = T_NAME[dtype]
    return f"mha_fwd_k<{t}>", f"mha_bwd_q_k<{t}>+mha_bwd_kv_k<{t}>"


def _mask(S, B, heads, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.bernoulli(torch.full((B * heads, S, S), 0.7), generator=g) / 0.7


def _grad_lim(ref, absum, path, dtype, cancel=None):
    ref, absum = ref.double(), absum.double()
    if dtype == torch.float32:
        return 1e-5 * absum
    if path == "vec":
        return _stored_lim(ref) + 1e-5 * absum
    return 2.0 ** -8 * (absum + ref.abs()) + 1e-6 * float(ref.abs().max())


def _mha(qkv, dout, S, B, heads, hd, mask, dtype, path, backward=True, grad_lim=_grad_lim, out_lim=None, pin=None):
    """pai_mha_fwd, then pai_mha_bwd from the fp32 cast of the reference probs, on host inputs already rounded through dtype;
    path "mfma": the default selection must be the matrix-core kernels; "vec": the vector kernels (bf16: tunable mha_mfma = 0).
    pin = False: no tunable, the selection itself must pick that path.  Returns the references and what the kernels wrote."""
    ops = _ops()
    E = heads * hd
    n_p = B * heads * S * S
    pin = (path == "vec" and dtype == torch.bfloat16) if pin is None else pin
    out, probs = _poisoned(S * B * E, dtype), _poisoned(n_p)
    dqkv, ds = _poisoned(S * B * 3 * E, dtype), _poisoned(n_p)
    ref = R.mha_fwd(qkv, S, B, heads, hd, mask)
    p32 = ref["probs"].float()
    refb = R.mha_bwd(dout, qkv, p32, S, B, heads, hd, mask) if backward else None
    if pin:
        ops.set_tunable("mha_mfma", 0)
    try:
        assert (ops.mha_kernel_name(dtype, S, hd, 0), ops.mha_kernel_name(dtype, S, hd, 1)) == _names(path, dtype)
        qd, md = _d(qkv, dtype), _d(mask)
        ops.mha_fwd(dtype, qd, S, B, heads, hd, out[:S * B * E], probs[:n_p], md)
        if backward:
            ops.mha_bwd(dtype, _d(dout, dtype), qd, _d(p32), S, B, heads, hd, dqkv[:S * B * 3 * E], ds[:n_p], md)
        torch.cuda.synchronize()
    finally:
        if pin:
            ops.set_tunable("mha_mfma")
    tag = f"mha {path} {_t(dtype)} {(S, B, heads, hd)}{' mask' if mask is not None else ''}"
    got_p = _written(probs, n_p, "probs").view(B * heads, S, S)
    print(f"{tag}: e_s {ref['e_s']:.3g}, mass {ref['mass']:.3g}")
    _within(got_p, ref["probs"], ref["probs"] * (2 * ref["e_s"] + 1e-6) + 1e-9, f"{tag} probs")
    rowsum = float((got_p.double().sum(-1) - 1).abs().max())
    print(f"{tag} probs row sums: max |sum - 1| {rowsum:.3g}")
    assert rowsum <= 1e-5
    got_o = _written(out, S * B * E, "out").view(S * B, E)
    if out_lim is not None:
        lim = out_lim
    elif dtype == torch.float32:
        lim = 1e-4 * float(ref["out"].abs().max())
    elif path == "vec":
        lim = _stored_lim(ref["out"])
    else:
        lim = 2.0 ** -7 * ref["mass"] * ref["vmax"]
    _within(got_o, ref["out"], lim, f"{tag} out")
    got_g = None
    if backward:
        got_g = _written(dqkv, S * B * 3 * E, "dqkv").view(S * B, 3 * E)
        for k, name in enumerate(("dQ", "dK", "dV")):
            sl = slice(k * E, (k + 1) * E)
            _within(got_g[:, sl], refb["dqkv"][:, sl], grad_lim(refb["dqkv"][:, sl], refb["abs"][:, sl], path, dtype, refb["cancel"][:, sl]),
                    f"{tag} {name}")
        if path == "vec":
            _written(ds, n_p, "ds workspace")
        else:
            _guard_ok(ds, n_p, "ds workspace")
    return ref, refb, got_o, got_g


def _random_case(S, B, heads, hd, dtype, masked):
    E = heads * hd
    return (q(rnd((S * B, 3 * E), 9 + S + hd) * 0.7, dtype), q(rnd((S * B, E), 10 + S + hd), dtype),
            _mask(S, B, heads) if masked else None)


MASKED = pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])


@MASKED
@pytest.mark.parametrize("S,B,heads,hd", MFMA_CASES, ids=lambda v: str(v))
def test_mha_matrix_core_path(pai, S, B, heads, hd, masked):
    """mha_fwd_mfma_k / mha_bwd_mfma_k against fp64: a full tile, ragged S = 31 / 17 / 7 / 1 (zero fragments, -inf padding
    keys), hd = 32 (three of the four waves idle in every product) .. 512 (the limit), 0 / (1 / 0.7) dropout masks."""
    qkv, dout, mask = _random_case(S, B, heads, hd, torch.bfloat16, masked)
    _mha(qkv, dout, S, B, heads, hd, mask, torch.bfloat16, "mfma")


@MASKED
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S,B,heads,hd", MFMA_CASES + VEC_ONLY_CASES, ids=lambda v: str(v))
def test_mha_vector_path(pai, S, B, heads, hd, dtype, masked):
    """mha_fwd_k / mha_bwd_q_k / mha_bwd_kv_k: the matrix-core shapes in fp32 and (tunable mha_mfma = 0) in bf16, and
    S = 300 > 256 (the per-thread key loops run twice), hd = 320 > 256 (so do the per-thread channel loops), hd = 1."""
    qkv, dout, mask = _random_case(S, B, heads, hd, dtype, masked)
    _mha(qkv, dout, S, B, heads, hd, mask, dtype, "vec")


@MASKED
@pytest.mark.parametrize("S,B,heads,hd", VEC_BF16_EDGE, ids=lambda v: str(v))
def test_mha_bf16_shapes_just_outside_the_matrix_core_conditions(pai, S, B, heads, hd, masked):
    """bf16 S = 33 and hd = 48: the selection itself (no tunable) must leave the matrix cores."""
    qkv, dout, mask = _random_case(S, B, heads, hd, torch.bfloat16, masked)
    _mha(qkv, dout, S, B, heads, hd, mask, torch.bfloat16, "vec", pin=False)


def _dominant(S, B, heads, hd, jk, dtype, lift, absolute):
    """The construction of test_sattn_dominant_key: for query S // 2 of every (b, h), key jk scores `lift` above every other
    key (absolute: scores `lift`)."""
    E = heads * hd
    qkv = rnd((S * B, 3 * E), 77) * 0.7
    v = qkv.view(S, B, 3, heads, hd)
    iq = S // 2
    for b in range(B):
        for h in range(heads):
            qv = v[iq, b, 0, h]
            others = (v[:, b, 1, h] @ qv) / math.sqrt(hd)
            others[jk] = -1e30
            target = lift if absolute else float(others.max()) + lift
            v[jk, b, 1, h] = qv * (target * math.sqrt(hd) / float(qv @ qv))
    return q(qkv, dtype), q(rnd((S * B, E), 78), dtype), iq


DOMINANT = [(7, 6), (32, 0), (32, 31)]


def _grad_lim_fp32_cancel(S, hd):
    """The fp32 gradient bound with the term its derivation misses when a key dominates a row: 1e-5 A + u (hd + S + 2) C,
    C = ``cancel`` of _vit_ref.mha_bwd."""
    def lim(ref, absum, path, dtype, cancel):
        assert dtype == torch.float32
        return 1e-5 * absum.double() + 2.0 ** -24 * (hd + S + 2) * cancel.double()
    return lim


@pytest.mark.parametrize("path,dtype", [("mfma", torch.bfloat16), ("vec", torch.bfloat16), ("vec", torch.float32)],
                         ids=["mfma", "vec-bf16", "vec-f32"])
@pytest.mark.parametrize("S,jk", DOMINANT, ids=lambda v: str(v))
def test_mha_dominant_key(pai, S, jk, path, dtype):
    """One key, the last of a ragged tile (S = 7, next to the -inf padding keys) or the first / last of a full one, scores 30
    above the rest for one query row of every (b, h).  Forward and backward, on both bf16 paths and in fp32.

    fp32 backward: the purely relative bound 1e-5 A of the other fp32 cases has no term for the cancellation in
    dS_ij = P_ij (dP_ij - dl_i), dl_i = sum_j P_ij dP_ij.  Where one key carries (nearly) all of a row's mass, dP_ij - dl_i is
    a small difference of two fp32 numbers of size |dP|: in the dominated row the true dS of the dominant key is e^-30 |dP|
    = 1e-13, below the fp32 resolution 6e-8 |dl| of dl (the kernel's value is exactly 0), and A collapses with it; rows in
    which the heavy key holds 0.9 .. 0.999 of the mass lose the same absolute amount against a dS of 1e-1 .. 1e-3 |dP|.  The
    rounding the derivation missed is that of dP and dl BEFORE the subtraction, so the bound here carries it a priori, in the
    style of e_s: an fp32 dot product of hd terms and a sum of S terms in any order are off by at most u (hd + S + 2) times
    their absolute terms Abar_ij = sum_d |dO_id v_jd|, hence |err dS_ij| <= u (hd + S + 2) P_ij (Abar_ij + sum_j' P_ij'
    Abar_ij') = u (hd + S + 2) C_ij, carried through the dQ / dK products like A.  dV has no such term.  The largest
    error / (1e-5 A) without it is printed too (an fp32 emulation of the formulas on the host: 1e5 in the dominated row, up
    to 6 in others); the bf16 bounds absorb the effect in their 2^-8 and 1e-6 max |ref| terms and stay as they are."""
    B, heads, hd = 2, 2, 64
    E = heads * hd
    qkv, dout, iq = _dominant(S, B, heads, hd, jk, dtype, 30.0, False)
    f32 = dtype == torch.float32
    ref, refb, _, got_g = _mha(qkv, dout, S, B, heads, hd, None, dtype, path,
                               grad_lim=_grad_lim_fp32_cancel(S, hd) if f32 else _grad_lim)
    p = ref["probs"].view(B, heads, S, S)
    assert float(p[:, :, iq, jk].min()) > 1 - 1e-9, "the construction holds after rounding"
    if f32:
        err = (got_g.double() - refb["dqkv"]).abs()
        plain = err / (1e-5 * refb["abs"]).clamp_min(1e-300)
        rows = torch.arange(S * B) // B == iq
        for k, name in enumerate(("dQ", "dK", "dV")):
            sl = slice(k * E, (k + 1) * E)
            print(f"mha vec f32 dominant {(S, jk)} {name}: max err / (1e-5 A) {float(plain[:, sl][~rows].max()):.3g} outside "
                  f"the dominated query rows, {float(plain[:, sl][rows].max()):.3g} in them")
        # dV, and dK outside nothing: these hold the plain bound of every other fp32 case
        assert bool((err[:, 2 * E:] <= 1e-5 * refb["abs"][:, 2 * E:]).all())


@pytest.mark.parametrize("path,dtype", [("mfma", torch.bfloat16), ("vec", torch.bfloat16), ("vec", torch.float32)],
                         ids=["mfma", "vec-bf16", "vec-f32"])
@pytest.mark.parametrize("S,jk", [(7, 6), (32, 0)], ids=lambda v: str(v))
def test_mha_large_score(pai, S, jk, path, dtype):
    """The same construction with the dominant score at 100 instead of 30 above the rest: expf(100) overflows fp32, so a
    softmax without the max-subtraction returns NaN here (with a score of 30 + max it would still pass).  Forward only."""
    B, heads, hd = 2, 2, 64
    qkv, dout, iq = _dominant(S, B, heads, hd, jk, dtype, 100.0, True)
    sc = torch.einsum("bhid,bhjd->bhij", *R.split_qkv(qkv, S, B, heads, hd)[:2]) / math.sqrt(hd)
    assert float(sc[:, :, iq, jk].min()) > 95
    _mha(qkv, dout, S, B, heads, hd, None, dtype, path, backward=False)


def _lane_map_data(S, B, heads, hd, paired):
    """Small-integer q, k, v, dO, every value and every intermediate of the six products exact in bf16 / fp32.
    Key j carries 16 on channel c(j), query i carries 16 on the channel of key sigma(i) = (7 i + 2) % S, so the matching score
    is 256 / sqrt(hd) >= 32 above the others.  onehot: c(j) = (5 j + 3) % hd, all different -- each query copies ONE row of the
    asymmetric v = d + 2 j + (b heads + h), dV_j is ONE row of the asymmetric dO; dS vanishes.  paired: keys 2 m and 2 m + 1 share
    c = (5 m + 3) % hd and differ in a channel no query looks at (16, 32 or 48 there), so P = 1/2, 1/2 and
    dS = -+ 1/2 sum_d dO_id for the pair: dQ = dS K and dK = dS^T Q are whole numbers times 16 scale / 2."""
    sigma = lambda i: (7 * i + 2) % S
    cj = (lambda j: (5 * (j // 2) + 3) % hd) if paired else (lambda j: (5 * j + 3) % hd)
    used = {cj(j) for j in range(S)}
    free = [c for c in range(hd) if c not in used]
    assert len(used) == (S // 2 if paired else S) and (not paired or (S % 2 == 0 and len(free) >= S))
    Q, K, V, dO = (torch.zeros(B, heads, S, hd) for _ in range(4))
    d = torch.arange(hd, dtype=torch.float32)
    for b in range(B):
        for h in range(heads):
            for i in range(S):
                Q[b, h, i, cj(sigma(i))] = 16.0
                K[b, h, i, cj(i)] = 16.0
                if paired:
                    K[b, h, i, free[i]] = 16.0 * (i % 3 + 1)
                V[b, h, i] = d + 2 * i + (b * heads + h)
                dO[b, h, i] = ((2 * i + 3 * d + b + 2 * h) % 7) - 3
                dO[b, h, i, i % hd] += (i % 4) + 1
    qkv = torch.cat([R._rows(t, S, B, heads, hd) for t in (Q, K, V)], dim=1)
    return qkv, R._rows(dO, S, B, heads, hd)


@pytest.mark.parametrize("S,B,heads,hd", [(32, 2, 2, 64), (20, 1, 1, 32)], ids=lambda v: str(v))
@pytest.mark.parametrize("paired", [False, True], ids=["onehot", "paired"])
def test_mha_lane_maps(pai, paired, S, B, heads, hd):
    """The construction of test_sattn_lane_maps_with_integer_data for the six MFMA products of the matrix-core path (K Q^T,
    P V, dO V^T, dS K, dS^T Q, P^T dO): exact answers, a swapped row / column of any fragment is off by 0.5 or more."""
    E = heads * hd
    qkv, dout = _lane_map_data(S, B, heads, hd, paired)
    assert torch.equal(q(qkv, torch.bfloat16), qkv) and torch.equal(q(dout, torch.bfloat16), dout)
    exact = lambda ref, absum, path, dtype, cancel: 2.0 ** -8 * ref.double().abs() + 0.01
    ref, refb, got_o, got_g = _mha(qkv, dout, S, B, heads, hd, None, torch.bfloat16, "mfma", grad_lim=exact, out_lim=0.01)
    # the construction has teeth: whole (half) numbers, different in every row and column
    o = ref["out"]
    assert float((o - o.round()).abs().max()) < 1e-6 and float(o.max()) < 256
    p = ref["probs"]
    assert float((p.max(-1).values - (0.5 if paired else 1.0)).abs().max()) < 1e-9
    g = refb["dqkv"]
    assert float(g[:, 2 * E:].abs().max()) >= 1
    if paired:
        assert float(g[:, :E].abs().max()) >= 1 and float(g[:, E:2 * E].abs().max()) >= 1
        assert int((g[:, :E].abs().sum(1) > 0.5).sum()) >= S * B // 2      # most query rows carry a non-zero dS


def test_mha_refuses_rows_beyond_its_lds(pai):
    """mha_check precedes any launch: tiny tensors suffice."""
    ops = _ops()
    t = torch.zeros(64, device=dev())
    with pytest.raises(ops.PaiError, match="64 KB"):
        ops.mha_fwd(torch.float32, t, 8192, 1, 1, 64, t, t)
    with pytest.raises(ops.PaiError, match="64 KB"):
        ops.mha_bwd(torch.float32, t, t, t, 8192, 1, 1, 64, t, t)
    with pytest.raises(ops.PaiError, match="64 KB"):
        ops.mha_kernel_name(torch.float32, 8192, 64, 0)
    with pytest.raises(ops.PaiError, match="op 2"):
        ops.mha_kernel_name(torch.float32, 8, 64, 2)


# ---- subsample2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,H,W,C", [(1, 2, 2, 1), (3, 6, 10, 3), (2, 12, 20, 24), (2, 128, 130, 66)], ids=lambda v: str(v))
def test_subsample2(pai, N, H, W, C, dtype):
    """Bit-exact copies; the adjoint zero-fills a NaN-filled dx, and at (2, 128, 130, 66) it wraps the 8192 x 256 grid."""
    ops = _ops()
    if H == 128:
        assert N * H * W * C > 8192 * 256
    x = rnd((N, H, W, C), 31).to(dtype)
    dout = rnd((N, H // 2, W // 2, C), 32).to(dtype)
    n_out, n_in = dout.numel(), x.numel()
    out, dx = _poisoned(n_out, dtype), _poisoned(n_in, dtype)
    ops.subsample2(dtype, x.to(dev()), N, H, W, C, out[:n_out])
    ops.subsample2_bwd(dtype, dout.to(dev()), N, H, W, C, dx[:n_in])
    torch.cuda.synchronize()
    _guard_ok(out, n_out, "out")
    _guard_ok(dx, n_in, "dx")
    assert torch.equal(out[:n_out].cpu().view(N, H // 2, W // 2, C), R.subsample2(x))
    assert torch.equal(dx[:n_in].cpu().view(N, H, W, C), R.subsample2_bwd(dout, H, W))


@pytest.mark.parametrize("H,W", [(3, 4), (4, 5)])
def test_subsample2_refuses_odd_sizes(pai, H, W):
    ops = _ops()
    t = torch.zeros(64, device=dev())
    with pytest.raises(ops.PaiError, match="even"):
        ops.subsample2(torch.float32, t, 1, H, W, 1, t.clone())
    with pytest.raises(ops.PaiError, match="even"):
        ops.subsample2_bwd(torch.float32, t, 1, H, W, 1, t.clone())


# ---- bn_stats -------------------------------------------------------------------------------------------------------------
BN_CASES = [(1, 1), (1, 300), (63, 3), (63, 513), (64, 24), (64, 256), (65, 3), (65, 300), (1000, 1), (1000, 24), (1000, 256),
            (1000, 513), (262144 + 77, 2)]


def _bn_stats(M, C, dtype, seed=41):
    """One pai_bn_stats call, every slab row against fp64; returns (host partial rows, z)."""
    ops = _ops()
    z = q(rnd((M, C), seed) * 1.5 + 0.7, dtype)
    rows = ops.bn_stats_rows(M)
    rps = 64 if M <= 64 * 4096 else 128
    assert rows == (M + rps - 1) // rps
    total = ops.bn_stats_buffer_rows(rows) * 2 * C
    assert total >= rows * 2 * C
    buf = _poisoned(total)
    ops.bn_stats(dtype, _d(z, dtype), M, C, buf[:total])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[rows * 2 * C:]).all()), "rows beyond bn_stats_rows(M) (and the guard) stay untouched"
    got = _written(buf[:rows * 2 * C + GUARD], rows * 2 * C, "stats").view(rows, 2, C)
    ref = R.bn_stats(z, rps)
    _sum_ok(got, ref["stats"], ref["abs"], f"bn_stats {_t(dtype)} {(M, C)}")
    return got, z


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,C", BN_CASES, ids=lambda v: str(v))
def test_bn_stats(pai, M, C, dtype):
    """C = 1 .. 3 (64 row lanes and more), 24, 256 (one lane), 300 and 513 (a second / third column chunk of 44 / 1 columns with
    its own lane count); M = 1, one row short of / exactly / one row over a slab, 16 slabs; 262221 rows: rows_per_slab doubles
    to 128, 2049 slabs."""
    if M > 262144:
        assert _ops().bn_stats_rows(M) == 2049
    _bn_stats(M, C, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_stats_into_bn_finalize(pai, dtype):
    """The partial rows as pai_bn_finalize consumes them: mean / rstd against fp64 of the STORED rows (checked against the data
    by _bn_stats) at the rtol = 1e-6 of tests/test_gpu_ops.py::test_bn_finalize_many_partial_rows."""
    ops = _ops()
    M, C = 1000, 24
    got, _ = _bn_stats(M, C, dtype, seed=43)
    rows = got.shape[0]
    stats = torch.zeros(ops.bn_stats_buffer_rows(rows) * 2 * C, device=dev())
    stats[:rows * 2 * C] = got.reshape(-1).to(dev())
    mean, rstd, scale, shift = (_poisoned(C) for _ in range(4))
    ops.bn_finalize(stats, rows, C, M, None, None, 1e-5, 0.1, 1, None, None, None, mean[:C], rstd[:C], scale[:C], shift[:C])
    torch.cuda.synchronize()
    s = got.double().sum(0).numpy()
    m = s[0] / M
    v = s[1] / M - m * m
    np.testing.assert_allclose(_written(mean, C, "mean").numpy(), m, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(_written(rstd, C, "rstd").numpy(), 1 / np.sqrt(v + 1e-5), rtol=1e-6)
    _written(scale, C, "scale"), _written(shift, C, "shift")


# ---- colsum, reduce_rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,C", [(1, 1), (32, 16384), (32, 20000), (257, 24), (1000, 300), (512 * 256 + 5, 3)],
                         ids=lambda v: str(v))
def test_colsum(pai, rows, C, dtype):
    """out += column sums: out starts from 1e-3 (small against the increments, so that the rounding of start + increment stays
    inside the sum bound) and the increment is compared.  C = 16384: exactly 64 column chunks; 20000: 79, the chunk loop
    strides; 257 rows: two row blocks meet through atomics; 131077 rows: 511 blocks of 257 rows."""
    ops = _ops()
    x = q(rnd((rows, C), 51) + 0.3, dtype)
    out = torch.cat([torch.full((C,), 1e-3, device=dev()), _poisoned(0)])
    ops.colsum(dtype, _d(x, dtype), rows, C, out[:C])
    torch.cuda.synchronize()
    got = _written(out, C, "out")
    ref = R.colsum(x)
    _sum_ok(got.double() - float(np.float32(1e-3)), ref["sum"], ref["abs"], f"colsum {_t(dtype)} {(rows, C)} increment")


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("rows", [1, 64])
@pytest.mark.parametrize("C", [1, 63, 130])
def test_reduce_rows(pai, C, rows, accumulate):
    ops = _ops()
    part = rnd((rows, C), 61) + 0.2
    out0 = rnd((C,), 62)
    out = _poisoned(C)
    if accumulate:
        out[:C] = out0.to(dev())
    ops.reduce_rows(_d(part), rows, C, out[:C], bool(accumulate))
    torch.cuda.synchronize()
    ref, ab = part.double().sum(0), part.double().abs().sum(0)
    if accumulate:
        ref, ab = ref + out0.double(), ab + out0.double().abs()
    _sum_ok(_written(out, C, "out"), ref, ab, f"reduce_rows {(rows, C)}")
