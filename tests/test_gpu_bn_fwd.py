"""GPU: the BatchNorm forward chain of csrc/bn.hip -- pai_bn_finalize (three reduction regimes: at most 16 partial rows, at
most 2048, more), pai_bn_eval_coeffs, pai_bn_apply and pai_bn2_add_act in their generic kernels -- element by element against
the fp64 host references of tests/_bn_ref.py (tied to PyTorch's double-precision F.batch_norm / relu / leaky_relu by
tests/test_bn_refs_host.py), and what a NaN does in the element-wise passes (pai_bn_apply, pai_bn2_add_act, pai_add_act,
generic and streaming, and the training-mode chain pai_bn_stats -> pai_bn_finalize -> pai_bn_apply).

Conventions (those of tests/test_gpu_step_ops.py): every reference starts from exactly what the kernel is handed -- finalize
from the fp32 partial rows as given, apply and the residual tail from the fp32 scale / shift arrays and the bf16-rounded
tensors -- and from the kernel's own fp32 constants (eps, momentum, 1.f - momentum formed in fp32).  Every output buffer is NaN
before the call and has 64 NaN guard elements behind it that must still be NaN afterwards (the counter: an int64 buffer of
-1); scale / shift and the partial rows carry guards too; inputs must be unchanged after the call; the generic kernels are
reached with the tunable ew_stream = 0; every tunable is restored in ``finally``; -s prints the largest error and the largest
error / bound per output.  The scratch rows behind the partial rows (pai_bn_stats_buffer_rows(R) - R) are NaN before the
call: the chunk kernel of the third regime must overwrite what the wide kernel then reads, and nothing stale is read.

Bounds -- none fitted to what a kernel produced (u = 2^-24):
  bf16 stored outputs   |got - ref| <= 2^-8 |ref| + 1e-6 max |ref|   (the project's bar, tests/test_gpu_step_ops.py)
  fp32 pai_bn_apply     one fma (error <= u |pre| <= u (|z scale| + |shift|), which is what is left where the fma cancels)
                        and at most one product (LeakyReLU: u |ref|):  2 u |ref| + u (|z scale| + |shift|)
  fp32 pai_bn2_add_act  fma, fma, add and up to two LeakyReLU products: the first branch carries u Ta from its fma and u |x|
                        <= u Ta from its product (Ta = |za sa| + |ha|), the second u Tb (Tb = |zb sb| + |hb|; identity skip: no
                        rounding), the sum u |x + y| and the outer product u |ref|; the outer activation scales what is before
                        it by at most 1 (0.2 where the sum is negative, where |x + y| = 5 |ref|):
                        2 u |ref| + 2 u Ta + u Tb
  fp32 pai_add_act      one add and at most one product: 2 u |ref|
  pai_bn_finalize       the sums are fp64 (any order: every regime adds at most 64 terms in sequence per lane, so the
                        reordering error is below 64 x 2^-53 relative to the absolute terms; the host asserts
                        (Q / count) / (var + eps) < 1e6 and sum |S_r| / |S| < 8e4, which keeps that term below 0.12 u of
                        rstd and 0.01 u of mean), everything after is a count of fp32 roundings, in absolute-term form
                        with a factor 2 over the count:
      mean     fp64, rounded once: u |ref|                                   bar 2 u |ref|
      rstd     fp64, rounded once: u |ref|                                   bar 2 u |ref|
      scale    one more product: 2 u |ref|                                   bar 4 u |ref|
      shift    beta - fl(fl(mean) scale): fl(mean), the product and the subtraction are 3 u (|beta| + |mean scale|), which
               the bar of 6 u (|beta| + |mean scale|) doubles; scale brings its own two roundings along, so the full count
               is 5 (4 with the multiply-add contracted; the host emulation reaches 3.1): the bar holds with less to spare
      running statistics after n updates: 1.5 u per update                   bar 3 n u (|r0| + |stat|); n = 0: the same bits
      counter  exact
                        The 1e-5 bars of tests/test_gpu_ops.py are about 170 u: they hide a missing count / (count - 1) at
                        count 4096 (momentum / 4095 = 2.4e-5 of var, 410 u) and a momentum applied once too few only by
                        luck of the tested counts.  tests/test_bn_refs_host.py runs an fp32 emulation of bn_finalize_k
                        (another summation order, every rounding, multiply-adds contracted and not) inside the derived
                        counts: measured 0.98 (mean), 0.97 (rstd), 1.73 (scale), 3.11 (shift), 1.28 / 2.56 / 2.43 (running
                        mean, n = 1 / 2 / 3) and 1.31 / 2.12 / 2.81 (running variance) u x terms.
  pai_bn_eval_coeffs    all fp32 -- add, sqrt, divide, product: 8 u |scale|; shift: 8 u (|beta| + |running_mean scale|)

Maxima measured on an MI355X (pytest -s; largest error / bound over all cases of a test; every bound held):
  pai_bn_finalize (96 cases, first and second call alike)   mean 0.49, rstd 0.49, scale 0.43, shift 0.48, running mean 0.25, running
                            variance 0.26 of their bars (0.49 of 2 u |ref| is one correctly rounded result: 0.98 u); counter exact
  pai_bn_eval_coeffs        scale 0.25, shift 0.24 of 8 u
  pai_bn_apply              f32 0.33 (9.1e-7 absolute at 349600 x 24), in place the same; bf16 0.994 (6.2e-2)
  pai_bn2_add_act           f32 0.63 (1.7e-6), bf16 0.994
  NaN cases                 bn_apply f32 0.33 / bf16 0.989 (generic and streaming), bn2_add_act f32 0.64 / bf16 0.995, add_act f32 0.875 /
                            bf16 0.996; NaN at exactly the expected positions, -inf under ReLU 0
  training chain            mean 0.45, rstd 0.36, scale 0.29, shift 0.26, running statistics 0.15 of their bars; out f32 0.32, bf16 0.98
The ratios near 1 are bf16 stored outputs (2^-8 |ref| IS half an ulp just above a power of two).

Not covered, on purpose (include/pai_hip.h says the same at pai_bn_apply): the on-load ReLU of the input prologue
(fmaxf(..., plo) in gg_pw.hip, gg_mfma.hip, gg_group.hip: it sits in matrix-kernel operand loads, where an extra instruction
per element has a cost nobody has measured), the fmaxf ReLU of gg_simt.hip and gate.hip, and the backward sign tests
act_grad / actg: these still turn a NaN into 0.  The fused launch bn_fin_apply_k is held bit-identical to the two-launch form
by tests/test_gpu_finish.py, which also carries its NaN case; the streaming kernels are held to the generic ones checked here
by tests/test_gpu_ew_stream.py, at one and at many sweep trips.  Partial overlap of out and z is not allowed by the header and
not tested; out == z is.  A NaN in the second trip of the generic add_act_k (its grid cap is 8192 blocks: 2,097,152 vectors)
is not reached either: the generic tensor of the NaN cases is one trip for it, the streaming form makes 22.

Which case fails which fault.  [m]: a one-line mutation of the kernel in a scratch copy, built and run once on an MI355X
against the cases named; [p]: the case also fails with the library built from the parent commit's sources.
  [m] `var` for `unbiased` in the running update (all three copies of the loop)
                                        test_bn_finalize: every case with running statistics and count <= 295040 (44; the two with
                                        count 262272 / 4194944 on one channel resp. nine pass: momentum / count is below the bar
                                        there), e.g. [16x9x4096-*], [32773x130x4096-*]; the training chain, both dtypes
  [m] the update loop run n_updates - 1 times   test_bn_finalize: all 72 cases with running statistics (n = 1, 2 and the second
                                        calls, n = 3 behind n = 0); the training chain
  [m] `*nbt += 1` for `+= n_updates`    test_bn_finalize: all 55 cases with a counter and n != 1 (n = 2 on 2^33 + 5, n = 3 without
                                        running statistics, n = 0 and the n = 3 behind it)
  [m] the 8 x 128 unrolled loop of bn_finalize_wide_k adds seven of its eight rows
                                        test_bn_finalize[1023x* / 1024x* / 1025x* / 2048x130x* / 2048x1x*], all four variants (20):
                                        exactly the row counts that enter the unrolled loop (the chunked regime hands it 228-257 rows)
  [m] no `var < 0` clamp                test_bn_finalize: 36 cases with constant channels (rstd off by 5e-5 relative where var comes out
                                        at -1e-9 against eps = 1e-5): 20 of [*-constant-n0-then-n3], in every regime, and 16 of
                                        [*-plain-n2-bigcounter] (every third channel constant), wherever a variance came out negative
  [m] `(i * 4) % C` for `(i * 8) % C` in bn_apply_k (the over-read of scale / shift lands in their guards)
                                        test_bn_apply_generic (all but [1x8-*]: one vector), test_bn_apply_past_the_grid_cap,
                                        test_nan_stays_nan[bn_apply-generic-*], the training chain
  [m] a sweep step of gridDim.x * 256 for gridDim.x * 256 * SV in bn_apply_stream_k: every vector is written up to four
      times with the same value, so no out-of-place comparison can see it (all of tests/test_gpu_ew_stream.py's passed, the
      many-trip ones included); tests/test_gpu_ew_stream.py::test_bn_apply_in_place_streaming[default_grid / 3_blocks] does:
      in place the second visit applies the BatchNorm to its own output
  [m][p] the old `v > 0.f ? v : 0.f` (the parent commit's library: it differs by this compare in act_apply and actc, the dtype
      checks and the version number)   test_nan_stays_nan, all nine; the training chain, both dtypes;
                                        tests/test_gpu_finish.py::test_nan_channel_stays_nan_through_conv_bn_relu, both
  [p] dtype codes other than PAI_F32 / PAI_BF16 run as bf16   test_refusals
  With the parent commit's library these 14 cases fail and no other case of this file, tests/test_gpu_ew_stream.py and
  tests/test_gpu_finish.py does.
  a write past an output, a written input   the guards and input comparisons of every test (not mutated)
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import _bn_ref as B
from _gpu_util import dev, rnd

pytestmark = pytest.mark.gpu

GUARD = 64
NAN, INF = float("nan"), float("inf")
U = B.U
EPS, MOM = 1e-5, 0.1
DTYPES = [torch.float32, torch.bfloat16]
ACTS = [B.ACT_NONE, B.ACT_RELU, B.ACT_LRELU]
ACT_NAME = {B.ACT_NONE: "none", B.ACT_RELU: "relu", B.ACT_LRELU: "lrelu"}


def _ops():
    from thesis_pai_reconstruction_amd import ops
    return ops


def _tn(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


# ---- device helpers ----------------------------------------------------------------------------------------------------------
def _poisoned(n, dtype=torch.float32):
    return torch.full((n + GUARD,), NAN, dtype=dtype, device=dev())


def _guarded(t, dtype=torch.float32, extra=0):
    """The host tensor on the device with ``extra`` + GUARD NaN elements behind it: (whole buffer, view of the n elements)."""
    n = t.numel()
    full = torch.full((n + extra + GUARD,), NAN, dtype=dtype, device=dev())
    full[:n] = t.reshape(-1).to(dtype).to(dev())
    return full, full[:n]


def _same(a, b):
    """Equal bit patterns (NaN payloads included: nothing here may rewrite an input)."""
    iv = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and bool((a.contiguous().view(iv) == b.contiguous().view(iv)).all())


def _guard_ok(full, n, what):
    assert bool(torch.isnan(full[n:]).all()), f"{what}: wrote outside its {n} elements"


def _unchanged(full, n, host, what):
    _guard_ok(full, n, what)
    assert _same(full[:n].cpu(), host.reshape(-1).to(full.dtype)), f"{what}: an input was written"


def _within(got, ref, lim, what):
    """NaN exactly where the reference is NaN, the same infinity where it is infinite, |got - ref| <= lim elsewhere; prints
    the largest error and the largest error / bound.  Returns that ratio."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    lim = lim.double().reshape(-1) if torch.is_tensor(lim) else torch.full_like(ref, float(lim))
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), (what, "NaN positions differ", int(torch.isnan(got).sum()), int(nan.sum()))
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), (what, "infinities differ")
    ok = ~(nan | inf)
    err = (got[ok] - ref[ok]).abs()
    ratio = float((err / lim[ok].clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max err {float(err.max()) if err.numel() else 0.0:.3g}, max err / bound {ratio:.3g}")
    bad = err > lim[ok]
    assert not bool(bad.any()), (what, int(bad.sum()), float((err - lim[ok]).max()))
    return ratio


def _finite_max(ref):
    r = ref.double().abs()
    r = r[torch.isfinite(r)]
    return float(r.max()) if r.numel() else 0.0


def _stored_lim(ref):
    return 2.0 ** -8 * torch.nan_to_num(ref.double().abs(), nan=0.0, posinf=0.0) + 1e-6 * _finite_max(ref)


def _apply_lim(r, dtype):
    return 2 * U * torch.nan_to_num(r["out"].abs(), nan=0.0, posinf=0.0) + U * torch.nan_to_num(r["terms"], nan=0.0, posinf=0.0) \
        if dtype == torch.float32 else _stored_lim(r["out"])


def _bn2_lim(r, dtype):
    c = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0)
    return 2 * U * c(r["out"].abs()) + 2 * U * c(r["terms_a"]) + U * c(r["terms_b"]) if dtype == torch.float32 else _stored_lim(r["out"])


def _add_lim(ref, dtype):
    return 2 * U * torch.nan_to_num(ref.abs(), nan=0.0, posinf=0.0) if dtype == torch.float32 else _stored_lim(ref)


class _tunables:
    """Set tunables for a block, back to their defaults afterwards."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            _ops().set_tunable(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            _ops().set_tunable(k)
        return False


# ---- pai_bn_finalize -----------------------------------------------------------------------------------------------------------
# (R, C, count): every regime (<= 16 rows: bn_finalize_k; <= 2048: bn_finalize_wide_k, whose 8 x 128-row unrolled stride
# starts at 1024 rows, tail behind it; more: 256 chunk sums first -- 2049 rows: per = 9, 228 chunks used) meets C = 1, a C that is
# no multiple of 8 and a C above 64; counts 2, 3, 64, 4096 and R x 128.
FIN_CASES = [
    (1, 1, 2), (1, 130, 128), (3, 7, 3), (3, 65, 64), (16, 9, 4096), (16, 512, 16 * 128), (16, 1, 64),
    (17, 1, 4096), (17, 65, 17 * 128), (127, 7, 64), (128, 130, 128 * 128), (129, 8, 3), (1023, 9, 4096), (1024, 64, 1024 * 128),
    (1025, 65, 2), (2048, 130, 2048 * 128), (2048, 1, 4096),
    (2049, 1, 2049 * 128), (2049, 65, 4096), (2305, 7, 64), (2305, 512, 2305 * 128), (32768 + 5, 9, (32768 + 5) * 128),
    (32768 + 5, 130, 4096), (32768 + 5, 1, 3),
]
# variant: (data kind, gamma / beta, running statistics, counter: preset | None, n_updates, second call)
FIN_VARIANTS = {
    "affine-n1-twice": ("normal", True, True, 0, 1, True),
    "plain-n2-bigcounter": ("mixed", False, True, 2 ** 33 + 5, 2, False),
    "norunning-n3": ("offset", True, False, None, 3, False),
    "constant-n0-then-n3": ("constant", True, True, 7, 0, True),
}


@lru_cache(maxsize=4)
def _partials(R, C, count, kind):
    return B.make_partials(R, C, count, 7 * R + C, kind)


def _fin_check(got, ref, n, what, worst):
    lim = B.finalize_bounds(ref, n)
    for k, g in got.items():
        if k in ("rm", "rv") and n == 0:
            continue
        worst[k] = max(worst.get(k, 0.0), _within(g, ref[k], lim[k], f"{what} {k}"))


@pytest.mark.parametrize("variant", list(FIN_VARIANTS))
@pytest.mark.parametrize("case", FIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bn_finalize(pai, case, variant):
    ops = _ops()
    R, C, count = case
    kind, affine, running, nbt0, n, twice = FIN_VARIANTS[variant]
    if variant == "norunning-n3" and (R + C) % 2:
        nbt0 = 11                                       # no running statistics but a counter: it still advances
    p = _partials(R, C, count, kind)
    gamma, beta = (1 + 0.25 * rnd((C,), 3), 0.5 * rnd((C,), 4)) if affine else (None, None)
    rm0, rv0 = (0.3 * rnd((C,), 5), 0.5 + rnd((C,), 6).abs()) if running else (None, None)
    ref = B.finalize(p, count, gamma, beta, EPS, MOM, n, rm0, rv0)
    what = f"finalize R {R} C {C} count {count} {variant}"
    assert float(ref["amplification"].max()) < 1e6, what
    cancel = p.double()[:, 0].abs().sum(0) / p.double()[:, 0].sum(0).abs().clamp_min(1e-300)
    assert float(cancel.max()) < 8e4, (what, "cancellation in the mean: the fp64 order would show")
    if kind == "constant" and C >= 64:
        raw = p.double()[:, 1].sum(0) / count - ref["mean"] ** 2
        assert bool((raw < 0).any()) and bool((raw > 0).any()), "the constant channels reach the clamp from both sides"

    rows = ops.bn_stats_buffer_rows(R)
    assert rows - R == (512 if R > 2048 else 128)
    stats, stats_v = _guarded(p, extra=(rows - R) * 2 * C)              # the scratch rows: NaN
    dv = lambda t: (None, None) if t is None else _guarded(t)
    (G, Gv), (Bt, Btv), (RM, RMv), (RV, RVv) = dv(gamma), dv(beta), dv(rm0), dv(rv0)
    nbt = None if nbt0 is None else torch.full((1 + 8,), -1, dtype=torch.int64, device=dev())
    if nbt is not None:
        nbt[0] = nbt0
    outs = {k: _poisoned(C) for k in ("mean", "rstd", "scale", "shift")}

    def call(n_):
        ops.bn_finalize(stats, R, C, count, Gv, Btv, B.f32c(EPS), B.f32c(MOM), n_, RMv, RVv, None if nbt is None else nbt[:1],
                        outs["mean"][:C], outs["rstd"][:C], outs["scale"][:C], outs["shift"][:C])
        torch.cuda.synchronize()
        for k, o in outs.items():
            _guard_ok(o, C, f"{what} {k}")
        got = {k: o[:C].cpu() for k, o in outs.items()}
        if running:
            _guard_ok(RM, C, f"{what} rm")
            _guard_ok(RV, C, f"{what} rv")
            got.update(rm=RM[:C].cpu(), rv=RV[:C].cpu())
        assert _same(stats[:R * 2 * C].cpu(), p.reshape(-1)), f"{what}: the partial rows were written"
        _guard_ok(stats, rows * 2 * C, f"{what} partial rows")
        for full, host, nm in ((G, gamma, "gamma"), (Bt, beta, "beta")):
            if full is not None:
                _unchanged(full, C, host, f"{what} {nm}")
        return got

    worst = {}
    got = call(n)
    _fin_check(got, ref, n, what, worst)
    if running and n == 0:
        assert _same(got["rm"], rm0) and _same(got["rv"], rv0), f"{what}: n_updates = 0 moved the running statistics"
    count_now = None if nbt0 is None else nbt0 + n
    if nbt is not None:
        assert nbt.cpu().tolist() == [count_now] + [-1] * 8, (what, nbt.cpu().tolist())
    if twice:       # the same buffers again: the running statistics advance from what the first call stored, the counter again
        n2 = 3 if n == 0 else n
        for o in outs.values():
            o.fill_(NAN)
        ref2 = B.finalize(p, count, gamma, beta, EPS, MOM, n2, got["rm"], got["rv"])
        got2 = call(n2)
        _fin_check(got2, ref2, n2, what + " second call", worst)
        assert not _same(got2["rm"], got["rm"]) and not _same(got2["rv"], got["rv"])
        assert nbt.cpu().tolist() == [count_now + n2] + [-1] * 8, (what, nbt.cpu().tolist())


# ---- pai_bn_eval_coeffs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("C", [1, 7, 64, 65, 130])
def test_bn_eval_coeffs(pai, C, affine):
    """running_var of 0 and of 1e-12 in channels 0 and C // 2 (C = 1: 0 alone): eps is the whole denominator."""
    ops = _ops()
    gamma, beta = (1 + 0.25 * rnd((C,), 13), 0.5 * rnd((C,), 14)) if affine else (None, None)
    rm, rv = rnd((C,), 15), 0.1 + rnd((C,), 16).abs()
    rv[C // 2] = 1e-12
    rv[0] = 0.0
    ref = B.eval_coeffs(gamma, beta, rm, rv, EPS)
    dv = lambda t: (None, None) if t is None else _guarded(t)
    (G, Gv), (Bt, Btv), (RM, RMv), (RV, RVv) = dv(gamma), dv(beta), dv(rm), dv(rv)
    sc, sh = _poisoned(C), _poisoned(C)
    ops.bn_eval_coeffs(C, Gv, Btv, RMv, RVv, B.f32c(EPS), sc[:C], sh[:C])
    torch.cuda.synchronize()
    what = f"eval_coeffs C {C} {'affine' if affine else 'plain'}"
    _guard_ok(sc, C, what)
    _guard_ok(sh, C, what)
    _within(sc[:C].cpu(), ref["scale"], 8 * U * ref["scale"].abs(), f"{what} scale")
    _within(sh[:C].cpu(), ref["shift"], 8 * U * ref["shift_abs"], f"{what} shift")
    for full, host, nm in ((G, gamma, "gamma"), (Bt, beta, "beta"), (RM, rm, "rm"), (RV, rv, "rv")):
        if full is not None:
            _unchanged(full, C, host, f"{what} {nm}")


# ---- pai_bn_apply / pai_bn2_add_act, generic kernels -----------------------------------------------------------------------------
EW_SHAPES = [(1, 8), (5, 24), (129, 72), (4097, 64), (37, 2048)]
BIG = (349600, 24)            # 1,048,800 vectors: 224 in the second trip behind the 4096-block cap, the last block of it ragged


@lru_cache(maxsize=4)
def _ew_host(M, C, dtype, seed):
    """z, zb [M][C] rounded to the storage type, scale / shift of two BatchNorms.  Row 0: z = +0 in channel 0 and -0 in channel
    1 with shift +0 / -0 there, so the pre-activations are exactly +0 and -0."""
    z = (rnd((M, C), seed) * 1.5 + 0.3).to(dtype)
    zb = (rnd((M, C), seed + 1) * 1.2 - 0.2).to(dtype)
    sa, ha = 0.5 + rnd((C,), seed + 2).abs(), 0.4 * rnd((C,), seed + 3)
    sb, hb = -(0.5 + rnd((C,), seed + 4).abs()), 0.4 * rnd((C,), seed + 5)       # a negative scale too
    z[0, 0], z[0, 1] = 0.0, -0.0
    ha[0], ha[1] = 0.0, -0.0
    return z, zb, sa, ha, sb, hb


def _run_apply(ops, dtype, z, sc, sh, a, alias=False):
    M, C = z.shape
    n = M * C
    Z, Zv = _guarded(z, dtype)
    (S, Sv), (H, Hv) = _guarded(sc), _guarded(sh)
    out = Z if alias else _poisoned(n, dtype)
    ops.bn_apply(dtype, Zv, M, C, Sv, Hv, a, out[:n])
    torch.cuda.synchronize()
    _guard_ok(out, n, "bn_apply out")
    if not alias:
        _unchanged(Z, n, z, "bn_apply z")
    _unchanged(S, C, sc, "bn_apply scale")
    _unchanged(H, C, sh, "bn_apply shift")
    return out[:n].cpu().view(M, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
@pytest.mark.parametrize("shape", EW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bn_apply_generic(pai, shape, dtype):
    ops = _ops()
    M, C = shape
    z, _, sc, sh, _, _ = _ew_host(M, C, dtype, 20)
    with _tunables(ew_stream=0):
        for a in ACTS:
            r = B.apply(z, sc, sh, a)
            assert float(r["out"][0, 0]) == 0.0 and float(r["out"][0, 1]) == 0.0
            if M * C >= 64:
                assert bool((r["out"] < 0).any()) == (a != B.ACT_RELU)
            got = _run_apply(ops, dtype, z, sc, sh, a)
            _within(got, r["out"], _apply_lim(r, dtype), f"bn_apply {_tn(dtype)} {M}x{C} {ACT_NAME[a]}")
            assert float(got[0, 0]) == 0.0 and float(got[0, 1]) == 0.0
        # out == z: every vector is read before the same thread writes it (include/pai_hip.h allows exactly this overlap)
        r = B.apply(z, sc, sh, B.ACT_LRELU)
        got = _run_apply(ops, dtype, z, sc, sh, B.ACT_LRELU, alias=True)
        _within(got, r["out"], _apply_lim(r, dtype), f"bn_apply {_tn(dtype)} {M}x{C} in place")


@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
def test_bn_apply_past_the_grid_cap(pai, dtype):
    """1,048,800 vectors: bn_apply_k's 4096 blocks take a second trip of 224 vectors.  C / 8 = 3 is no power of two, so bf16 stays
    on the generic kernel with ew_stream = 1 as well: the same bits under both settings."""
    ops = _ops()
    M, C = BIG
    z, _, sc, sh, _, _ = _ew_host(M, C, dtype, 30)
    r = B.apply(z, sc, sh, B.ACT_LRELU)
    got = {}
    for stream in (0, 1):
        with _tunables(ew_stream=stream):
            got[stream] = _run_apply(ops, dtype, z, sc, sh, B.ACT_LRELU)
    _within(got[0], r["out"], _apply_lim(r, dtype), f"bn_apply {_tn(dtype)} {M}x{C} second trip")
    assert _same(got[0], got[1]), "C / 8 = 3 must stay on the generic kernel"


def _run_bn2(ops, dtype, za, sa, ha, zb, sb, hb, act_a, a):
    M, C = za.shape
    n = M * C
    (ZA, ZAv), (ZB, ZBv) = _guarded(za, dtype), _guarded(zb, dtype)
    dv = lambda t: (None, None) if t is None else _guarded(t)
    (SA, SAv), (HA, HAv), (SB, SBv), (HB, HBv) = dv(sa), dv(ha), dv(sb), dv(hb)
    out = _poisoned(n, dtype)
    ops.bn2_add_act(dtype, ZAv, SAv, HAv, ZBv, SBv, HBv, M, C, act_a, a, out[:n])
    torch.cuda.synchronize()
    _guard_ok(out, n, "bn2_add_act out")
    _unchanged(ZA, n, za, "bn2_add_act za")
    _unchanged(ZB, n, zb, "bn2_add_act zb")
    for full, host, nm in ((SA, sa, "scale_a"), (HA, ha, "shift_a"), (SB, sb, "scale_b"), (HB, hb, "shift_b")):
        if full is not None:
            _unchanged(full, C, host, f"bn2_add_act {nm}")
    return out[:n].cpu().view(M, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
@pytest.mark.parametrize("skip", ["identity_skip", "bn_skip"])
@pytest.mark.parametrize("shape", EW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bn2_add_act_generic(pai, shape, skip, dtype):
    """All nine (act_a, act) pairs of {none, ReLU, LeakyReLU}."""
    ops = _ops()
    M, C = shape
    za, zb, sa, ha, sb, hb = _ew_host(M, C, dtype, 40)
    if skip == "identity_skip":
        sb = hb = None
    worst = 0.0
    with _tunables(ew_stream=0):
        for act_a in ACTS:
            for a in ACTS:
                r = B.bn2_add_act(za, sa, ha, zb, sb, hb, act_a, a)
                got = _run_bn2(ops, dtype, za, sa, ha, zb, sb, hb, act_a, a)
                worst = max(worst, _within(got, r["out"], _bn2_lim(r, dtype),
                                           f"bn2_add_act {_tn(dtype)} {M}x{C} {skip} {ACT_NAME[act_a]}/{ACT_NAME[a]}"))
    print(f"bn2_add_act {_tn(dtype)} {M}x{C} {skip}: worst err / bound {worst:.3g}")


def test_bn2_add_act_past_the_grid_cap(pai):
    ops = _ops()
    M, C = BIG
    za, zb, sa, ha, sb, hb = _ew_host(M, C, torch.float32, 30)
    r = B.bn2_add_act(za, sa, ha, zb, sb, hb, B.ACT_RELU, B.ACT_LRELU)
    with _tunables(ew_stream=0):
        got = _run_bn2(ops, torch.float32, za, sa, ha, zb, sb, hb, B.ACT_RELU, B.ACT_LRELU)
    _within(got, r["out"], _bn2_lim(r, torch.float32), f"bn2_add_act f32 {M}x{C} second trip")


def test_refusals(pai):
    """A dtype other than PAI_F32 / PAI_BF16 (it ran as bf16), C % 8 != 0 and a lone scale_b are refused; nothing is written."""
    ops = _ops()
    from thesis_pai_reconstruction_amd import lib as L
    M, C = 4, 16
    z, zb, sa, ha, sb, hb = _ew_host(M, C, torch.float32, 50)
    (_, Z), (_, ZB), (_, SA), (_, HA), (_, SB), (_, HB) = (_guarded(t) for t in (z, zb, sa, ha, sb, hb))
    out = _poisoned(M * C)
    lib = L.load()
    for code in (L.U8, 3, -1):
        assert code not in (L.F32, L.BF16)
        assert lib.pai_bn_apply(code, Z.data_ptr(), M, C, SA.data_ptr(), HA.data_ptr(), B.ACT_RELU, out.data_ptr(), None) != 0
        assert "dtype" in lib.pai_last_error().decode()
        assert lib.pai_bn2_add_act(code, Z.data_ptr(), SA.data_ptr(), HA.data_ptr(), ZB.data_ptr(), None, None, M, C, B.ACT_RELU,
                                   B.ACT_RELU, out.data_ptr(), None) != 0
        assert "dtype" in lib.pai_last_error().decode()
    with pytest.raises(ops.PaiError, match="multiple of 8"):
        ops.bn_apply(torch.float32, Z, 16, 4, SA, HA, B.ACT_RELU, out[:M * C])
    with pytest.raises(ops.PaiError, match="multiple of 8"):
        ops.bn2_add_act(torch.float32, Z, SA, HA, ZB, None, None, 16, 4, B.ACT_RELU, B.ACT_RELU, out[:M * C])
    with pytest.raises(ops.PaiError, match="go together"):
        ops.bn2_add_act(torch.float32, Z, SA, HA, ZB, SB, None, M, C, B.ACT_RELU, B.ACT_RELU, out[:M * C])
    with pytest.raises(ops.PaiError, match="go together"):
        ops.bn2_add_act(torch.float32, Z, SA, HA, ZB, None, HB, M, C, B.ACT_RELU, B.ACT_RELU, out[:M * C])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote its output"


# ---- a NaN stays a NaN ---------------------------------------------------------------------------------------------------------
# form: (dtype, ew_stream, ew_stream_blocks | None, (M, C)).  generic: the 1,048,800-vector tensor (a NaN in the second trip behind
# the 4096-block cap); streaming: bf16, 8195 x 64 at 3 blocks (22 ragged trips of 3072 vectors).
NAN_FORMS = {"generic-f32": (torch.float32, 0, None, BIG), "generic-bf16": (torch.bfloat16, 0, None, BIG),
             "stream-bf16": (torch.bfloat16, 1, 3, (4096 + 4099, 64))}


def _nan_positions(n, trip_elems):
    """Flat indices: the first and the last element, one element in each of the 8 lane positions of a vector (in 8 different
    vectors), one in the second sweep trip, one in the last vector."""
    pos = [0, n - 1, n - 8] + [8 * (100 + 37 * j) + j for j in range(8)] + [trip_elems + 8 * 5 + 3]
    assert max(pos) < n and trip_elems + 64 < n
    return torch.tensor(sorted(set(pos)))


def _inf_positions(n):
    return torch.tensor([16, n // 2 + 1, n - 17])


@lru_cache(maxsize=2)
def _nan_host(form):
    dtype, _, blocks, (M, C) = NAN_FORMS[form]
    za, zb, sa, ha, sb, hb = (t.clone() for t in _ew_host(M, C, dtype, 60))
    n = M * C
    trip = (4096 * 256 if blocks is None else blocks * 256 * 4) * 8
    pa, pb = _nan_positions(n, trip), _nan_positions(n, trip) + 8 * 7
    pb = pb[pb < n]
    za.view(-1)[pa] = NAN
    zb.view(-1)[pb] = NAN
    za.view(-1)[_inf_positions(n)] = -INF            # scale_a > 0: the pre-activation is -inf
    zb.view(-1)[_inf_positions(n) + 8] = INF
    return za, zb, sa, ha, sb, hb


@pytest.mark.parametrize("form", list(NAN_FORMS))
@pytest.mark.parametrize("op", ["bn_apply", "bn2_add_act", "add_act"])
def test_nan_stays_nan(pai, op, form):
    """NaN inputs come out as NaN at exactly their positions under ReLU and LeakyReLU (and without an activation), everything
    else inside the usual bound; -inf under ReLU is 0.  (add_act_k caps its grid at 8192 blocks: the generic tensor is one trip
    for it, the streaming form makes 22.)  bn2_add_act: NaNs in either branch, under either activation (the
    LeakyReLU tails of the streaming form run the generic kernel: same expectations)."""
    ops = _ops()
    dtype, stream, blocks, (M, C) = NAN_FORMS[form]
    za, zb, sa, ha, sb, hb = _nan_host(form)
    n = M * C
    tun = {"ew_stream": stream}
    if blocks is not None:
        tun["ew_stream_blocks"] = blocks
    ninf = _inf_positions(n)
    with _tunables(**tun):
        if op == "bn_apply":
            for a in (B.ACT_RELU, B.ACT_LRELU):
                r = B.apply(za, sa, ha, a)
                assert int(torch.isnan(r["out"]).sum()) == int(torch.isnan(za).sum()) > 10
                got = _run_apply(ops, dtype, za, sa, ha, a)
                _within(got, r["out"], _apply_lim(r, dtype), f"bn_apply NaN {form} {ACT_NAME[a]}")
                want = 0.0 if a == B.ACT_RELU else -INF
                assert got.view(-1)[ninf].tolist() == [want] * 3
        elif op == "bn2_add_act":
            for act_a, a, affb in ((B.ACT_RELU, B.ACT_RELU, True), (B.ACT_RELU, B.ACT_NONE, False), (B.ACT_NONE, B.ACT_RELU, False),
                                   (B.ACT_LRELU, B.ACT_LRELU, True), (B.ACT_RELU, B.ACT_LRELU, False)):
                s2, h2 = (sb, hb) if affb else (None, None)
                r = B.bn2_add_act(za, sa, ha, zb, s2, h2, act_a, a)
                assert int(torch.isnan(r["out"]).sum()) == int((torch.isnan(za) | torch.isnan(zb)).sum()) > 20
                got = _run_bn2(ops, dtype, za, sa, ha, zb, s2, h2, act_a, a)
                _within(got, r["out"], _bn2_lim(r, dtype), f"bn2_add_act NaN {form} {ACT_NAME[act_a]}/{ACT_NAME[a]} affb {affb}")
        else:
            (A, Av), (Bf, Bv) = _guarded(za, dtype), _guarded(zb, dtype)
            for a in (B.ACT_RELU, B.ACT_LRELU):
                ref = B.act(za.double() + zb.double(), a)
                assert int(torch.isnan(ref).sum()) == int((torch.isnan(za) | torch.isnan(zb)).sum()) > 20
                out = _poisoned(n, dtype)
                ops.add_act(dtype, Av, Bv, a, out[:n])
                torch.cuda.synchronize()
                _guard_ok(out, n, "add_act out")
                _within(out[:n].cpu(), ref, _add_lim(ref, dtype), f"add_act NaN {form} {ACT_NAME[a]}")
                want = 0.0 if a == B.ACT_RELU else -INF
                assert out[:n].cpu().view(-1)[ninf].tolist() == [want] * 3
            _unchanged(A, n, za, "add_act a")
            _unchanged(Bf, n, zb, "add_act b")


@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
def test_nan_channel_through_the_training_chain(pai, dtype):
    """pai_bn_stats -> pai_bn_finalize -> pai_bn_apply(ReLU) on 300 x 16 with one NaN in channel 5: the channel's partial sums,
    mean, rstd, scale, shift and running statistics are NaN and so is its whole output column -- not zeros with NaN running
    statistics behind a finite loss; every other channel is inside the bounds (finalize against the partial rows the kernel
    wrote, apply against the scale / shift the kernel wrote)."""
    ops = _ops()
    M, C, bad = 300, 16, 5
    z = (rnd((M, C), 70) * 1.5 + 0.3).to(dtype)
    z[123, bad] = NAN
    gamma, beta = 1 + 0.25 * rnd((C,), 71), 0.5 * rnd((C,), 72)
    rm0, rv0 = 0.3 * rnd((C,), 73), 0.5 + rnd((C,), 74).abs()
    R_ = ops.bn_stats_rows(M)
    rows = ops.bn_stats_buffer_rows(R_)
    stats = _poisoned(rows * 2 * C)
    Z, Zv = _guarded(z, dtype)
    (_, G), (_, Bt), (RM, RMv), (RV, RVv) = (_guarded(t) for t in (gamma, beta, rm0, rv0))
    outs = {k: _poisoned(C) for k in ("mean", "rstd", "scale", "shift")}
    out = _poisoned(M * C, dtype)
    nbt = torch.zeros(1, dtype=torch.int64, device=dev())
    with _tunables(ew_stream=0):
        ops.bn_stats(dtype, Zv, M, C, stats[:rows * 2 * C])
        ops.bn_finalize(stats, R_, C, M, G, Bt, B.f32c(EPS), B.f32c(MOM), 1, RMv, RVv, nbt, outs["mean"][:C], outs["rstd"][:C],
                        outs["scale"][:C], outs["shift"][:C])
        ops.bn_apply(dtype, Zv, M, C, outs["scale"][:C], outs["shift"][:C], B.ACT_RELU, out[:M * C])
    torch.cuda.synchronize()
    _guard_ok(out, M * C, "chain out")
    _unchanged(Z, M * C, z, "chain z")
    p = stats[:R_ * 2 * C].cpu().view(R_, 2, C)
    assert bool(torch.isnan(p[:, :, bad]).any()) and not bool(torch.isnan(p[:, :, [c for c in range(C) if c != bad]]).any())
    ref = B.finalize(p, M, gamma, beta, EPS, MOM, 1, rm0, rv0)
    got = {k: o[:C].cpu() for k, o in outs.items()}
    got.update(rm=RM[:C].cpu(), rv=RV[:C].cpu())
    lim = B.finalize_bounds(ref, 1)
    for k, g in got.items():
        assert bool(torch.isnan(g[bad])), f"chain {k}: channel {bad} is not NaN"
        assert bool(torch.isnan(ref[k][bad]))
        _within(g, ref[k], torch.nan_to_num(lim[k], nan=0.0), f"chain {_tn(dtype)} {k}")
    assert int(nbt) == 1
    r = B.apply(z, got["scale"], got["shift"], B.ACT_RELU)
    o = out[:M * C].cpu().view(M, C)
    assert bool(torch.isnan(o[:, bad]).all()), "the NaN channel was laundered into zeros"
    assert int(torch.isnan(o).sum()) == M
    _within(o, r["out"], _apply_lim(r, dtype), f"chain {_tn(dtype)} out")
