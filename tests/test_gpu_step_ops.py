"""GPU: the kernels every training step runs around the convolutions -- Adam (csrc/misc.hip), the mean-reduced losses,
denormalize and the metric glue (csrc/loss.hip, the fused denormalisation of csrc/ssim.hip), MaxPool / Upsample / add_act
(csrc/resnet.hip), act_bwd and the generic BatchNorm backward (csrc/bn.hip), InstanceNorm (csrc/inorm.hip) and the small
multi-tensor helpers of csrc/misc.hip -- each on its own through its ops.* wrapper, element by element against the fp64
host references of tests/_step_ref.py (tied to PyTorch's double-precision ops, autograd and torch.optim.Adam by
tests/test_step_refs_host.py), at the launch edges tests/test_gpu_ops.py and tests/test_gpu_discblock.py do not reach.

Every reference starts from exactly the tensors handed to the kernel (in bf16: the bf16-rounded values; the backward kernels
get the fp32 casts of the reference mean / rstd / sums, and their references use those casts) and from the kernel's own
fp32 constants (Adam: beta as fp32, omb = float32(1 - double(beta_f32)), lr / bc1 and 1 / sqrt(bc2) rounded once from
double).  The BatchNorm partial sums are DEFINED on du as stored: their reference takes the du the kernel wrote, which is
checked elementwise on its own.  Every output buffer is NaN before the call (an in-place buffer: its inputs) and carries 64
NaN guard elements behind it that must still be NaN afterwards; the generic kernels are reached with the tunable ew_stream
set to 0 and restored in ``finally``.

Bounds -- the project's existing bars (docstring of tests/test_gpu_vit_ops.py), none fitted to what a kernel produced
(u = 2^-24):
  fp32 elementwise outputs     |got - ref| <= 1e-5 max |ref|
  bf16 stored outputs          |got - ref| <= 2^-8 |ref| + 1e-6 max |ref|
  fp32 sums, per element       |got - ref| <= 1e-5 * (fp64 sum of the absolute terms of that element): loss sums, InstanceNorm
                               mean, upsample2_bwd (fp32), BatchNorm partial rows / sums / dgamma / dbeta (the += onto a
                               non-zero value adds one rounding of the result: + u |ref|)
  upsample2_bwd in bf16        an fp32 sum of four terms stored as bf16 carries both errors, so both bars are added:
                               |got - ref| <= 2^-8 |ref| + 1e-6 max |ref| + 1e-5 * (fp64 sum of the four absolute terms).  The
                               storage bar alone would be unmeetable where the four terms cancel (|ref| << the terms: the sum's
                               own error is then larger than half an ulp of the result); the third term is at most 1e-5 / 2^-8 =
                               0.26 % of the first wherever they do not
  rstd                         1e-5 relative
  selection, replication,      the same bits (a NaN matches a NaN): MaxPool and its backward, upsample2, cast / cast_multi,
  casts, one-rounding ops      zero_multi, lerp_multi (torch_ema's three roundings), scale_, dropout2d, pack_weights, denormalize and
                               its gradient, the L1 gradient (sign x the fp32 scale), scalar_take, the five Adam entry points
                               among each other
  Adam                         1e-5 max |p| would allow 5 % of the update, so the moments and the update are bounded separately,
                               in absolute-term form:  |m - ref| <= 1e-5 (|b1 m0| + |omb1 g|),  |v - ref| <= 1e-5 (|b2 v0| + omb2 g^2),
                               |p - ref| <= u |ref| + 1e-5 |delta_ref| + lr_over_bc1 1e-5 (|b1 m0| + |omb1 g|) / den_ref
                               (+ 4 x 2^-149 each: the subnormal floor of at most four roundings, for g = 1e-20).
                               Rounding counts of adam1: m = fma(b1, m0, round(omb1 g)): 2 roundings of at most u (|b1 m0| +
                               |omb1 g|) each, 2 u = 1.2e-7 against 1e-5; v = fma(b2, v0, round(round(omb2 g) g)): 3 u;
                               delta = round(lr m) / fma(sqrt(v), isb2, eps): product, root, fma, quotient: 4 roundings +
                               half the 3 u of v through the root: <= 6 u = 3.6e-7 relative against 1e-5 -- PROVIDED m is
                               accurate relative to itself, which it is not where b1 m0 and omb1 g cancel: the third term
                               carries the error of m (bounded above) through delta = lr m / den; the first term is the one
                               rounding of p - delta.  An fp32 emulation of adam1 on the host stays at 2.2e-7 of |delta| on
                               the p0 = 0 slice with betas (0.5, 0.999) and inside all three bounds (0.99 of the p bound where
                               |p0| ~ 1e3: u |ref| IS half an ulp) for steps 1, 2, 1000, 100000: tests/test_step_refs_host.py.
  BCE with logits              expf / log1pf accuracy cannot be derived: the bars are four times the error of PyTorch-CPU's own
                               fp32 binary_cross_entropy_with_logits(reduction="none") per unit of 1 + |x| and of
                               sigmoid(x) - t against fp64 on the logits of the largest case (a CPU measurement of the
                               reference, repeated and printed by tests/test_step_refs_host.py): measured 1.011e-7 and
                               8.886e-8, so 4.04e-7 (1 + |x|) per loss term (summed over the elements for the loss) and
                               3.55e-7 absolute per gradient, and never above 1e-5 (1 + |x|) resp. 1e-5
  metrics_take                 three fp64 formulas rounded once to fp32: 2^-23 relative
  InstanceNorm constant plane  |y| <= 2^-23 |c| / sqrt(eps): one rounding of the mean (an ulp of c at most) times rstd <= eps^-1/2
  InstanceNorm offset rstd     a priori from the one-pass formula, derived in test_instnorm_offset

Maxima measured on an MI355X (pytest -s; largest error and largest error / bound over all cases; every bound held).  The
InstanceNorm forward figures were measured with pixel 0 as the only pivot, before the second statistics sweep was added,
and test_adam_overflowing_square / test_instnorm_outlier_pivot have no recorded figure:
  Adam, all entry points   m 0.011 of its bound, v 0.090, p 0.9997 (|p0| ~ 1e3: u |ref| IS half an ulp; 3.2e-4 absolute)
  L1 / MSE                 loss: L1 exact, MSE 4.8e-7 (0.011); MSE gradient 0.011; L1 gradient, scalar_take: equal bits
  BCE                      gradient 0.26 of the 3.55e-7 bar, loss 0.25 of the summed bar
  metrics_take             exact (0 of 2^-23)
  upsample2_bwd            f32 4.8e-7 (0.010), bf16 1.56e-2 (0.983)
  add_act / act_bwd        f32 2.4e-7 (0.004), bf16 1.56e-2 (0.996)
  InstanceNorm             mean 3.9e-7 (0.024), rstd 3.3e-7 f32 / 1.0e-6 bf16 (0.065 / 0.21 of 1e-5 relative), y f32 2.4e-6 (0.050),
                           y bf16 1.48e-2 (0.995), dx f32 (0.012), dx bf16 (0.995); constant planes: mean, y exactly c, 0;
                           offset planes: rstd 1.9e-7 (0.004 of the a-priori bound at HW = 63), mean (0.005), y f32 (0.005)
  BatchNorm backward       du f32 2.4e-7 (0.005), du bf16 1.56e-2 (0.996); partial rows 1.3e-5 (0.031); sums 1.6e-4 (0.031);
                           dgamma / dbeta += 1.5e-4 (0.82: at M = 1 the bound is the one rounding of the +=); dz f32 1.5e-4
                           (0.013), dz bf16 7.8e-3 (0.995); bn2: partial rows (0.022), sums (0.010), dza / dzb f32 (0.009), bf16 (0.994)
  MaxPool and backward, upsample2, cast / cast_multi, zero_multi, lerp_multi, scale_, dropout2d, pack_weights, denormalize and
  its gradient, the Adam entry points among each other: equal bits
The ratios near 1 are bf16 stored outputs (2^-8 |ref| IS half an ulp just above a power of two) and the fp32 p of Adam.

Not covered: pai_adam_pack beyond one 64 x 64 x 1 weight with neighbours on either side; plan replay of the Adam
coefficients (tests/test_gpu_plan.py); the ew_stream forms of add_act / BatchNorm backward (tests/test_gpu_ew_stream.py
compares them with the generic kernels checked here); fp32 tensors past the 8192 x 256 grid of MaxPool / Upsample (the
bf16 instantiation runs the same loop); pack_weights_multi.

Which case fails which fault.  [m]: checked by a one-line mutation of the kernel in a scratch copy, built and run once on an
MI355X against the cases named -- they failed as listed, what is listed as passing passed; [p]: the case also fails with
the library built from the parent commit's sources (22 of the then 219 cases did: the [p] lines).  Lines without a mark
were not mutated: they rest on reading the kernel.
  [m][p] clamp before the NaN test in denorm_k  test_denormalize[16 / 5016 / 4194307]: the 1 / 6 / 4142 NaN elements come back 0
                                                (`('denormalize launders NaN', 1, ...)`)
  [m][p] the same in denorm_val (ssim.hip)      test_ssim_denorm_keeps_nan: out2 = [-0.0414, 938.12] where denorm = 0 gives [nan, nan]
  [m] adam_coeff_k does not store the count     test_adam_dev_counter[0 / 99999] and test_adam_entry_points[*] at `int(step_dev) == ...`
                                                (`assert 0 == 1`).  The coefficients of a first call are still those of preset + 1: only
                                                the counter asserts and the second call see this fault, coeff2_dev alone would not
  [m] a bias correction of the wrong step       (bc2 of step + 1 in pai::adam_coeffs) test_adam_entry_points and test_adam_multi at
                                                steps 1, 2, 1000 (p 4.8e-4 over its bound on the p0 = 0 slice; step 100000 passes:
                                                both corrections are 1 in fp32), test_adam_multi_97_tensors, test_adam_dev_counter[0]
                                                (the device's coefficients against the host's)
  [m] a skipped tail loop of adam_tensor        test_adam_multi[*], test_adam_multi_97_tensors: numel 1, 3, 5, 2049 and (4 << 20) + 5 keep
                                                p0, m0, v0 in their last elements
  [m] a grid-stride step of half the width      (gridDim.x * 256 for 512 in adam_tensor: vectors updated twice) test_adam_multi[*]
  a wrong vec test / NT instantiation           test_adam_multi: the two offset tensors (all four pointers, the gradient alone),
                                                (4 << 20) + 5 (NT, second grid-stride trip of one vector), (4 << 20) - 4.  Not mutated:
                                                the mutant would issue 16-byte accesses at 4-byte alignment
  [p] an empty tensor refused                   test_adam_multi[*], test_zero_multi (`pai_adam_multi: null tensor 2`, `pai_zero_multi:
                                                null tensor 10`)
  [m] a dropped `v != v` in maxpool2_k          test_maxpool[*] (all five): the windows with NaNs return the finite maximum
  [m] `>=` for `>` in the tie rule              test_maxpool[*] (all five): `the gradient did not go to the first maximum`
  [m] a sweep stride of 8 x for 4 x in loss_k   test_l1_mse[*-4194312-0]: the middle one of the three sweeps is never visited
  [m] the ragged exit of loss_k taken for all   (`i0 + 3 * stride >= n4` for `i >= n4`) test_l1_mse[*-4-0], [*-6148-0], [*-4194312-0]
      four vectors in flight
  [m] sign(0) = -1 in the vector path of L1     test_l1_mse[l1-4-0], [l1-6148-0], [l1-4194312-0]: `gradient is not sign x scale`
  [m] log1p(exp(x)) for the stable BCE form     test_bce[*-900], [*-4194307]: the loss is inf ([*-1] is the logit 0 alone and passes)
  [m][p] a plain one-pass InstanceNorm variance (no pivot) test_instnorm_constant_plane[3.3-4096-f32] alone: |y| exceeds 1.24e-4 by
                                                4.05e-4; [p] also test_instnorm[*-1-f32] at rstd (var of one pixel = the rounding of x^2)
  pixel 0 as the only InstanceNorm pivot        test_instnorm_outlier_pivot[4096-*]; by the fp32 emulation of the kernel's order on the
                                                host (tests/test_step_refs_host.py: 1.16 of the mean bar, 38 of the rstd bar), not mutated
  [m] a du that differs between the two sweeps  (in_du without `fp contract(off)`) test_instnorm[*-1-*], all eight: dx 3.3e-6 over its
      [p]                                       bound where it is 0 exactly
  a lane count for the wrong channel width      test_instnorm with C = 8, 24, 72 (a workgroup with missing channel lanes, a ragged second one)
  [m] an empty BatchNorm block that returns     test_bn_bwd[131073-8-*]: `partials: elements left unwritten`
  [m] one pass over 256 channel groups only     test_bn_bwd[*-4096-*], all ten: `du: elements left unwritten`
  act_grad(0) = 1                               test_act_bwd, test_bn_bwd: stored activations and pre-activations of exactly +0 / -0
                                                (common.h, shared by every kernel: not mutated)
  truncation in a cast                          test_cast: the ties-to-even pairs, 3.4e38 -> inf, NaN -> NaN (common.h: not mutated)
  [m] a contracted fma in ema1                  test_lerp_multi[0.001], [0.37]: 1 ulp off torch_ema's three roundings (weights 0 and 1 pass)
  a write past numel                            the guard of every test
"""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

import _step_ref as R
from _gpu_util import dev, q, rnd

pytestmark = pytest.mark.gpu

GUARD = 64
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
EPS = float(np.float32(1e-5))
ADAM_EPS = float(np.float32(R.ADAM_EPS))
ACTS = [R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU]
BCE_BOUND = min(4 * R.BCE_TORCH_ERR, 1e-5)            # per unit of 1 + |x|
BCE_GRAD_BOUND = min(4 * R.BCE_GRAD_TORCH_ERR, 1e-5)  # absolute
NAN = float("nan")


def _ops():
    from thesis_pai_reconstruction_amd import ops
    return ops


# ---- device helpers (as tests/test_gpu_vit_ops.py) -----------------------------------------------------------------------
def _d(t, dtype=torch.float32):
    return None if t is None else t.to(dev()).to(dtype).contiguous()


def _poisoned(n, dtype=torch.float32):
    """An output buffer of n elements followed by GUARD guard elements, all NaN (integer types: all ones)."""
    if dtype.is_floating_point:
        return torch.full((n + GUARD,), NAN, dtype=dtype, device=dev())
    return torch.full((n + GUARD,), -1 if dtype.is_signed else 255, dtype=dtype, device=dev())


def _guarded(t, dtype=torch.float32, lead=0):
    """The host tensor t on the device with ``lead`` NaN elements in front (lead = 1: an fp32 view that is not 16-byte aligned)
    and GUARD NaN elements behind; returns (whole buffer, the view holding t)."""
    n = t.numel()
    full = torch.full((lead + n + GUARD,), NAN, dtype=dtype, device=dev())
    full[lead:lead + n] = t.reshape(-1).to(dev()).to(dtype)
    return full, full[lead:lead + n]


def _guard_ok(full, n, what, lead=0):
    assert bool(torch.isnan(full[lead + n:]).all()) and bool(torch.isnan(full[:lead]).all()), f"{what}: wrote outside its {n} elements"


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
    print(f"{what}: max err {float(err.max()) if err.numel() else 0.0:.3g}, max err / bound {ratio:.3g}")
    bad = err > lim
    assert not bool(bad.any()), (what, int(bad.sum()), float((err - lim).max()))


def _stored_lim(ref):
    ref = ref.double()
    return 2.0 ** -8 * ref.abs() + 1e-6 * float(ref.abs().max())


def _elem_ok(got, ref, dtype, what):
    ref = ref.double()
    _within(got, ref, 1e-5 * float(ref.abs().max()) if dtype == torch.float32 else _stored_lim(ref), what)


def _sum_ok(got, ref, abs_terms, what, extra=0.0):
    _within(got, ref, 1e-5 * abs_terms.double() + extra, what)


def _bits_ok(full, n, ref, what):
    """The n elements in front of the guard are the bits of ref (any NaN for a NaN): written, selected and rounded alike."""
    _guard_ok(full, n, what)
    got = full[:n].cpu()
    assert R.same_bits(got.view(ref.shape), ref), (what, int((got.view(ref.shape).float() != ref.float()).sum()))
    print(f"{what}: equal bits ({n} elements)")


def _t(dtype):
    return IDS[DTYPES.index(dtype)]


def _with_dtypes(cases, big):
    """(case, dtype) for both dtypes; the one case past a grid-stride cap (``big``) in bf16 only: the same loop at half the bytes."""
    return [pytest.param(c, dt, id=f"{'x'.join(map(str, c)) if isinstance(c, tuple) else c}-{_t(dt)}")
            for c in cases for dt in DTYPES if not (c == big and dt == torch.float32)]


class _generic_kernels:
    """The generic kernels: the streaming forms (tunable ew_stream) would take the big bf16 calls."""

    def __enter__(self):
        _ops().set_tunable("ew_stream", 0)

    def __exit__(self, *exc):
        _ops().set_tunable("ew_stream")
        return False


# ---- Adam -------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _adam_host(n, seed):
    return R.adam_inputs(n, seed)


class _AdamState:
    """One tensor's p, g, m, v on the device, each with guards (``lead``: (p, g, m, v) leading elements -> unaligned views)."""

    def __init__(self, host, lead=(0, 0, 0, 0)):
        self.host, self.lead, self.n = host, lead, host[0].numel()
        self.full, self.view = zip(*[_guarded(t, lead=l) for t, l in zip(host, lead)])

    def args(self):
        return self.view

    def check(self, c, what):
        for k, name in ((0, "p"), (1, "g"), (2, "m"), (3, "v")):
            _guard_ok(self.full[k], self.n, f"{what} {name}", self.lead[k])
        p, g, m, v = (t.cpu() for t in self.view)
        assert torch.equal(g, self.host[1]), f"{what}: the gradient was written"
        if self.n == 0:
            return p, m, v
        ref = R.adam(*self.host, c, ADAM_EPS, fp32_range=True)
        over = torch.isinf(ref["v"])        # omb2 g^2 beyond fp32 (test_adam_overflowing_square only): v = +inf, p = p0
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v[~over]).all()), what
        assert torch.equal(torch.isinf(v) & (v > 0), over), f"{what}: v is not +inf exactly where omb2 g^2 overflows"
        assert torch.equal(p[over], self.host[0][over]), f"{what}: the update is not 0 where v = inf"
        lim_m, lim_v, lim_p = R.adam_bounds(ref, c)
        _within(m, ref["m"], lim_m, f"{what} m")
        _within(v[~over], ref["v"][~over], lim_v[~over], f"{what} v")
        _within(p, ref["p"], lim_p, f"{what} p")
        return p, m, v


ADAM_MULTI_SIZES = [(4 << 20) + 5, (4 << 20) - 4, 0, 1, 3, 5, 2049]


@pytest.mark.parametrize("betas", R.ADAM_BETAS, ids=str)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_adam_multi(pai, step, betas):
    """One chunk (the grid is sized by the largest tensor): (4 << 20) + 5 -- the non-temporal instantiation, ONE vector in the
    second grid-stride trip behind the 2048-block cap, a scalar tail of 1; (4 << 20) - 4 -- the last size of the plain
    path; 0, 1, 3, 5, 2049; a tensor whose four pointers are views offset by one float and one where only the gradient is
    (the scalar path for a pointer that is not 16-byte aligned)."""
    ops = _ops()
    c = R.adam_coeffs(R.ADAM_LR, betas[0], betas[1], step)
    states = [_AdamState(_adam_host(n, 100 + i)) for i, n in enumerate(ADAM_MULTI_SIZES)]
    states.append(_AdamState(_adam_host(2051, 120), lead=(1, 1, 1, 1)))
    states.append(_AdamState(_adam_host(2053, 121), lead=(0, 1, 0, 0)))
    assert states[-2].view[0].data_ptr() % 16 == 4 and states[-1].view[1].data_ptr() % 16 == 4
    assert states[-1].view[0].data_ptr() % 16 == 0 and states[2].n == 0
    cols = list(zip(*[s.args() for s in states]))
    ops.adam_multi(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), R.ADAM_LR, betas[0], betas[1], ADAM_EPS, step)
    torch.cuda.synchronize()
    for s in states:
        s.check(c, f"adam_multi step {step} n {s.n} lead {s.lead}")


def test_adam_multi_97_tensors(pai):
    """Three launches: chunks of 48, 48 and 1 tensors."""
    ops = _ops()
    step, betas = 1000, (0.9, 0.999)
    c = R.adam_coeffs(R.ADAM_LR, betas[0], betas[1], step)
    states = [_AdamState(_adam_host(1 + (37 * i) % 301, 200 + i)) for i in range(97)]
    cols = list(zip(*[s.args() for s in states]))
    ops.adam_multi(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), R.ADAM_LR, betas[0], betas[1], ADAM_EPS, step)
    torch.cuda.synchronize()
    for i in (0, 47, 48, 95, 96):           # the ends of the three chunks in full; p of every tensor below
        states[i].check(c, f"adam_multi 97[{i}]")
    for i, s in enumerate(states):
        ref = R.adam(*s.host, c, ADAM_EPS)
        lim = R.adam_bounds(ref, c)[2]
        assert bool(((s.view[0].cpu().double() - ref["p"]).abs() <= lim).all()), i


def test_adam_alone_past_its_cap(pai):
    """pai_adam at 8192 * 256 + 3 elements: three threads take a second grid-stride trip."""
    ops = _ops()
    step, betas = 2, (0.5, 0.999)
    s = _AdamState(_adam_host(8192 * 256 + 3, 300))
    ops.adam(*s.args(), R.ADAM_LR, betas[0], betas[1], ADAM_EPS, step)
    torch.cuda.synchronize()
    s.check(R.adam_coeffs(R.ADAM_LR, betas[0], betas[1], step), "adam 8192*256+3")


def test_adam_overflowing_square(pai):
    """g = +-1e21 in every other element: omb2 g^2 = 1e39 is beyond fp32 in either order of the product (g = 1e18, a slice of
    every case above, reaches only g^2 = 1e36, v ~ 1e33).  The reference in kind is what torch's fp32 formula gives
    (tests/test_step_refs_host.py): v = +inf exactly there, den = inf, an update of exactly 0 (p keeps its bits), m ~ 1e20
    finite and inside its bound; the neighbours meet the usual bounds.  adam (scalar loop) and adam_multi (vectors and a
    scalar tail of 3) give the same bits."""
    ops = _ops()
    step, betas = 2, (0.9, 0.999)
    c = R.adam_coeffs(R.ADAM_LR, betas[0], betas[1], step)
    host = R.adam_overflow_inputs(4099, 600)
    a, b = _AdamState(host), _AdamState(host)
    ops.adam(*a.args(), R.ADAM_LR, betas[0], betas[1], ADAM_EPS, step)
    ops.adam_multi(*[[t] for t in b.args()], R.ADAM_LR, betas[0], betas[1], ADAM_EPS, step)
    torch.cuda.synchronize()
    ra, rb = a.check(c, "adam g = 1e21"), b.check(c, "adam_multi g = 1e21")
    assert int(torch.isinf(ra[2]).sum()) == 2050
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)


PACK_OFF, PACK_N = 8, 8 + 64 * 64 + 37       # a 64 x 1 x 64 weight at element 8 of a range with neighbours on both sides


def _dev_scalars(preset):
    step_dev = torch.full((1,), preset, dtype=torch.int64, device=dev())
    return step_dev, _poisoned(2)


def _coeff_ok(coeff_full, c, what):
    got = _written(coeff_full, 2, what)
    want = torch.tensor([c["lr_over_bc1"], c["inv_sqrt_bc2"]], dtype=torch.float32)
    ulp = torch.from_numpy(np.spacing(want.numpy()))
    assert bool(((got.double() - want.double()).abs() <= ulp.double()).all()), (what, got.tolist(), want.tolist())
    return bool(torch.equal(got, want))


@pytest.mark.parametrize("betas", R.ADAM_BETAS, ids=str)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_adam_entry_points(pai, step, betas):
    """adam, adam_dev, adam_multi, adam_multi_dev and adam_pack on the same inputs share adam1: equal bits for p, m, v (the
    device-step forms: where their coefficients equal the host's, which the one-ulp check leaves open); each inside the fp64
    bounds; adam_pack's bf16 packs are the casts of the new weight."""
    ops = _ops()
    c = R.adam_coeffs(R.ADAM_LR, betas[0], betas[1], step)
    host = _adam_host(PACK_N, 400)
    hp = (R.ADAM_LR, betas[0], betas[1], ADAM_EPS)
    res, same_coeff = {}, {}

    s = _AdamState(host)
    ops.adam(*s.args(), *hp, step)
    res["adam"] = s
    s = _AdamState(host)
    ops.adam_multi(*[[t] for t in s.args()], *hp, step)
    res["adam_multi"] = s
    s = _AdamState(host)
    step_dev, coeff = _dev_scalars(step - 1)
    ops.adam_dev(*s.args(), *hp, step_dev, coeff[:2])
    res["adam_dev"], dev1 = s, (step_dev, coeff)
    s = _AdamState(host)
    step_dev, coeff = _dev_scalars(step - 1)
    ops.adam_multi_dev(*[[t] for t in s.args()], *hp, step_dev, coeff[:2])
    res["adam_multi_dev"], dev2 = s, (step_dev, coeff)
    s = _AdamState(host)
    wf, wd = _poisoned(64 * 64, torch.bfloat16), _poisoned(64 * 64, torch.bfloat16)
    ops.adam_pack(*s.args(), PACK_OFF, 64, 1, 64, wf[:4096], wd[:4096], *hp, step)
    res["adam_pack"] = s
    torch.cuda.synchronize()

    out = {k: v.check(c, f"{k} step {step}") for k, v in res.items()}
    for name, (step_dev, coeff) in (("adam_dev", dev1), ("adam_multi_dev", dev2)):
        assert int(step_dev) == step, (name, int(step_dev))
        same_coeff[name] = _coeff_ok(coeff, c, f"{name} coeff2_dev step {step}")
    for k in ("adam_multi", "adam_pack", "adam_dev", "adam_multi_dev"):
        if same_coeff.get(k, True):
            for a, b, what in zip(out["adam"], out[k], "pmv"):
                assert torch.equal(a, b), (k, what)
    assert torch.equal(out["adam_dev"][0], out["adam_multi_dev"][0])
    w = out["adam_pack"][0][PACK_OFF:PACK_OFF + 4096].view(64, 1, 64)
    ref_f, ref_d = R.pack_weights(w, torch.bfloat16)
    _bits_ok(wf, 4096, ref_f.reshape(-1), "adam_pack forward pack")
    _bits_ok(wd, 4096, ref_d.reshape(-1), "adam_pack input-gradient pack")


@pytest.mark.parametrize("preset", [0, 99999])
def test_adam_dev_counter(pai, preset):
    """The device counter advances by one per call and the coefficients are those of the NEW count: two calls from a preset
    of 0 and of 99999 (a frozen step would apply step 1's bias correction, 1 / (1 - beta1) times the late one)."""
    ops = _ops()
    betas = (0.9, 0.999)
    hp = (R.ADAM_LR, betas[0], betas[1], ADAM_EPS)
    step_dev, coeff = _dev_scalars(preset)
    for k, multi in ((1, False), (2, True)):
        c = R.adam_coeffs(R.ADAM_LR, betas[0], betas[1], preset + k)
        s = _AdamState(_adam_host(5000, 500 + k))
        if multi:
            ops.adam_multi_dev(*[[t] for t in s.args()], *hp, step_dev, coeff[:2])
        else:
            ops.adam_dev(*s.args(), *hp, step_dev, coeff[:2])
        torch.cuda.synchronize()
        assert int(step_dev) == preset + k
        same = _coeff_ok(coeff, c, f"coeff2_dev at count {preset + k}")
        got = s.check(c, f"adam{'_multi' if multi else ''}_dev at count {preset + k}")
        if same:
            h = _AdamState(s.host)
            ops.adam(*h.args(), *hp, preset + k)
            torch.cuda.synchronize()
            for a, b in zip(got, [t.cpu() for t in (h.view[0], h.view[2], h.view[3])]):
                assert torch.equal(a, b)


# ---- losses -----------------------------------------------------------------------------------------------------------------------
def _acc(value):
    full = torch.full((1 + GUARD,), NAN, dtype=torch.float64, device=dev())
    full[0] = value
    return full


LOSS_CASES = [(4, 0), (7, 0), (4099, 0), (3 * 2048 + 4, 0), (4 * (1 << 20) + 8, 0), (4096, 1)]


@pytest.mark.parametrize("numel,lead", LOSS_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_l1_mse(pai, kind, numel, lead):
    """4: one vector; 7, 4099: the scalar path (numel % 4); 3 * 2048 + 4: ragged against the four vectors in flight;
    4 * (1 << 20) + 8: three sweeps behind the 512-block cap; 4096 with the target a view offset by one float: the scalar
    path by alignment.  Two launches (with the gradient, then without) into ONE accumulator that starts at 3.25, scales
    other than 1; scalar_take returns float(acc) and leaves exactly 0."""
    ops = _ops()
    fn, ref_fn = (ops.l1, R.l1) if kind == "l1" else (ops.mse, R.mse)
    x, t = rnd((numel,), 11), rnd((numel,), 12)
    k = max(1, numel // 5)
    t[:k] = x[:k]                       # exact zero differences ...
    x[0], t[0] = -0.0, 0.0              # ... -0 against +0 among them
    X = _d(x)
    t_full, T = _guarded(t, lead=lead)
    assert T.data_ptr() % 16 == 4 * lead
    grad = _poisoned(numel)
    acc = _acc(3.25)
    ls1, gs1, ls2 = 0.75, 1.5, 2.0
    fn(X, T, ls1, acc[:1], gs1, grad[:numel])
    fn(X, T, ls2, acc[:1])
    torch.cuda.synchronize()
    ref = ref_fn(x, t)
    tag = f"{kind} n {numel} lead {lead}"
    got_acc = float(acc[0])
    assert bool(torch.isnan(acc[1:]).all()), "accumulator guard"
    w = (ls1 + ls2) / numel
    _within(torch.tensor([got_acc - 3.25]), torch.tensor([w * float(ref["sum"])]), 1e-5 * w * float(ref["abs"]) + 3.25 * 2.0 ** -50,
            f"{tag} loss (two launches onto 3.25)")
    gscale = float(np.float32(gs1 / numel))
    g = _written(grad, numel, f"{tag} grad")
    if kind == "l1":
        assert torch.equal(g, (ref["grad"] * gscale).float()), f"{tag}: gradient is not sign x scale"
        assert float(g[:k].abs().max()) == 0.0
    else:
        _within(g, ref["grad"] * gscale, 1e-5 * float((ref["grad"] * gscale).abs().max()), f"{tag} grad")
    out = _poisoned(1)
    ops.scalar_take(acc[:1], out[:1])
    torch.cuda.synchronize()
    assert float(_written(out, 1, "scalar_take")[0]) == float(torch.tensor(got_acc, dtype=torch.float64).float())
    assert float(acc[0]) == 0.0 and math.copysign(1.0, float(acc[0])) == 1.0 and bool(torch.isnan(acc[1:]).all())
    _guard_ok(t_full, numel, "target", lead)


@pytest.mark.parametrize("numel", R.BCE_NUMELS)
@pytest.mark.parametrize("target", R.BCE_TARGETS)
def test_bce(pai, target, numel):
    """Targets 0, 1 and 0.9; logits 0, +-1e-8, +-20, +-88, +-89 (expf overflows between them), +-100, +-1e4 mixed into
    normal data of scale 2; 2048 * 2048 + 3 elements: nine trips behind the 2048-block cap (2048 x 256 threads, one element
    each per trip).  Every gradient is finite and
    within the BCE bar of sigmoid(x) - t, the loss within the summed bar; with and without the gradient."""
    ops = _ops()
    x = R.bce_logits(numel)
    X = _d(x)
    grad = _poisoned(numel)
    acc = _acc(-1.5)
    ops.bce_logits(X, target, 0.5, acc[:1], numel * 0.25, grad[:numel])      # grad_scale / numel = 0.25: an exact scaling
    ops.bce_logits(X, target, 0.25, acc[:1])
    torch.cuda.synchronize()
    l, g = R.bce_terms(x, target)
    tag = f"bce t {target} n {numel}"
    got = _written(grad, numel, f"{tag} grad")
    _within(got.double() / 0.25, g, BCE_GRAD_BOUND, f"{tag} grad")
    w = 0.75 / numel
    lim = w * float((BCE_BOUND * (1 + x.double().abs())).sum()) + 1.5 * 2.0 ** -50
    loss = float(acc[0])
    assert math.isfinite(loss) and bool(torch.isnan(acc[1:]).all())
    _within(torch.tensor([loss + 1.5]), torch.tensor([w * float(l.sum())]), lim, f"{tag} loss")


def test_metrics_take(pai):
    import oracle
    ops = _ops()
    a, b = torch.rand(3, 1, 32, 48), torch.rand(3, 1, 32, 48)
    sse = float(((a.double() - b.double()) ** 2).sum())
    for ssum, s2, n_img in ((2.4375, sse, 3), (3.0, 0.0, 3)):
        sums = torch.full((2 + GUARD,), NAN, dtype=torch.float64, device=dev())
        sums[0], sums[1] = ssum, s2
        out = _poisoned(3)
        ops.metrics_take(sums[:2], n_img, a.numel(), out[:3])
        torch.cuda.synchronize()
        _guard_ok(out, 3, "out3")
        got, ref = out[:3].cpu(), R.metrics_take(ssum, s2, n_img, a.numel())
        assert sums[:2].tolist() == [0.0, 0.0] and bool(torch.isnan(sums[2:]).all())
        if s2 == 0.0:           # identical images: what oracle.psnr gives
            assert got.tolist() == [1.0, math.inf, 0.0] and float(oracle.psnr(a, a)) == math.inf
        else:
            _within(got, torch.tensor(ref), 2.0 ** -23 * torch.tensor(ref).abs(), "metrics_take")
            assert abs(float(got[1]) - float(oracle.psnr(a.double(), b.double()))) < 1e-5


# ---- denormalize -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numel", [16, 5016, 4096 * 1024 + 3])
def test_denormalize(pai, numel):
    """Forward: the bits of oracle.denormalize (torch.clamp(x * 0.5 + 0.5, 0, 1)) on data that includes exactly -1 and +1, one
    ulp on either side of each, +-inf and NaN -- NaN stays NaN (fminf(fmaxf(NaN, 0), 1) is 0: the parent commit fails here).
    Gradient: torch's clamp backward: 0 at a NaN and outside, 0.5 g on the closed boundaries."""
    import oracle
    ops = _ops()
    sp = R.denorm_specials()
    x = torch.cat([sp, rnd((numel - sp.numel(),), 21) * 1.2])
    if numel > 40:
        x[torch.arange(40, numel, 1013)] = NAN
    g = rnd((numel,), 22)
    X, G = _d(x), _d(g)
    out, gout = _poisoned(numel), _poisoned(numel)
    ops.denormalize(X, None, out[:numel])
    ops.denormalize(X, G, gout[:numel])
    torch.cuda.synchronize()
    want = oracle.denormalize(x)
    got = out[:numel].cpu()
    nan_kept = torch.isnan(got) == torch.isnan(want)
    assert bool(nan_kept.all()), ("denormalize launders NaN", int((~nan_kept).sum()), got[:16].tolist(), want[:16].tolist())
    _bits_ok(out, numel, want, f"denormalize n {numel}")
    xr = x.clone().requires_grad_(True)
    oracle.denormalize(xr).backward(g)
    got_g = _written(gout, numel, "denormalize gradient")
    assert torch.equal(got_g, xr.grad), int((got_g != xr.grad).sum())
    u = x * 0.5 + 0.5
    assert float(got_g[torch.isnan(x)].abs().max()) == 0.0 and bool((got_g[(u == 0) | (u == 1)] == 0.5 * g[(u == 0) | (u == 1)]).all())


def test_ssim_denorm_keeps_nan(pai):
    """ssim_sse, eval_planes and ssim_psnr_bwd with denorm = 1 and ONE NaN pixel in image 1 of 3: the sums (the gradient) of
    that image are NaN, as they are with denorm = 0 on the denormalised images, and never the finite values of a black
    pixel; the other images keep the bits of the run without the NaN."""
    import oracle
    ops = _ops()
    NC, H, W = 3, 32, 48
    p, t = torch.tanh(rnd((NC, 1, H, W), 31)), torch.tanh(rnd((NC, 1, H, W), 32))
    pn = p.clone()
    pn[1, 0, 7, 9] = NAN
    T = _d(t)
    sse_clean = torch.tensor([float(((oracle.denormalize(p).double() - oracle.denormalize(t).double()) ** 2).sum())],
                             dtype=torch.float64, device=dev())

    def run(pred, target, denorm):
        P = _d(pred)
        out2 = torch.zeros(2, dtype=torch.float64, device=dev())
        per, ssim_pl, sse_pl = (torch.zeros(NC, dtype=torch.float64, device=dev()) for _ in range(3))
        ops.ssim_sse(P, target, NC, H, W, denorm, out2, per, None)
        ops.eval_planes(P, target, NC, H, W, denorm, ssim_plane=ssim_pl, sse_plane=sse_pl)
        grad = _poisoned(NC * H * W)
        ws = torch.empty(ops.ssim_bwd_workspace_floats(NC, H, W), dtype=torch.float32, device=dev())
        ops.ssim_psnr_bwd(P, target, NC, H, W, denorm, 0.7, 0.3, sse_clean, grad[:NC * H * W], ws)
        torch.cuda.synchronize()
        _guard_ok(grad, NC * H * W, "ssim_psnr_bwd grad")
        return out2.cpu(), per.cpu(), ssim_pl.cpu(), sse_pl.cpu(), grad[:NC * H * W].cpu().view(NC, H, W)

    clean = run(p, T, 1)
    assert all(bool(torch.isfinite(v).all()) for v in clean)
    nan1 = run(pn, T, 1)
    nan0 = run(oracle.denormalize(pn), _d(oracle.denormalize(t)), 0)
    for name, c, a, b in zip(("out2", "per_image", "ssim_plane", "sse_plane", "grad"), clean, nan1, nan0):
        if name == "out2":
            assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()), (name, a.tolist(), b.tolist())
            continue
        assert bool(torch.isnan(a[1]).any()) and bool(torch.isnan(b[1]).any()), \
            (name, "denorm = 1 reports finite values for an image with a NaN pixel", a[1].reshape(-1)[:4].tolist())
        if name != "grad":
            assert math.isnan(float(a[1])) and math.isnan(float(b[1]))
        else:
            assert math.isnan(float(a[1, 7, 9])) or float(a[1, 7, 9]) == 0.0     # d clamp / d NaN = 0 times a NaN sum
        for i in (0, 2):
            assert R.same_bits(a[i], c[i]), (name, i)


# ---- MaxPool / Upsample / add_act / act_bwd ---------------------------------------------------------------------------------------
INF = float("inf")
POOL_SPECIALS = [[0, 0, 0, 0], [-INF] * 4, [-0.0, 0.0, 0.0, -0.0], [0.0, -0.0, -0.0, 0.0], [1, NAN, 5, 0], [NAN, 7, NAN, 1],
                 [NAN] * 4, [2, 2, 1, 2], [1, 2, 2, 0], [-INF, -INF, 3, 3], [-1, -1, -1, -1], [5, NAN, NAN, NAN]]
POOL_SHAPES = [(2, 4, 2, 8), (3, 6, 10, 24), (1, 2898, 2896, 8)]


def _pool_input(N, H, W, C, seed):
    """Small-integer data (most windows tie) as [N][H][W][C] fp32, the special windows planted in front: all zero, all -inf,
    -0 beside +0, one / two / three / four NaNs, ties at the first, second and third element."""
    g = torch.Generator().manual_seed(seed)
    nw = N * (H // 2) * (W // 2) * C
    xw = torch.randint(-2, 3, (nw, 4), generator=g, dtype=torch.int8).float()
    sp = torch.tensor(POOL_SPECIALS, dtype=torch.float32)
    xw[:len(sp)] = sp
    return xw.view(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C).contiguous()


@pytest.mark.parametrize("shape,dtype", _with_dtypes(POOL_SHAPES, POOL_SHAPES[-1]))
def test_maxpool(pai, shape, dtype):
    """Output, index (through maxpool2_bwd against autograd of F.max_pool2d) and every element of dx, in bits: W = 2, C = 8
    and 24, and (bf16) one tensor past 8192 * 256 vectors.  Integer data: every value is exact in bf16."""
    ops = _ops()
    N, H, W, C = shape
    x = _pool_input(N, H, W, C, 41)
    no = x.numel() // 4
    g = torch.Generator().manual_seed(42)
    dout = (torch.randint(-3, 3, (N, H // 2, W // 2, C), generator=g, dtype=torch.int8).float() + 0.5)
    out, idx, dx = _poisoned(no, dtype), _poisoned(no, torch.uint8), _poisoned(x.numel(), dtype)
    ops.maxpool2(dtype, _d(x, dtype), N, H, W, C, out[:no], idx[:no])
    ops.maxpool2_bwd(dtype, _d(dout, dtype), idx[:no], N, H, W, C, dx[:x.numel()])
    torch.cuda.synchronize()
    ref, bwd = R.maxpool2(x)
    tag = f"maxpool {_t(dtype)} {shape}"
    _bits_ok(out, no, ref.to(dtype).reshape(-1), f"{tag} out")
    assert bool((idx[:no] <= 3).all()) and bool((idx[no:] == 255).all()), f"{tag}: idx unwritten, out of range, or written past"
    got_dx = _written(dx, x.numel(), f"{tag} dx")
    assert torch.equal(got_dx, bwd(dout).reshape(-1)), f"{tag}: the gradient did not go to the first maximum / the last NaN"
    # without the index output
    out2 = _poisoned(no, dtype)
    ops.maxpool2(dtype, _d(x, dtype), N, H, W, C, out2[:no])
    torch.cuda.synchronize()
    _bits_ok(out2, no, ref.to(dtype).reshape(-1), f"{tag} out (no idx)")


UP_SHAPES = [(2, 2, 1, 8), (3, 3, 5, 24), (1, 1449, 1448, 8)]


@pytest.mark.parametrize("shape,dtype", _with_dtypes(UP_SHAPES, UP_SHAPES[-1]))
def test_upsample(pai, shape, dtype):
    """upsample2 in bits; upsample2_bwd against the fp64 sum of its four terms (the tensor past the grid, bf16: small integers,
    the sum is exact and the bits are compared)."""
    ops = _ops()
    N, H, W, C = shape
    big = shape == UP_SHAPES[-1]
    n_in = N * H * W * C
    tag = f"upsample {_t(dtype)} {shape}"
    if big:
        g = torch.Generator().manual_seed(43)
        x = torch.randint(-2, 3, (N, H, W, C), generator=g, dtype=torch.int8).float()
        dout = torch.randint(-2, 3, (N, 2 * H, 2 * W, C), generator=g, dtype=torch.int8).float()
    else:
        x, dout = q(rnd((N, H, W, C), 44), dtype), q(rnd((N, 2 * H, 2 * W, C), 45), dtype)
        x.view(-1)[:4] = torch.tensor([NAN, INF, -0.0, 0.0])
    out, dx = _poisoned(4 * n_in, dtype), _poisoned(n_in, dtype)
    ops.upsample2(dtype, _d(x, dtype), N, H, W, C, out[:4 * n_in])
    ops.upsample2_bwd(dtype, _d(dout, dtype), N, H, W, C, dx[:n_in])
    torch.cuda.synchronize()
    _bits_ok(out, 4 * n_in, R.upsample2(x).to(dtype).reshape(-1), f"{tag} out")
    if big:
        want = dout.view(N, H, 2, W, 2, C).sum((2, 4))
        _bits_ok(dx, n_in, want.to(dtype).reshape(-1), f"{tag} dx")
        return
    s, ab = R.upsample2_bwd(dout)
    got = _written(dx, n_in, f"{tag} dx")
    _within(got, s, 1e-5 * ab if dtype == torch.float32 else _stored_lim(s) + 1e-5 * ab, f"{tag} dx")


EW_NUMELS = [8, 8 * 1000, 8 * ((1 << 21) + 3)]


def _kinked(t):
    """Exact +0 / -0 among the activation arguments."""
    t = t.clone()
    t.view(-1)[1:5] = torch.tensor([0.0, -0.0, 0.0, -0.0])
    return t


@pytest.mark.parametrize("numel,dtype", _with_dtypes(EW_NUMELS, EW_NUMELS[-1]))
def test_add_act(pai, numel, dtype):
    """The generic add_act_k (ew_stream = 0), all three activations; 8 * (2^21 + 3): past the 8192-block grid (bf16)."""
    ops = _ops()
    big = numel == EW_NUMELS[-1]
    a, b = q(rnd((numel,), 51), dtype), q(rnd((numel,), 52), dtype)
    b[:8] = -a[:8]                                                  # exact zero sums
    A, B = _d(a, dtype), _d(b, dtype)
    with _generic_kernels():
        for act in ([R.ACT_LRELU] if big else ACTS):
            out = _poisoned(numel, dtype)
            ops.add_act(dtype, A, B, act, out[:numel])
            torch.cuda.synchronize()
            _elem_ok(_written(out, numel, "add_act"), R.add_act(a, b, act), dtype, f"add_act {_t(dtype)} n {numel} act {act}")


ACTB_NUMELS = [8, 8 * 1000, 8 * ((1 << 20) + 3)]


@pytest.mark.parametrize("numel,dtype", _with_dtypes(ACTB_NUMELS, ACTB_NUMELS[-1]))
def test_act_bwd(pai, numel, dtype):
    """du = g1 act1'(a) (+ g2 act2'(a)) with one and two gradients, all three activations, stored activations of exactly +0 /
    -0 (the slope of the negative side, torch's convention); 8 * (2^20 + 3): past the 4096-block grid (bf16)."""
    ops = _ops()
    big = numel == ACTB_NUMELS[-1]
    g1, g2, a = q(rnd((numel,), 53), dtype), q(rnd((numel,), 54), dtype), _kinked(q(rnd((numel,), 55), dtype))
    G1, G2, A = _d(g1, dtype), _d(g2, dtype), _d(a, dtype)
    pairs = [(R.ACT_LRELU, R.ACT_RELU)] if big else [(R.ACT_NONE, None), (R.ACT_LRELU, None), (R.ACT_RELU, None),
                                                      (R.ACT_LRELU, R.ACT_RELU), (R.ACT_RELU, R.ACT_NONE)]
    for act1, act2 in pairs:
        du = _poisoned(numel, dtype)
        ops.act_bwd(dtype, G1, act1, G2 if act2 is not None else None, act2 if act2 is not None else 0, A, numel, du[:numel])
        torch.cuda.synchronize()
        ref, ab = R.act_bwd(g1, act1, g2 if act2 is not None else None, act2, a)
        tag = f"act_bwd {_t(dtype)} n {numel} acts {act1},{act2}"
        got = _written(du, numel, tag)
        _elem_ok(got, ref, dtype, tag)
        k = slice(1, 5)     # the kink: exactly g1 * slope1 (+ g2 * slope2), no rounding beyond the storage type's
        want = (ref[k].float() if dtype == torch.float32 else ref[k].float().to(dtype).float())
        assert torch.allclose(got[k], want, rtol=2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -22, atol=0), (tag, got[k], want)


# ---- InstanceNorm ---------------------------------------------------------------------------------------------------------------
def _instnorm(x, g, dtype, acts, tag, rstd_lim=None, y_from_stored_stats=False):
    """instnorm_fwd / instnorm_bwd on host inputs [N][HW][C] (already rounded through dtype), all checks."""
    ops = _ops()
    N, HW, C = x.shape
    n = x.numel()
    X, G = _d(x, dtype), _d(g, dtype)
    ref = R.instnorm_fwd(x, EPS, R.ACT_NONE)
    for act in acts:
        y, mean, rstd = _poisoned(n, dtype), _poisoned(N * C), _poisoned(N * C)
        ops.instnorm_fwd(dtype, X, N, HW, C, EPS, act, y[:n], mean[:N * C], rstd[:N * C])
        torch.cuda.synchronize()
        got_m, got_r = _written(mean, N * C, "mean").view(N, C), _written(rstd, N * C, "rstd").view(N, C)
        _sum_ok(got_m, ref["mean"], ref["mean_abs"], f"{tag} act {act} mean")
        _within(got_r, ref["rstd"], (1e-5 if rstd_lim is None else rstd_lim) * ref["rstd"], f"{tag} act {act} rstd")
        yr = R.instnorm_fwd(x, EPS, act, mean=got_m, rstd=got_r) if y_from_stored_stats else R.instnorm_fwd(x, EPS, act)
        _elem_ok(_written(y, n, "y"), yr["y"], dtype, f"{tag} act {act} y")
        # backward from the fp32 casts of the reference statistics
        m32, r32 = ref["mean"].float(), ref["rstd"].float()
        dx = _poisoned(n, dtype)
        ops.instnorm_bwd(dtype, G, X, N, HW, C, act, _d(m32.reshape(-1)), _d(r32.reshape(-1)), dx[:n])
        torch.cuda.synchronize()
        _elem_ok(_written(dx, n, "dx"), R.instnorm_bwd(g, x, act, m32, r32), dtype, f"{tag} act {act} dx")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("HW", [1, 7, 31, 33, 63, 4096])
@pytest.mark.parametrize("C", [8, 24, 64, 72])
def test_instnorm(pai, C, HW, dtype):
    """N = 3; C = 8, 24 (one workgroup whose lanes of missing channels still reach the block sums), 64, 72 (a second, ragged
    workgroup); HW = 1 (variance 0), below / around the 32 pixel lanes, 4096 (128 terms per lane); all three activations,
    forward (mean, rstd against the fp64 statistics of the stored inputs, then y) and backward."""
    x, g = q(rnd((3, HW, C), 61) * 2.0 + 0.5, dtype), q(rnd((3, HW, C), 62), dtype)
    _instnorm(x, g, dtype, ACTS, f"instnorm {_t(dtype)} C {C} HW {HW}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("HW", [7, 63, 4096])
@pytest.mark.parametrize("c", [0.0, 3.3])
def test_instnorm_constant_plane(pai, c, HW, dtype):
    """A dead channel: every plane constant (var = 0, rstd = eps^-1/2 = 316).  Outputs finite; |y| <= 2^-23 |c| / sqrt(eps):
    the mean may be one rounding (an ulp of c) off c, times rstd; dx finite.  The plain one-pass sums E[x^2] - E[x]^2 of the
    parent commit gave |y| = 5.3e-4 against 1.24e-4 at c = 3.3, HW = 4096 (fp32 lane sums of 128 equal terms drift by 18
    ulp: the library built from the parent commit's csrc/inorm.hip exceeded the bound by 4.05e-4 on the device in
    [3.3-4096-f32]); the kernel now sums x - pivot, first pivot pixel 0: every difference of a constant plane is 0."""
    ops = _ops()
    N, C = 3, 24
    x = q(torch.full((N, HW, C), c), dtype)
    cq = float(x[0, 0, 0])
    g = q(rnd((N, HW, C), 63), dtype)
    n = x.numel()
    for act in ACTS:
        y, mean, rstd, dx = _poisoned(n, dtype), _poisoned(N * C), _poisoned(N * C), _poisoned(n, dtype)
        ops.instnorm_fwd(dtype, _d(x, dtype), N, HW, C, EPS, act, y[:n], mean[:N * C], rstd[:N * C])
        ops.instnorm_bwd(dtype, _d(g, dtype), _d(x, dtype), N, HW, C, act, mean[:N * C], rstd[:N * C], dx[:n])
        torch.cuda.synchronize()
        got_y, got_m, got_r = _written(y, n, "y"), _written(mean, N * C, "mean"), _written(rstd, N * C, "rstd")
        _written(dx, n, "dx")
        tag = f"instnorm constant {cq} {_t(dtype)} HW {HW} act {act}"
        _within(got_y, torch.zeros(n), 2.0 ** -23 * abs(cq) / math.sqrt(EPS), f"{tag} y")
        _within(got_m, torch.full((N * C,), cq), 2.0 ** -23 * abs(cq), f"{tag} mean")
        assert float(got_r.max()) <= 1.0001 / math.sqrt(EPS)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("HW", [63, 4096])
def test_instnorm_offset(pai, HW, dtype):
    """Plane mean = 10 standard deviations.  The rstd bound is derived a priori from the ONE-PASS formula var = E[x^2] - E[x]^2
    with fp32 per-lane sums of n = ceil(HW / 32) terms: the lane sums of x and of x^2 carry relative errors of at most
    d1 <= n u and d2 <= (n + 1) u (n - 1 additions resp. n fmas in sequence, one rounding of the lane total to fp32; the fp64
    combination of the lanes adds nothing at this level).  var_hat - var = d2 E[x^2] - 2 d1 mean^2 at most in magnitude
    (n + 1) u (E[x^2] + 2 mean^2) <= 3 (n + 1) u (mean^2 + var), so the relative error of var is at most
    3 (n + 1) u kappa with the condition number kappa = (mean^2 + var) / var, and that of rstd = (var + eps)^-1/2 at most half
    of it: 1.5 (n + 1) u kappa, on top of the 1e-5 bar every rstd has.  (HW = 4096, kappa = 101: 1.2e-3.)  The kernel sums
    x - pivot instead, twice (pivot = pixel 0, then the mean of that sweep), for which the same derivation holds with
    kappa ~ 1: it stays far inside; tests/test_step_refs_host.py runs both forms in the kernel's summation order on the host.  The mean keeps its
    absolute-term bound; y is referenced from the mean / rstd the kernel stored (each checked on its own): at |x| = 10 sigma
    an admissible 1e-5 relative error of the mean alone would move y by 1e-4."""
    rng = np.random.default_rng(5)
    x = q(torch.from_numpy((10.0 + rng.standard_normal((3, HW, 24))).astype(np.float32)), dtype)
    st = R.instnorm_fwd(x, EPS, R.ACT_NONE)
    assert float((st["mean"] / torch.sqrt(st["var"])).min()) > 8
    lim = R.instnorm_offset_rstd_bound(st["mean"], st["var"], HW)
    print(f"instnorm offset HW {HW}: a-priori rstd bound {float(lim.min()):.3g} .. {float(lim.max()):.3g}")
    _instnorm(x, q(rnd((3, HW, 24), 64), dtype), dtype, [R.ACT_LRELU], f"instnorm offset {_t(dtype)} HW {HW}", rstd_lim=lim,
              y_from_stored_stats=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("HW", [63, 4096])
def test_instnorm_outlier_pivot(pai, HW, dtype):
    """The worst plane for sums shifted by the first pixel: pixel 0 lies 100 standard deviations off the rest (x ~ N(0.5, 1),
    x[0] = 100.5).  With pixel 0 as the only pivot the sums of x - pivot have kappa = 1 + (pivot - mean)^2 / var ~ 2900 at
    HW = 4096 and the fp32 emulation of that order misses the mean bar (1.16 of 1e-5 mean |x|; rstd 3.8e-4 relative:
    tests/test_step_refs_host.py).  The kernel's second statistics sweep, around the mean of the first, has kappa ~ 1:
    mean, rstd, y and dx are held to the ordinary bars of test_instnorm."""
    rng = np.random.default_rng(6)
    x = torch.from_numpy((0.5 + rng.standard_normal((3, HW, 24))).astype(np.float32))
    x[:, 0, :] = 100.5
    _instnorm(q(x, dtype), q(rnd((3, HW, 24), 65), dtype), dtype, [R.ACT_LRELU], f"instnorm outlier pivot {_t(dtype)} HW {HW}")


# ---- generic BatchNorm backward -------------------------------------------------------------------------------------------------
BN_SHAPES = [(M, C) for C in (8, 64, 2048, 4096) for M in (1, 63, 64, 65, 129)] + [(2048 * 64 + 1, 8)]


def _bn_reduce_check(dtype, M, C, rows, rpb, du_buf, du_ref, part, sums, dgb, dgb0, z, mean, rstd, tag):
    """du (when stored) elementwise, then every partial row, sums, dgamma / dbeta (+=) from du AS STORED."""
    n = M * C
    if du_buf is not None:
        du_used = _written(du_buf, n, f"{tag} du").view(M, C)
        _elem_ok(du_used, du_ref, dtype, f"{tag} du")
    else:
        du_used = du_ref
    pr, ab = R.bn_bwd_partials(du_used, z, mean, rstd, rows, rpb)
    got_p = _written(part, rows * 2 * C, f"{tag} partials").view(rows, 2, C)
    _sum_ok(got_p, pr, ab, f"{tag} partial rows")
    empty = [b for b in range(rows) if b * rpb >= M]
    if empty:
        assert float(got_p[empty].abs().max()) == 0.0, f"{tag}: a block without rows left a non-zero partial"
    tot, tab = pr.sum(0), ab.sum(0)
    _sum_ok(_written(sums, 2 * C, f"{tag} sums").view(2, C), tot, tab, f"{tag} sums")
    if dgb is not None:
        got = _written(dgb, 2 * C, f"{tag} dgamma / dbeta").view(2, C)          # [0] dgamma += sums[1], [1] dbeta += sums[0]
        want = dgb0.double().view(2, C) + torch.stack([tot[1], tot[0]])
        _sum_ok(got, want, torch.stack([tab[1], tab[0]]), f"{tag} dgamma / dbeta (+=)", extra=R.U * want.abs())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,C", BN_SHAPES, ids=lambda v: str(v))
def test_bn_bwd(pai, M, C, dtype):
    """bn_bwd_reduce (one consumer; two: LeakyReLU + ReLU; du == g1 without a store), bn_bwd_reduce_affine (with and without a
    stored du), bn_bwd_apply, bn_bwd_apply_affine on the generic kernels: C = 8 (256 row lanes), 64, 2048 (1 row lane), 4096 (two
    passes over the channel groups); M = 1, 63, 64, 65, 129 and 2048 * 64 + 1 at C = 8, where blocks 2017 .. 2047 own no
    row and must write zero partials.  Activation arguments of exactly +0 / -0 in row 0."""
    ops = _ops()
    n = M * C
    rows = ops.bn_bwd_partial_rows(M)
    assert rows == min(2048, max(1, (M + 63) // 64))
    rpb = (M + rows - 1) // rows
    z, g1, g2 = q(rnd((M, C), 71) * 1.5 + 0.3, dtype), q(rnd((M, C), 72), dtype), q(rnd((M, C), 73), dtype)
    z[0, :C // 2], z[0, C // 2:] = 0.0, -0.0
    gamma, beta = 1 + 0.1 * rnd((C,), 74), 0.1 * rnd((C,), 75)
    zd = z.double()
    mean = zd.mean(0).float()
    rstd = (1.0 / torch.sqrt(((zd - zd.mean(0)) ** 2).mean(0) + EPS)).float()
    scale = (gamma * rstd).float()
    shift = (beta - mean * scale).float()
    shift[:2] = 0.0                                     # pre-activation of exactly 0 in row 0 (z = +-0)
    pre = R.bn_pre(z, scale, shift)
    a = q(R.act_fwd(pre, R.ACT_LRELU).float(), dtype)   # the stored activation: carries the sign of the pre-activation
    a[0, :C // 2], a[0, C // 2:] = 0.0, -0.0
    Z, G1, G2, A = (_d(t, dtype) for t in (z, g1, g2, a))
    MEAN, RSTD, SCALE, SHIFT, GAMMA = (_d(t) for t in (mean, rstd, scale, shift, gamma))
    dgb0 = rnd((2 * C,), 76)
    tag0 = f"bn_bwd {_t(dtype)} M {M} C {C}"

    def stored(t):      # du as the kernel forms it when it is not stored: the fp32 product rounded to the storage type
        return t.float().to(dtype).double()

    def bufs(with_du=True, with_dgb=True):
        dgb = None
        if with_dgb:
            dgb = _poisoned(2 * C)
            dgb[:2 * C] = dgb0.to(dev())
        return (_poisoned(n, dtype) if with_du else None), _poisoned(rows * 2 * C), _poisoned(2 * C), dgb

    with _generic_kernels():
        # -- pai_bn_bwd_reduce: one consumer, two consumers, du == g1
        for act1, g2h, G2d, act2, what in ((R.ACT_LRELU, None, None, 0, "reduce 1 consumer"),
                                          (R.ACT_LRELU, g2, G2, R.ACT_RELU, "reduce 2 consumers")):
            du, part, sums, dgb = bufs()
            ops.bn_bwd_reduce(dtype, G1, act1, G2d, act2, A, Z, M, C, MEAN, RSTD, du[:n], part[:rows * 2 * C], sums[:2 * C],
                              dgb[:C], dgb[C:2 * C])
            torch.cuda.synchronize()
            _bn_reduce_check(dtype, M, C, rows, rpb, du, R.bn_du(g1, act1, g2h, act2, a), part, sums, dgb, dgb0, z, mean, rstd,
                             f"{tag0} {what}")
        du, part, sums, dgb = bufs(with_du=False, with_dgb=False)
        ops.bn_bwd_reduce(dtype, G1, 0, None, 0, None, Z, M, C, MEAN, RSTD, None, part[:rows * 2 * C], sums[:2 * C], None, None)
        torch.cuda.synchronize()
        _bn_reduce_check(dtype, M, C, rows, rpb, None, g1.double(), part, sums, None, dgb0, z, mean, rstd, f"{tag0} reduce du == g1")
        # -- pai_bn_bwd_reduce_affine: the sign from z * scale + shift; with a stored du (two consumers) and without
        du, part, sums, dgb = bufs()
        ops.bn_bwd_reduce_affine(dtype, G1, R.ACT_RELU, G2, R.ACT_LRELU, Z, M, C, SCALE, SHIFT, MEAN, RSTD, du[:n],
                                 part[:rows * 2 * C], sums[:2 * C], dgb[:C], dgb[C:2 * C])
        torch.cuda.synchronize()
        _bn_reduce_check(dtype, M, C, rows, rpb, du, R.bn_du(g1, R.ACT_RELU, g2, R.ACT_LRELU, pre), part, sums, dgb, dgb0, z, mean,
                         rstd, f"{tag0} reduce_affine 2 consumers")
        du, part, sums, dgb = bufs(with_du=False)
        ops.bn_bwd_reduce_affine(dtype, G1, R.ACT_LRELU, None, 0, Z, M, C, SCALE, SHIFT, MEAN, RSTD, None, part[:rows * 2 * C],
                                 sums[:2 * C], dgb[:C], dgb[C:2 * C])
        torch.cuda.synchronize()
        du_a = stored(R.bn_du(g1, R.ACT_LRELU, None, 0, pre))
        _bn_reduce_check(dtype, M, C, rows, rpb, None, du_a, part, sums, dgb, dgb0, z, mean, rstd, f"{tag0} reduce_affine du not stored")
        # -- pass 2, from sums handed in (the fp32 casts of the reference totals)
        pr, _ = R.bn_bwd_partials(du_a, z, mean, rstd, rows, rpb)
        sums_h = pr.sum(0).float()
        SUMS = _d(sums_h.reshape(-1))
        for gm_h, gm_d in ((gamma, GAMMA), (None, None)):
            dz = _poisoned(n, dtype)
            ops.bn_bwd_apply(dtype, G2, Z, M, C, MEAN, RSTD, gm_d, SUMS, dz[:n])
            torch.cuda.synchronize()
            _elem_ok(_written(dz, n, "dz"), R.bn_bwd_apply(g2, z, mean, rstd, gm_h, sums_h), dtype,
                     f"{tag0} apply{'' if gm_h is not None else ' (no gamma)'}")
        dz = _poisoned(n, dtype)
        ops.bn_bwd_apply_affine(dtype, G1, R.ACT_LRELU, Z, M, C, SCALE, SHIFT, MEAN, RSTD, GAMMA, SUMS, dz[:n])
        torch.cuda.synchronize()
        _elem_ok(_written(dz, n, "dz"), R.bn_bwd_apply(du_a, z, mean, rstd, gamma, sums_h), dtype, f"{tag0} apply_affine")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,C", [(1, 8), (65, 64), (129, 2048)], ids=lambda v: str(v))
def test_bn2_bwd(pai, M, C, dtype):
    """bn2_bwd_reduce / bn2_bwd_apply on their small-tensor route (the one-branch kernels, twice): the residual branch with its
    ReLU (sign from za * scale_a + shift_a, du not stored) and the skip branch read the same gradient d."""
    ops = _ops()
    n = M * C
    rows = ops.bn_bwd_partial_rows(M)
    rpb = (M + rows - 1) // rows
    d, za, zb = q(rnd((M, C), 81), dtype), q(rnd((M, C), 82) * 1.5 + 0.3, dtype), q(rnd((M, C), 83) * 0.7 - 0.2, dtype)
    ga, gb = 1 + 0.1 * rnd((C,), 84), 1 + 0.1 * rnd((C,), 85)

    def stats(z):
        zd = z.double()
        return zd.mean(0).float(), (1.0 / torch.sqrt(((zd - zd.mean(0)) ** 2).mean(0) + EPS)).float()

    (mean_a, rstd_a), (mean_b, rstd_b) = stats(za), stats(zb)
    scale_a = (ga * rstd_a).float()
    shift_a = (0.1 - mean_a * scale_a).float()
    Dd, ZA, ZB = (_d(t, dtype) for t in (d, za, zb))
    dv = [_d(t) for t in (scale_a, shift_a, mean_a, rstd_a, mean_b, rstd_b, ga, gb)]
    SC, SH, MA, RA, MB, RB, GA, GB = dv
    tag = f"bn2_bwd {_t(dtype)} M {M} C {C}"
    du_a = R.bn_du(d, R.ACT_RELU, None, 0, R.bn_pre(za, scale_a, shift_a)).float().to(dtype).double()   # as the kernel forms it
    with _generic_kernels():
        pa, pb, sa, sb = _poisoned(rows * 2 * C), _poisoned(rows * 2 * C), _poisoned(2 * C), _poisoned(2 * C)
        ops.bn2_bwd_reduce(dtype, Dd, R.ACT_RELU, ZA, ZB, M, C, SC, SH, MA, RA, MB, RB, pa[:rows * 2 * C], pb[:rows * 2 * C],
                           sa[:2 * C], sb[:2 * C])
        torch.cuda.synchronize()
        _bn_reduce_check(dtype, M, C, rows, rpb, None, du_a, pa, sa, None, None, za, mean_a, rstd_a, f"{tag} branch a")
        _bn_reduce_check(dtype, M, C, rows, rpb, None, d.double(), pb, sb, None, None, zb, mean_b, rstd_b, f"{tag} branch b")
        sa_h = R.bn_bwd_partials(du_a, za, mean_a, rstd_a, rows, rpb)[0].sum(0).float()
        sb_h = R.bn_bwd_partials(d, zb, mean_b, rstd_b, rows, rpb)[0].sum(0).float()
        dza, dzb = _poisoned(n, dtype), _poisoned(n, dtype)
        ops.bn2_bwd_apply(dtype, Dd, R.ACT_RELU, ZA, ZB, M, C, SC, SH, MA, RA, GA, _d(sa_h.reshape(-1)), MB, RB, GB,
                          _d(sb_h.reshape(-1)), dza[:n], dzb[:n])
        torch.cuda.synchronize()
        _elem_ok(_written(dza, n, "dza"), R.bn_bwd_apply(du_a, za, mean_a, rstd_a, ga, sa_h), dtype, f"{tag} dza")
        _elem_ok(_written(dzb, n, "dzb"), R.bn_bwd_apply(d, zb, mean_b, rstd_b, gb, sb_h), dtype, f"{tag} dzb")


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _cast_data(numel, src_dtype, seed):
    sp = R.cast_specials()
    v = torch.cat([sp, rnd((max(numel - sp.numel(), 0),), seed) * 3.0])[:numel] if numel > 1 else torch.tensor([0.3], dtype=torch.float32)
    return v.to(src_dtype)


@pytest.mark.parametrize("dst_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("src_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("numel", [1, 1000, 4096 * 1024 + 5])
def test_cast(pai, numel, src_dtype, dst_dtype):
    """All four dtype pairs in bits against tensor.to(dtype): ties to even both ways, NaN, +-inf, 3.4e38 (rounds to inf in
    bf16), subnormals, -0; one element, 1000, and past the 4096-block grid."""
    ops = _ops()
    src = _cast_data(numel, src_dtype, 91)
    dst = _poisoned(numel, dst_dtype)
    ops.cast(src.to(dev()), dst[:numel])
    torch.cuda.synchronize()
    _bits_ok(dst, numel, src.to(dst_dtype), f"cast {_t(src_dtype)} -> {_t(dst_dtype)} n {numel}")


@pytest.mark.parametrize("dst_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("src_dtype", DTYPES, ids=IDS)
def test_cast_multi(pai, src_dtype, dst_dtype):
    """Eight tensors of unequal size in one launch (one past the 1024-block grid of 8-element vectors); the wrapper's fallback
    to single casts for nine pairs and for a pair that is not 16-byte aligned."""
    ops = _ops()
    sizes = [8, 16, 8 * 1000, 8 * (256 * 1024 + 3), 24, 8 * 37, 4096, 8 * 513]

    def run(sizes, lead=0):
        srcs = [_cast_data(n, src_dtype, 92 + i) for i, n in enumerate(sizes)]
        dsts = [_guarded(torch.zeros(n), dst_dtype, lead=lead) for n in sizes]
        for full, view in dsts:
            view.fill_(NAN)
        ops.cast_multi([(s.to(dev()), view) for s, (_, view) in zip(srcs, dsts)])
        torch.cuda.synchronize()
        for i, (s, (full, view)) in enumerate(zip(srcs, dsts)):
            _guard_ok(full, s.numel(), f"cast_multi[{i}]", lead)
            assert R.same_bits(view.cpu(), s.to(dst_dtype)), (i, s.numel())

    run(sizes)
    run(sizes + [40])           # nine pairs
    run([8, 16, 1001], lead=1)   # destinations one element off 16-byte alignment, one size no multiple of 8


def test_zero_multi(pai):
    """97 tensors (launches of 96 and 1), one past 256 * 1024 elements (the grid-stride loop), one of 0 elements."""
    ops = _ops()
    sizes = [1 + (53 * i) % 211 for i in range(97)]
    sizes[3], sizes[10], sizes[96] = 256 * 1024 + 3, 0, 77
    bufs = [_guarded(rnd((n,), 95 + i) if n else torch.zeros(0)) for i, n in enumerate(sizes)]
    ops.zero_multi([v for _, v in bufs])
    torch.cuda.synchronize()
    for i, (full, view) in enumerate(bufs):
        _guard_ok(full, sizes[i], f"zero_multi[{i}]")
        assert int(torch.count_nonzero(view)) == 0 and not bool(torch.signbit(view).any()), i


@pytest.mark.parametrize("weight", [1.0 - 0.999, 0.0, 1.0, 0.37])
def test_lerp_multi(pai, weight):
    """49 segments (launches of 48 and 1), one past 2048 * 1024 elements, one unaligned: torch_ema's three roundings in bits."""
    ops = _ops()
    sizes = [1 + (29 * i) % 173 for i in range(49)]
    sizes[5], sizes[48] = 2048 * 1024 + 5, 333
    w32 = float(np.float32(weight))
    host = [(rnd((n,), 300 + i), rnd((n,), 400 + i) * 0.9 + 0.1) for i, n in enumerate(sizes)]
    bufs = [(_guarded(sh, lead=1 if i == 7 else 0), _d(p)) for i, (sh, p) in enumerate(host)]
    ops.lerp_multi([(view.data_ptr(), P.data_ptr(), view.numel()) for (_, view), P in bufs], weight)
    torch.cuda.synchronize()
    for i, (((full, view), P), (sh, p)) in enumerate(zip(bufs, host)):
        _guard_ok(full, sizes[i], f"lerp_multi[{i}]", 1 if i == 7 else 0)
        assert torch.equal(P.cpu(), p)
        assert R.same_bits(view.cpu(), R.ema(sh, p, w32)), (i, sizes[i])


@pytest.mark.parametrize("n", [1, 3, 4, 7, 4096 * 1024 * 4 + 6])
def test_scale(pai, n):
    """x *= f: whole vectors, a tail of 1 .. 3 elements, no vector at all, past the 4096-block grid; one rounding: torch's bits."""
    ops = _ops()
    x = rnd((n,), 97)
    full, view = _guarded(x)
    ops.scale_(view, 1.0 / 3.0)
    torch.cuda.synchronize()
    _bits_ok(full, n, x * torch.tensor(1.0 / 3.0, dtype=torch.float32), f"scale_ n {n}")


def test_scale_refuses_an_unaligned_view(pai):
    ops = _ops()
    full, view = _guarded(rnd((9,), 98), lead=1)
    with pytest.raises(ops.PaiError, match="aligned"):
        ops.scale_(view, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(view.cpu(), rnd((9,), 98))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [8, 72])
def test_dropout2d(pai, C, dtype):
    """N = 3, HW = 5: the mask holds 0 and 1 / (1 - p); a NaN under a zero mask entry stays NaN (0 * NaN, as torch)."""
    ops = _ops()
    N, HW, p = 3, 5, 0.25
    g = torch.Generator().manual_seed(7)
    mask = (torch.bernoulli(torch.full((N, C), 1 - p), generator=g) / (1 - p)).float()
    mask[0, 0], mask[1, 1] = 0.0, 1 / (1 - p)
    x = q(rnd((N, HW, C), 99), dtype)
    x[0, 2, 0] = x[1, 3, 1] = NAN
    x[2, 0, 0] = INF
    n = x.numel()
    out = _poisoned(n, dtype)
    ops.dropout2d(dtype, _d(x, dtype), _d(mask), N, HW, C, out[:n])
    torch.cuda.synchronize()
    want = R.dropout2d(x.to(dtype), mask)
    assert math.isnan(float(want[0, 2, 0])) and math.isnan(float(want[1, 3, 1]))
    _bits_ok(out, n, want.reshape(-1), f"dropout2d {_t(dtype)} C {C}")


PACK_SHAPES = [(24, 9, 7), (1, 16, 64), (64, 16, 64), (192, 4, 64), (65, 1, 33)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_pack_weights(pai, shape, dtype):
    """(Cout, taps, Cin): the 32 x 32 tile kernel with ragged tiles either way and the 64 x 64 bf16 kernel; both packs, the
    forward pack alone, the input-gradient pack alone -- in bits against w.to(dtype) and its [Cin][taps][Cout] permutation."""
    ops = _ops()
    Cout, taps, Cin = shape
    w = rnd(shape, 101)
    w.view(-1)[:3] = torch.tensor([-0.0, 1.00390625, 3.4e38])      # a bf16 tie and an overflow to inf among the weights
    n = w.numel()
    ref_f, ref_d = R.pack_weights(w, dtype)
    W = _d(w)
    for with_f, with_d in ((True, True), (True, False), (False, True)):
        wf, wd = _poisoned(n, dtype), _poisoned(n, dtype)
        ops.pack_weights(dtype, W, Cout, taps, Cin, wf[:n] if with_f else None, wd[:n] if with_d else None)
        torch.cuda.synchronize()
        tag = f"pack_weights {_t(dtype)} {shape} fwd {with_f} dgrad {with_d}"
        if with_f:
            _bits_ok(wf, n, ref_f.reshape(-1), f"{tag} forward")
        else:
            assert bool(torch.isnan(wf).all())
        if with_d:
            _bits_ok(wd, n, ref_d.reshape(-1), f"{tag} input-gradient")
        else:
            assert bool(torch.isnan(wd).all())
