"""CPU: the fp64 references of tests/_bn_ref.py against PyTorch's own double-precision ops -- F.batch_norm in train mode with
running statistics called n_updates times and in eval mode, F.relu / F.leaky_relu with NaN, +-inf and +-0 -- and the fp32
emulation of bn_finalize_k's arithmetic against the reference, inside the bounds tests/test_gpu_bn_fwd.py holds the kernels
to: the bounds can be seen to hold for the arithmetic alone (fp64 sums in another order, every fp32 rounding, the multiply-adds
contracted and not), before any kernel is involved.  Run with -s for the emulation's largest error in units of u x terms."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn_ref as B

D64 = torch.float64
EPS = 1e-5


def _tensor_and_partials(M, C, R, seed):
    """A double tensor [M][C] and its exact partial rows: sums / sums of squares of R row slabs, kept in fp64 here (the
    reference takes what it is handed; fp32 rows are the kernels' case)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g, dtype=D64) * (0.5 + torch.rand(C, generator=g, dtype=D64)) + torch.randn(C, generator=g, dtype=D64)
    slabs = torch.tensor_split(x, R, dim=0)
    p = torch.stack([torch.stack([s.sum(0), (s * s).sum(0)]) for s in slabs])
    return x, p


@pytest.mark.parametrize("n_updates", [0, 1, 2, 3])
@pytest.mark.parametrize("M,C,R", [(2, 3, 1), (3, 8, 2), (64, 5, 7), (500, 16, 33)])
def test_finalize_is_batch_norm_in_train_mode(M, C, R, n_updates):
    x, p = _tensor_and_partials(M, C, R, 10 + M)
    g = torch.Generator().manual_seed(3)
    gamma, beta = torch.rand(C, generator=g, dtype=D64) + 0.5, torch.randn(C, generator=g, dtype=D64)
    rm0, rv0 = torch.randn(C, generator=g, dtype=D64), torch.rand(C, generator=g, dtype=D64) + 0.5
    mom = 0.25          # exact in fp32, so is 1 - 0.25: the fp32 constants of the reference are torch's doubles
    ref = B.finalize(p, M, gamma, beta, EPS, mom, n_updates, rm0, rv0)
    rm, rv = rm0.clone(), rv0.clone()
    y = None
    for _ in range(max(n_updates, 1)):
        y = F.batch_norm(x, rm if n_updates else None, rv if n_updates else None, gamma, beta, True, mom, B.f32c(EPS))
    got = B.apply(x, ref["scale"], ref["shift"], B.ACT_NONE)["out"]
    assert torch.allclose(got, y, rtol=1e-11, atol=1e-11)
    assert torch.allclose(ref["mean"], x.mean(0), rtol=1e-12, atol=1e-13)
    assert torch.allclose(ref["var"], x.var(0, unbiased=False), rtol=1e-10, atol=1e-13)
    assert torch.allclose(ref["rm"], rm, rtol=1e-12, atol=1e-13) and torch.allclose(ref["rv"], rv, rtol=1e-10, atol=1e-13)
    if n_updates == 0:
        assert torch.equal(ref["rm"], rm0) and torch.equal(ref["rv"], rv0)
    # gamma / beta None: the plain normalisation
    ref0 = B.finalize(p, M, None, None, EPS, mom, 0, None, None)
    y0 = F.batch_norm(x, None, None, None, None, True, mom, B.f32c(EPS))
    assert torch.allclose(B.apply(x, ref0["scale"], ref0["shift"], B.ACT_NONE)["out"], y0, rtol=1e-11, atol=1e-11)
    assert "rm" not in ref0


def test_finalize_constants_and_clamp():
    """momentum 0.1 is not an fp32 number: the reference uses float32(0.1) and 1.f - float32(0.1) formed in fp32; a variance
    that comes out below zero is 0; count 1 uses the biased variance for the running one."""
    assert B.one_minus_f32(0.1) == float(np.float32(1.0) - np.float32(0.1)) != 1.0 - B.f32c(0.1)
    p = torch.tensor([[[2.0, 3.0], [1.9, 4.5]]], dtype=torch.float32)         # mean (1, 1.5), Q / count (0.95, 2.25): var -0.05 -> 0, and 0
    ref = B.finalize(p, 2, None, None, EPS, 0.1, 1, torch.zeros(2), torch.ones(2))
    assert torch.equal(ref["var"], torch.zeros(2, dtype=D64))
    assert torch.allclose(ref["rstd"], torch.full((2,), 1.0 / np.sqrt(B.f32c(EPS)), dtype=D64), rtol=1e-15)
    assert torch.allclose(ref["rv"], torch.full((2,), B.one_minus_f32(0.1), dtype=D64), rtol=1e-15)
    assert torch.allclose(ref["rm"], B.f32c(0.1) * torch.tensor([1.0, 1.5], dtype=D64), rtol=1e-15)
    one = B.finalize(torch.tensor([[[3.0], [10.0]]]), 1, None, None, EPS, 0.5, 1, torch.zeros(1), torch.zeros(1))
    assert float(one["unbiased"]) == 1.0 and float(one["rv"]) == 0.5
    nan = B.finalize(torch.tensor([[[float("nan"), 1.0], [1.0, 2.0]]]), 4, None, None, EPS, 0.1, 1, torch.zeros(2), torch.ones(2))
    for k in ("mean", "rstd", "scale", "shift", "rm", "rv"):
        assert bool(torch.isnan(nan[k][0])) and bool(torch.isfinite(nan[k][1])), k


@pytest.mark.parametrize("affine", [True, False])
def test_eval_coeffs_is_batch_norm_in_eval_mode(affine):
    g = torch.Generator().manual_seed(5)
    C = 9
    x = torch.randn(20, C, generator=g, dtype=D64)
    gamma, beta = (torch.rand(C, generator=g, dtype=D64) + 0.5, torch.randn(C, generator=g, dtype=D64)) if affine else (None, None)
    rm, rv = torch.randn(C, generator=g, dtype=D64), torch.rand(C, generator=g, dtype=D64)
    rv[0], rv[1] = 0.0, 1e-12                        # eps is the whole denominator
    co = B.eval_coeffs(gamma, beta, rm, rv, EPS)
    y = F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, B.f32c(EPS))
    assert torch.allclose(B.apply(x, co["scale"], co["shift"], B.ACT_NONE)["out"], y, rtol=1e-11, atol=1e-9)


def test_activations_are_atens():
    nan, inf = float("nan"), float("inf")
    v = torch.tensor([nan, -inf, inf, 0.0, -0.0, -1.5, 2.5, -1e-30, 1e-30], dtype=D64)
    for a, fn in ((B.ACT_RELU, F.relu), (B.ACT_LRELU, lambda t: F.leaky_relu(t, B.SLOPE)), (B.ACT_NONE, lambda t: t)):
        got, want = B.act(v, a), fn(v)
        assert torch.equal(torch.isnan(got), torch.isnan(want)), a
        assert torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)]), a
    assert bool(torch.isnan(B.act(v, B.ACT_RELU)[0])) and float(B.act(v, B.ACT_RELU)[1]) == 0.0
    # the residual tail: a NaN in either branch comes out under every pair of activations
    za, zb = torch.tensor([[nan, 1.0, -1.0]], dtype=D64), torch.tensor([[1.0, nan, -1.0]], dtype=D64)
    one, zero = torch.ones(3, dtype=D64), torch.zeros(3, dtype=D64)
    for aa in (B.ACT_NONE, B.ACT_RELU, B.ACT_LRELU):
        for a in (B.ACT_NONE, B.ACT_RELU, B.ACT_LRELU):
            for sb, hb in ((None, None), (one, zero)):
                o = B.bn2_add_act(za, one, zero, zb, sb, hb, aa, a)["out"]
                assert torch.isnan(o).tolist() == [[True, True, False]], (aa, a)
    o = B.bn2_add_act(torch.tensor([[-3.0, 2.0]]), torch.ones(2), torch.zeros(2), torch.tensor([[1.0, -5.0]]), 2 * torch.ones(2),
                      torch.ones(2), B.ACT_RELU, B.ACT_LRELU)["out"]
    assert torch.allclose(o, torch.tensor([[3.0, B.SLOPE * (2.0 - 9.0)]], dtype=D64))


# derived rounding counts (docstring of tests/test_gpu_bn_fwd.py), in units of u x the absolute terms.  The bars are twice these,
# except shift: its bar of 6 u was set for a count of 3 (fl(mean), the product, the subtraction), which leaves out the two
# roundings scale brings along -- 5 in all (4 contracted), 3.1 measured here -- and still holds.
DERIVED = {"mean": 1.0, "rstd": 1.0, "scale": 2.0, "shift": 5.0}


def test_finalize_emulation_stays_inside_the_bounds():
    """bn_finalize_k's arithmetic emulated in fp32 (another fp64 summation order, every rounding, contracted and not) against
    the fp64 reference, over the data kinds and counts of the GPU test: every output inside its derived bound, hence inside
    the bar (twice that).  Prints the largest error in units of u x terms per output."""
    worst = {}
    g = torch.Generator().manual_seed(11)
    for R, C, count in ((1, 130, 2), (3, 65, 3), (16, 130, 64), (17, 65, 4096), (129, 130, 129 * 128), (1025, 65, 4096), (2049, 9, 2049 * 128)):
        for kind in ("normal", "mixed"):
            p = B.make_partials(R, C, count, 1000 + R, kind)
            gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
            rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
            for n in (0, 1, 2, 3):
                ref = B.finalize(p, count, gamma, beta, EPS, 0.1, n, rm0, rv0)
                assert float(ref["amplification"].max()) < 1e6
                lim = B.finalize_bounds(ref, n)
                for contract in (False, True):
                    em = B.finalize_f32_emulation(p, count, gamma, beta, EPS, 0.1, n, rm0, rv0, contract)
                    terms = {"mean": ref["mean"].abs(), "rstd": ref["rstd"].abs(), "scale": ref["scale"].abs(),
                             "shift": ref["shift_abs"], "rm": ref["rm_abs"], "rv": ref["rv_abs"]}
                    for k in ("mean", "rstd", "scale", "shift", "rm", "rv"):
                        err = (em[k].double() - ref[k]).abs()
                        assert bool((err <= lim[k]).all()), (k, R, count, kind, n, contract, float((err - lim[k]).max()))
                        if n == 0 and k in ("rm", "rv"):
                            assert torch.equal(em[k], (rm0 if k == "rm" else rv0)), k
                            continue
                        units = float((err / (B.U * terms[k]).clamp_min(1e-300)).max())
                        key = f"{k}[n={n}]" if k in ("rm", "rv") else k
                        worst[key] = max(worst.get(key, 0.0), units)
                        derived = 1.5 * n if k in ("rm", "rv") else DERIVED[k]
                        assert units <= derived, (key, units, derived, R, count, kind, contract)
    for k in sorted(worst):
        print(f"finalize emulation, {k}: largest error {worst[k]:.3g} u x terms")


def test_emulation_sees_the_faults_the_bars_are_for():
    """The bars separate the kernel's arithmetic from the faults of the mutation record: the biased variance in the running
    update at count 4096, one update too few, and a missing clamp all leave their bars by a wide margin."""
    R, C, count, n = 17, 65, 4096, 2
    p = B.make_partials(R, C, count, 7, "normal")
    rm0, rv0 = torch.zeros(C), torch.ones(C)
    ref = B.finalize(p, count, None, None, EPS, 0.1, n, rm0, rv0)
    lim = B.finalize_bounds(ref, n)
    omm, mom = B.one_minus_f32(0.1), B.f32c(0.1)
    rv_biased = rv0.double()
    for _ in range(n):
        rv_biased = omm * rv_biased + mom * ref["var"]
    assert bool(((rv_biased - ref["rv"]).abs() > 20 * lim["rv"]).all())           # var / 4095 x 0.19 against 6 u (1 + var)
    one_less = B.finalize(p, count, None, None, EPS, 0.1, n - 1, rm0, rv0)
    assert bool(((one_less["rv"] - ref["rv"]).abs() > lim["rv"]).any()) and bool(((one_less["rm"] - ref["rm"]).abs() > lim["rm"]).any())
    pc = B.make_partials(R, C, count, 8, "constant")
    refc = B.finalize(pc, count, None, None, EPS, 0.1, 1, rm0, rv0)
    raw = pc.double()[:, 1].sum(0) / count - refc["mean"] ** 2
    assert bool((raw < 0).any()) and bool((raw > 0).any()), "the constant channels must reach the clamp from both sides"
