"""CPU: the fp64 reference of the train-mode FiLM norm (tests/_film_norm_ref.py) against torch's double autograd of
``F.batch_norm(training=True) * (1 + scale) + shift -> F.silu -> * mask * k`` and against the fixture of the reference's own
ResBlock in training (tests/golden/ref_film_norm.npz, scripts/gen_film_norm_golden.py), both to 1e-12; the CPU measurement the
fp32 SiLU / SiLU' bounds of tests/test_gpu_film_norm.py rest on, printed; the entry points of ABI 139 in header, ctypes table
and library with their host-side queries and refusals (every refusal comes before a launch, so it needs no GPU)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _film_norm_ref as R
from oracle import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pai_film_norm_fwd", "pai_film_norm_bwd", "pai_film_norm_ws_floats", "pai_film_norm_slabs")


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("film,act,masked", [(True, "silu", True), (False, "silu", False), (False, "none", False),
                                             (True, "silu", False), (True, "none", True)])
@pytest.mark.parametrize("N,rows,C", [(2, 1, 8), (3, 37, 16)])
def test_ref_equals_double_autograd(N, rows, C, film, act, masked):
    gen = torch.Generator().manual_seed(100 * rows + C)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, g, gamma, beta = rn(N, rows, C) * 1.5 + 0.7, rn(N, rows, C), 1 + 0.5 * rn(C), rn(C)
    emb = torch.cat([0.4 * rn(N, C), rn(N, C), rn(N, R.PAD)], 1) if film else None
    mask = (torch.rand(N, rows, C, generator=gen) >= R.P_DROP).to(torch.uint8) if masked else None
    k = R.KEEP if masked else 1.0
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    er = emb.clone().requires_grad_(True) if film else None
    v = F.batch_norm(xr.permute(0, 2, 1), None, None, gr, br, True, 0.1, R.EPS).permute(0, 2, 1)     # [N, C, rows] inside
    u = v * (1 + er[:, None, :C]) + er[:, None, C:2 * C] if film else v
    y = F.silu(u) if act == "silu" else u
    if masked:
        y = y * mask.double() * k
    grads = torch.autograd.grad(y, [xr, gr, br] + ([er] if film else []), g)
    mean, rstd = R.batch_stats(x)
    ref = R.backward(g, x, mean, rstd, gamma, beta, emb, mask, k, act)
    assert _rel(ref["y"], y.detach()) <= 1e-12
    assert _rel(ref["dx"], grads[0]) <= 1e-12 * max(1.0, float(ref["dx_T"].max() / ref["dx"].abs().max()))
    assert _rel(ref["dgamma"], grads[1]) <= 1e-12 and _rel(ref["dbeta"], grads[2]) <= 1e-12
    if film:
        assert _rel(ref["demb"], grads[3][:, :2 * C]) <= 1e-12 and bool((grads[3][:, 2 * C:] == 0).all())
    # the absolute sums bound their sums, T bounds dx
    for key in ("S0", "S1", "dbeta", "dgamma"):
        assert bool((ref[key + "_abs"] >= ref[key].abs() * (1 - 1e-12)).all())
    assert bool((ref["dx_T"] >= ref["dx"].abs() * (1 - 1e-12)).all())


@pytest.fixture(scope="module")
def fix(golden_dir):
    return golden.load(golden_dir, "ref_film_norm")


def test_ref_equals_the_reference_resblock(fix):
    """_film_norm_ref on the norm input, emb_out, gamma and beta the reference's train-mode ResBlock saw is its SiLU output and
    its autograd.grad (fp64) to 1e-12; the running statistics after the step are those of the batch statistics."""
    t = lambda k: torch.from_numpy(fix[k])
    N, rows, C = (int(v) for v in fix["shape"])
    assert (N, rows, C) == (3, 25, 16) and t("x").dtype == torch.float64 and t("x").shape == (N, rows, C)
    assert t("emb_out").shape == (N, 2 * C)
    eps, mom = float(fix["eps"]), float(fix["momentum"])
    mean, rstd = R.batch_stats(t("x"), eps)
    ref = R.backward(t("dout"), t("x"), mean, rstd, t("gamma"), t("beta"), t("emb_out"))
    for key in ("y", "dx", "demb", "dgamma", "dbeta"):
        assert _rel(ref[key], t(key)) <= 1e-12, key
        assert 0 < float(fix["bf16_dev_" + key]) < 0.02
    M = N * rows
    var = 1.0 / rstd ** 2 - eps
    assert _rel(mom * mean, t("running_mean")) <= 1e-12
    assert _rel((1 - mom) + mom * var * M / (M - 1), t("running_var")) <= 1e-12


def _cases(pai):
    from thesis_pai_reconstruction_amd import ops
    return R.cases(ops.film_norm_slabs)


def test_torch_fp32_silu_error_is_what_the_bounds_assume(pai):
    """The measurement behind SILU_TORCH_ERR / SILU_BWD_TORCH_ERR of tests/_film_norm_ref.py (the fp32 bounds of
    tests/test_gpu_film_norm.py are four times these): max |F.silu fp32 - fp64| and max |gradient - fp64| / |dy| of PyTorch-CPU's
    own op over the arguments of the largest GPU case, printed.  One-sided, as the GELU measurement of
    tests/test_vit_refs_host.py: the recorded constants must not undercut the reference's own error by more than 10 %."""
    largest = _cases(pai)[4]
    u, _ = R.silu_args(largest)
    assert float(u.max()) > 99 and float(u.min()) < -99 and bool((u == 0).any())           # the planted +-100 and 0
    assert float(((u.abs() > 4) & (u.abs() < 12)).double().mean()) > 0.02                   # and a spread up to 12
    e_fwd, e_bwd = R.torch_fp32_silu_error(largest)
    print(f"torch fp32 CPU silu: max err {e_fwd:.4g} (recorded {R.SILU_TORCH_ERR:.4g}); "
          f"gradient per |dy|: {e_bwd:.4g} (recorded {R.SILU_BWD_TORCH_ERR:.4g})")
    assert e_fwd <= 1.1 * R.SILU_TORCH_ERR and e_bwd <= 1.1 * R.SILU_BWD_TORCH_ERR


def test_case_data_is_what_the_gpu_tests_describe(pai):
    for N, rows, C in _cases(pai)[:4]:
        d = R.case_data(N, rows, C)
        mean, rstd = R.batch_stats(d["x"])
        assert float(rstd[0]) == pytest.approx(R.EPS ** -0.5, rel=1e-9)                        # the constant channel
        if N * rows >= 100:
            assert 2.5 < float((mean * rstd).abs()[4]) < 3.5                                  # a mean 3 standard deviations from 0
        assert bool(torch.isnan(d["emb"][:, 2 * C:]).all()) and d["emb"].shape == (N, 2 * C + R.PAD)
        assert d["mask"].dtype == torch.uint8 and set(d["mask"].unique().tolist()) <= {0, 1}


def test_abi_139_entries(pai):
    src = open(os.path.join(ROOT, "include", "pai_hip.h")).read()
    decl = set(re.findall(r"\b(pai_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = pai.lib.load()
    for name in NEW:
        assert name in decl and name in pai.lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pai_version() >= 139


def test_host_side_queries_and_refusals(pai):
    """Slab count and workspace size are host code; every refusal comes before a launch and never touches a pointer."""
    from thesis_pai_reconstruction_amd import ops
    assert [ops.film_norm_slabs(r) for r in (1, 64, 65, 300, 16384, 16385, 1 << 20)] == [1, 1, 2, 5, 256, 256, 256]
    rows = R.ragged_rows(ops.film_norm_slabs)
    slabs = ops.film_norm_slabs(rows)
    rps = -(-rows // slabs)
    assert slabs - -(-rows // rps) >= 2 and rows < (1 << 15)                                  # the last slabs own no row
    assert ops.film_norm_ws_floats(2, rows, 64) == 2 * slabs * 2 * 64 + 2 * 64
    lib = pai.lib.load()
    fake = ctypes.c_void_p(0x100000)          # aligned, never dereferenced: the calls below are refused before any launch
    F32, BF16, SILU = pai.lib.F32, pai.lib.BF16, pai.lib.ACT_SILU

    def fwd(dtype=F32, rows=4, N=2, C=16, emb=fake, ld=48, act=SILU):
        return lib.pai_film_norm_fwd(dtype, fake, rows, N, C, fake, fake, fake, fake, emb, ld, None, 1.0, act, fake, None)

    def bwd(dtype=F32, rows=4, N=2, C=16, emb=fake, ld=48, act=SILU):
        return lib.pai_film_norm_bwd(dtype, fake, fake, rows, N, C, fake, fake, fake, fake, emb, ld, None, 1.0, act, fake,
                                     fake, fake, fake, fake, None)

    for call in (fwd, bwd):
        for kw, word in ((dict(dtype=2), b"dtype"), (dict(C=12), b"multiple of 8"), (dict(C=2056), b"2048"), (dict(C=0), b"C=0"),
                         (dict(ld=31), b"ld=31"), (dict(act=pai.lib.ACT_RELU), b"act=2"), (dict(act=pai.lib.ACT_TANH), b"act=3"),
                         (dict(N=65536), b"65535"), (dict(rows=0), b"rows=0")):
            assert call(**kw) != 0, kw
            assert word in lib.pai_last_error(), (kw, lib.pai_last_error())
