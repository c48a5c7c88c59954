"""CPU: the fp64 reference of the differentiable spatial attention (tests/_sattn_ref.py) against the fixture of the reference's
own QKVAttentionLegacy + autograd.grad (tests/golden/ref_sattn_grad.npz, scripts/gen_sattn_grad_golden.py) and against torch's
double autograd of the restated formula; the three entry points of ABI 138 in header, ctypes table and library; the host-side
kernel-name query; and the margins of the integer lane-map constructions that tests/test_gpu_sattn_bwd.py runs."""
import math
import os
import re

import pytest
import torch

import _sattn_ref as R
from oracle import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pai_sattn_fwd_lse", "pai_sattn_bwd", "pai_sattn_kernel_name")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def fix(golden_dir):
    return golden.load(golden_dir, "ref_sattn_grad")


def _case(fix, c):
    n, t, heads, ch = (int(v) for v in fix[f"shape{c}"])
    g = lambda k: torch.from_numpy(fix[f"{k}{c}"])
    return (n, t, heads, ch), g("qkv"), g("dout"), g("out"), g("dqkv")


@pytest.mark.parametrize("c", [0, 1, 2])
def test_ref_equals_the_reference_autograd(fix, c):
    """_sattn_ref.backward with the exact fp64 out / lse is the reference module's autograd.grad (fp64) to 1e-12."""
    (n, t, heads, ch), qkv, dout, out_f32, dqkv = _case(fix, c)
    assert (n, t, heads, ch) == [(1, 20, 2, 32), (2, 144, 4, 32), (1, 96, 1, 64)][c]
    assert torch.equal(qkv.bfloat16().float(), qkv) and torch.equal(dout.bfloat16().float(), dout)
    assert dqkv.dtype == torch.float64 and 0 < float(fix[f"bf16_dev{c}"]) < 0.05
    out, lse = R.forward(qkv, heads, ch)
    assert _rel(out, out_f32.double()) < 1e-6                  # the fixture stores the fp64 forward as fp32
    ref = R.backward(dout, qkv, out, lse, heads, ch)
    assert _rel(ref["dqkv"], dqkv) <= 1e-12
    assert bool((ref["abs"] >= ref["dqkv"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("N,T,heads,ch", [(2, 37, 3, 32), (1, 50, 2, 64)])
def test_ref_equals_double_autograd(N, T, heads, ch):
    """The same against torch's double autograd of softmax(scale2 q k^T) v written out here."""
    gen = torch.Generator().manual_seed(T)
    qkv = torch.randn(N, T, heads * 3 * ch, generator=gen, dtype=torch.float64) * 1.5
    dout = torch.randn(N, T, heads * ch, generator=gen, dtype=torch.float64)
    x = qkv.clone().requires_grad_(True)
    v = x.view(N, T, heads, 3, ch)
    w = torch.softmax(torch.einsum("nihc,njhc->nhij", v[:, :, :, 0], v[:, :, :, 1]) / math.sqrt(ch), dim=-1)
    y = torch.einsum("nhij,njhc->nihc", w, v[:, :, :, 2]).reshape(N, T, heads * ch)
    (g,) = torch.autograd.grad(y, x, dout)
    out, lse = R.forward(qkv, heads, ch)
    assert _rel(out, y.detach()) <= 1e-12
    ref = R.backward(dout, qkv, out, lse, heads, ch)
    assert _rel(ref["dqkv"], g) <= 1e-12
    assert _rel(ref["p"], w.detach()) <= 1e-12
    # C bounds what dP - delta can lose: it dominates |dS| carried through the same products
    assert bool((ref["cancel"][..., :heads * 3 * ch] + 1e-300 >= 0).all())
    cq = ref["cancel"].view(N, T, heads, 3, ch)
    aq = ref["abs"].view(N, T, heads, 3, ch)
    assert bool((cq[:, :, :, :2] >= aq[:, :, :, :2] * (1 - 1e-12)).all()) and float(cq[:, :, :, 2].abs().max()) == 0


def test_new_entry_points_in_header_table_and_library(pai):
    src = open(os.path.join(ROOT, "include", "pai_hip.h")).read()
    decl = set(re.findall(r"\b(pai_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = pai.lib.load()
    for name in NEW:
        assert name in decl, f"{name} is not declared in pai_hip.h"
        assert name in pai.lib.SIGNATURES, f"{name} is not in lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} is not exported by libpai_hip.so"
    assert lib.pai_version() >= 138
    from thesis_pai_reconstruction_amd import functional as PF
    assert callable(PF.spatial_attention)


def test_sattn_kernel_selection_without_gpu(pai):
    """pai_sattn_kernel_name is host logic and reads the selection the launchers branch on."""
    from thesis_pai_reconstruction_amd import ops
    bf, f32 = torch.bfloat16, torch.float32
    for ch in (32, 64, 128, 256):
        assert ops.sattn_kernel_name(bf, ch, 0) == f"sattn_bf16_k<{ch}>"
        kvb = 16 if ch == 256 else 32
        assert ops.sattn_kernel_name(f32, ch, 0) == f"sattn_f32_k<{ch}, {kvb}>"
        assert ops.sattn_kernel_name(f32, ch, 1) == (f"sattn_bwd_delta_k<float, {ch}>+sattn_bwd_f32_k<{ch}, {kvb}, true>+"
                                                      f"sattn_bwd_f32_k<{ch}, {kvb}, false>")
    for ch in (32, 64, 128):
        assert ops.sattn_kernel_name(bf, ch, 1) == (f"sattn_bwd_delta_k<unsigned short, {ch}>+sattn_bwd_kv_bf16_k<{ch}>+"
                                                     f"sattn_bwd_q_bf16_k<{ch}>")
    with pytest.raises(ops.PaiError, match="ch=48"):
        ops.sattn_kernel_name(bf, 48, 0)
    with pytest.raises(ops.PaiError, match="op 2"):
        ops.sattn_kernel_name(bf, 64, 2)


def test_bf16_backward_at_256_channels_is_refused_by_name(pai):
    from thesis_pai_reconstruction_amd import ops
    with pytest.raises(ops.PaiError, match="ch=256 has no bf16 backward"):
        ops.sattn_kernel_name(torch.bfloat16, 256, 1)
    assert ops.sattn_kernel_name(torch.bfloat16, 256, 0) == "sattn_bf16_k<256>"       # the forward stays


def test_public_function_refuses_host_tensors(pai):
    from thesis_pai_reconstruction_amd import functional as PF
    with pytest.raises(pai.PaiError, match="device"):
        PF.spatial_attention(torch.zeros(1, 8, 96), 1)


@pytest.mark.parametrize("paired", [False, True], ids=["onehot", "paired"])
@pytest.mark.parametrize("N,T,heads,ch", [(1, 64, 1, 32), (1, 160, 2, 64)], ids=lambda v: str(v))
def test_lane_map_constructions_have_their_margins(N, T, heads, ch, paired):
    """The integer data of tests/test_gpu_sattn_bwd.py::test_lane_maps: bf16-exact inputs, one-hot (paired: 1/2, 1/2)
    probabilities to 1e-9, whole- or half-number outputs and gradients that differ from row to row."""
    qkv, dout = R.lane_map_data(N, T, heads, ch, paired)
    assert torch.equal(qkv.bfloat16().float(), qkv) and torch.equal(dout.bfloat16().float(), dout)
    out, lse = R.forward(qkv, heads, ch)
    ref = R.backward(dout, qkv, out, lse, heads, ch)
    p = ref["p"]
    assert float((p.max(-1).values - (0.5 if paired else 1.0)).abs().max()) < 1e-9
    assert float((p.sum(-1) - 1).abs().max()) < 1e-9
    # the winner is sigma(i) (and its partner)
    win = p.argmax(-1)
    want = torch.tensor([(7 * i + 2) % T for i in range(T)])
    assert bool(((win // 2 == want // 2) if paired else (win == want)).all())
    assert float((out - out.round()).abs().max()) < 1e-6 and float(out.abs().max()) <= 256
    assert torch.equal(out.round().bfloat16().double(), out.round())
    g = ref["dqkv"].view(N, T, heads, 3, ch)
    dq, dk, dv = (g[:, :, :, k] for k in range(3))
    scale2 = 1 / math.sqrt(ch)
    assert float(dv.abs().max()) >= 1 and float((2 * dv - (2 * dv).round()).abs().max()) < 1e-6
    assert int((dv.abs().sum(-1) > 0.5).sum()) >= N * T * heads * 3 // 4
    if paired:
        # dS = +- 1/4 (dP_a - dP_b), a quarter of a whole number times 16 scale2 in dQ / dK, exact in bf16 before the last rounding
        for t in (dq, dk):
            u = t / (4 * scale2)
            assert float((u - u.round()).abs().max()) < 1e-6 and float(t.abs().max()) >= 1
        assert int((dq.abs().sum(-1) > 0.5).sum()) >= N * T * heads // 2      # most query rows carry a non-zero dS
        ds_bits = (dk / (16 * scale2)).abs().max()
        assert float(ds_bits) < 64, "dS = k / 4 with |k| < 256 is exact in bf16"
    else:
        assert float(dq.abs().max()) < 1e-9 and float(dk.abs().max()) < 1e-9  # dS vanishes
