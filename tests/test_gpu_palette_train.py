"""GPU: the train-mode pass of the Palette U-Net (``UNet.forward_train`` + backward) and the two kernels it adds, against
the reference's own training-mode forward + backward in fp64 (tests/golden/ref_palette_train_*.npz, recorded on the CPU by
scripts/gen_palette_train_golden.py with the weights of tests/_palette_util.py).

Kernels
  pai_avgpool2_bwd   bit-equal to 0.25 * dout at the four positions (the product is exact in both dtypes), dx pre-filled with NaN.
  pai_silu_bwd       against the fp64 formula on the same stored arguments.  fp32: the SiLU' bar of tests/_film_norm_ref.py
                     (four times the error PyTorch-CPU's own fp32 SiLU' was measured at) per unit |g|; bf16: that bar plus
                     2^-8 |ref| for the stored result.  Planted u = +-100, 0 and NaN; numel 1, 7 and 4099 for the ragged tails;
                     the aliased form gives the same bits.

U-Net (fp32 on a, b, c, d; bf16 on a and d: the reference under bf16 autocast is no yardstick for c -- 134 of 242 live gradients
past 0.125 -- nor for b, where attention at both levels puts 22 of 183 live gradients past 0.25, more than the 10 % the
generator tolerates; both are fp32-only fixtures)
  output, intermediates   fp32: 1e-4 of the largest value, the project's forward bound.  bf16 output: relative L2 at most twice
                          ``dev16_out``, the reference's own distance under autocast from fp64 (the factor 2: this path also stores
                          the activations in bf16); bf16 intermediates are printed, the reference records no yardstick for them.
  live gradients          fingerprint_close with rtol = max(1e-4, 4 * dev32) in fp32 -- dev32 bounds the reference's own summation
                          order only, the HIP path sums in others (slab sums, split K), hence 4 -- and 2 * dev16 in bf16; tensors
                          with dev16 > 0.25 (AttentionBlock norm.bias / qkv.bias) are printed, not bounded.
  dead gradients          the convolution biases in front of a BatchNorm: zero in exact arithmetic, rounding noise in any real
                          run.  L2 norm at most 4 x the noise norm the reference itself left there in the same precision.
  running statistics      after the forward and after the backward (the AttentionBlock norms advance twice): fp32 1e-5, bf16
                          2e-2, relative to max(1, |want|); num_batches_tracked exactly.
  dropout                 a_drop in fp32 with the recorded masks under the same bounds; one bf16 pass at p = 0.25 that draws its
                          own masks must give finite gradients.
  cache                   eval output after a training pass is bit-equal to that of a fresh model with the same state.
  no host synchronisation forward + backward under torch.cuda.set_sync_debug_mode("error") after one warm-up pass.
"""
import numpy as np
import pytest
import torch

import _film_norm_ref as R
import _palette_util as U
from _gpu_util import dev, max_err, rel_err
from oracle import golden
from oracle.fingerprint import fingerprint, fingerprint_close

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
IDS = ["fp32", "bf16"]
UNET_CASES = [("a", F32), ("b", F32), ("c", F32), ("d", F32), ("a", BF16), ("d", BF16)]
UNET_IDS = [f"{t}-{IDS[DTYPES.index(d)]}" for t, d in UNET_CASES]


@pytest.fixture(scope="module")
def recs(golden_dir):
    return {t: golden.load(golden_dir, f"ref_palette_train_{t}") for t in ("a", "b", "c", "d", "a_drop")}


# ---- pai_avgpool2_bwd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 4, 6, 8), (1, 2, 2, 264), (3, 6, 4, 136)])
def test_avgpool2_bwd(pai, shape, dtype):
    from thesis_pai_reconstruction_amd import nnops, ops
    N, H, W, C = shape                                   # of dx
    gen = torch.Generator().manual_seed(H * W + C)
    dout = torch.randn(N, H // 2, W // 2, C, generator=gen).to(dtype).to(dev())
    want = (dout.float() * 0.25).to(dtype).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(want.float(), (dout.float() * 0.25).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))   # exact
    dx = torch.full((N, H, W, C), float("nan"), dtype=dtype, device=dev())
    ops.avgpool2_bwd(dtype, dout, N, H, W, C, dx)
    assert torch.equal(dx, want)
    x = torch.randn(N, H, W, C, generator=gen).to(dtype).to(dev()).requires_grad_(True)
    y = nnops.AvgPool2.apply(x)
    ref = torch.empty_like(y)
    ops.avgpool2(dtype, x.detach(), N, H, W, C, ref)
    assert torch.equal(y.detach(), ref)
    y.backward(dout)
    assert torch.equal(x.grad, want)


# ---- pai_silu_bwd -----------------------------------------------------------------------------------------------------------------
PLANT = [100.0, -100.0, 0.0, float("nan")]


def _silu_case(numel, dtype, first):
    gen = torch.Generator().manual_seed(numel + first)
    u = 4.0 * torch.randn(numel, generator=gen)
    g = torch.randn(numel, generator=gen)
    where = list(range(min(numel, 4)))
    if numel > 4096:                                     # also in the ragged tail behind the last whole vector
        where += [numel - 4, numel - 3, numel - 2, numel - 1]
    for k, i in enumerate(where):
        u[i] = PLANT[(k + first) % 4]
    return u.to(dtype), g.to(dtype), where


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("numel", [1, 7, 4099])
def test_silu_bwd(pai, numel, dtype):
    from thesis_pai_reconstruction_amd import ops
    for first in (range(4) if numel == 1 else (0,)):     # one element: each planted value in turn
        u, g, where = _silu_case(numel, dtype, first)
        ref = g.double() * R.act_grad(u.double(), "silu")
        lim = R.SILU_BWD_BOUND * g.double().abs()
        if dtype == BF16:
            lim = lim + 2.0 ** -8 * ref.abs()
        ud, gd = u.to(dev()), g.to(dev())
        buf = torch.full((numel + 16,), float("nan"), dtype=dtype, device=dev())
        ops.silu_bwd(dtype, gd, ud, buf[:numel])
        got = buf[:numel].cpu()
        assert bool(torch.isnan(buf[numel:]).all()), "written past numel"
        nan = torch.isnan(u)
        assert bool(torch.isnan(got[nan]).all()) and bool(torch.isfinite(got[~nan]).all())
        err = (got.double() - ref)[~nan].abs()
        ratio = float((err / lim[~nan].clamp_min(1e-300)).max()) if err.numel() else 0.0
        print(f"silu_bwd {IDS[DTYPES.index(dtype)]} numel {numel} planted {[float(u[i]) for i in where]}: "
              f"max err / bound {ratio:.3f}")
        assert bool((err <= lim[~nan]).all())
        alias = gd.clone()
        ops.silu_bwd(dtype, alias, ud, alias)
        assert torch.equal(alias.cpu().view(torch.int16 if dtype == BF16 else torch.int32),
                           got.view(torch.int16 if dtype == BF16 else torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_silu_autograd(pai, dtype):
    """nnops.SiLU: the forward is pai_affine_act with unit coefficients, the backward pai_silu_bwd."""
    from thesis_pai_reconstruction_amd import nnops, ops
    gen = torch.Generator().manual_seed(3)
    u = (3.0 * torch.randn(3, 512, generator=gen)).to(dtype).to(dev()).requires_grad_(True)
    g = torch.randn(3, 512, generator=gen).to(dtype).to(dev())
    ones, zeros = torch.ones(512, device=dev()), torch.zeros(512, device=dev())
    y = nnops.SiLU.apply(u, ones, zeros)
    want = torch.empty_like(y)
    ops.affine_act(dtype, u.detach(), 1, 3, 512, ones, zeros, False, ops.ACT_SILU, want)
    assert torch.equal(y.detach(), want)
    y.backward(g)
    du = torch.empty_like(g)
    ops.silu_bwd(dtype, g, u.detach(), du)
    assert torch.equal(u.grad, du)


# ---- the U-Net ----------------------------------------------------------------------------------------------------------------------
def _bn_state(unet, names):
    mods = dict(unet.named_modules())
    return (torch.cat([mods[n].running_mean for n in names]).cpu().double().numpy(),
            torch.cat([mods[n].running_var for n in names]).cpu().double().numpy(),
            np.array([int(mods[n].num_batches_tracked) for n in names], np.int64))


def _model(pai, name, dtype, dropout=0.0):
    m = U.init_portable(pai.Palette(**dict(U.palette_kwargs(name), dropout=dropout)), U.CONFIGS[name][4]).to(dev())
    m.train()
    m.set_precision("32" if dtype == F32 else "bf16-mixed")
    return m


def _masks(rec):
    out = {}
    for k in rec:
        if k.startswith("mask:"):
            shape = tuple(int(v) for v in rec["mask_shape:" + k[5:]])
            bits = np.unpackbits(rec[k])[:int(np.prod(shape))]
            out[k[5:]] = torch.from_numpy(bits.reshape(shape)).to(dev())
    return out


_PASSES = {}


def _pass(pai, recs, tag, dtype):
    """One forward_train + backward of configuration ``tag`` (computed once per module run and shared by the tests below)."""
    key = (tag, dtype)
    if key not in _PASSES:
        rec = recs[tag]
        name = tag.split("_")[0]
        m = _model(pai, name, dtype, dropout=0.25 if tag.endswith("_drop") else 0.0)
        x, y = (t.to(dev()) for t in U.inputs(name))
        names = [str(n) for n in rec["bn_names"]]
        m.unet.debug_capture = cap = {}
        out = m.unet.forward_train(x, y, torch.from_numpy(rec["gammas"]).to(dev()),
                                   dropout_masks=_masks(rec) if tag.endswith("_drop") else None)
        m.unet.debug_capture = None
        assert out.dtype == F32 and out.requires_grad
        after_fwd = _bn_state(m.unet, names)
        out.backward(torch.from_numpy(rec["dout"]).to(dev()))
        after_bwd = _bn_state(m.unet, names)
        grads = {}
        for k, p in m.unet.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == F32, k
            grads[k] = p.grad.detach().cpu()
        _PASSES[key] = dict(out=out.detach().cpu(), cap={k: v.cpu() for k, v in cap.items()}, grads=grads, fwd=after_fwd,
                            bwd=after_bwd, first=U.first_modules(m.unet))
    return _PASSES[key]


def _check_output(rec, res, tag, dtype):
    want = torch.from_numpy(rec["out"])
    assert res["out"].shape == want.shape
    if dtype == F32:
        e = max_err(res["out"], want)
        print(f"palette train {tag} fp32 out: max err / max {e:.3e} (bound 1e-4)")
        assert e <= 1e-4
    else:
        e, yard = rel_err(res["out"], want), float(rec["dev16_out"])
        print(f"palette train {tag} bf16 out: rel L2 {e:.3e}, reference under autocast {yard:.3e}")
        assert e <= 2 * yard


def _check_grads(rec, res, tag, dtype):
    keys = [str(k) for k in rec["keys"]]
    assert list(res["grads"]) == keys
    prec = "32" if dtype == F32 else "16"
    worst = {"live": (0.0, ""), "dead": (0.0, "")}
    bad = []
    for k, d in zip(keys, rec["dead"]):
        got = res["grads"][k]
        assert bool(torch.isfinite(got).all()), k
        if d:
            noise = float(rec[f"noise{prec}:" + k])
            ratio = float(got.double().norm()) / (4 * noise)
            cls = "dead"
        else:
            dev_ = float(rec[f"dev{prec}:" + k])
            if dtype == BF16 and dev_ > 0.25:
                print(f"palette train {tag} bf16 {k}: rel L2 {rel_fp(got, rec['grad:' + k]):.3e}, reference under autocast "
                      f"{dev_:.3e} (not bounded)")
                continue
            rtol = max(1e-4, 4 * dev_) if dtype == F32 else 2 * dev_
            ok, ratio = fingerprint_close(fingerprint(got), rec["grad:" + k], rtol)
            cls = "live"
        if ratio > worst[cls][0]:
            worst[cls] = (ratio, k)
        if ratio > 1:
            bad.append((k, cls, round(ratio, 3)))
    for cls, (ratio, k) in worst.items():
        print(f"palette train {tag} {IDS[DTYPES.index(dtype)]} {cls} gradients: largest error / bound {ratio:.3f} ({k})")
    assert not bad, bad


def rel_fp(got, want_fp):
    """Relative distance of the L2 norms: what a fingerprint allows for a tensor that is printed, not bounded."""
    return abs(float(got.double().norm()) - float(want_fp[0])) / float(want_fp[0])


def _check_stats(rec, res, tag, dtype):
    tol = 1e-5 if dtype == F32 else 2e-2
    for when in ("fwd", "bwd"):
        mean, var, nbt = res[when]
        assert np.array_equal(nbt, rec[f"bn_nbt_{when}"]), (when, nbt, rec[f"bn_nbt_{when}"])
        for k, got in (("mean", mean), ("var", var)):
            want = rec[f"bn_{k}_{when}"]
            e = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
            print(f"palette train {tag} {IDS[DTYPES.index(dtype)]} running_{k} after {when}: {e:.3e} (bound {tol:.0e})")
            assert e <= tol, (when, k)


@pytest.mark.parametrize("tag,dtype", UNET_CASES, ids=UNET_IDS)
def test_output_and_intermediates(pai, recs, tag, dtype):
    rec, res = recs[tag], _pass(pai, recs, tag, dtype)
    for key in res["first"]:
        e = max_err(res["cap"][key][:, ::U.CROP], torch.from_numpy(rec["act:" + key]))
        print(f"palette train {tag} {IDS[DTYPES.index(dtype)]} {key}: max err / max {e:.3e}")
        if dtype == F32:
            assert e <= 1e-4, key
    _check_output(rec, res, tag, dtype)


@pytest.mark.parametrize("tag,dtype", UNET_CASES, ids=UNET_IDS)
def test_parameter_gradients(pai, recs, tag, dtype):
    _check_grads(recs[tag], _pass(pai, recs, tag, dtype), tag, dtype)


@pytest.mark.parametrize("tag,dtype", UNET_CASES, ids=UNET_IDS)
def test_running_statistics(pai, recs, tag, dtype):
    _check_stats(recs[tag], _pass(pai, recs, tag, dtype), tag, dtype)


def test_dropout_with_fed_masks(pai, recs):
    rec, res = recs["a_drop"], _pass(pai, recs, "a_drop", F32)
    _check_output(rec, res, "a_drop", F32)
    _check_grads(rec, res, "a_drop", F32)
    _check_stats(rec, res, "a_drop", F32)


def test_dropout_draws_its_own_masks_bf16(pai, recs):
    m = _model(pai, "a", BF16, dropout=0.25)
    x, y = (t.to(dev()) for t in U.inputs("a"))
    g = torch.from_numpy(U.GAMMAS[0]).to(dev())
    out = m.unet.forward_train(x, y, g)
    out.backward(torch.from_numpy(recs["a"]["dout"]).to(dev()))
    assert bool(torch.isfinite(out).all())
    for k, p in m.unet.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    # the masks are drawn: a second pass differs from the first by far more than rounding
    out2 = m.unet.forward_train(x, y, g)
    assert rel_err(out2.detach(), out.detach()) > 1e-2


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eval_cache_is_dropped(pai, recs, dtype):
    """The running statistics advance through raw pointers (no version counter moves): the eval coefficients cached before a
    training pass must not be served after it."""
    m = _model(pai, "a", dtype)
    x, y = (t.to(dev()) for t in U.inputs("a"))
    g = torch.from_numpy(U.GAMMAS[0]).to(dev())
    m.eval()
    before = m.unet(x, y, g).clone()                    # fills the cache
    m.train()
    m.unet.forward_train(x, y, g).backward(torch.from_numpy(recs["a"]["dout"]).to(dev()))
    m.eval()
    after = m.unet(x, y, g)
    fresh = pai.Palette(**U.palette_kwargs("a")).to(dev())
    fresh.load_state_dict(m.state_dict())
    fresh.eval()
    fresh.set_precision("32" if dtype == F32 else "bf16-mixed")
    want = fresh.unet(x, y, g)
    assert torch.equal(after, want)
    assert not torch.equal(after, before)


def test_no_host_synchronisation(pai, recs):
    m = _model(pai, "a", BF16, dropout=0.25)
    x, y = (t.to(dev()) for t in U.inputs("a"))
    g = torch.from_numpy(U.GAMMAS[0]).to(dev())
    dout = torch.from_numpy(recs["a"]["dout"]).to(dev())
    m.unet.forward_train(x, y, g).backward(dout)        # warm-up: workspaces, streams, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.unet.forward_train(x, y, g).backward(dout)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.unet.parameters())
