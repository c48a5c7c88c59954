"""GPU: the report's device evaluation (PF.eval_images / ops.eval_planes, csrc/eval.hip + the kernel in csrc/ssim.hip).

Against the oracle (oracle/metrics_ref.py, pinned to scikit-image) with the bounds tests/test_gpu_ops.py uses for the same
quantities, and against the device / host path the report used before: per-image metric calls, ``to_int`` of the fp32 SSIM
map, matplotlib's afmhot on the host.

Bound of the uint8 SSIM map against the oracle: the fp32 maps agree within 2e-5 (tests/test_gpu_ops.py), which is 0.005 of
one of the 255.999 levels, so the truncation can move a value by one level at most; how many pixels sit that close to a
level is not bounded."""
import numpy as np
import pytest
import torch

import oracle
from _gpu_util import dev
from oracle.metrics_ref import depth_ssim as oracle_depth_ssim

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1, 256, 256), (3, 1, 96, 200), (2, 3, 67, 131)]
STRIPS = {(5, 1, 256, 256): 16, (3, 1, 96, 200): 4, (2, 3, 67, 131): 0}      # 96 / 16 = 6 rows: below the window


def _pair(shape):
    """test_gpu_ops.test_ssim_psnr_rmse's inputs, plus planes that hold exact 0 and exact 1."""
    rng = np.random.default_rng(shape[2])
    a = torch.from_numpy(rng.random(shape, dtype=np.float32))
    b = torch.clamp(a + 0.1 * torch.from_numpy(rng.standard_normal(shape).astype(np.float32)), 0, 1)
    a[0, 0, : shape[2] // 2] = 0.0                  # half a plane of exact zeros, then exact ones
    a[0, 0, shape[2] // 2:] = 1.0
    b[-1, -1, :, : shape[3] // 3] = 1.0
    b[-1, -1, :, shape[3] // 3: 2 * (shape[3] // 3)] = 0.0
    return a, b


def _to_int(x):
    from thesis_pai_reconstruction_amd.models.utils import to_int
    return to_int(x)


def _host_hot(img):
    """The host rendering the report used before (matplotlib, then to_int): float [H, W] in [0, 1] -> uint8 [3, H, W]."""
    from matplotlib import colormaps
    rgb = colormaps["afmhot"](img.numpy()[None])[0, :, :, :3]
    return _to_int(torch.tensor(rgb, dtype=torch.float32).permute(2, 0, 1))


def _kernel_named(ops):
    name = ops.eval_kernel_name(0)
    assert name == "eval_planes_k"
    return name


def _check(PF, pred, target, denorm):
    """pred / target: host tensors as they go INTO eval_images; returns nothing, asserts everything."""
    shape = tuple(pred.shape)
    n, c, h, w = shape
    strips = STRIPS.get(shape, 0)        # other callers' shapes (tests/test_gpu_ssim_paths.py): whole images only
    dp, dt = (oracle.denormalize(pred), oracle.denormalize(target)) if denorm else (pred, target)
    P, T = pred.to(dev()), target.to(dev())
    res = PF.eval_images(P, T, denorm=denorm, strips=strips, ssim_map=True, hot=True)
    torch.cuda.synchronize()

    # ---- oracle ----
    per, full = oracle.ssim_full(dp, dt)
    got = res.ssim.cpu()
    print("ssim max abs diff", float((got - per).abs().max()))
    assert got.dtype == torch.float32 and float((got - per).abs().max()) < 5e-6
    assert torch.equal(torch.argsort(got), torch.argsort(per))
    for i in range(n):
        want_psnr = float(oracle.psnr(dp[i:i + 1], dt[i:i + 1]))
        want_mse = float(oracle.mse(dp[i:i + 1].double(), dt[i:i + 1].double()))
        print("image", i, "psnr", float(res.psnr[i]), want_psnr, "mse", float(res.mse[i]), want_mse)
        assert abs(float(res.psnr[i]) - want_psnr) < 2e-5
        assert abs(float(res.mse[i]) - want_mse) <= 1e-6 * want_mse
    if strips:
        tab = res.strip_ssim.cpu()
        assert tuple(tab.shape) == (n, strips)
        want = oracle_depth_ssim(dp, dt, strips)             # [strips, 2]: mean and std over the images
        print("strip mean / std diff", float((tab.mean(0) - want[:, 0]).abs().max()), float((tab.std(0) - want[:, 1]).abs().max()))
        assert float((tab.mean(0) - want[:, 0]).abs().max()) < 5e-6
        assert float((tab.std(0) - want[:, 1]).abs().max()) < 5e-6
        for k, (xp, xt) in enumerate(zip(dp.chunk(strips, dim=2), dt.chunk(strips, dim=2))):
            assert float((tab[:, k] - oracle.ssim_full(xp, xt)[0]).abs().max()) < 5e-6
    else:
        assert res.strip_ssim is None
    m8 = res.ssim_map_u8.cpu()
    assert m8.dtype == torch.uint8 and tuple(m8.shape) == shape
    dlevel = (m8.int() - _to_int(full.clamp(0, 1)).int()).abs()
    print("u8 map vs oracle: max level diff", int(dlevel.max()), "pixels differing", int((dlevel > 0).sum()))
    assert int(dlevel.max()) <= 1

    # ---- the path the report used before ----
    DP, DT = (PF.denormalize(P), PF.denormalize(T)) if denorm else (P, T)
    s_old, full_old = PF.ssim_per_image(DP, DT, return_full_image=True)
    assert torch.equal(m8, _to_int(full_old.clamp(0, 1)).cpu())
    psnr_old = torch.stack([PF.psnr(p[None], t[None]) for p, t in zip(DP, DT)]).cpu()
    mse_old = torch.stack([PF.rmse(p[None], t[None]) ** 2 for p, t in zip(DP, DT)]).cpu()
    for name, new, old in (("ssim", res.ssim.cpu(), s_old.cpu()), ("psnr", res.psnr.cpu(), psnr_old),
                           ("mse", res.mse.cpu(), mse_old)):
        rel = float(((new.double() - old.double()).abs() / old.double().abs()).max())
        print(name, "vs per-image calls: max rel diff", rel)
        assert rel <= 1e-6, name
    rmse_all = float(torch.sqrt(res.sse.sum() / dp.numel()).float())
    assert abs(rmse_all - float(PF.rmse(DP, DT))) <= 1e-6 * rmse_all
    if strips:
        for k, (xp, xt) in enumerate(zip(DP.chunk(strips, dim=2), DT.chunk(strips, dim=2))):
            old = PF.ssim_per_image(xp.contiguous(), xt.contiguous()).cpu()
            assert float(((res.strip_ssim[:, k].cpu() - old).abs() / old.abs()).max()) <= 1e-6
    hot = res.hot_u8.cpu()
    assert hot.dtype == torch.uint8 and tuple(hot.shape) == (n, c, 3, h, w)
    dpc = DP.cpu()
    for i in range(n):
        for ch in range(c):
            assert torch.equal(hot[i, ch], _host_hot(dpc[i, ch])), (i, ch)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_images_against_oracle_and_previous_path(pai, shape):
    from thesis_pai_reconstruction_amd import functional as PF, ops
    _kernel_named(ops)
    a, b = _pair(shape)
    _check(PF, b, a, denorm=False)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_images_fused_denormalisation(pai, shape):
    """Raw network range in, the clamp of models/utils.py:11 active on both sides."""
    from thesis_pai_reconstruction_amd import functional as PF, ops
    _kernel_named(ops)
    a, b = _pair(shape)
    _check(PF, b * 2.4 - 1.2, a * 2.4 - 1.2, denorm=True)


def test_eval_images_nan_renders_black_and_sums_accumulate(pai):
    from thesis_pai_reconstruction_amd import functional as PF, ops
    _kernel_named(ops)
    a, b = _pair((2, 1, 32, 48))
    b[1, 0, 7, 9] = float("nan")
    P, T = b.to(dev()), a.to(dev())
    res = PF.eval_images(P, T, hot=True)
    assert res.ssim_map_u8 is None and res.strip_ssim is None
    hot = res.hot_u8.cpu()
    assert tuple(hot[1, 0, :, 7, 9]) == (0, 0, 0)
    assert torch.equal(hot[0, 0], _host_hot(b[0, 0]))
    # the per-plane sums are +=: a second call on the same buffers doubles them
    acc = torch.zeros(2, 2, dtype=torch.float64, device=dev())
    for _ in range(2):
        ops.eval_planes(P[:1], T[:1], 1, 32, 48, 0, ssim_plane=acc[0, :1], sse_plane=acc[1, :1])
    one = PF.eval_images(P[:1], T[:1])
    assert abs(float(acc[1, 0]) - 2 * float(one.sse[0])) <= 1e-12 * float(acc[1, 0])
    assert abs(float(acc[0, 0]) / 2 - float(one.ssim[0])) < 1e-6 and float(acc[0, 1]) == 0.0


def test_eval_planes_refuses_bad_arguments(pai):
    from thesis_pai_reconstruction_amd import functional as PF, ops
    _kernel_named(ops)
    x = torch.zeros(2, 1, 32, 32)
    with pytest.raises(pai.PaiError):
        ops.eval_planes(x, x, 2, 32, 32, 0, ssim_plane=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(pai.PaiError):
        PF.eval_images(x, x)
    X = x.to(dev())
    with pytest.raises(pai.PaiError, match="11x11"):          # 96 / 16 = 6-row strips, as the per-strip loop before
        PF.eval_images(torch.zeros(1, 1, 96, 64, device=dev()), torch.zeros(1, 1, 96, 64, device=dev()), strips=16)
    with pytest.raises(pai.PaiError, match="multiple"):
        PF.eval_images(torch.zeros(1, 1, 67, 64, device=dev()), torch.zeros(1, 1, 67, 64, device=dev()), strips=16)
    with pytest.raises(pai.PaiError, match="no output"):
        ops.eval_planes(X, X, 2, 32, 32, 0)
    with pytest.raises(pai.PaiError, match="padded"):         # 3 bytes short of a whole word
        ops.eval_planes(torch.zeros(1, 1, 11, 13, device=dev()), torch.zeros(1, 1, 11, 13, device=dev()), 1, 11, 13, 0,
                        ssim_map_u8=torch.empty(143, dtype=torch.uint8, device=dev()))
    with pytest.raises(pai.PaiError, match="table"):
        ops.eval_planes(X, X, 2, 32, 32, 0, hot_u8=ops.padded_u8((2, 3, 32, 32), dev()))
