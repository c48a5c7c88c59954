"""CPU: the 256-entry colour table behind the report's device rendering (``PF.afmhot_lut_u8``) indexed with
``min(int(x * 256), 255)`` gives the bytes of the host path (report.output_hot_image: matplotlib's ``afmhot`` on the float
image, then ``to_int``) -- on a random image, at 0, 1, the neighbours of every bin edge k / 256, a subnormal and NaN."""
import numpy as np
import torch


def host_hot_bytes(img: np.ndarray) -> np.ndarray:
    """report.output_hot_image's arithmetic for a float32 [H, W] image: uint8 [3, H, W]."""
    from matplotlib import colormaps
    from thesis_pai_reconstruction_amd.models.utils import to_int
    with np.errstate(invalid="ignore"):
        rgb = colormaps["afmhot"](img[None])[0, :, :, :3]
    return to_int(torch.tensor(rgb, dtype=torch.float32).permute(2, 0, 1)).numpy()


def lut_hot_bytes(lut: torch.Tensor, img: np.ndarray) -> np.ndarray:
    """The device kernel's lookup, restated in fp32 on the host: uint8 [3, H, W]."""
    x = img.astype(np.float32)
    with np.errstate(invalid="ignore"):
        idx = np.minimum((x * np.float32(256.0)).astype(np.int64), 255)
    idx = np.clip(idx, 0, 255)
    out = lut.numpy()[idx]                      # [H, W, 3]
    out[np.isnan(x)] = 0
    return np.transpose(out, (2, 0, 1))


def edge_values() -> np.ndarray:
    one = np.float32(1.0)
    vals = [np.float32(0.0), one, np.nextafter(one, np.float32(0.0)), np.float32(1.0) - np.float32(2.0 ** -24),
            np.float32(2.0 ** -149)]
    for k in range(1, 257):
        e = np.float32(k / 256.0)
        vals += [np.nextafter(e, np.float32(0.0)), e]
        if k < 256:
            vals.append(np.nextafter(e, np.float32(2.0)))
    return np.array(vals, dtype=np.float32)


def test_afmhot_table_reproduces_host_rendering(pai):
    from thesis_pai_reconstruction_amd import functional as PF
    lut = PF.afmhot_lut_u8()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and not lut.is_cuda
    assert PF.afmhot_lut_u8() is lut                      # built once
    rng = np.random.default_rng(11)
    img = rng.random((256, 256), dtype=np.float32)
    assert np.array_equal(lut_hot_bytes(lut, img), host_hot_bytes(img))
    edges = edge_values()
    pad = (-edges.size) % 32
    grid = np.concatenate([edges, np.zeros(pad, np.float32)]).reshape(-1, 32)
    assert np.array_equal(lut_hot_bytes(lut, grid), host_hot_bytes(grid))


def test_afmhot_nan_is_black(pai):
    from thesis_pai_reconstruction_amd import functional as PF
    img = np.full((4, 8), 0.5, dtype=np.float32)
    img[1, 3] = np.nan
    want = host_hot_bytes(img)
    assert tuple(want[:, 1, 3]) == (0, 0, 0)
    assert np.array_equal(lut_hot_bytes(PF.afmhot_lut_u8(), img), want)


def test_eval_entry_points_refuse_cpu_tensors(pai):
    """No CPU fallback: the evaluation entry points raise on host tensors, and the kernel has a symbol."""
    import pytest
    from thesis_pai_reconstruction_amd import functional as PF, ops
    assert ops.eval_kernel_name(0)
    x = torch.zeros(1, 1, 32, 32)
    with pytest.raises(pai.PaiError):
        PF.eval_images(x, x)
    with pytest.raises(pai.PaiError):
        ops.eval_planes(x, x, 1, 32, 32, 0, ssim_plane=torch.zeros(1, dtype=torch.float64))
