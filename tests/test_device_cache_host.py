"""Host logic of the device-resident data set (dataset.aa_tables / epoch_indices / the data modules' cache switch): the
index order is DistributedSampler's, the filter tables reproduce aten's antialiased bilinear resize byte for byte, a cache
that exceeds its budget leaves the host loader in place and nothing is cached by default.  CPU only."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.data.distributed import DistributedSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_pairs(tmp_path, n, size=32, seed=0):
    from PIL import Image
    import yaml
    rng = np.random.default_rng(seed)
    os.makedirs(tmp_path / "img", exist_ok=True)
    items = []
    for i in range(n):
        for kind in ("in", "gt"):
            Image.fromarray(rng.integers(0, 256, (size, size), dtype=np.uint8), mode="L").save(
                tmp_path / "img" / f"{kind}_{i:03d}.png")
        items.append({"input": f"img/in_{i:03d}.png", "ground_truth": f"img/gt_{i:03d}.png"})
    with open(tmp_path / "list.yaml", "w") as f:
        yaml.safe_dump(items, f)
    return tmp_path / "list.yaml"


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("shuffle", [True, False])
def test_epoch_indices_are_distributed_samplers(pai, world, shuffle):
    """n = 11 does not divide by 2, 3 or 4: the wrap-around case of test_sharded_loader_partitions_the_list."""
    from thesis_pai_reconstruction_amd.dataset import epoch_indices
    n, seed = 11, 5
    for epoch in (0, 3):
        for rank in range(world):
            sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
                                         drop_last=False)
            sampler.set_epoch(epoch)
            assert epoch_indices(n, world, rank, seed, epoch, shuffle) == list(sampler), (world, rank, epoch)
    # more ranks than samples: the pad wraps around more than once
    for rank in range(5):
        sampler = DistributedSampler(range(2), num_replicas=5, rank=rank, shuffle=shuffle, seed=1, drop_last=False)
        sampler.set_epoch(2)
        assert epoch_indices(2, 5, rank, 1, 2, shuffle) == list(sampler)


def _pass(img, out_size):
    """One separable pass along the last axis with the tables of aa_tables: first term a product, every later term a
    fused multiply-add (an fp64 product-and-add rounded to fp32 once: exact products of a byte-derived fp32 value and an
    fp32 weight fit fp64, and so does their sum with an fp32 accumulator up to one rounding far below the fp32 one)."""
    from thesis_pai_reconstruction_amd.dataset import aa_tables
    in_size = img.shape[-1]
    if in_size == out_size:
        return img
    bounds, weights = (t.numpy() for t in aa_tables(in_size, out_size))
    assert bounds.dtype == np.int32 and weights.dtype == np.float32 and weights.shape[0] == out_size
    out = np.zeros(img.shape[:-1] + (out_size,), np.float32)
    for i in range(out_size):
        x0, taps = int(bounds[i, 0]), int(bounds[i, 1])
        assert 0 <= x0 and taps >= 1 and x0 + taps <= in_size and taps <= weights.shape[1]
        t = img[..., x0] * weights[i, 0]
        for j in range(1, taps):
            t = (t.astype(np.float64) + img[..., x0 + j].astype(np.float64) * np.float64(weights[i, j])).astype(np.float32)
        out[..., i] = t
    return out


@pytest.mark.parametrize("shape", [(512, 512), (300, 400), (128, 128), (257, 255)])
def test_aa_tables_reproduce_the_host_resize_bytes(pai, shape):
    """The shapes and the image recipe of test_resize_matches_antialiased_bilinear; W pass first, then H, fp32 in between."""
    rng = np.random.default_rng(7)
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    img = (127 + 80 * np.sin(yy / 7.0) * np.cos(xx / 5.0) + rng.normal(0, 20, (h, w))).clip(0, 255).astype(np.uint8)
    a = _pass(img.astype(np.float32), 256)
    a = _pass(np.ascontiguousarray(a.T), 256).T
    got = torch.from_numpy(np.ascontiguousarray(a)).round().to(torch.uint8)
    ref = F.interpolate(torch.from_numpy(img)[None, None].float(), size=(256, 256), mode="bilinear", antialias=True,
                        align_corners=False).round().to(torch.uint8)[0, 0]
    assert int((got != ref).sum()) == 0


def test_value_table_is_the_loader_expression(pai):
    from thesis_pai_reconstruction_amd.dataset import value_table
    b = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    assert torch.equal(value_table(True), b.to(torch.float32).div_(255) * 2 - 1)
    assert torch.equal(value_table(False), b.to(torch.float32).div_(255))


def test_budget_fallback_keeps_the_host_loader(pai, tmp_path, capsys):
    from thesis_pai_reconstruction_amd.dataset import ImageDataModule, ShardedLoader, SyntheticDataModule
    lst = _write_pairs(tmp_path, 3)
    dm = ImageDataModule(str(lst), str(lst), batch_size=2, world=1, rank=0, device_cache=True, cache_budget_bytes=1)
    dm.setup("fit")
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "host loader" in out                 # one line, nothing else changes
    assert dm.caches == {}
    for ld in (dm.train_dataloader(), dm.val_dataloader()):
        assert isinstance(ld, ShardedLoader)
    x, t = next(iter(dm.val_dataloader()))
    assert not x.is_cuda and tuple(x.shape) == (2, 1, 256, 256)
    sm = SyntheticDataModule(n_train=4, n_val=2, batch_size=2, size=16, world=1, rank=0, device_cache=True,
                             cache_budget_bytes=1)
    sm.setup("fit")
    assert sm.on_device == {} and isinstance(sm.train_dataloader(), ShardedLoader)


def test_no_cache_by_default(pai, tmp_path, monkeypatch):
    from thesis_pai_reconstruction_amd import dataset
    from thesis_pai_reconstruction_amd.dataset import ImageDataModule, ShardedLoader

    def boom(*a, **k):
        raise AssertionError("a DeviceImageCache was built without device_cache=True")
    monkeypatch.setattr(dataset.DeviceImageCache, "__init__", boom)
    lst = _write_pairs(tmp_path, 3)
    dm = ImageDataModule(str(lst), str(lst), batch_size=2, world=1, rank=0)
    for stage in ("fit", "validate", "test", "predict"):
        dm.setup(stage)
    assert dm.device_cache is False and dm.caches == {}
    for ld in (dm.train_dataloader(), dm.val_dataloader(), dm.test_dataloader(), dm.predict_dataloader()):
        assert isinstance(ld, ShardedLoader)
