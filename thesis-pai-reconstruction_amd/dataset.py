"""Data modules: the reference's YAML-listed image pairs (reference dataset.py:11-134) and the
synthetic pairs used by the benchmark.

Reference defect handled here: dataset.py:58 normalises 1-channel images with
3-tuples, which cannot broadcast; this module normalises with (0.5,)/(0.5,), i.e. x*2-1.

Opt-in device-resident path (``device_cache=True``): every file is decoded ONCE, resized on the GPU (csrc/data.hip,
byte-identical to ``load_gray_256``) and kept in HBM as uint8; a batch is one gather launch (``DeviceLoader``).  The
default loaders are unchanged.
"""
from __future__ import annotations

import functools
import math
import os
from typing import Optional

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

from .lightning import LightningDataModule


def load_gray_256(path: str, size: int = 256, normalize: bool = True) -> torch.Tensor:
    """read_image(GRAY) -> Resize((256,256), antialias=True) on uint8 -> float32/255 -> [-1,1]
    (reference dataset.py:51-59,129-132).  The resize is the reference's own operator: torchvision 0.15 casts the
    uint8 tensor to float32, runs aten's antialiased bilinear kernel (``interpolate(..., mode="bilinear",
    antialias=True, align_corners=False)``), rounds (half to even) and casts back to uint8 BEFORE the division by
    255 -- byte work, reproduced bit for bit (PIL's BILINEAR filter accumulates with 8-bit fixed-point weights and is
    one uint8 step off on ~1 % of the pixels; PIL only decodes here)."""
    from PIL import Image
    img = torch.from_numpy(np.asarray(Image.open(path).convert("L"), dtype=np.uint8).copy())
    if tuple(img.shape) != (size, size):
        img = torch.nn.functional.interpolate(img[None, None].to(torch.float32), size=(size, size), mode="bilinear",
                                              antialias=True, align_corners=False).round_().to(torch.uint8)[0, 0]
    x = img.to(torch.float32).div_(255).unsqueeze(0)
    return x * 2 - 1 if normalize else x


class ImageDataset(Dataset):
    """Pairs of (input, ground truth) image files (reference dataset.py:110-134)."""

    def __init__(self, data_tuples, normalize=True, size=256):
        super().__init__()
        self.data_tuples, self.normalize, self.size = data_tuples, normalize, size

    def __len__(self):
        return len(self.data_tuples)

    def __getitem__(self, idx):
        inp, gt = self.data_tuples[idx]
        return load_gray_256(inp, self.size, self.normalize), load_gray_256(gt, self.size, self.normalize)


def _read_list(list_file):
    import yaml
    with open(list_file, "r") as f:
        items = yaml.safe_load(f)
    base = os.path.dirname(str(list_file))
    return [(os.path.join(base, it["input"]), os.path.join(base, it["ground_truth"])) for it in items]


class ShardedLoader:
    """A DataLoader over this rank's shard of a dataset.  With ``world > 1`` the indices come from a
    ``DistributedSampler`` (what Lightning's DDP strategy wraps around the reference's loaders, reference
    main.py:123-136 + dataset.py:77-83): every epoch is ONE pass over the data split across the ranks, shuffled with
    a seed all ranks share and the epoch number (``set_epoch``), padded by wrap-around so that every rank draws the
    same number of batches (the collective gradient exchange needs that)."""

    def __init__(self, dataset, batch_size, shuffle, world=1, rank=0, seed=0, **loader_kw):
        self.sampler = (DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
                                           drop_last=False) if world > 1 else None)
        self.loader = DataLoader(dataset, batch_size=batch_size, shuffle=shuffle and self.sampler is None,
                                 sampler=self.sampler, drop_last=False, **loader_kw)
        self.dataset, self.batch_size = dataset, batch_size

    def set_epoch(self, epoch: int):
        if self.sampler is not None:
            self.sampler.set_epoch(epoch)

    def __iter__(self):
        return iter(self.loader)

    def __len__(self):
        return len(self.loader)


def _dist_info():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


# ---- device-resident data set ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def aa_tables(in_size: int, out_size: int):
    """Filter tables of aten's antialiased bilinear resize along one axis (``align_corners=False``), as its CPU kernel
    builds them: ``bounds`` int32 [out, 2] = (first source index, taps) and ``weights`` fp32 [out, K], zero padded, with
    K = 2 * ceil(support) + 1.  Every operation rounds to fp32.  Output i is
    ``t = src[x0] * w[0]; t = fma(src[x0 + j], w[j], t)`` for j = 1 .. taps - 1 (what csrc/data.hip computes)."""
    f32 = np.float32
    scale = f32(in_size) / f32(out_size)
    support = f32(scale) if scale >= 1 else f32(1.0)
    invscale = f32(1.0) / scale if scale >= 1 else f32(1.0)
    K = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((out_size, K), f32)
    for i in range(out_size):
        center = f32(scale * f32(i + f32(0.5)))
        lo = max(int(f32(center - support + f32(0.5))), 0)
        n = min(int(f32(center + support + f32(0.5))), in_size) - lo
        x = (np.arange(n, dtype=np.int64) + lo).astype(f32)
        x = ((x - center + f32(0.5)).astype(f32) * invscale).astype(f32)
        w = np.maximum(f32(1.0) - np.abs(x), f32(0.0)).astype(f32)
        total = f32(0.0)
        for v in w:                      # summed in ascending j, one fp32 rounding per term
            total = f32(total + v)
        weights[i, :n] = (w / total).astype(f32)
        bounds[i] = (lo, n)
    return torch.from_numpy(bounds), torch.from_numpy(weights)


def epoch_indices(n: int, world: int = 1, rank: int = 0, seed: int = 0, epoch: int = 0, shuffle: bool = True):
    """The indices ``DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
    drop_last=False)`` yields after ``set_epoch(epoch)`` (``world == 1`` included): a function of (seed, epoch) alone."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    total = -(-n // world) * world
    pad = total - n
    if pad and idx:
        idx += (idx * -(-pad // len(idx)))[:pad]           # wrap-around: every rank draws the same number
    return idx[rank:total:world]


def value_table(normalize: bool) -> torch.Tensor:
    """fp32 value of every byte, by the expression of ``load_gray_256`` (so that equality does not rest on the device's
    division)."""
    x = torch.arange(256, dtype=torch.int16).to(torch.uint8).to(torch.float32).div_(255)
    return x * 2 - 1 if normalize else x


def _decode_gray(path) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), dtype=np.uint8)


class DeviceImageCache:
    """Both images of every pair, resized to ``size`` x ``size``, as two uint8 [M, size, size] device tensors.  Each file
    is decoded once (PIL, a pool of at most 16 threads), uploaded at its native size in chunks of consecutive same-shape
    images and resized there.  With ``world > 1`` every rank holds the whole list: the shards change with the epoch."""

    DECODE_THREADS = 16          # a fixed cap, never the machine's CPU count (a shared box reports all of them)
    BLOCK = 256                  # pairs decoded before they are uploaded: bounds the host copy of native-size images
    CHUNK_BYTES = 256 << 20

    @staticmethod
    def bytes_needed(n_pairs: int, size: int) -> int:
        return 2 * n_pairs * size * size

    def __init__(self, data_tuples, size: int, device, threads: Optional[int] = None):
        from concurrent.futures import ThreadPoolExecutor
        from . import ops
        self.size, self.device = size, torch.device(device)
        M = len(data_tuples)
        self.inputs = torch.empty((M, size, size), dtype=torch.uint8, device=self.device)
        self.targets = torch.empty((M, size, size), dtype=torch.uint8, device=self.device)
        self.resized = 0                                     # images that went through the resize kernel
        self._tabs = {}
        workers = max(1, min(self.DECODE_THREADS, threads or self.DECODE_THREADS))
        with ThreadPoolExecutor(max_workers=workers) as pool:
            for b0 in range(0, M, self.BLOCK):
                block = data_tuples[b0:b0 + self.BLOCK]
                for col, dst in ((0, self.inputs), (1, self.targets)):
                    self._fill(ops, list(pool.map(_decode_gray, [p[col] for p in block])), dst, b0)

    def __len__(self):
        return int(self.inputs.shape[0])

    def _table(self, ops, n_in):
        if n_in == self.size:
            return None
        if n_in not in self._tabs:
            self._tabs[n_in] = ops.AATables(*aa_tables(n_in, self.size), self.device)
        return self._tabs[n_in]

    def _fill(self, ops, images, dst, at):
        i = 0
        while i < len(images):
            shape = images[i].shape
            cap = max(1, self.CHUNK_BYTES // max(1, shape[0] * shape[1]))
            j = i + 1
            while j < len(images) and j - i < cap and images[j].shape == shape:
                j += 1
            chunk = torch.from_numpy(np.stack(images[i:j])).to(self.device)
            out = dst[at + i:at + j]
            if shape == (self.size, self.size):
                out.copy_(chunk)
            else:
                ops.resize_aa_u8(chunk, out, self._table(ops, shape[1]), self._table(ops, shape[0]))
                self.resized += j - i
            i = j


class DeviceLoader:
    """Batches of a device-resident data set: per epoch ONE small index upload (``epoch_indices``: this rank's shard, as
    ``ShardedLoader`` draws it), per batch ONE gather launch (csrc/data.hip).  Yields fp32 device tensors
    ``[count, 1, S, S]`` x 2; ``drop_last=False``: the last batch may be short."""

    def __init__(self, inputs, targets, batch_size, shuffle, world=1, rank=0, seed=0, table=None):
        if inputs.shape != targets.shape or not inputs.is_cuda:
            raise ValueError("DeviceLoader: two device tensors of one shape expected")
        self.inputs, self.targets, self.table = inputs, targets, table
        self.batch_size, self.shuffle, self.world, self.rank, self.seed = batch_size, shuffle, world, rank, seed
        self.epoch = 0
        self.image_shape = tuple(inputs.shape[1:]) if inputs.dim() == 4 else (1,) + tuple(inputs.shape[1:])

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def __len__(self):
        shard = -(-int(self.inputs.shape[0]) // self.world)
        return -(-shard // self.batch_size)

    def __iter__(self):
        from . import ops
        dev = self.inputs.device
        idx = epoch_indices(int(self.inputs.shape[0]), self.world, self.rank, self.seed, self.epoch, self.shuffle)
        idx_dev = torch.tensor(idx, dtype=torch.int64).to(dev)
        for b0 in range(0, len(idx), self.batch_size):
            count = min(self.batch_size, len(idx) - b0)
            x = torch.empty((count,) + self.image_shape, dtype=torch.float32, device=dev)
            t = torch.empty_like(x)
            ops.batch_gather(self.inputs, self.targets, idx_dev[b0:b0 + count], count, self.table, x, t)
            yield x, t


def _cache_device(need: int, budget: Optional[int], device):
    """The device a cache of ``need`` bytes goes to, or None when it exceeds its budget.  The budget is a setting:
    ``cache_budget_bytes``, or half of the memory free on the device at setup (a set budget is checked without touching
    the device)."""
    def resolve():
        return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if budget is None:
        budget = torch.cuda.mem_get_info(resolve())[0] // 2
    if need > budget:
        print(f"device cache: {need} bytes needed, budget {budget}: using the host loader", flush=True)
        return None
    return resolve()


class ImageDataModule(LightningDataModule):
    """``ImageDataModule(data_list_file, val_list_file, batch_size, normalize)`` (reference
    dataset.py:11-107).  ``num_workers`` / ``pin_memory`` are additions: the reference decodes on
    the main process, which cannot feed a GPU at >2k images/s.  ``world`` / ``rank`` (default: taken from
    torch.distributed when it is initialised) shard every split across the data-parallel ranks.
    ``device_cache=True``: the splits of a stage are decoded once at ``setup`` into a ``DeviceImageCache`` on ``device``
    (default: the current HIP device) and all four loaders are ``DeviceLoader``s; a cache larger than
    ``cache_budget_bytes`` (default: half of the free device memory at setup) prints one line and leaves the host
    loaders in place."""

    def __init__(self, data_list_file: str, val_list_file: Optional[str] = None, batch_size: int = 1,
                 normalize: bool = True, num_workers: int = 0, pin_memory: bool = True,
                 world: Optional[int] = None, rank: Optional[int] = None, seed: int = 0,
                 device_cache: bool = False, device=None, cache_budget_bytes: Optional[int] = None, size: int = 256):
        super().__init__()
        self.device_cache, self.cache_device, self.cache_budget_bytes, self.size = \
            device_cache, device, cache_budget_bytes, size
        self.caches = {}            # id of a split's list -> DeviceImageCache (empty without device_cache)
        self.data_tuples = _read_list(data_list_file)
        self.val_tuples = _read_list(val_list_file) if val_list_file is not None else None
        self.batch_size, self.normalize = batch_size, normalize
        self.num_workers, self.pin_memory = num_workers, pin_memory
        dw, dr = _dist_info()
        self.world, self.rank, self.seed = (dw if world is None else world), (dr if rank is None else rank), seed

    def setup(self, stage: str):
        if stage == "fit":
            self.train_split, self.val_split = self.data_tuples, self.val_tuples
        if stage == "validate":
            self.val_split = self.data_tuples
        if stage == "test":
            self.test_split = self.data_tuples
        if stage == "predict":
            self.pred_split = self.data_tuples
        if self.device_cache:
            self._build_caches([s for s in ((self.data_tuples, self.val_tuples) if stage == "fit"
                                            else (self.data_tuples,)) if s])

    def _build_caches(self, splits):
        self.caches = {}
        need = sum(DeviceImageCache.bytes_needed(len(s), self.size) for s in splits)
        dev = _cache_device(need, self.cache_budget_bytes, self.cache_device)
        if dev is None:
            return
        self._table = value_table(self.normalize).to(dev)
        self.caches = {id(s): DeviceImageCache(s, self.size, dev) for s in splits}

    def _loader(self, split, shuffle):
        cache = self.caches.get(id(split))
        if cache is not None:
            return DeviceLoader(cache.inputs, cache.targets, self.batch_size, shuffle, self.world, self.rank, self.seed,
                                self._table)
        return ShardedLoader(ImageDataset(split, self.normalize, self.size), self.batch_size, shuffle, self.world, self.rank,
                             self.seed, num_workers=self.num_workers,
                             pin_memory=self.pin_memory and torch.cuda.is_available())

    def train_dataloader(self):
        return self._loader(self.train_split, True)

    def val_dataloader(self):
        return self._loader(self.val_split, False) if self.val_split else None

    def test_dataloader(self):
        return self._loader(self.test_split, False)

    def predict_dataloader(self):
        return self._loader(self.pred_split, False)


def synthetic_pairs(n: int, size: int = 256, seed: int = 1234, kind: str = "uniform"):
    """Canonical synthetic PAI pairs: numpy default_rng, fp32 in [-1, 1).
    ``kind='blobs'`` makes depth-attenuated blob images so that training has something to learn."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x = rng.random((n, 1, size, size), dtype=np.float32) * 2 - 1
        t = rng.random((n, 1, size, size), dtype=np.float32) * 2 - 1
        return torch.from_numpy(x), torch.from_numpy(t)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
    t = np.zeros((n, 1, size, size), np.float32)
    for i in range(n):
        for _ in range(int(rng.integers(3, 9))):
            cy, cx, r = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(3, 18)
            t[i, 0] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)) * rng.uniform(0.4, 1.0)
    t = np.clip(t, 0, 1)
    depth = np.exp(-yy / size * 2.5)[None, None]
    x = np.clip(t * depth + 0.05 * rng.standard_normal(t.shape).astype(np.float32), 0, 1)
    return torch.from_numpy(x * 2 - 1), torch.from_numpy(t * 2 - 1)


class _TensorPairs(Dataset):
    def __init__(self, x, t):
        self.x, self.t = x, t

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.t[i]


class SyntheticDataModule(LightningDataModule):
    """Synthetic pairs, the same data set on every rank (one seed), sharded across the ranks like ImageDataModule."""

    def __init__(self, n_train=256, n_val=32, batch_size=8, size=256, seed=1234, kind="blobs",
                 world: Optional[int] = None, rank: Optional[int] = None,
                 device_cache: bool = False, device=None, cache_budget_bytes: Optional[int] = None):
        super().__init__()
        self.device_cache, self.cache_device, self.cache_budget_bytes = device_cache, device, cache_budget_bytes
        self.on_device = {}         # id of a host data set -> its (inputs, targets) on the device
        self.n_train, self.n_val, self.batch_size, self.size, self.seed, self.kind = \
            n_train, n_val, batch_size, size, seed, kind
        dw, dr = _dist_info()
        self.world, self.rank = (dw if world is None else world), (dr if rank is None else rank)

    def setup(self, stage: str):
        self.train = _TensorPairs(*synthetic_pairs(self.n_train, self.size, self.seed, self.kind))
        self.val = _TensorPairs(*synthetic_pairs(self.n_val, self.size, self.seed + 1, self.kind))
        self.on_device = {}
        if self.device_cache:
            sets = (self.train, self.val)
            need = sum(2 * d.x.numel() * 4 for d in sets)
            dev = _cache_device(need, self.cache_budget_bytes, self.cache_device)
            if dev is not None:
                self.on_device = {id(d): (d.x.to(dev).contiguous(), d.t.to(dev).contiguous()) for d in sets}

    def _loader(self, data, shuffle, world, rank, sharded=True):
        pair = self.on_device.get(id(data))
        if pair is not None:
            return DeviceLoader(pair[0], pair[1], self.batch_size, shuffle, world, rank, self.seed)
        if sharded:
            return ShardedLoader(data, self.batch_size, shuffle, world, rank, self.seed)
        return DataLoader(data, batch_size=self.batch_size, shuffle=shuffle)

    def train_dataloader(self):
        return self._loader(self.train, True, self.world, self.rank)

    def val_dataloader(self):
        return self._loader(self.val, False, self.world, self.rank)

    def predict_dataloader(self):
        return self._loader(self.val, False, 1, 0, sharded=False)
