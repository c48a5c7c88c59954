"""Input pipeline against the training step on ONE box: `Trainer.fit` of the bench.py workload (Pix2Pix, bs 64,
bf16-mixed) from PNG files, through the host loader (``--workers`` decoders: 0 and 15 by default) and through the
device-resident data set (``device_cache=True``), arms interleaved.  One JSON line per arm and repetition:

    {"arm": ..., "setup_s": ..., "first_epoch_s": ..., "images_per_s": ..., "epochs": ..., "pairs": ...}

``setup_s`` is ``datamodule.setup("fit")`` (for the cache: decode + upload + resize of every file, synchronised);
``images_per_s`` is taken over the epochs after the first, with a host clock between device synchronisations at the epoch
boundaries.  No profiler in this process; the per-launch times of batch_gather_k / resize_aa_u8_k come from

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_data.py --arms cache --pairs 512
    python scripts/bench_data.py --kernel-stats DIR --pairs 512 [--batch-size 64]

15 workers, not 16: with the training process that is the 16 processes of a 16-CPU share.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_pairs(root, n, size, seed):
    import yaml
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    yy, xx = np.mgrid[0:size, 0:size]

    def one(i):
        rng = np.random.default_rng(seed + i)
        for kind in ("in", "gt"):
            img = 127 + 80 * np.sin(yy / (7.0 + i % 13)) * np.cos(xx / 5.0 + (kind == "gt")) + rng.normal(0, 20, (size, size))
            Image.fromarray(img.clip(0, 255).astype(np.uint8), mode="L").save(
                os.path.join(root, "img", f"{kind}_{i:05d}.png"), compress_level=1)
        return {"input": f"img/in_{i:05d}.png", "ground_truth": f"img/gt_{i:05d}.png"}
    with ThreadPoolExecutor(max_workers=16) as pool:
        items = list(pool.map(one, range(n)))
    path = os.path.join(root, "list.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(items, f)
    return path


class EpochClock:
    """Wraps the training loader: `set_epoch` (called by Trainer.fit at every epoch boundary) synchronises the device
    and stamps the host clock."""

    def __init__(self, loader, device):
        self.loader, self.device, self.stamps = loader, device, []

    def set_epoch(self, epoch):
        torch.cuda.synchronize(self.device)
        self.stamps.append(time.perf_counter())
        if hasattr(self.loader, "set_epoch"):
            self.loader.set_epoch(epoch)

    def __iter__(self):
        return iter(self.loader)

    def __len__(self):
        return len(self.loader)


def run_arm(pai, arm, lst, args, device):
    from thesis_pai_reconstruction_amd.dataset import ImageDataModule
    from thesis_pai_reconstruction_amd.lightning import Trainer
    cache = arm == "cache"
    workers = 0 if cache else int(arm[4:])
    epochs = args.cache_epochs if cache else args.host_epochs
    dm = ImageDataModule(lst, None, batch_size=args.batch_size, num_workers=workers, world=1, rank=0, device_cache=cache,
                         device=device)
    t0 = time.perf_counter()
    dm.setup("fit")
    torch.cuda.synchronize(device)
    setup_s = time.perf_counter() - t0
    clock = EpochClock(dm.train_dataloader(), device)
    dm.setup = lambda stage: None                   # Trainer.fit would set the splits (and the cache) up again
    dm.train_dataloader = lambda: clock
    torch.manual_seed(0)
    model = pai.Pix2Pix(1, 1, (1, 2, 4, 8, 8, 8, 8, 8), 0.0, "gan")
    trainer = Trainer(max_epochs=epochs, log_every_n_steps=10 ** 9, logger=None, precision="bf16-mixed", device=device,
                      enable_progress_bar=False)
    trainer.fit(model, dm)
    torch.cuda.synchronize(device)
    end = time.perf_counter()
    s = clock.stamps
    plan = trainer.planned_step.describe() if trainer.planned_step is not None else {}
    return {"arm": arm, "setup_s": round(setup_s, 3), "first_epoch_s": round(s[1] - s[0], 3),
            "images_per_s": round(args.pairs * (epochs - 1) / (end - s[1]), 1), "epochs": epochs, "pairs": args.pairs,
            "batch_size": args.batch_size, "device_loader": type(clock.loader).__name__,
            "plan_replays": plan.get("replays"), "plan_disabled": plan.get("disabled")}


def kernel_stats(d, args):
    """Time per launch of the two data kernels from a rocprofv3 --kernel-trace --stats directory, with the bytes each launch
    moves and the rate that gives."""
    rows = list(csv.DictReader(open(glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)[0])))
    S, src = 256, args.size
    full = args.batch_size * 2 * S * S * (1 + 4)                 # uint8 read + fp32 written, both tensors of a pair
    for name in ("batch_gather_k", "resize_aa_u8_k"):
        mine = [r for r in rows if name in r["Kernel_Name"]]
        if not mine:
            print(json.dumps({"kernel": name, "launches": 0}))
            continue
        groups = {}
        for r in mine:
            groups.setdefault((int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])), []).append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for grid, us in sorted(groups.items()):
            us.sort()
            if name == "batch_gather_k":
                nbytes = grid[1] * 2 * S * S * (1 + 4)           # grid.y = images of the batch
            else:
                nbytes = grid[1] * (src * src + S * S)           # grid.y = images of the chunk: source read + result written
            med = us[len(us) // 2]
            print(json.dumps({"kernel": name, "grid": grid, "launches": len(us), "median_us": round(med, 2),
                              "min_us": round(us[0], 2), "bytes": nbytes, "GB_per_s": round(nbytes / med / 1e3, 1),
                              "full_batch_bytes": full}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--arms", default="host0,host15,cache")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-epochs", type=int, default=3)
    ap.add_argument("--cache-epochs", type=int, default=8)
    ap.add_argument("--kernel-stats", default=None, help="summarise a rocprofv3 output directory instead of running")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args)
    import pai_bootstrap
    pai = pai_bootstrap.load()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    root = tempfile.mkdtemp(prefix="pai_bench_data_")
    try:
        t0 = time.perf_counter()
        lst = write_pairs(root, args.pairs, args.size, seed=1000)
        print(json.dumps({"wrote_pairs": args.pairs, "size": args.size, "seconds": round(time.perf_counter() - t0, 1)}), flush=True)
        for _ in range(args.reps):
            for arm in args.arms.split(","):
                print(json.dumps(run_arm(pai, arm, lst, args, device)), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
