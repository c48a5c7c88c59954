"""The device-resident data set on the GPU (csrc/data.hip, dataset.DeviceImageCache / DeviceLoader): the resize kernel
gives the host operator's bytes, every batch of ``ImageDataModule(device_cache=True)`` / ``SyntheticDataModule(
device_cache=True)`` is bit for bit the host-built batch of the same indices, no file is opened after setup, training
and evaluation run from it (reference dataset.py:11-134, main.py:106-136, report.py:117-127)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
SHAPES = ((256, 256), (300, 280), (200, 333), (256, 256), (256, 256), (512, 512), (128, 96))


def _image(h, w, rng, phase=0.0):
    yy, xx = np.mgrid[0:h, 0:w]
    return (127 + 80 * np.sin(yy / 7.0 + phase) * np.cos(xx / 5.0) + rng.normal(0, 20, (h, w))).clip(0, 255).astype(np.uint8)


def _write_pairs(root, n, seed, shapes=SHAPES, name="list.yaml"):
    """n PNG pairs of mixed native sizes (some exactly 256 x 256, some runs of one shape) + the YAML list."""
    import yaml
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root / "img", exist_ok=True)
    items = []
    for i in range(n):
        h, w = shapes[i % len(shapes)]
        for kind in ("in", "gt"):
            Image.fromarray(_image(h, w, rng, i + (kind == "gt")), mode="L").save(root / "img" / f"{kind}_{seed}_{i:03d}.png")
        items.append({"input": f"img/in_{seed}_{i:03d}.png", "ground_truth": f"img/gt_{seed}_{i:03d}.png"})
    with open(root / name, "w") as f:
        yaml.safe_dump(items, f)
    return root / name


@pytest.mark.parametrize("shape", [(512, 512), (300, 400), (128, 128), (257, 255), (1024, 768), (200, 1000)])
def test_resize_kernel_gives_the_host_bytes(pai, shape):
    from thesis_pai_reconstruction_amd import ops
    from thesis_pai_reconstruction_amd.dataset import aa_tables
    rng = np.random.default_rng(7)
    h, w = shape
    src = torch.from_numpy(np.stack([_image(h, w, rng, k) for k in range(3)]))
    ref = F.interpolate(src[:, None].float(), size=(256, 256), mode="bilinear", antialias=True,
                        align_corners=False).round_().to(torch.uint8)[:, 0]
    out = torch.full((3, 256, 256), 7, dtype=torch.uint8, device=DEV)
    wtab = ops.AATables(*aa_tables(w, 256), DEV)
    htab = ops.AATables(*aa_tables(h, 256), DEV)
    ops.resize_aa_u8(src.to(DEV), out, wtab, htab)
    torch.cuda.synchronize()
    differing = int((out.cpu() != ref).sum())
    print(f"resize {h} x {w} -> 256: {differing} differing bytes")
    assert differing == 0
    assert ops.data_kernel_name(0) == "resize_aa_u8_k"
    assert ops.data_kernel_name(1, torch.uint8) == "batch_gather_k<unsigned char>"
    assert ops.data_kernel_name(1, torch.float32) == "batch_gather_k<float>"


def test_resize_kernel_one_axis_only(pai):
    """An axis that already has the output size takes no table and is copied."""
    from thesis_pai_reconstruction_amd import ops
    from thesis_pai_reconstruction_amd.dataset import aa_tables
    rng = np.random.default_rng(11)
    for h, w in ((256, 400), (300, 256)):
        src = torch.from_numpy(np.stack([_image(h, w, rng, k) for k in range(2)]))
        ref = F.interpolate(src[:, None].float(), size=(256, 256), mode="bilinear", antialias=True,
                            align_corners=False).round_().to(torch.uint8)[:, 0]
        out = torch.zeros((2, 256, 256), dtype=torch.uint8, device=DEV)
        ops.resize_aa_u8(src.to(DEV), out, None if w == 256 else ops.AATables(*aa_tables(w, 256), DEV),
                         None if h == 256 else ops.AATables(*aa_tables(h, 256), DEV))
        assert int((out.cpu() != ref).sum()) == 0, (h, w)
    with pytest.raises(ops.PaiError, match="table"):
        ops.resize_aa_u8(torch.zeros((1, 300, 256), dtype=torch.uint8, device=DEV), out[:1], None, None)


@pytest.mark.parametrize("normalize", [True, False])
def test_every_batch_equals_the_host_batch(pai, tmp_path, normalize):
    from thesis_pai_reconstruction_amd.dataset import (DeviceLoader, ImageDataModule, ImageDataset, _read_list,
                                                       epoch_indices)
    n, bs, seed = 11, 4, 3
    lst = _write_pairs(tmp_path, n, seed=1)
    host = ImageDataset(_read_list(str(lst)), normalize)
    items = [host[i] for i in range(n)]
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        dm = ImageDataModule(str(lst), str(lst), batch_size=bs, normalize=normalize, world=world, rank=rank, seed=seed,
                             device_cache=True, device=DEV)
        dm.setup("fit")
        cache = dm.caches[id(dm.train_split)]
        assert len(cache) == n and cache.resized == 2 * sum(1 for i in range(n) if SHAPES[i % len(SHAPES)] != (256, 256))
        for loader, shuffle in ((dm.train_dataloader(), True), (dm.val_dataloader(), False)):
            assert isinstance(loader, DeviceLoader)
            for epoch in (0, 1):
                loader.set_epoch(epoch)
                idx = epoch_indices(n, world, rank, seed, epoch, shuffle)
                batches = list(loader)
                assert len(batches) == len(loader) == -(-len(idx) // bs)
                assert batches[-1][0].shape[0] == len(idx) - bs * (len(batches) - 1) < bs     # the short last batch
                for b, (x, t) in enumerate(batches):
                    want = idx[b * bs:(b + 1) * bs]
                    for got, col in ((x, 0), (t, 1)):
                        assert got.device == DEV and got.dtype == torch.float32 and got.is_contiguous()
                        assert tuple(got.shape) == (len(want), 1, 256, 256)
                        assert torch.equal(got.cpu(), torch.stack([items[i][col] for i in want])), (world, rank, epoch, b)
    for stage, get in (("test", "test_dataloader"), ("predict", "predict_dataloader"), ("validate", "val_dataloader")):
        dm = ImageDataModule(str(lst), None, batch_size=bs, normalize=normalize, world=1, rank=0, device_cache=True, device=DEV)
        dm.setup(stage)
        loader = getattr(dm, get)()
        assert isinstance(loader, DeviceLoader)
        x = torch.cat([b[0] for b in loader]).cpu()
        assert torch.equal(x, torch.stack([it[0] for it in items])), stage


def test_no_file_is_opened_after_setup(pai, tmp_path, monkeypatch):
    from PIL import Image
    from thesis_pai_reconstruction_amd.dataset import ImageDataModule
    lst = _write_pairs(tmp_path, 6, seed=2)
    dm = ImageDataModule(str(lst), str(lst), batch_size=4, world=1, rank=0, device_cache=True, device=DEV)
    dm.setup("fit")
    first = [x.cpu() for x, _ in dm.val_dataloader()]

    def closed(*a, **k):
        raise AssertionError("PIL.Image.open after setup")
    monkeypatch.setattr(Image, "open", closed)
    train, val = dm.train_dataloader(), dm.val_dataloader()
    for epoch in (1, 2):
        train.set_epoch(epoch)
        assert sum(x.shape[0] for x, _ in train) == 6
        again = [x.cpu() for x, _ in val]
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_synthetic_batches_equal_the_host_tensors(pai):
    from thesis_pai_reconstruction_amd.dataset import DeviceLoader, SyntheticDataModule, epoch_indices
    for world, rank in ((1, 0), (2, 1)):
        dm = SyntheticDataModule(n_train=10, n_val=6, batch_size=4, size=32, seed=77, world=world, rank=rank,
                                 device_cache=True, device=DEV)
        dm.setup("fit")
        for loader, data, shuffle, w, r in ((dm.train_dataloader(), dm.train, True, world, rank),
                                            (dm.val_dataloader(), dm.val, False, world, rank),
                                            (dm.predict_dataloader(), dm.val, False, 1, 0)):
            assert isinstance(loader, DeviceLoader)
            loader.set_epoch(1)
            idx = epoch_indices(len(data), w, r, 77, 1, shuffle)
            for b, (x, t) in enumerate(loader):
                want = idx[4 * b:4 * b + 4]
                assert x.device == DEV and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (len(want), 1, 32, 32)
                assert torch.equal(x.cpu(), data.x[want]) and torch.equal(t.cpu(), data.t[want])


def _small_model(pai, seed=0):
    torch.manual_seed(seed)
    return pai.Pix2Pix(1, 1, (1, 2, 2, 4), 0.0, "gan")


@pytest.mark.parametrize("source", ["png", "synthetic"])
def test_trainer_fits_from_the_device_cache(pai, tmp_path, source):
    from thesis_pai_reconstruction_amd.dataset import DeviceLoader, ImageDataModule, SyntheticDataModule
    from thesis_pai_reconstruction_amd.lightning import CSVLogger, ModelCheckpoint, Trainer
    if source == "png":
        shapes = ((64, 64), (80, 96), (100, 70), (64, 64), (128, 128))
        dm = ImageDataModule(str(_write_pairs(tmp_path, 26, 5, shapes, "train.yaml")),
                             str(_write_pairs(tmp_path, 6, 6, shapes, "val.yaml")), batch_size=4, world=1, rank=0,
                             device_cache=True, device=DEV, size=64)
    else:
        dm = SyntheticDataModule(n_train=26, n_val=6, batch_size=4, size=64, world=1, rank=0, device_cache=True, device=DEV)
    logger = CSVLogger(str(tmp_path / "logs"), name="fit")
    trainer = Trainer(max_epochs=2, log_every_n_steps=2, check_val_every_n_epoch=1, logger=[logger], precision="bf16-mixed",
                      callbacks=[ModelCheckpoint(save_top_k=1, monitor="val_ssim", mode="max", filename="best")],
                      device=DEV, enable_progress_bar=False)
    trainer.fit(_small_model(pai), dm)
    assert isinstance(dm.train_dataloader(), DeviceLoader) and isinstance(dm.val_dataloader(), DeviceLoader)
    rows = open(os.path.join(logger.log_dir, "metrics.csv")).read().strip().splitlines()
    assert "val_ssim" in rows[0] and "loss" in rows[0] and len(rows) >= 5
    assert os.path.exists(os.path.join(logger.log_dir, "checkpoints", "best.ckpt"))
    plan = trainer.planned_step.describe()
    assert plan["disabled"] is None and plan["replays"] > 0, plan
    assert trainer.batches_seen == 2 * 7 and trainer.global_step == 2 * trainer.batches_seen


def test_main_cli_trains_with_device_cache(tmp_path):
    """``main.py --device-cache`` (beside ``--synthetic``, and with a YAML list) trains and checkpoints."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    shapes = ((256, 256), (300, 280))
    train, val = _write_pairs(tmp_path, 10, 5, shapes, "train.yaml"), _write_pairs(tmp_path, 4, 6, shapes, "val.yaml")
    for name, data in (("syn", ["--synthetic", "24", "--image-size", "64"]), ("png", ["-d", str(train), "-vd", str(val)])):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), name, *data, "--device-cache", "--batch-size", "4",
                              "--channel-mults", "1,2,2,4", "-e", "2", "--val-epochs", "1", "--precision", "bf16-mixed"],
                             cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "using the host loader" not in run.stdout
        vdir = tmp_path / "logs" / name / "version_0"
        assert "val_ssim" in open(vdir / "metrics.csv").readline() and (vdir / "checkpoints" / "best.ckpt").exists()


def test_logged_losses_equal_the_host_path(pai, tmp_path):
    """One epoch of ``training_step`` by hand, twice from the same initial state: on the device-cache batches and on the
    host-built batches of the same indices.  The inputs are bit-equal, so every logged value must be equal."""
    from thesis_pai_reconstruction_amd.dataset import ImageDataModule, ImageDataset, _read_list, epoch_indices
    shapes = ((64, 64), (80, 96), (100, 70), (64, 64), (128, 128))
    lst = _write_pairs(tmp_path, 14, 8, shapes)
    dm = ImageDataModule(str(lst), None, batch_size=4, world=1, rank=0, seed=2, device_cache=True, device=DEV, size=64)
    dm.setup("fit")
    loader = dm.train_dataloader()
    loader.set_epoch(0)
    idx = epoch_indices(14, 1, 0, 2, 0, True)
    host = ImageDataset(_read_list(str(lst)), True, 64)
    host_batches = [tuple(torch.stack([host[i][c] for i in idx[b:b + 4]]).to(DEV) for c in (0, 1)) for b in range(0, 14, 4)]
    ref = _small_model(pai, 4)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    runs = []
    for batches in (list(loader), host_batches):
        m = _small_model(pai, 4)
        m.load_state_dict(state)
        m.to(DEV)
        m.set_precision("bf16-mixed")
        m.train()
        logs = []
        for bi, batch in enumerate(batches):
            m.logged = {}
            m.training_step(batch, bi)
            torch.cuda.synchronize()
            logs.append({k: float(v) for k, v in m.logged.items()})
        runs.append(logs)
    for bi, (a, b) in enumerate(zip(*runs)):
        print(f"batch {bi}: device cache {a} | host {b}")
    assert len(runs[0]) == len(runs[1]) == 4
    for bi, (a, b) in enumerate(zip(*runs)):
        assert set(a) == set(b) and {"loss", "d_loss"} <= set(a)
        for k in a:
            assert a[k] == b[k], (bi, k, a[k], b[k])


def test_report_writes_the_same_csv_from_the_device_cache(pai, tmp_path):
    from thesis_pai_reconstruction_amd.lightning import Trainer
    lst = _write_pairs(tmp_path, 6, seed=9)
    m = _small_model(pai, 1)
    trainer = Trainer(device=None)
    trainer.model = m
    ckpt = tmp_path / "m.ckpt"
    trainer.save_checkpoint(str(ckpt))
    env = dict(os.environ, PYTHONPATH=ROOT)
    for name, flag in (("host", []), ("cached", ["--device-cache"])):
        rep = subprocess.run([sys.executable, os.path.join(ROOT, "report.py"), name, "-c", str(ckpt), "-d", str(lst), "-bs", "4",
                              "-m", "pix2pix", *flag], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert rep.returncode == 0, rep.stdout[-2000:] + rep.stderr[-2000:]
    a = open(tmp_path / "reports" / "host" / "ssim_per_image.csv").read()
    b = open(tmp_path / "reports" / "cached" / "ssim_per_image.csv").read()
    assert len(a.strip().splitlines()) == 7 and a == b
