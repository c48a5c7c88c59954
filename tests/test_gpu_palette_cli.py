"""GPU: report.py -m palette end to end on a checkpoint of a portable-initialised pai.Palette((1, 1, 1, 2),
attention_res=(8,), inference_steps=4) and two 256 x 256 PNG pairs: the report tree is complete and its per-image SSIM
values are those of an in-process ``model(x)`` under the same seed."""
import os

import numpy as np
import pytest
import torch

import _palette_util as U
from _gpu_util import dev

pytestmark = pytest.mark.gpu


def _write_pairs(root):
    import yaml
    from PIL import Image
    rng = np.random.default_rng(3)
    os.makedirs(root / "img", exist_ok=True)
    items = []
    for i in range(2):
        yy, xx = np.mgrid[0:256, 0:256]
        gt = 110 + 100 * np.sin(xx / (9.0 + i)) * np.cos(yy / (13.0 + i))
        noisy = gt * np.exp(-yy / 256 * 1.5) + rng.normal(0, 10, (256, 256))
        for kind, img in (("in", noisy), ("gt", gt)):
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), mode="L").save(root / "img" / f"{kind}_{i}.png")
        items.append({"input": f"img/in_{i}.png", "ground_truth": f"img/gt_{i}.png"})
    with open(root / "pairs.yaml", "w") as f:
        yaml.safe_dump(items, f)
    return root / "pairs.yaml"


def test_report_palette(pai, tmp_path, monkeypatch):
    import report
    from thesis_pai_reconstruction_amd import functional as PF
    from thesis_pai_reconstruction_amd.dataset import ImageDataModule
    src = U.init_portable(pai.Palette(1, 1, (1, 1, 1, 2), attention_res=(8,), dropout=0.0, inference_steps=4), 21)
    ckpt = tmp_path / "palette.ckpt"
    torch.save({"hyper_parameters": src.hparams, "state_dict": src.state_dict()}, ckpt)
    data = _write_pairs(tmp_path)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(9)
    out = report.main(report.build_parser().parse_args(["pal", "-c", str(ckpt), "-d", str(data), "-bs", "2", "-m", "palette"]))
    assert out["arm"] == "device"
    rep = tmp_path / "reports" / "pal"
    names = ["00000.png", "00001.png"]
    for f in ("stats.txt", "ssim_per_image.csv", "psnr_per_image.csv", "mse_per_image.csv", "depth_ssim.csv"):
        assert (rep / f).exists(), f
    assert sorted(os.listdir(rep / "outputs")) == names and sorted(os.listdir(rep / "ssim_images")) == names
    rows = open(rep / "ssim_per_image.csv").read().strip().splitlines()
    assert rows[0] == "image,ssim" and len(rows) == 3
    ssims = [float(r.split(",")[1]) for r in rows[1:]]
    assert all(np.isfinite(ssims))
    stats = dict(l.strip().split(": ") for l in open(rep / "stats.txt"))
    assert int(stats["FLOPs"]) == 4 * src.unet.macs(256, 256) and int(stats["Parameter count"]) > 0

    model = pai.Palette.load_from_checkpoint(ckpt, map_location=dev())
    model.freeze()
    dm = ImageDataModule(data, batch_size=2, device=dev())
    dm.setup("predict")
    (batch,) = list(dm.predict_dataloader())
    torch.manual_seed(9)
    with torch.no_grad():
        pred = model(batch[0].to(dev()))
    res = PF.eval_images(pred.contiguous(), batch[1].to(dev()).contiguous(), denorm=True, strips=16, ssim_map=True, hot=True)
    want = res.ssim.cpu().tolist()
    print("palette report ssim", ssims, want)
    assert all(abs(a - b) <= 1e-6 for a, b in zip(ssims, want))
