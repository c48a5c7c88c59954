"""GPU: report.py end to end, the device path (default) against --host-render on one checkpoint and one set of PNG files:
the same output tree, PNG files that decode to identical arrays, numbers that agree to a few fp32 ulps.

Both are fp64 sums of the same terms in another order, rounded once to fp32 (the MSE is squared in fp32 after that):
1e-6 relative.  The std column of depth_ssim.csv is a difference of nearly equal fp32 numbers: 1e-6 absolute."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _write_pairs(root, n, seed):
    """n PNG pairs, sizes that do and do not need the resize, and their YAML list (reference dataset.py:22-32)."""
    import numpy as np
    import yaml
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root / "img", exist_ok=True)
    items = []
    for i in range(n):
        h, w = ((256, 256), (300, 280), (200, 333), (256, 256))[i % 4]
        yy, xx = np.mgrid[0:h, 0:w]
        gt = 110 + 100 * np.sin(xx / (9.0 + i)) * np.cos(yy / (13.0 + i))
        noisy = gt * np.exp(-yy / h * 1.5) + rng.normal(0, 10, (h, w))
        for kind, img in (("in", noisy), ("gt", gt)):
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), mode="L").save(root / "img" / f"{kind}_{i:03d}.png")
        items.append({"input": f"img/in_{i:03d}.png", "ground_truth": f"img/gt_{i:03d}.png"})
    with open(root / "pairs.yaml", "w") as f:
        yaml.safe_dump(items, f)
    return root / "pairs.yaml"


def _csv(path):
    rows = open(path).read().strip().splitlines()
    return rows[0], [r.split(",") for r in rows[1:]]


def _close(a: str, b: str, rel=1e-6, abs_=0.0):
    a, b = float(a), float(b)
    return abs(a - b) <= max(rel * abs(b), abs_)


def test_device_report_equals_host_render(pai, tmp_path):
    import numpy as np
    from PIL import Image
    from thesis_pai_reconstruction_amd import ops
    assert ops.eval_kernel_name(0) == "eval_planes_k"
    data = _write_pairs(tmp_path, 8, seed=5)
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "rep_run", "-d", str(data), "-vd", str(data),
                          "--batch-size", "4", "--channel-mults", "1,2,2,4,4", "-e", "2", "--val-epochs", "1",
                          "-m", "pix2pix"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    ckpt = tmp_path / "logs" / "rep_run" / "version_0" / "checkpoints" / "best.ckpt"
    assert ckpt.exists()
    for name, extra in (("dev", []), ("host", ["--host-render"])):
        rep = subprocess.run([sys.executable, os.path.join(ROOT, "report.py"), name, "-c", str(ckpt), "-d", str(data),
                              "-bs", "3", "-m", "pix2pix", *extra],
                             cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert rep.returncode == 0, rep.stdout[-2000:] + rep.stderr[-2000:]
    d, h = tmp_path / "reports" / "dev", tmp_path / "reports" / "host"
    names = [f"{i:05d}.png" for i in range(8)]
    for sub, mode in (("outputs", "RGB"), ("ssim_images", "L")):
        assert sorted(os.listdir(d / sub)) == names and sorted(os.listdir(h / sub)) == names
        for f in names:
            a, b = Image.open(d / sub / f), Image.open(h / sub / f)
            assert a.mode == b.mode == mode and a.size == b.size == (256, 256)
            assert np.array_equal(np.asarray(a), np.asarray(b)), (sub, f)
    for f in ("ssim_per_image.csv", "psnr_per_image.csv", "mse_per_image.csv"):
        (hd, rd), (hh, rh) = _csv(d / f), _csv(h / f)
        assert hd == hh and len(rd) == len(rh) == 8
        for x, y in zip(rd, rh):
            print(f, x, y)
            assert x[0] == y[0] and _close(x[1], y[1]), (f, x, y)
    (hd, rd), (hh, rh) = _csv(d / "depth_ssim.csv"), _csv(h / "depth_ssim.csv")
    assert hd == hh == "depth,mean,std" and len(rd) == len(rh) == 16
    for x, y in zip(rd, rh):
        print("depth_ssim", x, y)
        assert x[0] == y[0] and _close(x[1], y[1]) and _close(x[2], y[2], rel=0.0, abs_=1e-6), (x, y)
    sd = dict(l.strip().split(": ") for l in open(d / "stats.txt"))
    sh = dict(l.strip().split(": ") for l in open(h / "stats.txt"))
    print(sd, sh)
    assert list(sd) == list(sh) == ["SSIM", "PSNR", "RMSE", "FLOPs", "Parameter count"]
    for k in ("SSIM", "PSNR", "RMSE"):
        assert _close(sd[k], sh[k]), (k, sd[k], sh[k])
    assert sd["FLOPs"] == sh["FLOPs"] and sd["Parameter count"] == sh["Parameter count"]
