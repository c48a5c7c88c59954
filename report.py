"""Evaluation CLI -- same flags and output tree as the reference's report.py:236-270
(reports/<name>/{depth_ssim.csv, outputs/, ssim_images/, stats.txt, ssim_per_image.csv,
psnr_per_image.csv, mse_per_image.csv}); the eval-mode generator forward and the SSIM / PSNR / MSE
arithmetic run on the MI355X kernels.

The metrics and both sets of images are computed on the device, one chunk of at most 64 images at a time
(PF.eval_images: two launches per chunk): per-image SSIM / PSNR / MSE, the SSIM of the 16 depth strips, the SSIM map and
the afmhot rendering of the prediction as bytes.  Only those bytes (1 + 3 per pixel) and the per-image numbers leave the
device, through pinned buffers on a copy stream, while the next chunk computes; a thread pool writes the PNG files.

Added (build-only) flags: --device-cache (resize the images on the GPU and read the batches from device memory),
--host-render (the per-image metric calls, the host colormap and the serial PNG loop this CLI used before: the A/B arm
of scripts/bench_report.py and the path of images whose height is not a multiple of 16), --stage-times (synchronise
between the stages and print their wall times as one JSON line).

Reference defect handled here: report.py:152 counts FLOPs with a 3-channel input;
this counts the loaded model's own convolutions (1 "FLOP" per MAC, fvcore's convention).
"""
import json
import os
import pathlib
import time
from argparse import ArgumentParser
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import pai_bootstrap

pai = pai_bootstrap.load()
from thesis_pai_reconstruction_amd import functional as PF  # noqa: E402
from thesis_pai_reconstruction_amd.dataset import ImageDataModule, SyntheticDataModule  # noqa: E402
from thesis_pai_reconstruction_amd.models.utils import get_parameter_count, to_int  # noqa: E402


CHUNK = 64                # images per PF.eval_images call
NUM_DEPTHS = 16
PNG_THREADS = 16          # a fixed cap, never the machine's CPU count (a shared box reports all of them)


class StageClock:
    """Wall time per stage of the report.  ``mark`` closes the current interval (after a device synchronise when stage
    timing is on; otherwise the stages overlap and only the total means something)."""

    def __init__(self, sync: bool):
        self.sync, self.times, self.t0, self.png_seconds = sync, {}, time.perf_counter(), 0.0
        self.start = self.t0

    def mark(self, stage: str):
        if not self.sync:
            return
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.times[stage] = self.times.get(stage, 0.0) + now - self.t0
        self.t0 = now

    def png(self, seconds: float):
        """Time spent encoding PNG files inside the stage that is open: booked as "png" instead."""
        if self.sync:
            self.png_seconds += seconds

    def mark_less_png(self, stage: str):
        """``mark``, with the PNG seconds noted since the last mark going to the "png" stage."""
        self.mark(stage)
        if self.sync:
            self.times[stage] -= self.png_seconds
            self.times["png"] = self.times.get("png", 0.0) + self.png_seconds
            self.png_seconds = 0.0


def save_png(a: np.ndarray, filename: str):
    """[C x H x W] uint8 array -> PNG file (C = 1: grey, C = 3: RGB)."""
    from PIL import Image
    Image.fromarray(a[0] if a.shape[0] == 1 else np.transpose(a, (1, 2, 0))).save(filename)


def write_png(img_u8: torch.Tensor, filename: str, clock=None):
    """torchvision.io.write_png replacement: [C x H x W] uint8."""
    a = img_u8.cpu().numpy()
    t0 = time.perf_counter()
    save_png(a, filename)
    if clock is not None:
        clock.png(time.perf_counter() - t0)


def depth_ssim(preds: torch.Tensor, targets: torch.Tensor, num_depths: int = 16) -> torch.Tensor:
    """Mean / std of the per-image SSIM over `num_depths` horizontal strips (reference report.py:188-217)."""
    out = []
    for xp, xt in zip(preds.chunk(num_depths, dim=2), targets.chunk(num_depths, dim=2)):
        s = PF.ssim_per_image(xp.contiguous(), xt.contiguous())
        out.append((s.mean(), s.std()))
    return torch.tensor(out)


def output_hot_image(img: torch.Tensor, filename: str, clock=None):
    """afmhot colormap PNG (reference report.py:220-233)."""
    from matplotlib import colormaps
    rgb = colormaps["afmhot"](img.cpu().numpy())[0, :, :, :3]
    write_png(to_int(torch.tensor(rgb, dtype=torch.float32).permute(2, 0, 1)), filename, clock)


def count_macs(model) -> int:
    unet = getattr(model, "unet", None)
    if isinstance(model, pai.Palette):       # one sampling call: inference_steps U-Net passes (conv + linear + attention)
        return model.diffusion_inf.timesteps * unet.macs(256, 256)
    if unet is not None and hasattr(unet, "vit_bottleneck"):      # TransUNet: convs at their output resolution + ViT
        def conv_macs(c, sp_out):
            return sp_out * sp_out * c.weight.shape[0] * c.weight.shape[1] * c.weight.shape[2] * c.weight.shape[3]
        size = unet.image_size
        total, sp = conv_macs(unet.in_conv, size), size
        for enc in unet.encoders:
            d = enc.decode
            total += conv_macs(d[0], sp) + conv_macs(d[3], sp // 2) + conv_macs(d[6], sp // 2) + conv_macs(enc.skip[0], sp // 2)
            sp //= 2
        vit = unet.vit_bottleneck
        P, D = vit.num_patches, vit.patch_dim
        per_token = D * D + sum(l.self_attn.in_proj_weight.numel() + l.self_attn.out_proj.weight.numel() +
                                l.linear1.weight.numel() + l.linear2.weight.numel() for l in vit.transformer.layers)
        total += P * per_token         # (attention over the batch axis adds 2 * N * D MACs per token, batch-dependent)
        for dec in unet.decoders:
            total += conv_macs(dec.decode[0], sp) + conv_macs(dec.decode[3], sp)
            sp *= 2
        return total + conv_macs(unet.out[0], sp)
    if unet is not None and hasattr(unet, "in_conv"):      # residual U-Net: every conv at the resolution it runs at
        def conv_macs(c, sp):
            return sp * sp * c.weight.shape[0] * c.weight.shape[1] * c.weight.shape[2] * c.weight.shape[3]
        size, total = 256, 0
        total += conv_macs(unet.in_conv, size)
        sp = size
        for enc in unet.encoders:
            total += sum(conv_macs(m, sp) for m in enc.encode[0].modules() if isinstance(m, torch.nn.Conv2d))
            sp //= 2
        for dec in unet.decoders:
            total += sum(conv_macs(m, sp) for m in dec.decode[0].modules() if isinstance(m, torch.nn.Conv2d))
            sp *= 2
        return total + conv_macs(unet.out[0], sp)
    if unet is None or not hasattr(unet, "engine"):
        return 0
    eng, size, total = unet.engine, 256, 0
    cin = eng.in_ch
    for i, c in enumerate(eng.enc_c):
        total += (size >> (i + 1)) ** 2 * 16 * cin * c
        cin = c
    for j, c in enumerate(eng.dec_c):
        hin = size >> (eng.L - j)
        k = eng.enc_c[-1] if j == 0 else eng.dec_c[j - 1] + eng.enc_c[eng.L - 1 - j]
        total += hin * hin * 16 * k * c
    for j, g in enumerate(getattr(eng, "gates", []), 1):      # attention gates: two C -> K pointwise convs, K -> 1
        sp = size >> (eng.L - j)
        total += sp * sp * (2 * g.C * g.K + g.K)
    return total


def main(hparams):
    dev = torch.device("cuda", 0)
    if hparams.model == "pix2pix":
        model = pai.Pix2Pix.load_from_checkpoint(hparams.checkpoint, map_location=dev)
        model.freeze()
    elif hparams.model == "attention_unet":
        model = pai.AttentionUnetGAN.load_from_checkpoint(hparams.checkpoint, map_location=dev)
        model.freeze()
    elif hparams.model in ("res18_unet", "res50_unet", "resv2_unet", "resnext_unet"):
        model = pai.ResUnetGAN.load_from_checkpoint(hparams.checkpoint, map_location=dev)
        model.freeze()
    elif hparams.model == "trans_unet":
        model = pai.TransUnetGAN.load_from_checkpoint(hparams.checkpoint, map_location=dev)
        model.freeze()
    elif hparams.model == "palette":
        model = pai.Palette.load_from_checkpoint(hparams.checkpoint, map_location=dev)
        model.freeze()
    elif hparams.model == "identity":
        def model(x):
            return x
    else:
        raise NotImplementedError(f"model {hparams.model!r} is not built on the HIP path yet")

    if hparams.data is None:
        data_module = SyntheticDataModule(n_val=16, batch_size=hparams.batch_size, device_cache=hparams.device_cache,
                                          device=dev)
        data_module.setup("predict")
    else:
        data_module = ImageDataModule(hparams.data, batch_size=hparams.batch_size, device_cache=hparams.device_cache,
                                      device=dev)
        data_module.setup("predict")
    dataloader = data_module.predict_dataloader()

    report_dir = os.path.join("reports", hparams.name)
    clock = StageClock(getattr(hparams, "stage_times", False))
    arm = "device"
    if getattr(hparams, "host_render", False) or not device_report(model, dataloader, dev, report_dir, clock):
        arm = "host"                            # asked for, or images the device path does not take
        host_report(model, dataloader, dev, report_dir, clock)
    torch.cuda.synchronize()
    out = {"arm": arm,
           "total_s": round(time.perf_counter() - clock.start, 4), **{k + "_s": round(v, 4) for k, v in clock.times.items()}}
    if clock.sync:
        print(json.dumps(out), flush=True)
    return out


def write_tables(report_dir, model, ssims, psnrs, mses, rmse_stat: float):
    """stats.txt and the three per-image CSV files from fp32 host tensors [M]."""
    with open(os.path.join(report_dir, "stats.txt"), "w") as f:
        f.write(f"SSIM: {ssims.mean()}\n")
        f.write(f"PSNR: {psnrs.mean()}\n")
        f.write(f"RMSE: {rmse_stat}\n")
        f.write(f"FLOPs: {count_macs(model) if isinstance(model, torch.nn.Module) else 0}\n")
        f.write(f"Parameter count: {get_parameter_count(model)}\n")
    for fname, header, vals in (("ssim_per_image.csv", "image,ssim", ssims),
                                ("psnr_per_image.csv", "image,psnr", psnrs),
                                ("mse_per_image.csv", "image,mse", mses)):
        with open(os.path.join(report_dir, fname), "w") as f:
            f.write(header + "\n")
            for index, v in enumerate(vals):
                f.write(f"{str(index).zfill(5)},{v}\n")


def host_report(model, dataloader, dev, report_dir, clock):
    """--host-render: per-image metric calls, 16 strip passes over the whole data set, matplotlib and one PNG after the
    other on the host."""
    with torch.no_grad():
        preds = torch.cat([PF.denormalize(model(b[0].to(dev))) for b in dataloader], 0)
        targets = torch.cat([PF.denormalize(b[1].to(dev)) for b in dataloader], 0)
    clock.mark("forward")

    ssims, ssim_images, psnrs, mses = [], [], [], []
    for pred, target in zip(preds.split(64), targets.split(64)):
        s, full = PF.ssim_per_image(pred, target, return_full_image=True)
        ssims.append(s)
        ssim_images.append(full)
        psnrs.append(torch.stack([PF.psnr(p[None], t[None]) for p, t in zip(pred, target)]))
        mses.append(torch.stack([PF.rmse(p[None], t[None]) ** 2 for p, t in zip(pred, target)]))
    ssims, ssim_images = torch.cat(ssims).cpu(), torch.cat(ssim_images).cpu()
    psnrs, mses = torch.cat(psnrs).cpu(), torch.cat(mses).cpu()

    ssim_over_depth = depth_ssim(preds, targets)
    os.makedirs(report_dir, exist_ok=True)
    with open(os.path.join(report_dir, "depth_ssim.csv"), "w") as f:
        f.write("depth,mean,std\n")
        for depth, (mean, std) in enumerate(ssim_over_depth, 1):
            f.write(f"{depth},{mean},{std}\n")
    outputs_dir = os.path.join(report_dir, "outputs")
    os.makedirs(outputs_dir, exist_ok=True)
    for index, pred in enumerate(preds.cpu()):
        output_hot_image(pred, os.path.join(outputs_dir, f"{str(index).zfill(5)}.png"), clock)
    ssim_dir = os.path.join(report_dir, "ssim_images")
    os.makedirs(ssim_dir, exist_ok=True)
    for index, img in enumerate(ssim_images):
        write_png(to_int(img.clamp(0, 1)), os.path.join(ssim_dir, f"{str(index).zfill(5)}.png"), clock)

    rmse_stat = PF.rmse(preds, targets)
    clock.mark_less_png("eval")             # metrics, copies to the host and the colormap; the PNG files on their own
    write_tables(report_dir, model, ssims, psnrs, mses, float(rmse_stat))
    clock.mark("tables")


class _PinnedSet:
    """Host side of one chunk in flight: pinned buffers the copy stream fills and the PNG threads read."""

    def __init__(self, c, h, w):
        self.maps = torch.empty((CHUNK, c, h, w), dtype=torch.uint8).pin_memory()
        self.hot = torch.empty((CHUNK, 3, h, w), dtype=torch.uint8).pin_memory()
        self.nums = torch.empty((CHUNK, 3 + NUM_DEPTHS), dtype=torch.float32).pin_memory()
        self.sse = torch.empty((CHUNK,), dtype=torch.float64).pin_memory()
        self.copied = torch.cuda.Event()
        self.files = []               # PNG jobs that still read this set


def device_report(model, dataloader, dev, report_dir, clock) -> bool:
    """The report with everything between the forward pass and the PNG encoder on the device.  Returns False, having
    written nothing, for images whose height is not a multiple of the 16 depth strips (the host path chunks those
    unevenly)."""
    outputs_dir, ssim_dir = os.path.join(report_dir, "outputs"), os.path.join(report_dir, "ssim_images")
    copy_stream = torch.cuda.Stream(dev)
    sets, rows, sse_rows = [], [], []
    state = {"index": 0, "chunk": 0, "pending": None}

    def finish(pending):
        """The copy of a chunk has been queued: wait for it, keep its numbers, hand its images to the PNG threads."""
        ps, n, _keep = pending
        ps.copied.synchronize()
        rows.append(ps.nums[:n].clone())
        sse_rows.append(ps.sse[:n].clone())
        maps, hot = ps.maps.numpy(), ps.hot.numpy()
        for i in range(n):
            name = f"{str(state['index'] + i).zfill(5)}.png"
            ps.files.append(pool.submit(save_png, hot[i], os.path.join(outputs_dir, name)))
            ps.files.append(pool.submit(save_png, maps[i], os.path.join(ssim_dir, name)))
        state["index"] += n

    def drain(ps):
        for f in ps.files:
            f.result()
        ps.files = []

    def evaluate(pred, target):
        n, c, h, w = pred.shape
        if not sets:
            for d in (outputs_dir, ssim_dir):
                os.makedirs(d, exist_ok=True)
            sets.extend(_PinnedSet(c, h, w) for _ in range(2))
        ps = sets[state["chunk"] % 2]
        state["chunk"] += 1
        drain(ps)                                  # the chunk before the previous one: its files are written
        res = PF.eval_images(pred, target, denorm=True, strips=NUM_DEPTHS, ssim_map=True, hot=True)
        nums = torch.cat([torch.stack([res.ssim, res.psnr, res.mse], 1), res.strip_ssim], 1)
        copy_stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(copy_stream):
            ps.maps[:n].copy_(res.ssim_map_u8, non_blocking=True)
            ps.hot[:n].copy_(res.hot_u8[:, 0], non_blocking=True)      # channel 0, as reference report.py:230
            ps.nums[:n].copy_(nums, non_blocking=True)
            ps.sse[:n].copy_(res.sse, non_blocking=True)
            ps.copied.record(copy_stream)
        # this chunk is queued on the device: now wait for the previous one and start its PNG files
        if state["pending"] is not None:
            finish(state["pending"])
        state["pending"] = (ps, n, (res, nums, pred, target))
        if clock.sync:                             # stage timing: no overlap, every stage runs to its end
            finish(state["pending"])
            state["pending"] = None
            clock.mark("eval")
            drain(ps)
            clock.mark("png")

    with ThreadPoolExecutor(max_workers=PNG_THREADS) as pool, torch.no_grad():
        held_p, held_t, held = [], [], 0
        for b in dataloader:
            pred, target = model(b[0].to(dev)), b[1].to(dev)
            if not sets and not held and pred.shape[2] % NUM_DEPTHS:
                return False
            held_p.append(pred)
            held_t.append(target)
            held += pred.shape[0]
            while held >= CHUNK:
                clock.mark("forward")
                p, t = torch.cat(held_p, 0), torch.cat(held_t, 0)
                evaluate(p[:CHUNK].contiguous(), t[:CHUNK].contiguous())
                held_p, held_t, held = [p[CHUNK:]], [t[CHUNK:]], held - CHUNK
        clock.mark("forward")
        if held:
            evaluate(torch.cat(held_p, 0).contiguous(), torch.cat(held_t, 0).contiguous())
        if state["pending"] is not None:
            finish(state["pending"])
        for ps in sets:
            drain(ps)
    if not rows:
        raise RuntimeError("the data set is empty")
    nums, sse = torch.cat(rows), torch.cat(sse_rows)
    ssims, psnrs, mses, strips = nums[:, 0].contiguous(), nums[:, 1].contiguous(), nums[:, 2].contiguous(), nums[:, 3:]
    c, h, w = sets[0].maps.shape[1:]
    os.makedirs(report_dir, exist_ok=True)
    with open(os.path.join(report_dir, "depth_ssim.csv"), "w") as f:
        f.write("depth,mean,std\n")
        table = torch.stack([strips.double().mean(0), strips.double().std(0)], 1).float()
        for depth, (mean, std) in enumerate(table, 1):
            f.write(f"{depth},{mean},{std}\n")
    rmse_stat = torch.sqrt(sse.sum() / (sse.numel() * c * h * w)).float()
    write_tables(report_dir, model, ssims, psnrs, mses, float(rmse_stat))
    clock.mark("tables")
    return True


def build_parser():
    parser = ArgumentParser()
    parser.add_argument("name")
    parser.add_argument("-c", "--checkpoint", type=pathlib.Path, help="Path to checkpoint")
    parser.add_argument("-d", "--data", type=pathlib.Path, help="YAML file of all data points")
    parser.add_argument("-bs", "--batch-size", default=2, type=int)
    parser.add_argument("-m", "--model", default="pix2pix",
                        choices=["pix2pix", "attention_unet", "res18_unet", "res50_unet", "resv2_unet",
                                 "resnext_unet", "trans_unet", "palette", "identity"])
    parser.add_argument("--device-cache", default=False, action="store_true",
                        help="resize on the GPU and read the batches from device memory")
    parser.add_argument("--host-render", default=False, action="store_true",
                        help="metrics per image, colormap and PNG files on the host, one after the other")
    parser.add_argument("--stage-times", default=False, action="store_true",
                        help="synchronise between the stages and print their wall times as one JSON line")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
