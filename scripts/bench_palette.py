"""Palette sampling on one GPU: images/s and ms per U-Net forward of ``pai.Palette.forward``, and ``pai_sattn_fwd`` alone
beside ``torch.nn.functional.scaled_dot_product_attention`` on the same data (both as TFLOP/s of 4 N heads T^2 ch), then
``pai_sattn_bwd`` (its three launches) beside the backward of the same SDPA call (both as TFLOP/s of the algorithmic
10 N heads T^2 ch; the kernels recompute S and execute 14).
Random normal data throughout (never zeros: MI355X_MICROARCH, data-dependent power).  One JSON line per measurement.

    python scripts/bench_palette.py [--precision bf16-mixed] [--batch 8] [--size 256] [--steps 100] [--mults 1,1,2,2,4,4]
                                    [--attention-res 16,8] [--no-sampler] [--no-attention] [--forward-only K]

``--forward-only K`` runs K U-Net forward passes and nothing else (the run to put under a kernel trace).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import pai_bootstrap  # noqa: E402

pai = pai_bootstrap.load()
from thesis_pai_reconstruction_amd import nnops, ops  # noqa: E402

ATTN_SHAPES = [(1024, 128), (256, 128), (16384, 64)]          # (T, ch): the class defaults at 256 x 256, and the CLI's worst


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def bench_attention(dtype, n, heads):
    for T, ch in ATTN_SHAPES:
        qkv = torch.randn(n, T, heads * 3 * ch, device="cuda").to(dtype)
        out = torch.empty(n, T, heads * ch, dtype=dtype, device="cuda")
        flop = 4.0 * n * heads * T * T * ch
        iters = 5 if T > 4096 else 50
        ms = timed(lambda: ops.sattn_fwd(dtype, qkv, n, T, heads, ch, out), 2, iters)
        row = {"bench": "sattn_fwd", "dtype": str(dtype), "N": n, "heads": heads, "T": T, "ch": ch, "ms": round(ms, 4),
               "tflops": round(flop / ms / 1e9, 2)}
        q, k, v = (t.permute(0, 2, 1, 3) for t in qkv.view(n, T, heads, 3, ch).unbind(3))      # [n, heads, T, ch] views
        try:
            sd = timed(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v), 2, iters)
            ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n, T, heads * ch)
            row.update(sdpa_ms=round(sd, 4), sdpa_tflops=round(flop / sd / 1e9, 2),
                       max_diff=float((ref.float() - out.float()).abs().max()))
        except RuntimeError as e:           # e.g. the materialised form running out of memory at T = 16384
            row.update(sdpa_ms=None, sdpa_error=str(e).splitlines()[0][:120])
        print(json.dumps(row), flush=True)
        bench_attention_bwd(dtype, n, heads, T, ch, qkv, iters)


def bench_attention_bwd(dtype, n, heads, T, ch, qkv, iters):
    out = torch.empty(n, T, heads * ch, dtype=dtype, device="cuda")
    lse = torch.empty(n, heads, T, device="cuda")
    ops.sattn_fwd_lse(dtype, qkv, n, T, heads, ch, out, lse)
    dout = torch.randn(n, T, heads * ch, device="cuda").to(dtype)
    dqkv, ws = torch.empty_like(qkv), torch.empty(n * heads * T, device="cuda")
    flop = 10.0 * n * heads * T * T * ch
    ms = timed(lambda: ops.sattn_bwd(dtype, dout, qkv, out, lse, n, T, heads, ch, dqkv, ws), 2, iters)
    row = {"bench": "sattn_bwd", "dtype": str(dtype), "N": n, "heads": heads, "T": T, "ch": ch, "ms": round(ms, 4),
           "tflops": round(flop / ms / 1e9, 2)}
    try:
        q, k, v = (t.permute(0, 2, 1, 3).detach().requires_grad_(True) for t in qkv.view(n, T, heads, 3, ch).unbind(3))
        o = torch.nn.functional.scaled_dot_product_attention(q, k, v)
        do = dout.view(n, T, heads, ch).permute(0, 2, 1, 3)
        sd = timed(lambda: torch.autograd.grad(o, (q, k, v), do, retain_graph=True), 2, iters)
        ref = torch.stack(torch.autograd.grad(o, (q, k, v), do), 3).permute(0, 2, 1, 3, 4).reshape(n, T, heads * 3 * ch)
        row.update(sdpa_ms=round(sd, 4), sdpa_tflops=round(flop / sd / 1e9, 2),
                   max_diff=float((ref.float() - dqkv.float()).abs().max()))
    except RuntimeError as e:
        row.update(sdpa_ms=None, sdpa_error=str(e).splitlines()[0][:120])
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16-mixed")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--mults", default="1,1,2,2,4,4")
    ap.add_argument("--attention-res", default="16,8")
    ap.add_argument("--no-sampler", action="store_true")
    ap.add_argument("--no-attention", action="store_true")
    ap.add_argument("--forward-only", type=int, default=0)
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    mults, att = tuple(int(v) for v in a.mults.split(",")), tuple(int(v) for v in a.attention_res.split(","))
    model = pai.Palette(1, 1, mults, att, 0.0, "linear", False, inference_steps=a.steps)
    with torch.no_grad():                    # a fresh model predicts zero (zeroed last convolutions): give every tensor values
        for k, v in model.unet.state_dict().items():
            if k.endswith("running_var"):
                v.uniform_(1.0, 1.2)
            elif v.dim() > 1:               # every convolution / Linear weight, the zeroed ones included
                v.normal_(0.0, 0.02)
    model.to(dev)
    model.freeze()
    model.set_precision(a.precision)
    dtype = model.unet.compute_dtype
    x = torch.randn(a.batch, 1, a.size, a.size, device=dev)
    if a.forward_only or not a.no_sampler:
        xy = nnops.to_nhwc(torch.cat([x, torch.randn_like(x)], 1), dtype)
        g = torch.rand(a.batch, device=dev)
        ms = timed(lambda: model.unet.run(xy, g), 3, a.forward_only or 10)
        print(json.dumps({"bench": "unet_forward", "precision": a.precision, "N": a.batch, "size": a.size, "mults": mults,
                          "attention_res": att, "ms": round(ms, 3),
                          "tflops": round(2 * a.batch * model.unet.macs(a.size, a.size) / ms / 1e9, 2)}), flush=True)
    if a.forward_only:
        return
    if not a.no_sampler:
        ms = timed(lambda: model(x), 1, 1)               # one whole sampling call discarded as warm-up
        print(json.dumps({"bench": "palette_sample", "precision": a.precision, "N": a.batch, "size": a.size, "steps": a.steps,
                          "seconds": round(ms / 1e3, 3), "images_per_s": round(a.batch / (ms / 1e3), 3),
                          "ms_per_unet_forward": round(ms / a.steps, 3)}), flush=True)
    if not a.no_attention:
        bench_attention(dtype, a.batch, 4)


if __name__ == "__main__":
    main()
