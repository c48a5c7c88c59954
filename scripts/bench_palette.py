"""Palette sampling on one GPU: images/s and ms per U-Net forward of ``pai.Palette.forward``, and ``pai_sattn_fwd`` alone
beside ``torch.nn.functional.scaled_dot_product_attention`` on the same data (both as TFLOP/s of 4 N heads T^2 ch), then
``pai_sattn_bwd`` (its three launches) beside the backward of the same SDPA call (both as TFLOP/s of the algorithmic
10 N heads T^2 ch; the kernels recompute S and execute 14).
Last the train-mode norm site ``pai_film_norm_fwd`` / ``pai_film_norm_bwd`` (FiLM + SiLU + mask, bf16) at the class-default levels,
as GB/s of the bytes the passes must move (forward: 2 tensors + the mask; backward: 5 tensors + 2 masks), beside torch's own
``batch_norm`` + FiLM + ``silu`` + mask forward and autograd on the same shapes (NCHW, torch's layout) and charged the same bytes.
``--train`` adds the row ``unet_train``: ms per ``UNet.forward_train`` + backward at the class defaults (dropout 0.1, masks drawn
per pass) at ``--train-batch`` images (default 4: the pass keeps every block's input, norm input and mask for the backward), with
``--count-launches`` also the kernel launches of one such pass as the profiler sees them; and ``avgpool2_bwd`` alone as GB/s
of the bytes it must move (read dout, write dx), the figure to put beside scripts/bench_hbm.py's rate.
Random normal data throughout (never zeros: MI355X_MICROARCH, data-dependent power).  One JSON line per measurement.

    python scripts/bench_palette.py [--precision bf16-mixed] [--batch 8] [--size 256] [--steps 100] [--mults 1,1,2,2,4,4]
                                    [--attention-res 16,8] [--no-sampler] [--no-attention] [--forward-only K]
                                    [--no-film-norm] [--film-norm-only] [--train] [--train-only] [--train-batch 4]
                                    [--count-launches] [--device-rng] [--planned]

``--device-rng`` adds a line after every film_norm row (``film_norm_device_rng``: the mask forms, the ``_rng`` forms and the three
torch launches that draw a mask, timed in turn on the same tensors; ``parent_path_ms`` = draw + forward + backward with a mask
against ``rng_path_ms`` = the two ``_rng`` calls) and a second sampling call with ``Palette.device_rng`` set
(``palette_sample_device_rng``).
``--planned`` runs nothing but the A/B of the planned sampler (``Palette.sampler_plan``) against the eager loop of the same build:
for every batch size of ``--planned-batches`` (default 1,2,8) one model with ``device_rng`` set, one warm-up call each way, then
``--planned-rounds`` (default 3) rounds of an eager and a planned sampling call in turn; the medians, the eager rounds' own
spread (the margin a difference has to clear), the host issue time of one reverse step each way (the Python loop timed
WITHOUT a synchronisation, on an idle device) beside its GPU time, and ``launches_per_step``.  One ``palette_planned`` line per
batch size.
``--forward-only K`` runs K U-Net forward passes and nothing else (the run to put under a kernel trace); ``--film-norm-only``
runs the film_norm rows and nothing else (no model is built).
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


FILM_NORM_SHAPES = [(65536, 64), (16384, 128), (1024, 256), (256, 256)]      # (rows, C) per sample: the class defaults at 256 x 256


def bench_film_norm_rng(dtype, n, rows, C, t):
    """The --device-rng line of one shape: the mask forms, the _rng forms (keep bits from csrc/philox.h, no mask tensor) and
    the three torch launches that draw a mask, timed in turn on the same tensors, three rounds, the median of each."""
    x, g, emb, gamma, beta, mask, keep, mean, rstd, out, dx, demb, dgb, ws, iters = t
    thr, seed = ops.dropout_thr(0.1), 0x9E3779B97F4A7C15
    runs = {
        "mask_fwd_ms": lambda: ops.film_norm_fwd(dtype, x, rows, n, C, mean, rstd, gamma, beta, emb, 2 * C, mask, keep, ops.ACT_SILU, out),
        "rng_fwd_ms": lambda: ops.film_norm_fwd_rng(dtype, x, rows, n, C, mean, rstd, gamma, beta, emb, 2 * C, seed, 16, 1, thr, keep,
                                                    ops.ACT_SILU, out),
        "mask_bwd_ms": lambda: ops.film_norm_bwd(dtype, g, x, rows, n, C, mean, rstd, gamma, beta, emb, 2 * C, mask, keep, ops.ACT_SILU,
                                                 dx, demb, dgb[:C], dgb[C:], ws),
        "rng_bwd_ms": lambda: ops.film_norm_bwd_rng(dtype, g, x, rows, n, C, mean, rstd, gamma, beta, emb, 2 * C, seed, 16, 1, thr, keep,
                                                    ops.ACT_SILU, dx, demb, dgb[:C], dgb[C:], ws),
        "mask_draw_ms": lambda: (torch.rand(x.shape, device=x.device) >= 0.1).to(torch.uint8),
    }
    seen = {k: [] for k in runs}
    for _ in range(3):
        for k, fn in runs.items():
            seen[k].append(timed(fn, 3, iters))
    row = {"bench": "film_norm_device_rng", "dtype": str(dtype), "N": n, "rows": rows, "C": C}
    row.update({k: round(sorted(v)[1], 4) for k, v in seen.items()})
    row["parent_path_ms"] = round(row["mask_draw_ms"] + row["mask_fwd_ms"] + row["mask_bwd_ms"], 4)
    row["rng_path_ms"] = round(row["rng_fwd_ms"] + row["rng_bwd_ms"], 4)
    print(json.dumps(row), flush=True)


def bench_film_norm(dtype, n, device_rng=False):
    es = torch.empty(0, dtype=dtype).element_size()
    for rows, C in FILM_NORM_SHAPES:
        numel = n * rows * C
        x, g = (torch.randn(n, rows, C, device="cuda").to(dtype) for _ in range(2))
        emb = (0.3 * torch.randn(n, 2 * C, device="cuda")).to(dtype)
        gamma, beta = 1 + 0.1 * torch.randn(C, device="cuda"), 0.1 * torch.randn(C, device="cuda")
        mask = (torch.rand(n, rows, C, device="cuda") >= 0.1).to(torch.uint8)
        keep = 1.0 / 0.9
        mean, rstd = x.float().mean((0, 1)), 1.0 / torch.sqrt(x.float().var((0, 1), unbiased=False) + 1e-5)
        out, dx, demb = torch.empty_like(x), torch.empty_like(x), torch.empty_like(emb)
        dgb = torch.zeros(2 * C, device="cuda")
        ws = torch.empty(ops.film_norm_ws_floats(n, rows, C), device="cuda")
        iters = 20 if numel > (1 << 24) else 100
        fwd_bytes, bwd_bytes = numel * (2 * es + 1), numel * (5 * es + 2)
        fms = timed(lambda: ops.film_norm_fwd(dtype, x, rows, n, C, mean, rstd, gamma, beta, emb, 2 * C, mask, keep, ops.ACT_SILU,
                                              out), 3, iters)
        bms = timed(lambda: ops.film_norm_bwd(dtype, g, x, rows, n, C, mean, rstd, gamma, beta, emb, 2 * C, mask, keep,
                                              ops.ACT_SILU, dx, demb, dgb[:C], dgb[C:], ws), 3, iters)
        row = {"bench": "film_norm", "dtype": str(dtype), "N": n, "rows": rows, "C": C, "fwd_ms": round(fms, 4),
               "fwd_GBps": round(fwd_bytes / fms / 1e6, 1), "bwd_ms": round(bms, 4), "bwd_GBps": round(bwd_bytes / bms / 1e6, 1)}
        # torch: the same site in its own layout, statistics included (it has no entry without them)
        side = int(rows ** 0.5)
        xt = x.view(n, side, side, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        gt = g.view(n, side, side, C).permute(0, 3, 1, 2).contiguous()
        mt = mask.view(n, side, side, C).permute(0, 3, 1, 2).contiguous().to(dtype) * keep
        et = emb.detach().requires_grad_(True)
        gw, bw = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

        def torch_fwd():
            v = torch.nn.functional.batch_norm(xt.float(), None, None, gw, bw, True, 0.1, 1e-5).to(dtype)
            return torch.nn.functional.silu(v * (1 + et[:, :C, None, None]) + et[:, C:, None, None]) * mt

        tf = timed(torch_fwd, 3, iters)
        yt = torch_fwd()
        tb = timed(lambda: torch.autograd.grad(yt, (xt, et, gw, bw), gt, retain_graph=True), 3, iters)
        row.update(torch_fwd_ms=round(tf, 4), torch_fwd_GBps=round(fwd_bytes / tf / 1e6, 1), torch_bwd_ms=round(tb, 4),
                   torch_bwd_GBps=round(bwd_bytes / tb / 1e6, 1))
        print(json.dumps(row), flush=True)
        if device_rng:
            bench_film_norm_rng(dtype, n, rows, C, (x, g, emb, gamma, beta, mask, keep, mean, rstd, out, dx, demb, dgb, ws, iters))


AVGPOOL_SHAPES = [(256, 128), (128, 128), (64, 256), (32, 256), (16, 512)]     # (H = W of dx, C): the class defaults at 256 x 256


def bench_avgpool_bwd(dtype, n):
    es = torch.empty(0, dtype=dtype).element_size()
    for side, C in AVGPOOL_SHAPES:
        dout = torch.randn(n, side // 2, side // 2, C, device="cuda").to(dtype)
        dx = torch.empty(n, side, side, C, dtype=dtype, device="cuda")
        ms = timed(lambda: ops.avgpool2_bwd(dtype, dout, n, side, side, C, dx), 3, 100)
        print(json.dumps({"bench": "avgpool2_bwd", "dtype": str(dtype), "N": n, "H": side, "W": side, "C": C, "ms": round(ms, 4),
                          "GBps": round((dout.numel() + dx.numel()) * es / ms / 1e6, 1)}), flush=True)


def bench_train(a, mults, att):
    """ms per forward_train + backward at the class defaults (dropout 0.1); optionally the launches of one pass."""
    dev = torch.device("cuda:0")
    model = pai.Palette(1, 1, mults, att, 0.1, "linear", False)
    with torch.no_grad():
        for k, v in model.unet.state_dict().items():
            if k.endswith("running_var"):
                v.uniform_(1.0, 1.2)
            elif v.dim() > 1:
                v.normal_(0.0, 0.02)
    model.to(dev)
    model.train()
    model.set_precision(a.precision)
    n = a.train_batch
    x, y = torch.randn(n, 1, a.size, a.size, device=dev), torch.randn(n, 1, a.size, a.size, device=dev)
    g = torch.rand(n, device=dev)
    dout = torch.randn(n, 1, a.size, a.size, device=dev)

    def step():
        for p in model.unet.parameters():
            p.grad = None
        model.unet.forward_train(x, y, g).backward(dout)

    ms = timed(step, 2, 5)
    row = {"bench": "unet_train", "precision": a.precision, "N": n, "size": a.size, "mults": mults, "attention_res": att,
           "dropout": 0.1, "ms": round(ms, 3), "tflops": round(6 * n * model.unet.macs(a.size, a.size) / ms / 1e9, 2),
           "peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "launches": None}
    if a.count_launches:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.name
                   and "Memset" not in e.name]
        row["launches"] = len(kernels)
        row["library_launches"] = sum(1 for e in kernels if not e.name.startswith("void at::") and "at::native" not in e.name)
    print(json.dumps(row), flush=True)


def bench_planned(a, model, dev):
    """Eager against planned sampling, interleaved; ``model`` is frozen, at its precision, with a DeviceRNG."""
    import time

    def call(planned, x):
        model.sampler_plan = planned
        t0 = time.perf_counter()
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        model(x)
        b0.record()
        host = time.perf_counter() - t0             # the loop has been issued; nothing has been waited for
        torch.cuda.synchronize()
        return a0.elapsed_time(b0), host * 1e3

    for n in [int(v) for v in a.planned_batches.split(",")]:
        x = torch.randn(n, 1, a.size, a.size, device=dev)
        model.device_rng = pai.DeviceRNG(0)
        for planned in (False, True):               # warm-up: descriptors, workspace, the recording call
            call(planned, x)
        seen = {False: [], True: []}
        for _ in range(max(a.planned_rounds, 3)):
            for planned in (False, True):
                seen[planned].append(call(planned, x))
        med = lambda v: sorted(v)[len(v) // 2]
        e_ms, p_ms = [g for g, _ in seen[False]], [g for g, _ in seen[True]]
        e_host, p_host = [h for _, h in seen[False]], [h for _, h in seen[True]]
        info = model.sampler_plan_info()
        print(json.dumps({"bench": "palette_planned", "precision": a.precision, "N": n, "size": a.size, "steps": a.steps,
                          "rounds": len(e_ms), "eager_ms": round(med(e_ms), 2), "planned_ms": round(med(p_ms), 2),
                          "eager_spread_ms": round(max(e_ms) - min(e_ms), 2), "planned_spread_ms": round(max(p_ms) - min(p_ms), 2),
                          "eager_all_ms": [round(v, 2) for v in e_ms], "planned_all_ms": [round(v, 2) for v in p_ms],
                          "eager_step_gpu_ms": round(med(e_ms) / a.steps, 3), "planned_step_gpu_ms": round(med(p_ms) / a.steps, 3),
                          "eager_step_host_ms": round(med(e_host) / a.steps, 3),
                          "planned_step_host_ms": round(med(p_host) / a.steps, 3),
                          "launches_per_step": info["launches_per_step"], "records": info["records"], "replays": info["replays"],
                          "disabled": info["disabled"]}), flush=True)
    model.sampler_plan, model.device_rng = False, None


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
    ap.add_argument("--no-film-norm", action="store_true")
    ap.add_argument("--film-norm-only", action="store_true")
    ap.add_argument("--device-rng", action="store_true",
                    help="add a line with the device generator (pai.DeviceRNG) to the film-norm and sampler timings")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-only", action="store_true")
    ap.add_argument("--train-batch", type=int, default=4)
    ap.add_argument("--count-launches", action="store_true")
    ap.add_argument("--planned", action="store_true", help="A/B of the planned sampler against the eager loop, nothing else")
    ap.add_argument("--planned-batches", default="1,2,8")
    ap.add_argument("--planned-rounds", type=int, default=3)
    a = ap.parse_args()
    if a.train_only:
        torch.manual_seed(0)
        bench_train(a, tuple(int(v) for v in a.mults.split(",")), tuple(int(v) for v in a.attention_res.split(",")))
        bench_avgpool_bwd(torch.bfloat16, a.batch)
        return
    if a.film_norm_only:
        torch.manual_seed(0)
        bench_film_norm(torch.bfloat16, a.batch, a.device_rng)
        return
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
    if a.planned:
        bench_planned(a, model, dev)
        return
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
        if a.device_rng:
            model.device_rng = pai.DeviceRNG(0)
            ms = timed(lambda: model(x), 1, 1)
            model.device_rng = None
            print(json.dumps({"bench": "palette_sample_device_rng", "precision": a.precision, "N": a.batch, "size": a.size,
                              "steps": a.steps, "seconds": round(ms / 1e3, 3), "images_per_s": round(a.batch / (ms / 1e3), 3),
                              "ms_per_unet_forward": round(ms / a.steps, 3)}), flush=True)
    if not a.no_attention:
        bench_attention(dtype, a.batch, 4)
    if not a.no_film_norm:
        bench_film_norm(torch.bfloat16, a.batch, a.device_rng)
    if a.train:
        del model
        bench_train(a, mults, att)
        bench_avgpool_bwd(torch.bfloat16, a.batch)


if __name__ == "__main__":
    main()
