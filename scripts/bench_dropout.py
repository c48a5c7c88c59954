"""What Dropout2d costs on the GAN step, and what the device generator changes: Pix2Pix at the BASELINE configs[1] shape
(256 x 256, batch 64, bf16) with the class default ``dropout = 0.5``, three paths of one build on one box:

  torch_eager   masks drawn by torch (full + bernoulli + div per site and forward), the step issued from Python -- the only
                path a model with dropout had before ``UnetWrapper.device_rng``
  rng_eager     ``model.device_rng = DeviceRNG(0)``: the keep flags formed inside pai_dropout2d_rng_dev, issued from Python
  rng_planned   the same step replayed from a recorded launch plan (plan.PlannedStep)

The paths run in turn, ``--rounds`` rounds of ``--steps`` timed steps each, after a common warm-up (the plan's three eager
calls and its two recordings fall there).  Per path: ms per step of every round and their median, the spread of the rounds, the
host time to issue one step (a loop timed without a synchronisation) and the launches of one step (library launches + kernels
torch launches itself).  One JSON line per path, then one ``dropout_summary`` line with the claim checked: planned <= torch_eager
beyond the torch_eager rounds' own spread.

    python scripts/bench_dropout.py [--rounds 3 --steps 100 --batch 64 --size 256 --dropout 0.5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MULTS = (1, 2, 4, 8, 8, 8, 8, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--precision", default="bf16-mixed")
    args = ap.parse_args()

    import pai_bootstrap
    pai = pai_bootstrap.load()
    from thesis_pai_reconstruction_amd import plan as pplan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(1234)
    x = torch.from_numpy(rng.random((args.batch, 1, args.size, args.size), dtype=np.float32) * 2 - 1).to(dev)
    t = torch.from_numpy(rng.random((args.batch, 1, args.size, args.size), dtype=np.float32) * 2 - 1).to(dev)
    batch = (x, t)

    def build(device_rng):
        torch.manual_seed(0)
        m = pai.Pix2Pix(1, 1, MULTS, args.dropout, "gan")
        m.to(dev)
        m.set_precision(args.precision)
        m.train()
        m.optimizers()
        if device_rng:
            m.device_rng = pai.DeviceRNG(0)
        return m

    paths = {}
    for name, device_rng, planned in (("torch_eager", False, False), ("rng_eager", True, False), ("rng_planned", True, True)):
        m = build(device_rng)
        paths[name] = {"model": m, "step": pplan.PlannedStep(m, warmup=3) if planned else m.training_step, "ms": []}

    for i in range(args.warmup):                    # clocks, lazy allocations, the plan's warm-up and recordings
        for p in paths.values():
            p["step"](batch, i)
    torch.cuda.synchronize()
    ps = paths["rng_planned"]["step"]
    if ps.disabled is not None or ps.replays < 1:
        raise SystemExit(f"the planned path did not replay: {ps.describe()}")

    for r in range(args.rounds):
        for p in paths.values():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                p["step"](batch, i)
            torch.cuda.synchronize()
            p["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)

    for name, p in paths.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(3):                          # three steps, as bench.py --full: more would fill the launch queue and
            p["step"](batch, i)                     # time the GPU through its back-pressure
        p["host_issue_ms"] = (time.perf_counter() - t0) / 3 * 1e3
        torch.cuda.synchronize()
        if name == "rng_planned":
            node = ps.describe()["nodes"][0]
            p["launches"], p["torch_kernels"] = node["launches"], 0
        else:
            rec = pplan._Recorder()                 # one eager step under the recorder: library launches and torch's own
            with rec:
                rec.begin()
                try:
                    p["model"].training_step(batch, 0)
                finally:
                    rec.end()
            p["launches"] = sum(it[1].info()["launches"] for it in rec.items if it[0] == "plan")
            p["torch_kernels"] = len(rec.foreign)
            torch.cuda.synchronize()

    out = {}
    for name, p in paths.items():
        out[name] = {"metric": "dropout_step", "path": name, "ms_per_step": round(statistics.median(p["ms"]), 4),
                     "rounds_ms": [round(v, 4) for v in p["ms"]], "spread_ms": round(max(p["ms"]) - min(p["ms"]), 4),
                     "host_issue_ms": round(p["host_issue_ms"], 3), "launches_per_step": p["launches"],
                     "torch_kernels_per_step": p["torch_kernels"], "batch": args.batch, "size": args.size,
                     "dropout": args.dropout, "precision": args.precision, "steps": args.steps}
        print(json.dumps(out[name]), flush=True)
    te, pl = out["torch_eager"], out["rng_planned"]
    print(json.dumps({"metric": "dropout_summary", "planned_minus_torch_eager_ms": round(pl["ms_per_step"] - te["ms_per_step"], 4),
                      "torch_eager_spread_ms": te["spread_ms"],
                      "planned_no_slower": pl["ms_per_step"] <= te["ms_per_step"] + te["spread_ms"],
                      "plan": ps.describe()["nodes"][0]}), flush=True)


if __name__ == "__main__":
    main()
