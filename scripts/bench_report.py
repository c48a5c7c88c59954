"""The report on ONE box: `report.py` of a Pix2Pix checkpoint (bench.py's generator, freshly initialised) over PNG pairs,
through the device evaluation (default) and through ``--host-render`` (per-image metric calls, matplotlib and a serial PNG
loop on the host: the path this CLI had before), arms interleaved, in one process.  Per arm and repetition two runs and one
JSON line each:

    {"arm": ..., "mode": "plain",  "total_s": ..., "images_per_s": ...}
    {"arm": ..., "mode": "staged", "total_s": ..., "forward_s": ..., "eval_s": ..., "png_s": ..., "tables_s": ...}

``plain`` is the report as a user runs it (the stages of the device arm overlap; only the total means something).
``staged`` synchronises between the stages: ``forward_s`` is the loader plus the generator, ``eval_s`` everything between
the forward pass and the PNG encoder (metrics, SSIM maps, colormap, bytes on the host), ``png_s`` encoding and writing the
files, ``tables_s`` the CSV files and stats.txt.  Model load and ``datamodule.setup`` (with ``--device-cache``, the
default here: decode + upload of every file) are outside the clock in both.

No profiler in this process; the launches of the evaluation kernel come from

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_report.py --arms device --pairs 512 --reps 1 --modes plain
    python scripts/bench_report.py --kernel-stats DIR --pairs 512
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

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


REPORT_SIZE = 256      # ImageDataModule resizes every file to 256 x 256 (--size is the size of the PNG files, not of the planes)


def write_checkpoint(pai, path):
    torch.manual_seed(0)
    model = pai.Pix2Pix(1, 1, (1, 2, 4, 8, 8, 8, 8, 8), 0.0, "gan")
    torch.save({"state_dict": {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()},
                "hyper_parameters": model.hparams}, path)


def run_arm(report, arm, mode, lst, ckpt, args):
    argv = [f"{arm}_{mode}", "-c", ckpt, "-d", lst, "-bs", str(args.batch_size), "-m", "pix2pix"]
    argv += ["--device-cache"] if args.device_cache else []
    argv += ["--host-render"] if arm == "host" else []
    argv += ["--stage-times"] if mode == "staged" else []
    out = report.main(report.build_parser().parse_args(argv))
    out["mode"], out["pairs"], out["batch_size"] = mode, args.pairs, args.batch_size
    out["images_per_s"] = round(args.pairs / out["total_s"], 1)
    return out


def kernel_stats(d, args):
    """Launches of the evaluation kernel from a rocprofv3 --kernel-trace --stats directory by grid, with the bytes a launch
    moves and the rate that gives; then every kernel that ran at least once per image (none is expected) and ssim_k."""
    rows = list(csv.DictReader(open(glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True)[0])))
    S = REPORT_SIZE
    mine = [r for r in rows if "eval_planes_k" in r["Kernel_Name"]]
    groups = {}
    for r in mine:
        groups.setdefault((int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])), []).append(
            (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for grid, us in sorted(groups.items()):
        us.sort()
        planes = grid[2]                                         # grid.z = planes (whole images, or 16 strips of each)
        whole = grid[1] * 32 >= S                                # grid.y = rows of 32-pixel tiles
        pixels = planes * S * (S if whole else S // 16)
        nbytes = pixels * (8 + (4 if whole else 0))              # two fp32 reads; the whole-image pass writes 1 + 3 bytes
        med = us[len(us) // 2]
        print(json.dumps({"kernel": "eval_planes_k", "pass": "images" if whole else "strips", "grid": grid, "launches": len(us),
                          "median_us": round(med, 2), "min_us": round(us[0], 2), "bytes": nbytes,
                          "GB_per_s": round(nbytes / med / 1e3, 1), "Mpixel_per_s": round(pixels / med, 1)}))
    counts = {}
    for r in rows:
        counts[r["Kernel_Name"]] = counts.get(r["Kernel_Name"], 0) + 1
    print(json.dumps({"images": args.pairs, "chunks": -(-args.pairs // 64), "eval_planes_k_launches": len(mine),
                      "ssim_k_launches": sum(v for k, v in counts.items() if "ssim_k" in k),
                      "kernels_with_a_launch_per_image_or_more": {k[:60]: v for k, v in counts.items() if v >= args.pairs}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--arms", default="host,device")
    ap.add_argument("--modes", default="plain,staged")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-loader", dest="device_cache", default=True, action="store_false",
                    help="decode the files in the report's host loader (inside the clock) instead of --device-cache")
    ap.add_argument("--kernel-stats", default=None, help="summarise a rocprofv3 output directory instead of running")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args)
    from bench_data import write_pairs
    cwd = os.getcwd()
    root = tempfile.mkdtemp(prefix="pai_bench_report_")
    try:
        os.chdir(root)                                            # report.py writes reports/<name> under the working directory
        import report
        torch.cuda.set_device(0)
        t0 = time.perf_counter()
        lst = write_pairs(root, args.pairs, args.size, seed=2000)
        ckpt = os.path.join(root, "bench.ckpt")
        write_checkpoint(report.pai, ckpt)
        print(json.dumps({"wrote_pairs": args.pairs, "size": args.size, "seconds": round(time.perf_counter() - t0, 1)}), flush=True)
        for _ in range(args.reps):
            for mode in args.modes.split(","):
                for arm in args.arms.split(","):
                    print(json.dumps(run_arm(report, arm, mode, lst, ckpt, args)), flush=True)
                    shutil.rmtree(os.path.join(root, "reports"), ignore_errors=True)
    finally:
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
