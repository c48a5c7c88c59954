"""Train pai.Palette with ``Palette.fit_step`` and write a checkpoint that ``pai.Palette.load_from_checkpoint`` and
``report.py -m palette`` load.

    python scripts/train_palette.py NAME --synthetic 64 --image-size 64 --steps 100
    python scripts/train_palette.py NAME -d train.yaml --steps 20000 --precision bf16-mixed

The loop is the one main.py does not have for this model: draw t, noise the target, the train-mode U-Net pass, the MSE +
variational-bound objective, backward, Adam, LinearLR -- all inside ``fit_step``, which returns the loss as a device scalar.
The loss is copied to the host only every ``--log-every`` steps.  The checkpoint goes to logs/NAME/palette.ckpt (or ``--out``)
with the hyper-parameters, the weights, the optimizer and scheduler states and the step count.

    python scripts/train_palette.py NAME --synthetic 64 --steps 200 --device-rng --seed 7
    python scripts/train_palette.py NAME --synthetic 64 --steps 400 --device-rng --resume logs/NAME/palette.ckpt

``--device-rng`` (default off) draws t, u, z and every dropout mask inside the kernels from ``pai.DeviceRNG(--seed)`` instead of
torch's generator; the checkpoint then also holds the generator's two integers (``device_rng``).  ``--resume CKPT`` restores
model, optimizer, scheduler, step count and that state and trains on to ``--steps``; with the device generator the draws of
step k are the same whether or not the run was interrupted before it.  The batches are not: the checkpoint holds the epoch
count, not the position inside an epoch, so a run resumed away from an epoch boundary starts a new epoch.  A checkpoint that
holds rng state is resumed with ``--device-rng`` only.  ``--deterministic`` adds ``pai.set_deterministic(True)``: together with
``--device-rng`` a run resumed at an epoch boundary ends in the bits of the uninterrupted one.
"""
import argparse
import os
import pathlib
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pai_bootstrap  # noqa: E402

pai = pai_bootstrap.load()


def to_tuple(text):
    return tuple(int(v) for v in str(text).split(",") if v != "")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("name")
    p.add_argument("-d", "--data", type=pathlib.Path, help="YAML list of training pairs (dataset.ImageDataModule)")
    p.add_argument("--synthetic", default=0, type=int, help="train on N synthetic pairs instead")
    p.add_argument("--image-size", default=256, type=int)
    p.add_argument("-s", "--steps", default=100, type=int)
    p.add_argument("--batch-size", default=2, type=int)
    p.add_argument("--precision", default="32")
    p.add_argument("--channel-mults", default="1,1,2,2,4,4")
    p.add_argument("--attention-res", default="16,8")
    p.add_argument("--dropout", default=0.1, type=float)
    p.add_argument("--schedule", default="linear", choices=["linear", "cosine"])
    p.add_argument("--learn-variance", default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("--inference-steps", default=100, type=int)
    p.add_argument("--log-every", default=10, type=int)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--device-rng", default=False, action=argparse.BooleanOptionalAction,
                   help="draw inside the kernels from pai.DeviceRNG(--seed); its state goes into the checkpoint")
    p.add_argument("--deterministic", default=False, action="store_true",
                   help="pai.set_deterministic: no sum depends on the arrival order of workgroups or atomics; with --device-rng "
                        "two runs from one seed, or an interrupted and an uninterrupted one, end in the same bits (the shuffle of an "
                        "epoch is then seeded by (--seed, epoch); without --device-rng torch's generator is left alone and a "
                        "resumed run sees other batches and draws)")
    p.add_argument("--resume", type=pathlib.Path, help="checkpoint of this script to continue from")
    p.add_argument("--out", type=pathlib.Path, help="checkpoint path (default logs/NAME/palette.ckpt)")
    return p


def main(args):
    from thesis_pai_reconstruction_amd.dataset import ImageDataModule, SyntheticDataModule
    if not torch.cuda.is_available():
        raise pai.PaiError("train_palette needs a HIP device; there is no CPU path")
    if bool(args.synthetic) == (args.data is not None):
        raise SystemExit("give either --synthetic N or -d LIST")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    if args.deterministic:
        pai.set_deterministic(True)      # before the model is built: its workspaces are sized for the mode
    model = pai.Palette(in_channels=1, out_channels=1, channel_mults=to_tuple(args.channel_mults),
                        attention_res=to_tuple(args.attention_res), dropout=args.dropout, schedule_type=args.schedule,
                        learn_var=args.learn_variance, inference_steps=args.inference_steps).to(dev)
    model.set_precision(args.precision)
    model.train()
    if args.synthetic:
        data = SyntheticDataModule(n_train=args.synthetic, n_val=args.batch_size, batch_size=args.batch_size, size=args.image_size,
                                   seed=1234, world=1, rank=0)
    else:
        data = ImageDataModule(args.data, None, batch_size=args.batch_size, normalize=True, world=1, rank=0, size=args.image_size)
    data.setup("fit")
    loader = data.train_dataloader()
    (opt,), (sched,) = model.make_optimizers()
    step, epoch, loss = 0, 0, None
    if args.device_rng:
        model.device_rng = pai.DeviceRNG(args.seed)
    if args.resume is not None:
        ckpt = torch.load(str(args.resume), map_location="cpu", weights_only=False)
        model.load_state_dict(ckpt["state_dict"])
        opt.load_state_dict(ckpt["optimizer_states"][0])
        sched.load_state_dict(ckpt["lr_schedulers"][0])
        step, epoch = int(ckpt["global_step"]), int(ckpt["epoch"])
        if args.device_rng:
            if "device_rng" not in ckpt:
                raise SystemExit(f"{args.resume} holds no device_rng state: it was not trained with --device-rng")
            model.device_rng.load_state_dict(ckpt["device_rng"])
        elif "device_rng" in ckpt:
            raise SystemExit(f"{args.resume} was trained with --device-rng: resume it with --device-rng (its draws continue from "
                             f"the stored state), not with torch's generator")
        print(f"resumed {args.resume} at step {step}", flush=True)
        if step >= args.steps:
            raise SystemExit(f"{args.resume} is already at step {step}: nothing to do for --steps {args.steps}")
    while step < args.steps:
        if hasattr(loader, "set_epoch"):
            loader.set_epoch(epoch)
        if args.deterministic and args.device_rng:
            # The single-process host loader shuffles from torch's generator: make the order of an epoch a function of (seed,
            # epoch), so that a run resumed at an epoch boundary sees the batches of the uninterrupted one.  Only with the
            # device generator, where nothing else of the step draws from torch's: without it t, the noise and the dropout
            # masks come from this stream, and re-seeding it per epoch would correlate the epochs' draws.
            torch.manual_seed(args.seed + 1000003 * (epoch + 1))
        seen = 0
        for x, y in loader:
            seen += 1
            loss = model.fit_step((x.to(dev), y.to(dev)), opt, sched)
            step += 1
            if step % args.log_every == 0 or step == args.steps:
                print(f"[step {step}] " + " ".join(f"{k}={float(v):.5g}" for k, v in model.logged.items())
                      + f" lr={opt.param_groups[0]['lr']:.4g}", flush=True)
            if step >= args.steps:
                break
        if not seen:
            raise SystemExit("the data set gives no batch")
        epoch += 1
    out = args.out or pathlib.Path("logs") / args.name / "palette.ckpt"
    os.makedirs(out.parent, exist_ok=True)
    tmp = str(out) + ".tmp"
    torch.save({"epoch": epoch, "global_step": step, "hyper_parameters": model.hparams,
                "state_dict": {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()},
                "optimizer_states": [opt.state_dict()], "lr_schedulers": [sched.state_dict()],
                **({"device_rng": model.device_rng.state_dict()} if model.device_rng is not None else {})}, tmp)
    os.replace(tmp, str(out))
    print(f"wrote {out} after {step} steps, loss {float(loss):.5g}", flush=True)
    return {"checkpoint": str(out), "steps": step, "loss": float(loss)}


if __name__ == "__main__":
    main(build_parser().parse_args())
