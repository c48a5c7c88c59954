"""GPU: the deterministic mode on whole training steps.  Two fresh models from one seed end in the same bits -- every
parameter, Adam moment, BatchNorm running statistic and logged value -- eagerly, from a recorded launch plan, and at a size
whose weight gradients are split over the pixels; the reference fixture still holds inside the tolerances of
tests/test_gpu_model.py; pai_order_dependent_launches does not move over any of it.  Palette: two fit_steps with the device
generator, and a run interrupted at an epoch boundary and resumed against an uninterrupted one (DESIGN.md 7c's NOT MEASURED
line)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import oracle
from oracle.gen_golden import synth_batch

import _palette_util as U
import test_gpu_model as tgm
from _gpu_util import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF = torch.float32, torch.bfloat16


@pytest.fixture
def det(pai):
    from thesis_pai_reconstruction_amd import ops
    pai.set_deterministic(True)          # before any model of the test is built
    start = ops.order_dependent_launches()
    yield ops
    try:
        assert ops.order_dependent_launches() == start, "a launch under the mode took an arrival-order path"
    finally:
        ops.set_tunable("deterministic")


def _snapshot(m):
    """Every tensor of the training state, on the host: parameters and buffers, Adam moments, logged values."""
    torch.cuda.synchronize()
    out = {"state." + k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for i, opt in enumerate(m._all_optimizers()):
        if hasattr(opt, "_engine"):
            a = opt._engine.arena()
            out[f"opt{i}.m"], out[f"opt{i}.v"] = a.mflat.detach().cpu().clone(), a.vflat.detach().cpu().clone()
        else:
            for j, p in enumerate(opt.param_groups[0]["params"]):
                for key in ("exp_avg", "exp_avg_sq"):
                    out[f"opt{i}.{j}.{key}"] = opt.state[p][key].detach().cpu().clone()
    for k, v in m.logged.items():
        out["log." + k] = torch.as_tensor(v).detach().cpu().clone().reshape(-1)
    return out


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    assert any(k.startswith("opt") for k in a) and any(k.startswith("log.") for k in a), sorted(a)[:5]
    bad = [k for k in a if not (a[k].shape == b[k].shape and torch.equal(a[k], b[k]))]
    assert not bad, (what, len(bad), bad[:6])
    assert all(bool(torch.isfinite(v.double()).all()) for v in a.values()), what


def _gan_run(pai, mults, seed, n, size, dtype, steps, planned=False):
    m, _, _ = tgm.build(pai, mults, "gan", seed, dtype)
    x, t = synth_batch(seed + 100, n, size)
    batch = (x.to(dev()), t.to(dev()))
    step = m.training_step
    if planned:
        from thesis_pai_reconstruction_amd import plan
        step = plan.PlannedStep(m)
    snaps = []
    for s in range(steps):
        step(batch, s)
        snaps.append(_snapshot(m))
    return m, snaps, step


def _tiny(golden_dir):
    z = tgm._load(golden_dir, "ref_gan_tiny")
    return [int(v) for v in z["meta.mults"]], int(z["meta.seed"]), int(z["meta.n"]), int(z["meta.size"])


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_gan_step_twice_same_bits(pai, det, golden_dir, dtype):
    mults, seed, n, size = _tiny(golden_dir)
    _, a, _ = _gan_run(pai, mults, seed, n, size, dtype, 3)
    _, b, _ = _gan_run(pai, mults, seed, n, size, dtype, 3)
    for s in range(3):
        _same(a[s], b[s], f"step {s}")


def test_gan_step_planned_equals_eager(pai, det, golden_dir):
    """Three eager warm-up calls, then recorded and replayed steps, against six eager steps of a second model."""
    mults, seed, n, size = _tiny(golden_dir)
    _, eager, _ = _gan_run(pai, mults, seed, n, size, BF, 6)
    _, planned, step = _gan_run(pai, mults, seed, n, size, BF, 6, planned=True)
    assert step.disabled is None and step.records >= 1 and step.replays >= 1, step.describe()
    for s in range(6):
        _same(eager[s], planned[s], f"step {s}")
    # the mode is part of the plan signature: a step recorded under it is not replayed after the switch
    x, t = synth_batch(seed + 100, n, size)
    batch = (x.to(dev()), t.to(dev()))
    sig_on = step._signature(batch)
    pai.set_deterministic(False)
    try:
        assert step._signature(batch) != sig_on and step._signature(batch) not in step.plans
    finally:
        pai.set_deterministic(True)
    assert step._signature(batch) == sig_on


def test_gan_step_with_split_weight_gradients(pai, det):
    """64 x 64, batch 8: the queries report pixel-split weight gradients (a slab workspace in default mode) for at least two
    layers of the generator and of the discriminator's doubled batch; two runs agree bit for bit over three steps."""
    ops = det
    mults, seed, n, size = (1, 2, 4, 4), 5, 8, 64
    m, a, _ = _gan_run(pai, mults, seed, n, size, BF, 3)
    descs = []
    for mod in m.modules():
        eng = getattr(mod, "engine", None) if hasattr(type(mod), "engine") else None
        for P in (eng._plans.values() if eng is not None and hasattr(eng, "_plans") else ()):
            descs += P.get("desc", []) + P.get("enc_desc", []) + P.get("dec_desc", [])
    assert len(descs) >= 12, len(descs)
    pai.set_deterministic(False)
    try:
        split = [ops.conv_kernel_name(d, 2) for d in descs if ops.conv_wgrad_workspace_bytes(d) > 0]
        dependent = [d for d in descs if not ops.conv_wgrad_order_free(d, True)]
    finally:
        pai.set_deterministic(True)
    assert len(split) >= 2 and all(s.startswith("gg_wgrad_patch3_k") for s in split), split
    assert len(dependent) >= 2
    assert all(ops.conv_wgrad_order_free(d, True) for d in descs)
    _, b, _ = _gan_run(pai, mults, seed, n, size, BF, 3)
    for s in range(3):
        _same(a[s], b[s], f"step {s}")


@pytest.mark.parametrize("reuse", [True, False], ids=["one_forward", "two_forwards"])
def test_reference_fixture_under_the_mode(pai, det, golden_dir, reuse):
    """tests/test_gpu_model.py's comparison with ref_gan_tiny, its tolerances, under the mode."""
    tgm.test_gan_training_step_matches_reference_fixture(pai, golden_dir, "ref_gan_tiny", reuse)


def _palette_run(pai, dtype, steps=2):
    m = U.init_portable(pai.Palette(**dict(U.palette_kwargs("a"), dropout=0.1)), U.CONFIGS["a"][4]).to(dev())
    m.train()
    m.set_precision("32" if dtype == F32 else "bf16-mixed")
    m.device_rng = pai.DeviceRNG(123)
    (opt,), (sched,) = m.make_optimizers()
    x, y0 = (t.to(dev()) for t in U.inputs("a"))
    losses = [m.fit_step((x, y0), opt, sched).detach().cpu().clone() for _ in range(steps)]
    torch.cuda.synchronize()
    out = {"state." + k: v.detach().cpu().clone() for k, v in m.state_dict().items() if k.startswith("unet.")}
    for j, p in enumerate(opt.param_groups[0]["params"]):
        for key, v in opt.state[p].items():
            if torch.is_tensor(v):
                out[f"opt.{j}.{key}"] = v.detach().cpu().clone()
    for i, l in enumerate(losses):
        out[f"log.loss{i}"] = l.reshape(-1)
    return out


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_palette_fit_steps_same_bits(pai, det, dtype):
    a, b = _palette_run(pai, dtype), _palette_run(pai, dtype)
    assert sum(k.startswith("state.unet.") for k in a) > 20
    _same(a, b, "palette")


def test_palette_resume_equals_uninterrupted(pai, det, tmp_path, monkeypatch):
    """scripts/train_palette.py --synthetic 4 --device-rng --deterministic: 4 steps, against 2 steps + --resume for 2 more
    (batch 2: the interruption falls on an epoch boundary, where the loader's position is part of the checkpoint)."""
    spec = importlib.util.spec_from_file_location("_train_palette_det", os.path.join(ROOT, "scripts", "train_palette.py"))
    tp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tp)
    monkeypatch.chdir(tmp_path)
    common = ["--synthetic", "4", "--image-size", "16", "--batch-size", "2", "--channel-mults", "1,2", "--attention-res", "2",
              "--inference-steps", "2", "--log-every", "1", "--seed", "77", "--device-rng", "--deterministic"]
    run = lambda name, *more: tp.main(tp.build_parser().parse_args([name] + common + list(more)))
    whole = run("whole", "--steps", "4")
    part = run("part", "--steps", "2")
    run("part", "--steps", "4", "--resume", part["checkpoint"])
    a = torch.load(whole["checkpoint"], map_location="cpu", weights_only=False)
    b = torch.load(part["checkpoint"], map_location="cpu", weights_only=False)
    assert a["global_step"] == b["global_step"] == 4 and a["device_rng"] == b["device_rng"] and a["epoch"] == b["epoch"]

    def tensors(obj, prefix, out):
        if torch.is_tensor(obj):
            out[prefix] = obj
        elif isinstance(obj, dict):
            for k, v in obj.items():
                tensors(v, f"{prefix}.{k}", out)
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                tensors(v, f"{prefix}.{i}", out)
        return out

    ta, tb = tensors(a, "ckpt", {}), tensors(b, "ckpt", {})
    assert ta.keys() == tb.keys() and len(ta) > 40
    assert any(".optimizer_states." in k for k in ta)
    bad = [k for k in ta if not torch.equal(ta[k], tb[k])]
    assert not bad, (len(bad), bad[:6])
    assert a["lr_schedulers"] == b["lr_schedulers"]
