"""Generate tests/golden/ref_palette_objective_*.npz by running the REAL reference Palette training objective on the CPU.

Build container only (it needs the reference checkout):

    python scripts/gen_palette_objective_golden.py [k1 k2 k3 k4 a b b01 opt]

The reference is imported as scripts/gen_palette_golden.py imports it (the stand-in packages of oracle/shims ahead of it on
sys.path).  Only data is written; no reference source is copied.  Every run is made twice: in fp64 (the recorded truth) and in
fp32 (the yardstick).  ``torch.randint``, ``torch.randn_like`` and ``torch.rand_like`` are replaced by the recorded draws, and
``log`` by a recorder.  The fp64 runs keep the fp32 VALUES of the schedule buffers (``.double()`` of the buffers the reference
builds in fp32): the truth is exact arithmetic on the schedule the kernels read.

k1 .. k4  (kernel fixtures, KERNEL below: N, C, H, W, learn_var, t)
    The reference's ``DiffusionModel.forward`` / ``vlb_term`` / ``F.mse_loss`` on a synthetic model_out ~ N(0, 1), var channels
    x 0.5; y0 on the uint8 grid k / 255 * 2 - 1 with exact -1 and +1 planted at the first two pixels of every sample.
        y0, z, u, t, model_out          the inputs (fp32 values; NCHW)
        gamma, y_t64                    ``forward`` in fp64
        y_t, noise                      ``forward`` in fp32: the objective's inputs in BOTH runs, so that truth and kernel read the
                                        same numbers (at t <= 1, 1 - gamma is 1e-6 and y_t moves by 1e-5 between the precisions)
        mse, vlb_n, vlb, loss, dout     fp64
        dev32_vlb [N], dev32_gvar [N]   the fp32 run's relative deviation of vlb_n and (L2, over the sample) of the var gradient
        dev32_geps, dev32_mse           the same for the eps gradient (whole tensor) and the MSE
a, b, b01  (end to end: configuration a at t = (0, 700), b at t = (5, 1500), b at t = (0, 1))
    The reference's ``Palette.training_step`` + backward with the weights and x of tests/_palette_util.py at N = 2; y0 is that
    module's second input squashed onto the uint8 grid.
        x, y0, t, z, u                  the batch and the draws
        model_out                       the U-Net output (fp64)
        mse_loss, vlb_loss, loss        the logged values (fp64) and dev32_<name>
        keys, grad:<key>, dead, dev32:<key>, noise32:<key>, bn_*     as scripts/gen_palette_train_golden.py records them
        ref32_nan                       parameter gradients with a NaN in the reference's fp32 run: 0, except b01 (every one); there
                                        dev32:<key> / noise32:<key> come from the fp32 noising and U-Net under the fp64 objective
opt  three consecutive steps of configuration b under the reference's Adam + LinearLR (``configure_optimizers``)
        x, y0, t [3, N], z [3, ...], u [3, N], loss [3] (fp64), dev32_loss [3], lr [4] (before the first and after every step)

The assertions below are facts about the reference the tests rely on; a fixture that breaks one would pin nothing.

TEST INFRASTRUCTURE ONLY.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("PAI_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "shims"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from models.palette import DiffusionModel, Palette    # noqa: E402  (the reference's)
from oracle import golden                               # noqa: E402
from oracle.fingerprint import fingerprint              # noqa: E402
import _palette_util as U                               # noqa: E402
from gen_palette_golden import AsDouble, rel_l2         # noqa: E402
from gen_palette_train_golden import DEAD, _Null, bn_modules, bn_state      # noqa: E402

KERNEL = {
    "k1": (4, 1, 16, 16, True, [0, 1, 700, 1999]),
    "k2": (4, 1, 16, 16, False, [0, 0, 5, 1500]),
    "k3": (1, 3, 5, 7, True, [0]),                          # odd P: the pixel-by-pixel path
    "k4": (5, 3, 36, 36, True, [1, 5, 0, 1500, 1999]),      # two slabs, the second one ragged
}
E2E = {"a": ("a", (0, 700)), "b": ("b", (5, 1500)), "b01": ("b", (0, 1))}
OPT_T = ((5, 1500), (700, 3), (0, 1200))
GVAR_CAP, GVAR_T = 0.05, 1500


class Draws:
    """torch.randint / randn_like / rand_like replaced by the recorded draws (cast to the dtype of the argument)."""

    def __init__(self, t, z, u):
        self.t, self.z, self.u = t, z, u

    def __enter__(self):
        self.keep = (torch.randint, torch.randn_like, torch.rand_like)
        torch.randint = lambda *a, **k: self.t.clone()
        torch.randn_like = lambda v: self.z.to(v.dtype).reshape(v.shape)
        torch.rand_like = lambda v: self.u.to(v.dtype).reshape(v.shape)
        return self

    def __exit__(self, *exc):
        torch.randint, torch.randn_like, torch.rand_like = self.keep
        return False


def rel(a, b):
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / abs(b) if b != 0 else float("inf")


def rel_l2_or_zero(a, b):
    nb = float(b.double().norm())
    if nb == 0.0:
        return 0.0 if float(a.double().norm()) == 0.0 else float("inf")
    return rel_l2(a, b)


def grid_image(rng, shape):
    y0 = (rng.integers(0, 256, shape) / 255.0 * 2 - 1).astype(np.float32)
    y0.reshape(shape[0], shape[1], -1)[:, :, 0] = -1.0
    y0.reshape(shape[0], shape[1], -1)[:, :, 1] = 1.0
    return y0


def objective(dm, model_out, noise, y0, y_t, t, C):
    mo = model_out.clone().requires_grad_(True)
    eps = mo.split(C, dim=1)[0] if dm.learn_var else mo
    mse = F.mse_loss(eps, noise)
    vlb_n = dm.vlb_term(mo, y0, y_t, t)
    vlb = vlb_n.mean()
    loss = mse + 0.001 * vlb if dm.learn_var else mse
    loss.backward()
    return mse.detach(), vlb_n.detach(), vlb.detach(), loss.detach(), mo.grad.detach()


def generate_kernel(tag):
    N, C, H, W, learn_var, ts = KERNEL[tag]
    rng = np.random.default_rng(7000 + int(tag[1:]))
    co = 2 * C if learn_var else C
    y0 = torch.from_numpy(grid_image(rng, (N, C, H, W)))
    z = torch.from_numpy(rng.standard_normal((N, C, H, W)).astype(np.float32))
    u = torch.from_numpy(rng.random(N).astype(np.float32))
    mo = rng.standard_normal((N, co, H, W)).astype(np.float32)
    if learn_var:
        mo[:, C:] *= np.float32(0.5)
    mo = torch.from_numpy(mo)
    t = torch.tensor(ts, dtype=torch.int64)
    dm32 = DiffusionModel("linear", 2000, 1e-6, 0.01, learn_var=learn_var)
    dm64 = DiffusionModel("linear", 2000, 1e-6, 0.01, learn_var=learn_var).double()
    assert torch.equal(dm64.gammas, dm32.gammas.double())
    with Draws(t, z, u):
        y_t64, noise64, gamma64 = dm64(y0.double(), t)
        y_t32, noise32, gamma32 = dm32(y0, t)
    assert torch.equal(noise64, noise32.double())
    mse, vlb_n, vlb, loss, dout = objective(dm64, mo.double(), noise32.double(), y0.double(), y_t32.double(), t, C)
    m32, v32, _, l32, d32 = objective(dm32, mo, noise32, y0, y_t32, t, C)
    rec = {"meta": np.array([N, C, H, W, int(learn_var)], np.int64), "t": t.numpy(), "y0": y0.numpy(), "z": z.numpy(), "u": u.numpy(),
           "model_out": mo.numpy(), "gamma": gamma64.numpy(), "y_t64": y_t64.numpy(), "y_t": y_t32.numpy(), "noise": noise32.numpy(),
           "mse": mse.numpy(), "vlb_n": vlb_n.numpy(), "vlb": vlb.numpy(), "loss": loss.numpy(), "dout": dout.numpy(),
           "dev32_mse": np.array(rel(m32, mse)), "dev32_loss": np.array(rel(l32, loss)),
           "dev32_vlb": np.array([rel(v32[n], vlb_n[n]) for n in range(N)]),
           "dev32_geps": np.array(rel_l2(d32[:, :C], dout[:, :C]))}
    if learn_var:
        rec["dev32_gvar"] = np.array([rel_l2_or_zero(d32[n, C:], dout[n, C:]) for n in range(N)])
        for n, tn in enumerate(ts):
            if tn <= GVAR_T:
                assert rec["dev32_gvar"][n] < GVAR_CAP, (tag, n, tn, rec["dev32_gvar"][n])
        assert int((rec["dev32_gvar"] > GVAR_CAP).sum()) <= 1, rec["dev32_gvar"]
    else:
        assert dout.shape[1] == C and float(loss) == float(mse)
        for n, tn in enumerate(ts):
            if tn == 0:
                assert float(vlb_n[n]) == 0.0, (tag, n, float(vlb_n[n]))
    assert float(rec["dev32_mse"]) < 1e-6 and float(rec["dev32_geps"]) < 1e-6
    print(tag, "t", ts, "vlb_n", vlb_n.numpy(), "dev32_vlb", rec["dev32_vlb"], "dev32_gvar", rec.get("dev32_gvar"),
          "dev32_geps", float(rec["dev32_geps"]), "y_t 32 vs 64", float((y_t32.double() - y_t64).abs().max()))
    golden.save(OUT, f"ref_palette_objective_{tag}", rec)


def e2e_batch(name):
    x, y = U.inputs(name)
    y0 = torch.round((torch.tanh(y) * 0.5 + 0.5) * 255) / 255 * 2 - 1
    return x, y0.float()


def build(name, mode):
    torch.manual_seed(0)
    model = Palette(**U.palette_kwargs(name))
    U.init_portable(model, U.CONFIGS[name][4])
    model.train()
    if mode == "f64":
        model.double()
    if mode == "mixed":
        import copy
        dm64 = copy.deepcopy(model.diffusion).double()
        model.diffusion.vlb_term = lambda mo, y_0, y_t, t: dm64.vlb_term(mo, y_0.double(), y_t.double(), t)
    return model


def draws_of(name, seed, t):
    _, _, (h, w), _, _, _ = U.CONFIGS[name]
    rng = np.random.default_rng(seed)
    z = torch.from_numpy(rng.standard_normal((U.N, 1, h, w)).astype(np.float32))
    u = torch.from_numpy(rng.random(U.N).astype(np.float32))
    return torch.tensor(t, dtype=torch.int64), z, u


def step(model, mode, x, y0, draws):
    """One reference training_step + backward; the U-Net output is grabbed by a forward hook.  mode "mixed": the fp32 noising
    and the fp32 U-Net under an fp64 objective (the hook hands the output on as double, ``vlb_term`` is that of a double copy of
    the schedule and ``F.mse_loss`` takes its target as double)."""
    cast = torch.float64 if mode == "f64" else torch.float32
    grabbed = {}

    def grab(m, i, o):
        grabbed["out"] = o.detach().clone()
        return o.double() if mode == "mixed" else None

    hook = model.unet.register_forward_hook(grab)
    mse = F.mse_loss
    if mode == "mixed":
        F.mse_loss = lambda a, b: mse(a, b.to(a.dtype))
    with (AsDouble() if mode == "f64" else _Null()), Draws(*draws):
        loss = model.training_step((x.to(cast), y0.to(cast)))
        fwd = bn_state(model.unet)
        logged = {k: float(v) for k, v in model.logged.items()}
        loss.backward()
        bwd = bn_state(model.unet)
    hook.remove()
    F.mse_loss = mse
    return logged, grabbed["out"].double(), fwd, bwd


def generate_e2e(tag):
    name, t = E2E[tag]
    x, y0 = e2e_batch(name)
    draws = draws_of(name, 8000 + sorted(E2E).index(tag), t)
    res = {}
    for mode in ("f64", "f32", "mixed"):
        model = build(name, mode)
        logged, out, fwd, bwd = step(model, mode, x, y0, draws)
        grads = {k: p.grad.detach().double() for k, p in model.unet.named_parameters()}
        res[mode] = (logged, out, fwd, bwd, grads, model)
    logged, out, fwd, bwd, g64, model = res["f64"]
    l32, out32, _, _, g32, _ = res["f32"]
    # b01: the reference's own fp32 backward returns NaN at t = 0 with this untrained network (a variance output of -18 takes
    # pow(a, 3) to inf, whose backward is 0 * inf).  Its gradient yardsticks are then those of the reference's fp32 noising and
    # fp32 U-Net under its objective in fp64: their own fp32 error, carried through the exact objective of this very fixture.
    nan32 = sum(int(torch.isnan(g32[k]).any()) for k in g64)
    assert (nan32 > 0) == (tag == "b01"), (tag, nan32)
    if nan32:
        g32 = res["mixed"][4]
        assert not any(bool(torch.isnan(v).any()) for v in g32.values())
    keys = list(g64)
    rec = {"x": x.numpy(), "y0": y0.numpy(), "t": draws[0].numpy(), "z": draws[1].numpy(), "u": draws[2].numpy(),
           "model_out": out.numpy(), "dev32_out": np.array(rel_l2(out32, out)), "keys": np.array(keys)}
    for k in ("mse_loss", "vlb_loss", "loss"):
        rec[k] = np.array(logged[k])
        rec["dev32_" + k] = np.array(rel(l32[k], logged[k]))
    bns = bn_modules(model.unet)
    rec["bn_names"] = np.array([n for n, _ in bns])
    rec["bn_sizes"] = np.array([m.num_features for _, m in bns], np.int64)
    for k, (a, b) in zip(("mean", "var", "nbt"), zip(fwd, bwd)):
        rec[f"bn_{k}_fwd"], rec[f"bn_{k}_bwd"] = a, b
    norms = {k: float(v.norm()) for k, v in g64.items()}
    dead = [k for k in keys if DEAD.search(k)]
    live = [k for k in keys if k not in dead]
    # dead: zero in exact arithmetic (fp64 rounding noise of the largest gradient); live: at least a million times that
    assert max(norms[k] for k in dead) < 1e-11 * max(norms.values()), (max(norms[k] for k in dead), max(norms.values()))
    assert min(norms[k] for k in live) >= 1e6 * max(norms[k] for k in dead) and min(norms[k] for k in live) >= 1e-4
    rec["dead"] = np.array([int(k in dead) for k in keys], np.int64)
    for k in keys:
        rec["grad:" + k] = fingerprint(g64[k])
    for k in live:
        rec["dev32:" + k] = np.array(rel_l2(g32[k], g64[k]))
    for k in dead:
        rec["noise32:" + k] = np.array(float(g32[k].norm()))
    rec["ref32_nan"] = np.array(nan32, np.int64)
    worst = max(float(rec["dev32:" + k]) for k in live)
    print(tag, "t", t, {k: logged[k] for k in logged}, "dev32", {k: float(rec["dev32_" + k]) for k in logged},
          f"out {float(rec['dev32_out']):.2e} worst grad {worst:.2e} min live norm {min(norms[k] for k in live):.2e} "
          f"max dead norm {max(norms[k] for k in dead):.2e} noise32 {max(float(rec['noise32:' + k]) for k in dead):.2e}")
    golden.save(OUT, f"ref_palette_objective_{tag}", rec)


def generate_opt():
    name = "b"
    x, y0 = e2e_batch(name)
    all_draws = [draws_of(name, 8100 + i, t) for i, t in enumerate(OPT_T)]
    losses, lrs = {}, None
    for mode in ("f64", "f32"):
        model = build(name, mode)
        (opt,), (sched,) = model.configure_optimizers()
        lrs = [opt.param_groups[0]["lr"]]
        out = []
        for draws in all_draws:
            opt.zero_grad()
            logged, _, _, _ = step(model, mode, x, y0, draws)
            opt.step()
            sched.step()
            out.append(logged["loss"])
            lrs.append(opt.param_groups[0]["lr"])
        losses[mode] = out
    g = opt.param_groups[0]
    assert (g["betas"], g["eps"], g["weight_decay"]) == ((0.9, 0.999), 1e-8, 0) and type(opt).__name__ == "Adam"
    rec = {"x": x.numpy(), "y0": y0.numpy(), "t": np.stack([d[0].numpy() for d in all_draws]),
           "z": np.stack([d[1].numpy() for d in all_draws]), "u": np.stack([d[2].numpy() for d in all_draws]),
           "loss": np.array(losses["f64"]), "dev32_loss": np.array([rel(a, b) for a, b in zip(losses["f32"], losses["f64"])]),
           "lr": np.array(lrs)}
    for k, lr in enumerate(lrs):
        assert abs(lr - 1e-4 * (1 / 3 + (2 / 3) * k / 10000)) < 1e-18, (k, lr)
    print("opt", "loss", rec["loss"], "dev32", rec["dev32_loss"], "lr", rec["lr"])
    golden.save(OUT, "ref_palette_objective_opt", rec)


if __name__ == "__main__":
    for tag in (sys.argv[1:] or list(KERNEL) + list(E2E) + ["opt"]):
        if tag in KERNEL:
            generate_kernel(tag)
        elif tag in E2E:
            generate_e2e(tag)
        else:
            generate_opt()
