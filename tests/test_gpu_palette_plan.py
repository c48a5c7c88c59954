"""GPU: the planned Palette sampler.  The Palette kernels are recorded by a launch plan; the device-state forms of the step
kernel, the Philox fill and the counters have the bits of the by-value forms; a sampling call replayed from a recorded reverse
step has the bits of the eager loop of the same build, for recorded noise (the whole-chain fixtures) and for the device
generator, across weight reloads and batch-size changes, with ``output_process``, and without a host synchronisation."""
import numpy as np
import pytest
import torch

import _palette_util as U
from _gpu_util import dev
from oracle import golden

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CHAINS = ("a", "b")
POISON = 0x7FC12345          # a NaN pattern as int32 bits


def u32(v):
    """One uint32 as the int32 device scalar the counters are held in."""
    v = int(v) & 0xFFFFFFFF
    return torch.tensor([v - (1 << 32) if v >= 1 << 31 else v], dtype=torch.int32, device=dev())


def value(counter):
    return int(counter.cpu()[0]) & 0xFFFFFFFF


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def rnd(shape, seed, dtype=F32, scale=1.0):
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32)).to(dev()).to(dtype)


# ---- 1. recording coverage ---------------------------------------------------------------------------------------------------------
def _coverage_ops(ops):
    """name -> (output tensor, call): one call of each Palette entry point, one launch each."""
    n, rows, c = 2, 24, 16
    x = rnd((n, rows, c), 1)
    A, B = rnd((n, c), 2), rnd((n, c), 3)
    a, b = rnd((c,), 4), rnd((c,), 5)
    emb = rnd((n, 2 * c), 6, scale=0.3)
    out = {}
    o1 = torch.empty_like(x)
    out["pai_affine_act"] = (o1, lambda: ops.affine_act(F32, x, rows, n, c, A, B, True, ops.ACT_SILU, o1))
    o2 = torch.empty(2, n, c, device=dev())
    out["pai_film_coeffs"] = (o2, lambda: ops.film_coeffs(c, n, a, b, emb, 2 * c, o2[0], o2[1]))
    xp = rnd((n, 4, 6, 8), 7)
    o3 = torch.empty(n, 2, 3, 8, device=dev())
    out["pai_avgpool2"] = (o3, lambda: ops.avgpool2(F32, xp, n, 4, 6, 8, o3))
    g = torch.tensor([0.9, 0.2], device=dev())
    o4 = torch.empty(n, 32, device=dev())
    out["pai_gamma_embedding"] = (o4, lambda: ops.gamma_embedding(g, n, 32, o4))
    heads, ch, T = 2, 32, 40
    qkv = rnd((n, T, heads * 3 * ch), 8)
    o5 = torch.empty(n, T, heads * ch, device=dev())
    out["pai_sattn_fwd"] = (o5, lambda: ops.sattn_fwd(F32, qkv, n, T, heads, ch, o5))
    mo, y, z = rnd((37, 1), 9), rnd((37, 1), 10), rnd((37, 1), 11)
    o6 = torch.empty(37, 1, device=dev())
    out["pai_palette_step"] = (o6, lambda: ops.palette_step(F32, mo, y, z, 37, 1, False, True, (0.3, 1.1, 0.2, 0.7, -3.0, -2.0), o6))
    o7 = torch.empty(1021, device=dev())
    out["pai_philox_fill"] = (o7, lambda: ops.philox_fill(ops.PHILOX_NORMAL, o7, 77, 1, 3, 5))
    mean, rstd, gam = rnd((c,), 12, scale=0.1), 1 + rnd((c,), 13, scale=0.1).abs(), 1 + 0.1 * a
    o8 = torch.empty_like(x)
    out["pai_film_norm_fwd"] = (o8, lambda: ops.film_norm_fwd(F32, x, rows, n, c, mean, rstd, gam, b, emb, 2 * c, None, 1.0,
                                                              ops.ACT_SILU, o8))
    return out


def test_palette_launches_are_recorded(pai):
    """Every Palette entry point goes through the plan recorder: a plan recorded around one call holds its launch, and the
    replay into a poisoned output reproduces the eager bits.  (Before these launches were routed through the recorder the
    plan stayed empty.)"""
    from thesis_pai_reconstruction_amd import ops
    for name, (out, call) in _coverage_ops(ops).items():
        call()
        want = out.clone()
        out.view(torch.int32).fill_(POISON)
        plan = ops.Plan()
        with plan.recording():
            call()
        assert plan.info()["launches"] == 1, (name, plan.info())
        assert same_bits(out, want), name
        out.view(torch.int32).fill_(POISON)
        plan.run()
        assert same_bits(out, want), name
        plan.destroy()


# ---- 2. the step kernels --------------------------------------------------------------------------------------------------------------
T5 = 5


def _table5():
    g = np.random.default_rng(50)
    t = np.stack([g.uniform(0.05, 0.95, T5), g.uniform(1.0, 40.0, T5), g.uniform(0.01, 0.9, T5), g.uniform(0.1, 0.99, T5),
                  g.uniform(-9.0, -5.0, T5), g.uniform(-4.5, -1.0, T5)], 1).astype(np.float32)
    return torch.from_numpy(t).to(dev()), torch.from_numpy(g.uniform(0.001, 0.999, T5).astype(np.float32)).to(dev())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("learn_var", [False, True], ids=["fixed_var", "learn_var"])
def test_step_dev_forms_have_the_bits_of_the_value_forms(pai, dtype, learn_var):
    from thesis_pai_reconstruction_amd import ops
    table, gammas = _table5()
    rows = [tuple(float(v) for v in r) for r in table.cpu()]
    n, seed, rstep = 3, 0x123456789ABCDEF, (1 << 32) - 3
    for C in (1, 3):
        for pixels in (37, 512):
            mo = rnd((pixels, 2 * C if learn_var else C), 60 + C + pixels, dtype)
            y_t = rnd((pixels, C), 61 + C + pixels)
            stack = rnd((T5 + 1, pixels * C), 62 + C + pixels)
            step_dev = u32(rstep)
            last = {}
            for k in (1, 2, 3, 4, 5, 6):                     # 6 = T + 1: clamped to T
                kc = min(k, T5)
                i = T5 - kc
                pos = u32(k)
                for rng in (False, True):
                    y_w, xy_w = torch.empty(pixels, C, device=dev()), torch.zeros(pixels, 2 * C, dtype=dtype, device=dev())
                    y_g, xy_g = torch.empty_like(y_w), torch.zeros_like(xy_w)
                    gnext = torch.full((n,), -1.0, device=dev())
                    if rng:
                        ops.palette_step_rng(dtype, mo, y_t, pixels, C, learn_var, i > 1, rows[i], seed, kc, rstep, y_w, xy_w)
                        ops.palette_step_rng_dev(dtype, mo, y_t, pixels, C, learn_var, table, pos, gammas, n, gnext, seed, step_dev,
                                                 y_g, xy_g)
                    else:
                        ops.palette_step(dtype, mo, y_t, stack[kc].reshape(pixels, C), pixels, C, learn_var, i > 1, rows[i], y_w, xy_w)
                        ops.palette_step_dev(dtype, mo, y_t, stack, pixels, C, learn_var, table, pos, gammas, n, gnext, y_g, xy_g)
                    what = (C, pixels, k, rng)
                    assert same_bits(y_g, y_w) and same_bits(xy_g, xy_w), what
                    assert bool(torch.isfinite(y_g).all()), what
                    assert torch.equal(gnext, gammas[max(i - 1, 0)].expand(n)), what
                    assert value(pos) == k and value(step_dev) == rstep, what          # only read
                    last[(k, rng)] = y_g
            for rng in (False, True):
                assert same_bits(last[(6, rng)], last[(5, rng)])                        # the clamp


# ---- 3. counters and the fill ---------------------------------------------------------------------------------------------------------
def test_counters_wrap(pai):
    from thesis_pai_reconstruction_amd import ops
    c = u32(0)
    ops.counter_set(c, (1 << 32) - 1)
    assert value(c) == (1 << 32) - 1
    ops.counter_add(c, 1)
    assert value(c) == 0
    ops.counter_add(c, 7)
    ops.counter_add(c, (1 << 32) - 2)
    assert value(c) == 5
    ops.counter_set(c, 41)
    assert value(c) == 41


@pytest.mark.parametrize("kind", ["normal", "raw"])
def test_philox_fill_dev_has_the_bits_of_philox_fill(pai, kind):
    from thesis_pai_reconstruction_amd import ops
    code = {"normal": ops.PHILOX_NORMAL, "raw": ops.PHILOX_RAW}[kind]
    dt = ops.PHILOX_DTYPES[code]
    for step in (0, 1, (1 << 32) - 1):
        sd = u32(step)
        for n in (1, 7, 1024):
            want, got = torch.empty(n, dtype=dt, device=dev()), torch.empty(n, dtype=dt, device=dev())
            ops.philox_fill(code, want, 0xC0FFEE12345, 2, 3, step)
            ops.philox_fill_dev(code, got, 0xC0FFEE12345, 2, 3, sd)
            assert same_bits(got, want), (kind, step, n)
        assert value(sd) == step


# ---- 4 .. 9. the sampler ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recs(golden_dir):
    return {name: golden.load(golden_dir, f"ref_palette_{name}") for name in CHAINS}


def build(pai, name, dtype=F32, steps=None, planned=False):
    kw = U.palette_kwargs(name)
    if steps is not None:
        kw["inference_steps"] = steps
    m = U.init_portable(pai.Palette(**kw), U.CONFIGS[name][4]).to(dev())
    m.freeze()
    if dtype == BF16:
        m.set_precision("bf16-mixed")
    assert m.unet.compute_dtype == dtype
    m.sampler_plan = planned
    return m


@pytest.mark.parametrize("name", CHAINS)
def test_planned_chain_with_recorded_noise(pai, recs, name):
    """The reference's 100-step chains: the planned call has the bits of the eager call, and is within the fixture's own bound
    of the reference's final image."""
    rec = recs[name]
    m = build(pai, name)
    noise = torch.from_numpy(rec["noise"])
    m.noise_fn = lambda k, shape: noise[k]
    x = torch.from_numpy(rec["x"]).to(dev())
    eager = m(x)
    m.sampler_plan = True
    planned = m(x)
    again = m(x)                                            # every step of the second call is a replay
    info = m.sampler_plan_info()
    assert info["disabled"] is None and info["records"] == 1 and info["plans"] == 1, info
    assert info["replays"] == 98 + 100 and info["launches_per_step"] > 50, info
    assert same_bits(planned, eager) and same_bits(again, eager)
    err = float((planned.cpu().double() - torch.from_numpy(rec["final"]).double()).abs().max())
    bound = 2 * float(rec["chain_dev"]) + float(rec["chain_floor"])
    print(f"palette {name} planned chain: final image max err {err:.3e} (bound {bound:.3e}); {info}")
    assert err <= bound


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", CHAINS)
def test_planned_with_device_rng(pai, name, dtype):
    x = U.inputs(name)[0].to(dev())
    eager, planned = build(pai, name, dtype, steps=6), build(pai, name, dtype, steps=6, planned=True)
    eager.device_rng, planned.device_rng = pai.DeviceRNG(1234567, (1 << 32) - 1), pai.DeviceRNG(1234567, (1 << 32) - 1)
    state = torch.cuda.get_rng_state(dev())
    want = [eager(x), eager(x)]
    got = [planned(x), planned(x)]
    assert torch.equal(torch.cuda.get_rng_state(dev()), state)             # torch's generator is not touched
    for a, b in zip(got, want):
        assert same_bits(a, b) and bool(torch.isfinite(a).all())
    assert not same_bits(got[0], got[1])                                     # the step advanced: other draws
    info = planned.sampler_plan_info()
    assert info["records"] == 1 and info["replays"] >= 2 * 6 - 2 and info["disabled"] is None, info
    assert planned.device_rng.step == eager.device_rng.step == 1            # 2^32 - 1, 0, 1: wrapped with the host
    assert eager.device_rng._mirrors == {}                                  # no planned consumer: nothing on the device
    assert value(planned.device_rng.device_step(dev())) == 1
    # a reload of the generator's state reaches the device mirror
    planned.device_rng.load_state_dict({"seed": 1234567, "step": (1 << 32) - 1})
    assert same_bits(planned(x), want[0])
    planned.device_rng.step = (1 << 32) - 1                                 # and so does a direct assignment
    assert same_bits(planned(x), want[0])
    assert same_bits(planned(x), want[1])
    assert planned.sampler_plan_info()["records"] == 1


def test_invalidation_by_weights_and_batch(pai):
    x = U.inputs("a")[0].to(dev())
    m = build(pai, "a", steps=6, planned=True)
    m.device_rng = pai.DeviceRNG(99)
    old = m(x)
    assert m.sampler_plan_info()["records"] == 1
    sd = {k: (v + 0.01 * torch.randn_like(v) if v.is_floating_point() and k.startswith("unet.") else v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    m.device_rng.step = 0
    new = m(x)
    info = m.sampler_plan_info()
    assert info["records"] == 2 and info["plans"] == 1 and info["disabled"] is None, info     # re-recorded, the stale plan dropped
    e = build(pai, "a", steps=6)
    e.load_state_dict(sd)
    e.device_rng = pai.DeviceRNG(99)
    assert same_bits(new, e(x)) and not same_bits(new, old)
    # N = 2, N = 1, N = 2: two plans, the first one is found again
    want = {}
    for n in (2, 1):
        e.device_rng.step = 3
        want[n] = e(x[:n])
    for n in (2, 1, 2):
        m.device_rng.step = 3                               # the same generator object: its seed and mirror are in the signature
        assert same_bits(m(x[:n]), want[n]), n
    info = m.sampler_plan_info()
    assert info["plans"] == 2 and info["records"] == 3, info


def test_output_process_and_no_host_sync(pai):
    x = U.inputs("a")[0].to(dev())
    e, m = build(pai, "a", steps=15), build(pai, "a", steps=15, planned=True)
    e.device_rng, m.device_rng = pai.DeviceRNG(5), pai.DeviceRNG(5)
    want_y, want_p = e(x, output_process=True)
    got_y, got_p = m(x, output_process=True)                                 # the warm-up call: records
    assert tuple(got_p.shape) == tuple(want_p.shape) == (2, 9, 1, 16, 16)
    assert same_bits(got_y, want_y) and same_bits(got_p, want_p)
    want2 = e(x)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got2 = m(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert same_bits(got2, want2)
    assert m.sampler_plan_info()["records"] == 1


def test_refusal_without_a_noise_source(pai):
    x = U.inputs("a")[0].to(dev())
    e, m = build(pai, "a", steps=4), build(pai, "a", steps=4, planned=True)
    torch.manual_seed(3)
    want = e(x)
    torch.manual_seed(3)
    got = m(x)
    info = m.sampler_plan_info()
    assert same_bits(got, want)
    assert info["records"] == 0 and info["replays"] == 0 and "torch draws the noise" in info["disabled"], info
    m.device_rng = pai.DeviceRNG(1)                                         # the reason was this call's, not for good
    m(x)
    assert m.sampler_plan_info()["disabled"] is None and m.sampler_plan_info()["records"] == 1
