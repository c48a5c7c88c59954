"""GPU: the device generator (csrc/philox.h) through every entry point that draws with it, against the host restatement of
tests/_philox_ref.py (tied to the published known answers by tests/test_philox_ref_host.py).

Conventions of tests/test_gpu_film_norm.py: every output buffer is NaN (integer buffers: a poison pattern) before the call and
carries 64 guard elements behind it that must survive.

  philox_fill      raw, uniform, integer (T = 2000 and T = 1) and keep (p = 0, 0.1, 0.25, 0.5) BIT-EQUAL to the reference at
                   n in {1, 3, 4, 5, 7, 8, 9, 1027}; seed with a non-zero high word, sub, stream, step non-zero and distinct
  normal fill      |got - ref| <= 8 * 2^-24 * r, r the fp64 radius of the element's pair.  u1 and 2 v are exact, logf and
                   sincospif are documented at 1 to 2 ulp, sqrtf and the product are correctly rounded: under 4 ulp of r, the
                   bound is a factor 2 over it.  Largest ratio measured on an MI355X (pytest -s prints it): 0.358
  dropout          film_norm_act(dropout_rng=) against film_norm_act(dropout_mask=M), M the reference keep mask of the same
                   tuple: y, dx, dweight, dbias, demb bit-equal (the arithmetic is shared), both dtypes, FiLM + SiLU
  noising          palette_noise_rng: t equals the reference integers; noise, y_t, gamma bit-equal to palette_noise fed t, u, z
                   of philox_fill with the same tuples; one sample forced to t = 0 by choosing the seed on the host
  sampler step     palette_step_rng bit-equal to palette_step fed the fill normals
  model            tiny configuration "a" of tests/_palette_util.py with dropout 0.25, 16 x 16, N = 2, fp32: torch's generator
                   state untouched; forward bit-equal to noise_fn fed the fill normals; training_loss equal to the explicit
                   draws= + dropout_masks= path built from the fills (bit-equal where that path is bit-equal run to run)
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import _palette_util as U
import _philox_ref as R
from _gpu_util import dev

pytestmark = pytest.mark.gpu

GUARD = 64
SEED, SUB, STREAM, STEP = 0xC0FFEE1234567891, 5, 19, 11          # high word non-zero; sub, stream, step non-zero and distinct
LENGTHS = [1, 3, 4, 5, 7, 8, 9, 1027]
POISON = {torch.float32: float("nan"), torch.bfloat16: float("nan"), torch.int32: -0x5A5A5A5B, torch.uint8: 0xA5}


def _mods():
    import pai_bootstrap
    pai_bootstrap.load()
    from thesis_pai_reconstruction_amd import functional as PF
    from thesis_pai_reconstruction_amd import nnops, ops
    return PF, ops, nnops


def _poisoned(n, dtype):
    return torch.full((n + GUARD,), POISON[dtype], dtype=dtype, device=dev())


def _guard_ok(buf, n, dtype):
    tail = buf[n:]
    return bool(torch.isnan(tail).all()) if dtype == torch.float32 else bool((tail == POISON[dtype]).all())


def _fill(kind, n, param=0, tup=(SEED, SUB, STREAM, STEP)):
    PF, ops, _ = _mods()
    dtype = ops.PHILOX_DTYPES[{"raw": 0, "uniform": 1, "normal": 2, "int": 3, "keep": 4}[kind]]
    buf = _poisoned(n, dtype)
    PF.philox_fill(kind, None, *tup, param=param, out=buf[:n])
    torch.cuda.synchronize()
    assert _guard_ok(buf, n, dtype), f"{kind} n={n}: wrote past its {n} elements"
    return buf[:n].cpu().numpy()


# ---- 1. philox_fill ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_fill_bit_equal(pai, n):
    tup = (SEED, SUB, STREAM, STEP)
    assert np.array_equal(_fill("raw", n).view(np.uint32), R.raw(n, *tup))
    got = _fill("uniform", n)
    assert np.array_equal(got.view(np.uint32), R.uniform(n, *tup).view(np.uint32)) and (got >= 0).all() and (got < 1).all()
    assert np.array_equal(_fill("int", n, 2000), R.integer(n, 2000, *tup))
    assert np.array_equal(_fill("int", n, 1), np.zeros(n, np.int32))
    for p in (0.0, 0.1, 0.25, 0.5):
        thr = R.thr_of(p)
        got = _fill("keep", n, thr)
        assert np.array_equal(got, R.keep(n, thr, *tup)), (p, n)
        if p == 0.0:
            assert got.all()


def test_fill_misaligned_and_refusals(pai):
    """A view that starts in the middle of a vector gives the same elements (element-wise stores); bad arguments are refused
    before any launch and leave the buffer alone."""
    PF, ops, _ = _mods()
    buf = _poisoned(41, torch.float32)
    PF.philox_fill("uniform", None, SEED, SUB, STREAM, STEP, out=buf[1:38])
    k = _poisoned(41, torch.uint8)
    PF.philox_fill("keep", None, SEED, SUB, STREAM, STEP, param=R.thr_of(0.5), out=k[3:40])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[38:]).all())
    assert np.array_equal(buf[1:38].cpu().numpy(), R.uniform(37, SEED, SUB, STREAM, STEP))
    assert bool((k[:3] == 0xA5).all()) and bool((k[40:] == 0xA5).all())
    assert np.array_equal(k[3:40].cpu().numpy(), R.keep(37, R.thr_of(0.5), SEED, SUB, STREAM, STEP))
    out = _poisoned(8, torch.int32)
    with pytest.raises(ops.PaiError, match="T=0"):
        ops.philox_fill(ops.PHILOX_INT, out[:8], 1, 0, 0, 0, 0)
    with pytest.raises(ops.PaiError, match="thr"):
        ops.philox_fill(ops.PHILOX_KEEP, _poisoned(8, torch.uint8)[:8], 1, 0, 0, 0, 65537)
    with pytest.raises(ops.PaiError, match="expected"):
        ops.philox_fill(ops.PHILOX_UNIFORM, out[:8], 1, 0, 0, 0)
    lib = pai.lib.load()
    assert lib.pai_philox_fill(9, out.data_ptr(), 8, 1, 0, 0, 0, 0, None) != 0 and b"kind=9" in lib.pai_last_error()
    torch.cuda.synchronize()
    assert bool((out == POISON[torch.int32]).all())


def test_fill_normal(pai):
    """|got - ref| <= 8 * 2^-24 * r elementwise (module docstring), at every length of LENGTHS and at 2^16 + 3 elements."""
    worst = 0.0
    for n in LENGTHS + [(1 << 16) + 3]:
        got = _fill("normal", n).astype(np.float64)
        ref, r = R.normal(n, SEED, SUB, STREAM, STEP)
        assert np.isfinite(got).all()
        err, lim = np.abs(got - ref), 8 * 2.0 ** -24 * r
        ratio = float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0
        worst = max(worst, ratio)
        assert (err <= lim).all(), (n, ratio)
    print(f"philox normal fill: largest |got - ref| / (8 * 2^-24 r) = {worst:.3f}")


# ---- 2. dropout inside the norm kernels ----------------------------------------------------------------------------------------
DROP_CASES = [((2, 1, 8), 0.25), ((3, 37, 8), 0.25), ((2, 5, 264), 0.25), ((2, 1000, 256), 0.25), ((3, 37, 8), 0.1)]


@lru_cache(maxsize=None)
def _drop_data(case):
    N, rows, C = case
    g = torch.Generator().manual_seed(100 + rows)
    return (torch.randn(N, rows, C, generator=g), 0.3 * torch.randn(N, 2 * C + 8, generator=g), 1 + 0.1 * torch.randn(C, generator=g),
            0.1 * torch.randn(C, generator=g), torch.randn(N, rows, C, generator=g))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case,p", DROP_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_dropout_rng_equals_mask(pai, case, p, dtype):
    PF, ops, _ = _mods()
    N, rows, C = case
    seed, stream, step = SEED, R.STREAM_DROPOUT + 3, STEP
    mask = torch.from_numpy(R.keep(N * rows * C, R.thr_of(p), seed, 0, stream, step)).view(N, rows, C).to(dev())
    kept = float(mask.float().mean())
    assert 0.0 < kept < 1.0 or N * rows * C < 32
    res = []
    for how in ("mask", "rng"):
        x, emb, w, b, dout = _drop_data(case)
        x, emb, dout = (t.to(dev()).to(dtype).contiguous() for t in (x, emb, dout))
        x.requires_grad_(True), emb.requires_grad_(True)
        w, b = w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
        kw = dict(dropout_mask=mask) if how == "mask" else dict(dropout_rng=(seed, stream, step))
        y = PF.film_norm_act(x, w, b, emb, p=p, **kw)
        y.backward(dout)
        torch.cuda.synchronize()
        res.append({"y": y.detach(), "dx": x.grad, "dweight": w.grad, "dbias": b.grad, "demb": emb.grad})
    for k in res[0]:
        a, c = res[0][k], res[1][k]
        assert bool(torch.isfinite(a.float()).all()), k
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           c.view(torch.int32 if c.dtype == torch.float32 else torch.int16)), f"{k}: rng form differs from the mask form"
    assert bool(((res[1]["y"] == 0).view(N, rows, C) | (mask != 0)).all())           # what the mask drops is zero


def test_dropout_rng_guards_and_refusals(pai):
    """The raw entry points write exactly their outputs (NaN guards survive), and refuse a threshold above 65536."""
    PF, ops, _ = _mods()
    N, rows, C = 3, 37, 8
    n = N * rows * C
    x, _, w, b, dout = _drop_data((N, rows, C))
    x, dout, w, b = (t.to(dev()).contiguous() for t in (x, dout, w, b))
    mean, rstd = torch.zeros(C, device=dev()), torch.ones(C, device=dev())
    out, dx = _poisoned(n, torch.float32), _poisoned(n, torch.float32)
    wsn = ops.film_norm_ws_floats(N, rows, C)
    ws, dgb = _poisoned(wsn, torch.float32), torch.zeros(2 * C, device=dev())
    thr = R.thr_of(0.25)
    ops.film_norm_fwd_rng(torch.float32, x, rows, N, C, mean, rstd, w, b, None, 0, SEED, 17, STEP, thr, 4 / 3, ops.ACT_SILU, out[:n])
    ops.film_norm_bwd_rng(torch.float32, dout, x, rows, N, C, mean, rstd, w, b, None, 0, SEED, 17, STEP, thr, 4 / 3, ops.ACT_SILU,
                          dx[:n], None, dgb[:C], dgb[C:], ws[:wsn])
    torch.cuda.synchronize()
    for buf, m in ((out, n), (dx, n), (ws, wsn)):
        assert bool(torch.isnan(buf[m:]).all()) and bool(torch.isfinite(buf[:m]).all())
    keep = torch.from_numpy(R.keep(n, thr, SEED, 0, 17, STEP)).to(dev())
    assert bool(((out[:n] == 0) | (keep != 0)).all()) and bool((out[:n] != 0).any())
    again = _poisoned(n, torch.float32)
    with pytest.raises(ops.PaiError, match="thr=65537"):
        ops.film_norm_fwd_rng(torch.float32, x, rows, N, C, mean, rstd, w, b, None, 0, SEED, 17, STEP, 65537, 1.0, ops.ACT_SILU, again[:n])
    torch.cuda.synchronize()
    assert bool(torch.isnan(again).all())


# ---- 3. forward noising ---------------------------------------------------------------------------------------------------------
def _seed_with_t0(N, T, step):
    """The first seed (from SEED upwards) whose reference t has a zero and a non-zero sample: chosen on the host."""
    for k in range(200000):
        t = R.integer(N, T, SEED + k, 0, R.STREAM_T, step)
        if (t == 0).any() and (t != 0).any():
            return SEED + k, t
    raise AssertionError("no seed with a t = 0 sample found")


@pytest.mark.parametrize("P,C", [(5, 1), (5, 3), (64, 1), (64, 3)])
def test_noise_rng(pai, P, C):
    PF, ops, _ = _mods()
    N, T = 3, 2000
    seed, t_ref = _seed_with_t0(N, T, STEP)
    m = pai.DiffusionModel("linear", T).to(dev())
    g = torch.Generator().manual_seed(P * 10 + C)
    y0 = torch.randn(N * P * C, generator=g).to(dev())
    n = N * P * C
    f32 = torch.float32
    bufs = {k: _poisoned(n, f32) for k in ("y_t", "noise", "y_t2", "noise2")}
    gam, gam2, t = _poisoned(N, f32), _poisoned(N, f32), _poisoned(N, torch.int32)
    ops.palette_noise_rng(y0, m.gammas, m.gammas_prev, N, P, C, seed, STEP, t[:N], bufs["y_t"][:n], bufs["noise"][:n], gam[:N])
    tt = PF.philox_fill("int", (N,), seed, 0, R.STREAM_T, STEP, param=T, device=dev())
    uu = PF.philox_fill("uniform", (N,), seed, 0, R.STREAM_U, STEP, device=dev())
    zz = PF.philox_fill("normal", (n,), seed, 0, R.STREAM_Z, STEP, device=dev())
    ops.palette_noise(y0, zz, uu, tt, m.gammas, m.gammas_prev, N, P, C, bufs["y_t2"][:n], bufs["noise2"][:n], gam2[:N])
    torch.cuda.synchronize()
    assert _guard_ok(t, N, torch.int32) and np.array_equal(t[:N].cpu().numpy(), t_ref) and (t_ref == 0).any()
    for buf, k in ((gam, N), (gam2, N)) + tuple((b, n) for b in bufs.values()):
        assert bool(torch.isnan(buf[k:]).all()) and bool(torch.isfinite(buf[:k]).all())
    i32 = lambda v: v.view(torch.int32)
    assert torch.equal(i32(gam[:N]), i32(gam2[:N])), "gamma"
    assert torch.equal(i32(bufs["noise"][:n]), i32(bufs["noise2"][:n])), "noise"
    assert torch.equal(i32(bufs["y_t"][:n]), i32(bufs["y_t2"][:n])), "y_t"
    zero = int(np.flatnonzero(t_ref == 0)[0])
    assert bool((bufs["noise"][zero * P * C:(zero + 1) * P * C] == 0).all())       # the (t > 0) product
    assert bool((bufs["noise"][:n] != 0).any())


# ---- 4. sampler step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("add_noise", [False, True], ids=["mean", "noise"])
@pytest.mark.parametrize("learn_var", [False, True], ids=["fixed", "learned"])
@pytest.mark.parametrize("pixels,C", [(5, 1), (5, 3), (256, 1), (256, 3)])
def test_step_rng(pai, pixels, C, learn_var, add_noise):
    _step_rng(pixels, C, learn_var, add_noise, torch.float32)


def test_step_rng_bf16(pai):
    """The bf16 model output and [x | y] tensor (the storage type of bf16-mixed sampling)."""
    _step_rng(256, 3, True, True, torch.bfloat16)
    _step_rng(5, 1, False, True, torch.bfloat16)


def _step_rng(pixels, C, learn_var, add_noise, dt):
    PF, ops, _ = _mods()
    n, f32 = pixels * C, torch.float32
    g = torch.Generator().manual_seed(pixels + C)
    mo = torch.randn(pixels * (2 * C if learn_var else C), generator=g).to(dev()).to(dt)
    y = torch.randn(n, generator=g).to(dev())
    scal = (0.6, 1.25, 0.3, 0.69, -4.0, -2.5)
    a, b = _poisoned(n, f32), _poisoned(n, f32)
    xa, xb = _poisoned(2 * n, dt), _poisoned(2 * n, dt)
    bits = lambda v: v.view(torch.int32 if v.dtype == f32 else torch.int16)
    ops.palette_step_rng(dt, mo, y, pixels, C, learn_var, add_noise, scal, SEED, SUB, STEP, a[:n], xa[:2 * n])
    z = PF.philox_fill("normal", (n,), SEED, SUB, R.STREAM_SAMPLER, STEP, device=dev())
    ops.palette_step(dt, mo, y, z, pixels, C, learn_var, add_noise, scal, b[:n], xb[:2 * n])
    torch.cuda.synchronize()
    assert bool(torch.isnan(a[n:]).all()) and bool(torch.isnan(xa[2 * n:]).all()) and bool(torch.isfinite(a[:n]).all())
    assert torch.equal(bits(a[:n]), bits(b[:n]))
    assert torch.equal(bits(xa), bits(xb))                                        # the y half written, the x half still NaN
    assert bool(torch.isfinite(xa[:2 * n].view(pixels, 2 * C)[:, C:]).all())
    if add_noise:
        ops.palette_step(dt, mo, y, torch.zeros_like(z), pixels, C, learn_var, True, scal, b[:n], None)
        torch.cuda.synchronize()
        assert not torch.equal(a[:n], b[:n])                                      # the noise took part


# ---- 5. model -------------------------------------------------------------------------------------------------------------------
P_DROP = 0.25


def _model(pai):
    m = U.init_portable(pai.Palette(**dict(U.palette_kwargs("a"), dropout=P_DROP, inference_steps=4)), U.CONFIGS["a"][4]).to(dev())
    m.set_precision("32")
    return m


def _batch():
    x, y = U.inputs("a")
    return x.to(dev()), torch.tanh(y).to(dev())


def test_forward_under_device_rng(pai):
    """Four inference steps: torch's generator state is untouched, the output has the bits of the same model with noise_fn
    returning the fill normals of (seed, sub = k, stream 3, step), and the step advances once."""
    PF, ops, _ = _mods()
    m = _model(pai).eval()
    x, _ = _batch()
    n, c, h, w = x.shape
    m.device_rng = pai.DeviceRNG(SEED, step=STEP)
    state = torch.cuda.get_rng_state()
    with torch.no_grad():
        got = m(x)
    torch.cuda.synchronize()
    assert torch.equal(torch.cuda.get_rng_state(), state), "torch's generator was used"
    assert m.device_rng.step == STEP + 1
    calls = []

    def noise_fn(k, shape):
        calls.append(k)
        z = PF.philox_fill("normal", (n, h, w, c), SEED, k, R.STREAM_SAMPLER, STEP, device=dev())
        return z.permute(0, 3, 1, 2)

    m.device_rng, m.noise_fn = None, noise_fn
    with torch.no_grad():
        want = m(x)
    torch.cuda.synchronize()
    assert calls == [0, 1, 2, 3, 4]
    assert bool(torch.isfinite(got).all()) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    m.noise_fn, m.device_rng = None, pai.DeviceRNG(SEED, step=STEP + 1)
    with torch.no_grad():
        other = m(x)
    assert not torch.equal(other, got)                                            # the next sampling call draws anew


def _explicit(pai, m, batch, seed, step):
    """draws= and dropout_masks= of the tuple (seed, step) built from the fills."""
    PF, ops, _ = _mods()
    x, y0 = batch
    n, c, h, w = y0.shape
    T = m.diffusion.timesteps
    t = PF.philox_fill("int", (n,), seed, 0, R.STREAM_T, step, param=T, device=dev())
    u = PF.philox_fill("uniform", (n,), seed, 0, R.STREAM_U, step, device=dev())
    z = PF.philox_fill("normal", (n, h, w, c), seed, 0, R.STREAM_Z, step, device=dev()).permute(0, 3, 1, 2)
    m.unet.debug_capture = {}
    try:
        rm = {k: v.detach().clone() for k, v in m.unet.state_dict().items()}      # the shape pass advances the running statistics
        m.unet.forward_train(x, y0, torch.full((n,), 0.5, device=dev()), dropout_rng=(seed, step))
        shapes = {k: tuple(v.shape) for k, v in m.unet.debug_capture.items()}
        m.unet.load_state_dict(rm)
    finally:
        m.unet.debug_capture = None
    masks = {}
    blocks = [(name, mod) for name, mod in m.unet.named_modules() if type(mod).__name__ == "ResBlock"]
    assert len(blocks) >= 4
    for i, (name, _) in enumerate(blocks):
        nn_, cc, hh, ww = shapes[name]
        masks[name] = PF.philox_fill("keep", (nn_, hh, ww, cc), seed, 0, R.STREAM_DROPOUT + i, step, param=R.thr_of(P_DROP),
                                     device=dev())
    return (t, z, u), masks


def _loss_and_grads(m, run):
    _, _, nnops = _mods()
    for p in m.unet.parameters():
        p.grad = None
    loss = run()
    loss.backward()
    nnops.join_wgrads()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.unet.named_parameters()}


def test_training_loss_under_device_rng(pai, monkeypatch):
    """training_loss + backward with device_rng set: torch's generator state is untouched, and the loss and every parameter
    gradient equal those of training_loss(draws=) with dropout_masks= built from the fills of the same tuples.  The explicit
    path runs twice first: where it is bit-equal run to run the comparison is bit-equality of everything.

    Measured on an MI355X: the explicit path is NOT bit-equal run to run.  Its loss is (spread 0); its gradients are not: the
    fp32 weight- and bias-gradient kernels of the convolutions add across workgroups with atomics, in arrival order.  The
    spread between the two runs: D = 7.629e-6 in three runs and 3.815e-6 in a fourth, the largest absolute difference of any element of any tensor (one ulp of a
    gradient element between 64 and 128).  The comparison:
      loss                                   bit-equal (the forward pass has no sum in arrival order)
      BatchNorm weight / bias gradients      bit-equal: they come from pai_film_norm_bwd, which has the same bits on every run,
                                             and they are the sums over exactly the elements the regenerated keep bits gate
      every other parameter gradient         within the spread observed between the two explicit runs: per tensor the larger
                                             of its own spread and D (a tensor whose two runs happened to agree, such as a
                                             bias of 64 elements, is still a sum in arrival order).
    THIS TEST CAN FAIL, and did in one of five runs on an MI355X (the fifth passed, its figures were not printed).  Figures of the first four (D; largest difference of the
    device_rng run from the first explicit run): 7.629e-6; 7.629e-6 -- 7.629e-6; 7.629e-6 -- 7.629e-6; 7.629e-6 -- 3.815e-6;
    7.629e-6 (failed: `input_blocks.0.0.weight`, own spread below D, differed by 7.629e-6 = one ulp of an element in
    [64, 128), where the two explicit runs of that session had differed by half that elsewhere and not at all there).  In
    every run the loss and all BatchNorm gradients were bit-equal.  Explanation: the device_rng run computes the same forward
    bits and the same keep bits, so its convolution gradients are a third sample of the same atomic sums; the difference of a
    third sample from the first is distributed like that of the second from the first, and the largest of one such sample
    does not bound the largest of another.  The bound is the issue's and stays; the noise is that of the fp32 convolution
    weight-gradient kernels (csrc/gg_simt.hip, atomicAdd into dw / dbias), which this generator does not touch."""
    PF, ops, _ = _mods()
    m = _model(pai).train()
    batch = _batch()
    draws, masks = _explicit(pai, m, batch, SEED, STEP)
    unet_train = m.unet.forward_train
    monkeypatch.setattr(m.unet, "forward_train", lambda x, y, g, **kw: unet_train(x, y, g, dropout_masks=masks, **kw))
    l1, g1 = _loss_and_grads(m, lambda: m.training_loss(batch, draws))
    l2, g2 = _loss_and_grads(m, lambda: m.training_loss(batch, draws))
    monkeypatch.undo()
    exact = torch.equal(l1, l2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    spread = {k: float((g1[k] - g2[k]).abs().max()) for k in g1}
    top = {k: float(g1[k].abs().max()) for k in g1}
    rel = max(spread[k] / top[k] for k in g1 if top[k] > 0)
    lspread = float((l1 - l2).abs())
    print(f"explicit path run to run: {'bit-equal' if exact else 'NOT bit-equal'}; loss spread {lspread:.3e}, largest gradient "
          f"spread {max(spread.values()):.3e} absolute, {rel:.3e} of the tensor's largest element")
    m.device_rng = pai.DeviceRNG(SEED, step=STEP)
    state = torch.cuda.get_rng_state()
    l3, g3 = _loss_and_grads(m, lambda: m.training_loss(batch))
    assert torch.equal(torch.cuda.get_rng_state(), state), "torch's generator was used"
    assert m.device_rng.step == STEP + 1
    assert bool(torch.isfinite(l3)) and any(bool((g != 0).any()) for g in g3.values())
    norm = {f"{name}.{leaf}" for name, mod in m.unet.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)
            for leaf in ("weight", "bias")}
    assert len(norm) >= 8 and norm <= set(g1)
    if exact:
        assert torch.equal(l3, l1), (float(l3), float(l1))
        bad = [k for k in g1 if not torch.equal(g3[k], g1[k])]
        assert not bad, bad[:5]
    else:
        assert float((l3 - l1).abs()) <= lspread
        for k in sorted(norm):
            assert spread[k] == 0.0, f"{k}: the norm backward differs run to run"
            assert torch.equal(g3[k], g1[k]), f"{k}: differs from the explicit path"
        worst = max(float((g3[k] - g1[k]).abs().max()) / top[k] for k in g1 if top[k] > 0)
        wabs = max(float((g3[k] - g1[k]).abs().max()) for k in g1)
        print(f"device_rng against the explicit path: largest gradient difference {wabs:.3e} absolute, {worst:.3e} of the tensor's "
              f"largest element")
        dmax = max(spread.values())
        bad = [k for k in g1 if float((g3[k] - g1[k]).abs().max()) > max(spread[k], dmax)]
        assert not bad, bad[:5]


def test_same_seed_same_t(pai):
    """Two DeviceRNGs with the same seed give the same t; after advance() a different one."""
    PF, _, _ = _mods()
    m = pai.DiffusionModel("linear", 2000).to(dev())
    y0 = torch.zeros(8, 1, 4, 4, device=dev())
    a, b = pai.DeviceRNG(SEED), pai.DeviceRNG(SEED)
    ta = PF.palette_noise_rng(y0, a.seed, a.step, m)[3]
    tb = PF.palette_noise_rng(y0, b.seed, b.step, m)[3]
    b.advance()
    tc = PF.palette_noise_rng(y0, b.seed, b.step, m)[3]
    torch.cuda.synchronize()
    assert ta.dtype == torch.int32 and torch.equal(ta, tb) and not torch.equal(ta, tc)
    assert np.array_equal(ta.cpu().numpy(), R.integer(8, 2000, SEED, 0, R.STREAM_T, 0))
    assert np.array_equal(tc.cpu().numpy(), R.integer(8, 2000, SEED, 0, R.STREAM_T, 1))


def test_train_script_device_rng_and_resume(pai, tmp_path, monkeypatch):
    """scripts/train_palette.py --device-rng: the checkpoint holds the generator's state, --resume continues from the step
    count and the rng state of the checkpoint, and the resumed step draws what step 2 of an uninterrupted run draws (its t
    equals the reference integers of (seed, step 2)).  A checkpoint with rng state is not resumed without --device-rng."""
    import importlib.util
    import os
    PF, _, _ = _mods()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_train_palette_rng", os.path.join(root, "scripts", "train_palette.py"))
    tp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tp)
    monkeypatch.chdir(tmp_path)
    drawn, noise_rng = [], PF.palette_noise_rng

    def recording(y0, seed, step, diffusion):
        out = noise_rng(y0, seed, step, diffusion)
        drawn.append((seed, step, out[3]))
        return out

    monkeypatch.setattr(PF, "palette_noise_rng", recording)
    common = ["r", "--synthetic", "4", "--image-size", "16", "--batch-size", "2", "--channel-mults", "1,2", "--attention-res", "2",
              "--inference-steps", "2", "--log-every", "1", "--dropout", "0.25", "--seed", "77"]
    out = tp.main(tp.build_parser().parse_args(common + ["--device-rng", "--steps", "2"]))
    path = tmp_path / "logs" / "r" / "palette.ckpt"
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert out["steps"] == 2 and np.isfinite(out["loss"])
    assert ckpt["device_rng"] == {"seed": 77, "step": 2} and ckpt["global_step"] == 2
    out = tp.main(tp.build_parser().parse_args(common + ["--device-rng", "--steps", "3", "--resume", str(path)]))
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert out["steps"] == 3 and np.isfinite(out["loss"])
    assert ckpt["device_rng"] == {"seed": 77, "step": 3} and ckpt["global_step"] == 3
    assert ckpt["lr_schedulers"][0]["last_epoch"] == 3
    assert [(s, k) for s, k, _ in drawn] == [(77, 0), (77, 1), (77, 2)]
    for _, k, t in drawn:
        assert np.array_equal(t.cpu().numpy(), R.integer(2, 2000, 77, 0, R.STREAM_T, k)), k
    with pytest.raises(SystemExit, match="already at step 3"):
        tp.main(tp.build_parser().parse_args(common + ["--device-rng", "--steps", "3", "--resume", str(path)]))
    with pytest.raises(SystemExit, match="--device-rng"):
        tp.main(tp.build_parser().parse_args(common + ["--steps", "4", "--resume", str(path)]))
