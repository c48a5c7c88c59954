"""GPU, kernel level: pai_dropout2d_rng / pai_dropout2d_rng_dev against pai_dropout2d on the mask of the host restatement
(tests/_philox_ref.py), bit for bit -- bf16 and fp32, out of place and in place, inf and NaN in kept and dropped positions --
the _dev form against the by-value form over a device counter, the separation of sub / stream / step, every refusal, the
recording of both launches into a plan, and the backward of nnops.Dropout2dRng / functional.dropout2d.

Shapes (N, HW, C): (3, 5, 8) one vector per pixel and odd counts; (2, 1, 24) the token form; (2, 64, 512) a real site;
(4096 * 64 + 37, 3, 8): with C = 8 and HW = 3 a workgroup covers 64 columns, so the grid's cap of 4096 workgroups in x is
passed and the last 37 columns are a second trip of the column loop."""
import functools

import numpy as np
import pytest
import torch

import _philox_ref as R
from _gpu_util import dev

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
SEED, SUB, STREAM, STEP = 0x0123456789ABCDEF, (3 << 16) | 1, 4096 + 2, 77
SHAPES = [(3, 5, 8), (2, 1, 24), (2, 64, 512), (4096 * 64 + 37, 3, 8)]
IDS = ["n3hw5c8", "token", "site", "two_trips"]
INT_OF = {F32: torch.int32, BF: torch.int16}


@pytest.fixture(scope="module")
def ops(pai):
    from thesis_pai_reconstruction_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _keep(n, thr, seed, sub, stream, step):
    k = R.keep(n, thr, seed, sub, stream, step)
    k.setflags(write=False)
    return k


def _mask(N, C, p, tup=(SEED, SUB, STREAM, STEP)):
    """fp32 [N, C] of {0, float32(1 / (1 - p))} on the device, and the uint8 keep flags on the host."""
    keep = _keep(N * C, R.thr_of(p), *tup)
    scale = np.float32(1.0 / (1.0 - p))
    return torch.from_numpy(keep.astype(np.float32) * scale).reshape(N, C).to(dev()), keep.reshape(N, C)


def _input(N, HW, C, dtype, keep):
    g = torch.Generator().manual_seed(N * 131 + HW * 17 + C)
    x = (torch.randn(N, HW, C, generator=g) * 3).to(dtype)
    kept, dropped = np.argwhere(keep == 1), np.argwhere(keep == 0)
    for where in (kept, dropped):
        if len(where):
            x[where[0][0], 0, where[0][1]] = float("inf")
            x[where[-1][0], HW - 1, where[-1][1]] = float("nan")
    return x.to(dev())


def _bits(t):
    return t.contiguous().view(INT_OF[t.dtype])


def _reference(ops, x, mask):
    N, HW, C = x.shape
    want = torch.empty_like(x)
    ops.dropout2d(x.dtype, x, mask, N, HW, C, want)
    return want


@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.3])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bits_of_dropout2d_on_the_reference_mask(ops, shape, dtype, p, inplace):
    """(a), (b): the bits of pai_dropout2d given the host restatement's mask; with p = 0 that is x itself."""
    N, HW, C = shape
    mask, keep = _mask(N, C, p)
    x = _input(N, HW, C, dtype, keep)
    want = _reference(ops, x, mask)
    if p == 0.0:
        assert keep.all() and torch.equal(_bits(want), _bits(x))
    else:
        assert 0 < keep.sum() < keep.size
        # the restatement's rate: a binomial count within six standard deviations
        assert abs(keep.mean() - (1 - p)) <= 6 * (p * (1 - p) / keep.size) ** 0.5 + 1.0 / keep.size
    x0 = x.clone()
    out = x if inplace else torch.full_like(x, 7.0)
    ops.dropout2d_rng(dtype, x, N, HW, C, SEED, SUB, STREAM, STEP, ops.dropout_thr(p), 1.0 / (1.0 - p), out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    if not inplace:
        assert torch.equal(_bits(x), _bits(x0))
    # the inf and the NaN were multiplied, not replaced: inf * 0 and NaN * 0 are NaN, inf * scale stays inf
    o = out.float().cpu()
    kept, dropped = np.argwhere(keep == 1), np.argwhere(keep == 0)
    assert torch.isnan(o[kept[-1][0], HW - 1, kept[-1][1]])
    if len(kept) > 1 or HW > 1:
        assert torch.isinf(o[kept[0][0], 0, kept[0][1]])
    if len(dropped):
        assert torch.isnan(o[dropped[0][0], 0, dropped[0][1]]) and torch.isnan(o[dropped[-1][0], HW - 1, dropped[-1][1]])


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[:3])
def test_dev_form_follows_the_counter(ops, shape, dtype):
    """(c): with the counter at `step` the _dev form gives the by-value bits; after counter_add(1) those of step + 1 (also
    across the wrap at 2^32)."""
    N, HW, C = shape
    p = 0.5
    thr, scale = ops.dropout_thr(p), 1.0 / (1.0 - p)
    x = _input(N, HW, C, dtype, _mask(N, C, p)[1])
    for step in (STEP, (1 << 32) - 1):
        nxt = (step + 1) & 0xFFFFFFFF
        want = [torch.empty_like(x) for _ in range(2)]
        ops.dropout2d_rng(dtype, x, N, HW, C, SEED, SUB, STREAM, step, thr, scale, want[0])
        ops.dropout2d_rng(dtype, x, N, HW, C, SEED, SUB, STREAM, nxt, thr, scale, want[1])
        counter = torch.zeros(1, dtype=torch.int32, device=dev())
        ops.counter_set(counter, step)
        got = [torch.empty_like(x) for _ in range(2)]
        ops.dropout2d_rng_dev(dtype, x, N, HW, C, SEED, SUB, STREAM, counter, thr, scale, got[0])
        ops.counter_add(counter, 1)
        ops.dropout2d_rng_dev(dtype, x, N, HW, C, SEED, SUB, STREAM, counter, thr, scale, got[1])
        torch.cuda.synchronize()
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
        assert torch.equal(_bits(want[1]), _bits(_reference(ops, x, _mask(N, C, p, (SEED, SUB, STREAM, nxt))[0])))
        assert not torch.equal(_bits(want[0]), _bits(want[1]))


def test_tuples_separate_the_flags(ops):
    """(d): another sub, stream, step or seed gives other flags; the same tuple the same flags."""
    N, HW, C = 4, 2, 64
    x = torch.ones(N, HW, C, device=dev())

    def flags(seed=SEED, sub=SUB, stream=STREAM, step=STEP):
        out = torch.empty_like(x)
        ops.dropout2d_rng(F32, x, N, HW, C, seed, sub, stream, step, ops.dropout_thr(0.5), 2.0, out)
        f = out.cpu()
        assert torch.equal(f[:, 0], f[:, 1]) and set(f.unique().tolist()) == {0.0, 2.0}      # one flag per (n, c)
        return f

    base = flags()
    assert torch.equal(base, flags())
    others = [flags(sub=SUB ^ 1), flags(sub=SUB ^ (1 << 16)), flags(stream=STREAM + 1), flags(step=STEP + 1), flags(seed=SEED + 1),
              flags(seed=SEED ^ (1 << 40))]
    for i, o in enumerate(others):
        assert not torch.equal(base, o), i
        for j in range(i):
            assert not torch.equal(others[j], o), (j, i)
    want = torch.from_numpy(R.keep(N * C, R.thr_of(0.5), SEED, SUB ^ 1, STREAM, STEP).astype(np.float32) * 2).reshape(N, C)
    assert torch.equal(others[0][:, 0], want)


def test_refusals_leave_out_untouched(pai, ops):
    """(e): every refusal raises before any launch."""
    N, HW, C = 2, 3, 16
    x = torch.ones(N, HW, C, device=dev())
    out = torch.full_like(x, 7.0)
    counter = torch.zeros(1, dtype=torch.int32, device=dev())
    good = dict(x=x, N=N, HW=HW, C=C, thr=1 << 15, out=out, counter=counter)
    cases = [dict(x=None), dict(out=None), dict(C=12), dict(C=0), dict(N=0), dict(HW=0), dict(thr=65537),
             dict(N=(1 << 31) - 1, C=24)]                      # N C / 8 = 3 (2^31 - 1) > 2^32
    for case in cases:
        a = dict(good, **case)
        with pytest.raises(pai.PaiError, match="pai_dropout2d_rng"):
            ops.dropout2d_rng(F32, a["x"], a["N"], a["HW"], a["C"], SEED, SUB, STREAM, STEP, a["thr"], 2.0, a["out"])
        with pytest.raises(pai.PaiError, match="pai_dropout2d_rng_dev"):
            ops.dropout2d_rng_dev(F32, a["x"], a["N"], a["HW"], a["C"], SEED, SUB, STREAM, a["counter"], a["thr"], 2.0, a["out"])
    with pytest.raises(pai.PaiError, match="pai_dropout2d_rng_dev"):
        ops.dropout2d_rng_dev(F32, x, N, HW, C, SEED, SUB, STREAM, None, 1 << 15, 2.0, out)      # NULL step_dev
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((x == 1.0).all()) and int(counter.item()) == 0
    # thr = 65536 is p = 1 rounded: allowed, everything is dropped
    ops.dropout2d_rng(F32, x, N, HW, C, SEED, SUB, STREAM, STEP, 65536, 2.0, out)
    assert bool((out == 0.0).all())


def test_both_launches_are_recorded_by_a_plan(ops):
    """A plan holds both launches; replayed, the by-value one repeats its flags and the _dev one follows the counter."""
    N, HW, C = 3, 5, 8
    x = torch.ones(N, HW, C, device=dev())
    a, b = torch.zeros_like(x), torch.zeros_like(x)
    counter = torch.zeros(1, dtype=torch.int32, device=dev())
    ops.counter_set(counter, STEP)
    thr = ops.dropout_thr(0.5)
    plan = ops.Plan()
    try:
        plan.begin()
        try:
            ops.dropout2d_rng(F32, x, N, HW, C, SEED, SUB, STREAM, STEP, thr, 2.0, a)
            ops.dropout2d_rng_dev(F32, x, N, HW, C, SEED, SUB, STREAM, counter, thr, 2.0, b)
        finally:
            plan.end()
        assert plan.info()["launches"] == 2
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        first = a.clone()
        ops.counter_add(counter, 1)
        a.zero_()
        b.zero_()
        plan.run(0)
        torch.cuda.synchronize()
        want = torch.from_numpy(R.keep(N * C, thr, SEED, SUB, STREAM, STEP + 1).astype(np.float32) * 2).reshape(N, 1, C)
        assert torch.equal(a, first) and torch.equal(b.cpu(), want.expand(N, HW, C))
    finally:
        plan.destroy()


@pytest.mark.parametrize("dev_step", [False, True], ids=["by_value", "dev"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_autograd_backward_is_the_forward_mask(pai, ops, dtype, dev_step):
    """(f): the gradient is g times the forward's mask, bit for bit; nothing is saved for it."""
    from thesis_pai_reconstruction_amd import functional as PF
    from thesis_pai_reconstruction_amd import nnops
    N, H, W, C, p = 3, 2, 3, 24, 0.3
    mask, keep = _mask(N, C, p)
    g0 = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, W, C, generator=g0).to(dtype).to(dev()).requires_grad_(True)
    g = torch.randn(N, H, W, C, generator=g0).to(dtype).to(dev())
    step = STEP
    if dev_step:
        step = torch.zeros(1, dtype=torch.int32, device=dev())
        ops.counter_set(step, STEP)
    y = nnops.Dropout2dRng.apply(x, (SEED, SUB, STREAM, step), p)
    assert y.grad_fn.saved_tensors == ()
    y.backward(g)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y.detach()), _bits(_reference(ops, x.detach().view(N, H * W, C), mask).view(N, H, W, C)))
    assert torch.equal(_bits(x.grad), _bits(_reference(ops, g.view(N, H * W, C), mask).view(N, H, W, C)))
    # the public form, on the token layout [N, C] and on [N, rows, C]
    for shape in ((N, C), (N, H * W, C)):
        xs = torch.randn(*shape, generator=g0).to(dtype).to(dev()).requires_grad_(True)
        gs = torch.randn(*shape, generator=g0).to(dtype).to(dev())
        ys = PF.dropout2d(xs, p, rng=(SEED, SUB, STREAM, step))
        ys.backward(gs)
        torch.cuda.synchronize()
        assert ys.shape == xs.shape
        assert torch.equal(_bits(ys.detach()), _bits(_reference(ops, xs.detach().view(N, -1, C), mask).view(shape)))
        assert torch.equal(_bits(xs.grad), _bits(_reference(ops, gs.view(N, -1, C), mask).view(shape)))
    with pytest.raises(pai.PaiError):
        PF.dropout2d(xs.detach(), p, rng=(SEED, STREAM, STEP))
    with pytest.raises(pai.PaiError):
        PF.dropout2d(torch.ones(2, 12, device=dev()), p, rng=(SEED, SUB, STREAM, STEP))
