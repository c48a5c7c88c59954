"""The first layer's weight and bias gradient formed in the store of the next layer's input gradient
(pai_conv_dgrad_act_wthin, gg_dgrad_wthin_k<T> + wthin_reduce_k) against the two launches it replaces: pai_conv_dgrad_act
(pai_conv_dgrad_bn with a skip gradient) into a tensor, then the thin pai_conv_wgrad that reads the tensor back.

Shapes: "h x w" below is the size of the INCOMING gradient (the output of the layer behind the thin one), i.e. the grid the
8 x 16-pixel patch tiles of one output phase divide; the gradient tensor that is no longer written has 2h x 2w pixels, the
thin inputs 4h x 4w.  8 x 16 is one tile per image and phase (the smallest problem the kernel takes), 16 x 16 and the
non-square 16 x 32 have the tile rows / columns that touch the zero padding on one side only, 32 x 32 at N = 3 has interior
tiles and 96 workgroups on 7 slabs (a slab count that does not divide them).

Integer-valued data: the incoming gradient is a multiple of 5, so that LeakyReLU'(.) = 0.2 leaves integers as well, and the
test itself checks sum |du| * max |x| + |prior| < 2^24 per output element: every fp32 partial sum of either path is then
exact in any order, and the two paths must agree bit for bit.  Random data: both paths against one fp64 restatement."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gpu_util import dev, fwd_pack, max_err, nhwc, rel_err, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
# (N, h, w, slab count or None for the default)
SHAPES = [(2, 8, 16, None), (2, 16, 16, None), (2, 16, 32, None), (3, 32, 32, 7)]
# (thin channels T, skip gradient in the store): D block 1 -> block 0 (xin | yin), encoders[1] -> encoders[0] (x, + gskip)
FORMS = [(2, False), (1, True)]


def _ints(shape, seed, lo, hi, density=1.0):
    rng = np.random.default_rng(seed)
    v = rng.integers(lo, hi + 1, size=shape).astype(np.float32)
    if density < 1.0:
        v *= rng.random(shape) < density
    return torch.from_numpy(v)


class _Problem:
    """Device tensors of one (shape, form) and the two ways to the thin layer's gradients."""

    def __init__(self, ops, N, h, w, T, with_add, integer, seed=0):
        self.ops, self.N, self.T = ops, N, T
        self.d1 = ops.make_desc(BF, 0, N, 2 * h, 2 * w, 64, 0, 128, 2, 0, 0, ops.ACT_LRELU)
        self.d0 = ops.make_desc(BF, 0, N, 4 * h, 4 * w, 1, T - 1, 64, 2, 0, 0, ops.ACT_LRELU)
        if integer:
            self.dy = _ints((N, 128, h, w), seed + 1, -1, 1, 0.25) * 5
            self.w1 = _ints((128, 64, 4, 4), seed + 2, -1, 1, 0.25)
            self.a1 = _ints((N, 64, 2 * h, 2 * w), seed + 3, -2, 2)           # zeros included: LeakyReLU' = 0.2 at 0
            self.add = _ints((N, 64, 2 * h, 2 * w), seed + 4, -3, 3) if with_add else None
            self.x = [_ints((N, 1, 4 * h, 4 * w), seed + 5 + t, -2, 2) for t in range(T)]
        else:
            q = lambda t: t.to(BF).float()
            self.dy = q(rnd((N, 128, h, w), seed + 1))
            self.w1 = q(rnd((128, 64, 4, 4), seed + 2, 0.05))
            self.a1 = q(rnd((N, 64, 2 * h, 2 * w), seed + 3))
            self.add = q(rnd((N, 64, 2 * h, 2 * w), seed + 4)) if with_add else None
            self.x = [q(rnd((N, 1, 4 * h, 4 * w), seed + 5 + t)) for t in range(T)]
        ops.ensure_workspace(max(ops.conv_workspace_bytes(self.d1, op) for op in (0, 1)), dev())
        ops.ensure_scratch(ops.scratch_bytes_for([self.d0, self.d1]), dev())
        wm = fwd_pack(self.w1, False)
        self.wd = torch.empty(wm.numel(), dtype=BF, device=dev())
        ops.pack_weights(BF, wm, 128, 16, 64, None, self.wd)
        self.upload()

    def upload(self):
        self.DY, self.A1 = nhwc(self.dy, BF), nhwc(self.a1, BF)
        self.ADD = nhwc(self.add, BF) if self.add is not None else None
        self.X = [t.reshape(-1).to(dev()).to(BF) for t in self.x]
        self.X2 = self.X[1] if self.T == 2 else None

    def du(self):
        """The gradient tensor as the two-launch path stores it."""
        ops = self.ops
        du = torch.empty(self.A1.numel(), dtype=BF, device=dev())
        if self.ADD is None:
            ops.conv_dgrad_act(self.d1, self.DY, self.wd, du, None, self.A1, ops.ACT_LRELU)
        else:
            ops.conv_dgrad_bn(self.d1, self.DY, self.wd, du, None, self.A1, ops.ACT_LRELU, self.ADD, ops.ACT_NONE)
        return du

    def two_launch(self, dw, db, overwrite=False):
        (self.ops.conv_wgrad_overwrite if overwrite else self.ops.conv_wgrad)(self.d0, self.X[0], self.X2, self.du(), dw, db)

    def fused(self, dw, db, overwrite=0):
        ops = self.ops
        assert ops.conv_dgrad_act_wthin_ok(self.d1, self.d0)
        assert ops.conv_dgrad_act_wthin_kernel_name(self.d1, self.d0) == "gg_dgrad_wthin_k<%d>" % self.T
        slabs = torch.full((ops.conv_dgrad_act_wthin_slab_bytes(self.d1, self.d0) // 4,), float("nan"), device=dev())
        ops.conv_dgrad_act_wthin(self.d1, self.DY, self.wd, self.A1, ops.ACT_LRELU, self.ADD, ops.ACT_NONE, self.d0,
                                 self.X[0], self.X2, dw, db, slabs, overwrite)

    def prior(self, seed):
        n = 64 * 16 * self.T
        return _ints((n,), seed, -3, 3).to(dev()), _ints((64,), seed + 1, -3, 3).to(dev())


def _same(a, b):
    """Equal bits outside the NaNs, NaNs in the same places (the two paths may carry different NaN payloads)."""
    na, nb = a.isnan(), b.isnan()
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)))


@pytest.fixture(autouse=True)
def unsplit_input_gradient():
    """Problems this small are split along K when a split-K workspace is registered (an earlier test of the process may have
    registered one) and then run the tile kernels, which have no such store: pin the un-split patch kernel, for both paths."""
    from thesis_pai_reconstruction_amd import ops
    ops.set_tunable("fwd_ksplit", 1)
    yield
    ops.set_tunable("fwd_ksplit")


@pytest.fixture
def slab_count(request):
    from thesis_pai_reconstruction_amd import ops

    def set_(n):
        if n is not None:
            ops.set_tunable("wthin_slabs", n)
    yield set_
    ops.set_tunable("wthin_slabs")


@pytest.mark.parametrize("form", FORMS, ids=["t2_disc", "t1_enc_add"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_%dx%d" % s[:3])
def test_equal_bits_on_integer_data(pai, shape, form, slab_count):
    """Add mode on a nonzero prior content, overwrite of both, and overwrite of the weights only -- each against the same
    mode of the two-launch path (pai_conv_wgrad, _overwrite, _overwrite_w)."""
    from thesis_pai_reconstruction_amd import ops
    N, h, w, nslab = shape
    T, with_add = form
    slab_count(nslab)
    p = _Problem(ops, N, h, w, T, with_add, integer=True, seed=10 * h + w)
    du = p.du().float().view(N, 2 * h, 2 * w, 64)
    # exactness of every partial sum, whatever the order: integers, and the sum of magnitudes stays below 2^24
    assert bool((du == du.round()).all())
    bound = float(du.abs().sum((0, 1, 2)).max()) * 2 + 3
    print(f"sum |du| * max |x| + |prior| = {bound:.0f} (< 2^24 = {2 ** 24})")
    assert bound < 2 ** 24
    pw, pb = p.prior(77)
    for mode, two in ((0, ops.conv_wgrad), (1, ops.conv_wgrad_overwrite), (2, ops.conv_wgrad_overwrite_w)):
        dw_a, db_a, dw_b, db_b = pw.clone(), pb.clone(), pw.clone(), pb.clone()
        two(p.d0, p.X[0], p.X2, p.du(), dw_a, db_a)
        p.fused(dw_b, db_b, mode)
        torch.cuda.synchronize()
        assert float(dw_a.abs().max()) > 0 and float(db_a.abs().max()) > 0
        assert torch.equal(dw_a.view(torch.int32), dw_b.view(torch.int32)), (shape, form, mode, "dw")
        assert torch.equal(db_a.view(torch.int32), db_b.view(torch.int32)), (shape, form, mode, "dbias")
    # no bias gradient asked for: the weights alone
    dw_a, dw_b = pw.clone(), pw.clone()
    ops.conv_wgrad(p.d0, p.X[0], p.X2, p.du(), dw_a, None)
    p.fused(dw_b, None, 0)
    torch.cuda.synchronize()
    assert torch.equal(dw_a.view(torch.int32), dw_b.view(torch.int32))


def _fp64_reference(p):
    """Host restatement in fp64 from the same bf16-valued inputs: du = act'(a1) * dgrad (+ add), then the thin layer's
    weight / bias gradient, in the forward pack's order [64][4][4][T]."""
    g = F.conv_transpose2d(p.dy.double(), p.w1.double(), stride=2, padding=1)
    du = torch.where(p.a1.double() > 0, g, 0.2 * g)
    if p.add is not None:
        du = du + p.add.double()
    x = torch.cat([t.double() for t in p.x], 1)
    w0 = torch.zeros(64, p.T, 4, 4, dtype=torch.float64, requires_grad=True)
    b0 = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w0, b0, stride=2, padding=1).backward(du)
    return w0.grad.permute(0, 2, 3, 1).reshape(-1), b0.grad


@pytest.mark.parametrize("form", FORMS, ids=["t2_disc", "t1_enc_add"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_%dx%d" % s[:3])
def test_random_data_against_fp64(pai, shape, form, slab_count):
    """Both paths round the same du to bf16 and differ in the order of the fp32 sums only.  The fused path's error against
    the fp64 restatement may be at most twice the two-launch path's own, measured here on the same inputs (no constant)."""
    from thesis_pai_reconstruction_amd import ops
    N, h, w, nslab = shape
    T, with_add = form
    slab_count(nslab)
    p = _Problem(ops, N, h, w, T, with_add, integer=False, seed=1000 + 10 * h + w)
    want_w, want_b = _fp64_reference(p)
    dw_a, db_a = torch.zeros(64 * 16 * T, device=dev()), torch.zeros(64, device=dev())
    dw_b, db_b = torch.zeros_like(dw_a), torch.zeros_like(db_a)
    p.two_launch(dw_a, db_a)
    p.fused(dw_b, db_b)
    torch.cuda.synchronize()
    for name, a, b, want in (("dw", dw_a, dw_b, want_w), ("dbias", db_a, db_b, want_b)):
        for metric in (rel_err, max_err):
            e_two, e_fused = metric(a.cpu(), want), metric(b.cpu(), want)
            print(f"{name} {metric.__name__}: two-launch {e_two:.3e} fused {e_fused:.3e}")
            assert e_two < 0.1, (name, "the reference does not describe the two-launch path", e_two)
            assert e_fused <= 2 * e_two, (name, metric.__name__, e_fused, e_two)


@pytest.mark.parametrize("where", ["a1", "dy_nan", "dy_inf"])
def test_nonfinite_values_propagate_alike(pai, where):
    """NaN / +-inf in the stored activation a1 only pick a branch of LeakyReLU' (NaN > 0 is false): finite results, equal
    bits.  In the incoming gradient they reach every channel of the pixels under the filter: the same elements are NaN in
    both paths, the others (integer data: exact sums) have equal bits."""
    from thesis_pai_reconstruction_amd import ops
    N, h, w, T = 2, 16, 16, 2
    p = _Problem(ops, N, h, w, T, False, integer=True, seed=31)
    if where == "a1":
        for i, v in enumerate((float("nan"), float("inf"), float("-inf"))):
            p.a1[i % N, 7 * i + 1, 3 + i, 2 * i] = v
            p.a1[(i + 1) % N, i, 2 * h - 1 - i, 2 * w - 1] = v
    elif where == "dy_nan":
        p.dy[0, 5, 0, 0] = float("nan")
        p.dy[1, 100, h - 1, w // 2] = float("nan")
    else:
        p.dy[0, 9, 1, w - 1] = float("inf")
        p.dy[1, 64, h // 2, 3] = float("-inf")
    p.upload()
    dw_a, db_a = torch.zeros(64 * 16 * T, device=dev()), torch.zeros(64, device=dev())
    dw_b, db_b = torch.zeros_like(dw_a), torch.zeros_like(db_a)
    p.two_launch(dw_a, db_a)
    p.fused(dw_b, db_b)
    torch.cuda.synchronize()
    print(where, "NaN elements: dw", int(dw_a.isnan().sum()), int(dw_b.isnan().sum()), "dbias", int(db_a.isnan().sum()),
          int(db_b.isnan().sum()))
    if where == "a1":
        assert not bool(dw_a.isnan().any()) and not bool(dw_a.isinf().any())
    else:
        assert bool(dw_a.isnan().any() or dw_a.isinf().any())
    assert _same(dw_a, dw_b) and _same(db_a, db_b)


def _integer_disc(pai):
    """A Discriminator whose D-phase backward pass is exact: weights in {0, 1} (sparse), biases 1 -- every activation is
    positive, LeakyReLU' = 1 -- and integer images; with logit gradients in {-5, 0, 5} every du is an integer."""
    from thesis_pai_reconstruction_amd.models.wrapper import Discriminator
    disc = Discriminator(1)
    dens = [0.25, 1 / 32, 1 / 64, 1 / 128, 1 / 16]       # (the test checks that the sums these leave stay below 2^24)
    with torch.no_grad():
        for k, conv in enumerate([disc.discriminator[i].block[0] for i in range(4)] + [disc.discriminator[4]]):
            conv.weight.copy_(_ints(tuple(conv.weight.shape), 50 + k, 1, 1, dens[k]))
            if conv.bias is not None:
                conv.bias.fill_(1.0)
    disc.to(dev())
    disc.compute_dtype = BF
    return disc


def test_disc_backward_eager_and_planned(pai):
    """DiscEngine.backward of the D phase (need_params, no need_dy) on integer data: block 0's weight and bias gradient
    have the same bits with the tunable dgrad_wthin off (the two launches) and on, and when the fused pass is replayed
    from a recorded launch plan (ops.Plan, the C-side plan PlannedStep replays: the slab clear, the launch and the slab sum
    are nodes of it); the fused pass allocates no du[0] and launches nothing on the tail stream."""
    from thesis_pai_reconstruction_amd import ops
    disc = _integer_disc(pai)
    eng = disc.engine
    N, H = 2, 64
    x, y = (_ints((N, 1, H, H), 60 + i, 0, 2).to(dev()) for i in range(2))
    gl = None

    def run(record=None):
        nonlocal gl
        _, S = eng.forward(x, y, BF)
        if gl is None:
            gl = (_ints(tuple(S["logits"].shape), 70, -1, 1) * 5).to(dev())
        A = eng.arena()
        A.flat.zero_()
        torch.cuda.synchronize()
        if record is None:
            eng.backward(S, gl, need_params=True, need_dy=False)
        else:
            with record.recording():
                eng.backward(S, gl, need_params=True, need_dy=False)
        torch.cuda.synchronize()
        c0 = eng.convs[0]
        out = A.seg(c0.weight).clone(), A.seg(c0.bias).clone()
        return S, A, out

    ops.set_tunable("dgrad_wthin", 0)
    try:
        S, A, (w_two, b_two) = run()
        du0 = S["grads"]["du"][0].float()
        eng.release(S)
    finally:
        ops.set_tunable("dgrad_wthin")
    assert bool((du0 == du0.round()).all()) and float(du0.abs().max()) > 0
    bound = float(du0.view(-1, 64).abs().sum(0).max()) * 2
    print(f"sum |du0| * max |x| = {bound:.0f} (< 2^24)")
    assert bound < 2 ** 24
    assert float(w_two.abs().max()) > 0 and float(b_two.abs().max()) > 0

    eng2 = _integer_disc(pai).engine           # a fresh engine: its slot has never seen the two-launch pass
    eng, eng_two = eng2, eng
    assert ops.conv_dgrad_act_wthin_ok(eng._plan(N, H, H, BF, x.device)["desc"][1], eng._plan(N, H, H, BF, x.device)["desc"][0])
    S, A, (w_f, b_f) = run()
    assert S["grads"]["du"][0] is None and eng._side.stream2 is None
    assert torch.equal(w_two.view(torch.int32), w_f.view(torch.int32))
    assert torch.equal(b_two.view(torch.int32), b_f.view(torch.int32))
    eng.release(S)
    plan = ops.Plan()
    S, A, (w_r, b_r) = run(plan)               # recorded while it runs
    assert torch.equal(w_two.view(torch.int32), w_r.view(torch.int32))
    A.flat.zero_()
    torch.cuda.synchronize()
    plan.run()
    torch.cuda.synchronize()
    c0 = eng.convs[0]
    assert plan.info()["runs"] == 1
    assert torch.equal(w_two.view(torch.int32), A.seg(c0.weight).view(torch.int32))
    assert torch.equal(b_two.view(torch.int32), A.seg(c0.bias).view(torch.int32))
    eng.release(S)
    del eng_two
