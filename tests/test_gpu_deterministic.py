"""GPU: the deterministic mode, site by site.  One case per place where a float sum crosses workgroups in arrival order in
default mode; each case at the smallest shape at which at least two workgroups meet in one output element
there -- asserted through pai_conv_wgrad_order_free == 0 and pai_conv_kernel_name, not assumed from the shape.

Per case: (a) on small-integer data (every sum exact below 2^24) the mode's result is the default mode's, bit for bit, when
adding to a buffer and when overwriting one; (b) on data whose magnitudes span 2^12 (another association changes low bits)
three launches under the mode agree bit for bit; (c) the error against an fp64 restatement stays inside the bound the
family's own test applies (tests/test_gpu_conv.py: relative L2 error 1e-4 for fp32 storage, 3e-3 for bf16;
tests/test_gpu_vit_ops.py for pai_colsum; tests/test_gpu_gate.py for the gate); (d) pai_order_dependent_launches stays put
over the launches under the mode and moves over the default ones; (e) with the workspace the order-free form needs
unregistered, the launch under the mode fails with an error that names it, and writes nothing."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gpu_util import dev, nhwc, q, rel_err, rnd

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
TOL_W = {F32: 1e-4, BF: 3e-3}      # tests/test_gpu_conv.py, weight / bias gradient

# (name, dtype, transposed, stride, kernel, N, H, W, C1, C2, Cout, kernel-name prefix in default mode, workspace whose absence refuses)
CONV_CASES = [
    # k4 s2, 1024 output pixels in two pixel splits: slabs for dW, the bias sums by atomics per wave
    ("patch3", BF, 0, 2, 4, 4, 32, 32, 64, 0, 128, "gg_wgrad_patch3_k", "wgrad"),
    # tile / patch kernels: > 4096 pixels and one or few channel tiles -> 16 pixel splits that meet by atomics
    ("tile_3x3", BF, 0, 1, 3, 2, 64, 64, 64, 0, 64, "gg_wgrad_", "wgrad"),
    ("tile_1x1", BF, 0, 1, 1, 2, 64, 64, 64, 0, 64, "gg_wgrad_", "wgrad"),
    # four-phase transposed layer with a bias: the phases' bias sums meet by atomics even un-split
    ("convt_4phase", BF, 1, 2, 4, 2, 32, 32, 64, 0, 64, "gg_wgrad_", "wgrad"),
    # thin forms
    ("thin_conv_1", BF, 0, 2, 4, 2, 32, 32, 1, 0, 64, "thin_mfma_bf16", "scratch"),
    ("thin_conv_2", BF, 0, 2, 4, 2, 32, 32, 1, 1, 64, "thin_mfma_bf16", "scratch"),
    ("thin_convt", BF, 1, 2, 4, 2, 32, 32, 64, 0, 1, "thin_mfma_bf16", "scratch"),
    ("thin_k4s1", BF, 0, 1, 4, 2, 32, 32, 128, 0, 1, "thin_mfma_bf16", "scratch"),
    ("thin_3x3", BF, 0, 1, 3, 2, 32, 32, 1, 0, 64, "thin_mfma_bf16", "scratch"),
    ("thin_3x3_out", BF, 0, 1, 3, 2, 32, 32, 64, 0, 1, "thin_mfma_bf16", "scratch"),
    # fp32 parity path, odd channel counts, 180 output pixels in three splits
    ("simt_f32", F32, 0, 2, 4, 3, 12, 20, 3, 0, 5, "gg_simt", "wgrad"),
    # one or two filters in fp32: the row-dot kernel (LDS and global atomics); under the mode gg_simt un-split
    ("rowdot_f32", F32, 0, 1, 4, 2, 16, 16, 16, 0, 1, "gg_rowdot", "wgrad"),
]


@pytest.fixture
def det(pai):
    """det(flag) switches the mode; the built-in default comes back whatever the test leaves."""
    from thesis_pai_reconstruction_amd import ops
    yield pai.set_deterministic
    ops.set_tunable("deterministic")


def _desc(ops, case):
    name, dtype, tr, s, k, N, H, W, C1, C2, Cout, prefix, ws = case
    return ops.make_desc(dtype, tr, N, H, W, C1, C2, Cout, s, 0, 0, ops.ACT_NONE, kernel=k)


def _register(ops, d):
    """Workspaces for the layer, sized under the mode (never less than the default mode's)."""
    ops.ensure_workspace(max(ops.conv_workspace_bytes(d, 0), ops.conv_workspace_bytes(d, 1)), dev())
    ops.ensure_scratch(ops.scratch_bytes_for([d]), dev())
    ops.ensure_wgrad_workspace([d], dev())


def _ints(shape, seed, lo=-2, hi=2):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))


def _wide(shape, seed):
    """Normal values times 2^e, e uniform in 0..12: sums cancel, so the association shows in the low bits."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal(shape) * np.exp2(rng.integers(0, 13, size=shape))).astype(np.float32))


def _inputs(case, gen, seed):
    name, dtype, tr, s, k, N, H, W, C1, C2, Cout, prefix, ws = case
    pad = 0 if k == 1 else 1
    OH, OW = (2 * H, 2 * W) if tr else ((H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1)
    x1 = q(gen((N, C1, H, W), seed), dtype)
    x2 = q(gen((N, C2, H, W), seed + 1), dtype) if C2 else None
    dy = q(gen((N, Cout, OH, OW), seed + 2), dtype)
    return x1, x2, dy


def _ref(case, x1, x2, dy):
    """fp64 weight and bias gradient, dw in the library's layout [Cout][kh][kw][Cin]."""
    name, dtype, tr, s, k, N, H, W, C1, C2, Cout, prefix, ws = case
    x = (torch.cat([x1, x2], 1) if C2 else x1).double()
    Cin = C1 + C2
    w = torch.zeros((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), dtype=torch.float64, requires_grad=True)
    pad = 0 if k == 1 else 1
    y = F.conv_transpose2d(x, w, None, stride=2, padding=1) if tr else F.conv2d(x, w, None, stride=s, padding=pad)
    y.backward(dy.double())
    dw = w.grad.permute(1, 2, 3, 0) if tr else w.grad.permute(0, 2, 3, 1)
    return dw.contiguous().reshape(-1), dy.double().sum((0, 2, 3))


def _run(ops, case, d, X, overwrite, init=None):
    name, dtype, tr, s, k, N, H, W, C1, C2, Cout, prefix, ws = case
    nw = Cout * k * k * (C1 + C2)
    if overwrite:
        dw = torch.full((nw,), float("nan"), device=dev())
        db = torch.full((Cout,), float("nan"), device=dev())
        ops.conv_wgrad_overwrite(d, X[0], X[1], X[2], dw, db)
    else:
        dw = torch.full((nw,), float(init), device=dev())
        db = torch.full((Cout,), float(init) + 2.0, device=dev())
        ops.conv_wgrad(d, X[0], X[1], X[2], dw, db)
    torch.cuda.synchronize()
    return dw, db


def _dev_inputs(case, x1, x2, dy):
    dtype = case[1]
    return nhwc(x1, dtype), nhwc(x2, dtype) if x2 is not None else None, nhwc(dy, dtype)


def _unregister(pai, ops, which):
    h = ops.handle_for(dev())
    lib = pai.lib.load()
    if which == "wgrad":
        assert lib.pai_handle_set_wgrad_workspace(h._h, None, 0) == 0
    else:
        assert lib.pai_handle_set_scratch(h._h, None, 0) == 0


def _reregister(pai, ops):
    h = ops.handle_for(dev())
    lib = pai.lib.load()
    if h.wgrad_workspace is not None:
        assert lib.pai_handle_set_wgrad_workspace(h._h, ctypes.c_void_p(h.wgrad_workspace.data_ptr()), h.wgrad_workspace.numel() * 4) == 0
    if h.scratch is not None:
        assert lib.pai_handle_set_scratch(h._h, ctypes.c_void_p(h.scratch.data_ptr()), h.scratch.numel() * 4) == 0


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_wgrad_site(pai, det, case):
    from thesis_pai_reconstruction_amd import ops
    name, dtype, tr, s, k, N, H, W, C1, C2, Cout, prefix, ws = case
    d = _desc(ops, case)
    det(True)
    _register(ops, d)
    det(False)
    # the default-mode launch of this shape IS order-dependent, on the family the case is here for
    assert not ops.conv_wgrad_order_free(d, True), name
    assert ops.conv_kernel_name(d, 2).startswith(prefix), (name, ops.conv_kernel_name(d, 2))

    # (a) + (d): integer data, add and overwrite
    Xi = _dev_inputs(case, *_inputs(case, _ints, 11))
    c0 = ops.order_dependent_launches()
    add_def, addb_def = _run(ops, case, d, Xi, False, 3)
    ovr_def, ovrb_def = _run(ops, case, d, Xi, True)
    c1 = ops.order_dependent_launches()
    assert c1 == c0 + 2, (name, c0, c1)
    det(True)
    assert ops.conv_wgrad_order_free(d, True), name
    add_det, addb_det = _run(ops, case, d, Xi, False, 3)
    ovr_det, ovrb_det = _run(ops, case, d, Xi, True)
    ref_w, ref_b = _ref(case, *_inputs(case, _ints, 11))
    assert float(ref_w.abs().max()) < 2 ** 24 and float(ref_b.abs().max()) < 2 ** 24
    assert torch.equal(ovr_det.cpu().double(), ref_w) and torch.equal(ovrb_det.cpu().double(), ref_b), name    # exact sums
    assert torch.equal(add_det, add_def) and torch.equal(addb_det, addb_def), name
    assert torch.equal(ovr_det, ovr_def) and torch.equal(ovrb_det, ovrb_def), name
    assert torch.equal(add_det.cpu().double(), ref_w + 3) and torch.equal(addb_det.cpu().double(), ref_b + 5), name

    # (b): magnitudes over 2^12, three launches
    Xw = _dev_inputs(case, *_inputs(case, _wide, 21))
    runs = [_run(ops, case, d, Xw, True) for _ in range(3)]
    for dw, db in runs[1:]:
        assert torch.equal(dw, runs[0][0]) and torch.equal(db, runs[0][1]), name
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())

    # (c): the family's bound against fp64, on normal data as its own test draws it
    xs = _inputs(case, rnd, 31)
    dw, db = _run(ops, case, d, _dev_inputs(case, *xs), True)
    ref_w, ref_b = _ref(case, *xs)
    ew, eb = rel_err(dw.cpu(), ref_w), rel_err(db.cpu(), ref_b)
    print(f"{name}: dw rel err {ew:.3g}, dbias rel err {eb:.3g} (bound {TOL_W[dtype]:g})")
    assert ew < TOL_W[dtype] and eb < TOL_W[dtype], (name, ew, eb)
    assert ops.order_dependent_launches() == c1, name          # (d): nothing under the mode took an arrival-order path

    # (e): refusal, nothing written
    _unregister(pai, ops, ws)
    try:
        dw = torch.full((Cout * k * k * (C1 + C2),), 7.0, device=dev())
        db = torch.full((Cout,), 9.0, device=dev())
        with pytest.raises(ops.PaiError, match="deterministic mode needs [0-9]+ bytes of " +
                           ("weight-gradient workspace" if ws == "wgrad" else "scratch")):
            ops.conv_wgrad(d, Xi[0], Xi[1], Xi[2], dw, db)
        torch.cuda.synchronize()
        assert bool((dw == 7.0).all()) and bool((db == 9.0).all()), name
    finally:
        _reregister(pai, ops)
    assert ops.order_dependent_launches() == c1, name


def test_patch3_atomic_store_is_refused_not_taken(pai, det):
    """gg_wgrad_patch3_k without its slab buffer adds the pixel splits with atomics in default mode (and the query says
    so); under the mode the same registration is an error."""
    from thesis_pai_reconstruction_amd import ops
    case = CONV_CASES[0]
    d = _desc(ops, case)
    det(True)
    _register(ops, d)
    det(False)
    assert ops.conv_wgrad_order_free(d, False)           # slabs registered: order-free today already, without a bias
    _unregister(pai, ops, "wgrad")
    try:
        assert not ops.conv_wgrad_order_free(d, False)   # atomics
        det(True)
        X = _dev_inputs(case, *_inputs(case, _ints, 5))
        dw = torch.zeros(128 * 16 * 64, device=dev())
        with pytest.raises(ops.PaiError, match="weight-gradient workspace"):
            ops.conv_wgrad(d, X[0], None, X[2], dw, None)
    finally:
        _reregister(pai, ops)


# ---- pai_colsum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,C,blocks", [(1000, 96, 4), (32, 16384, 1), (777, 1, 4)], ids=["1000x96", "32x16384", "777x1"])
def test_colsum_site(pai, det, rows, C, blocks, dtype):
    """1000 x 96: four row blocks meet in every column by atomics in default mode.  32 x 16384 (the positional-embedding
    gradient) has ONE row block: its default launch is order-free already and the counter says so; it is here for the
    column-chunk stride of the partial-row form.  777 x 1: the bias gradient of a one-filter layer, ragged last block."""
    from thesis_pai_reconstruction_amd import ops
    lib = pai.lib.load()
    assert lib.pai_colsum_scratch_bytes(rows, C) == blocks * C * 4

    def run(x, init):
        out = torch.full((C,), float(init), device=dev())
        ops.colsum(dtype, x, rows, C, out)
        torch.cuda.synchronize()
        return out

    xi = q(_ints((rows, C), 3, -3, 3), dtype)
    Xi = xi.to(dev()).to(dtype).contiguous()
    c0 = ops.order_dependent_launches()
    base = run(Xi, 4)
    c1 = ops.order_dependent_launches()
    assert c1 - c0 == (1 if blocks > 1 else 0)
    det(True)
    got = run(Xi, 4)
    assert torch.equal(got, base) and torch.equal(got.cpu().double(), xi.double().sum(0) + 4)
    xw = q(_wide((rows, C), 4), dtype)
    Xw = xw.to(dev()).to(dtype).contiguous()
    outs = [run(Xw, 0) for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # the bound of tests/test_gpu_vit_ops.py (test_colsum, _sum_ok): 1e-5 of the sum of |terms| per column, on its data
    xn = q(rnd((rows, C), 51) + 0.3, dtype)
    got = run(xn.to(dev()).to(dtype).contiguous(), 0).cpu().double()
    err = (got - xn.double().sum(0)).abs()
    print(f"colsum {rows}x{C}: max err / sum|terms| {float((err / xn.double().abs().sum(0)).max()):.3g}")
    assert bool((err <= 1e-5 * xn.double().abs().sum(0)).all())
    assert ops.order_dependent_launches() == c1
    # (e) without scratch: refused, nothing written
    h = ops.handle_for(dev())
    assert lib.pai_handle_set_scratch(h._h, None, 0) == 0
    try:
        out = torch.full((C,), 7.0, device=dev())
        r = lib.pai_colsum(ops.code_of(dtype), ctypes.c_void_p(Xi.data_ptr()), rows, C, ctypes.c_void_p(out.data_ptr()), None)
        assert r != 0 and b"bytes of scratch" in lib.pai_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    finally:
        _reregister(pai, ops)


# ---- losses -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l1", "mse", "bce"])
def test_loss_site(pai, det, kind):
    """loss_k: one fp64 atomic per workgroup.  Under the mode the workgroups' terms are multiples of 2^-36, so their fp64 sum
    is exact in every order: it equals the sum of the same terms added in any order on the host, and repeats bit for bit."""
    from thesis_pai_reconstruction_amd import ops
    n = 256 * 8 * 5 + 24          # several workgroups, a ragged tail

    def run(x, t, scale=100.0):
        loss = torch.zeros(1, dtype=torch.float64, device=dev())
        grad = torch.empty(n, device=dev())
        if kind == "l1":
            ops.l1(x, t, scale, loss, 1.0, grad)
        elif kind == "mse":
            ops.mse(x, t, scale, loss, 1.0, grad)
        else:
            ops.bce_logits(x, 1.0, scale, loss, 1.0, grad)
        torch.cuda.synchronize()
        return loss, grad

    # (a) integer data: every term and sum exact -> the two modes agree bit for bit
    xi, ti = _ints((n,), 1, -4, 4).to(dev()), _ints((n,), 2, -4, 4).to(dev())
    c0 = ops.order_dependent_launches()
    base, gbase = run(xi, ti, float(n))          # scale / n = 1: the terms are integers
    c1 = ops.order_dependent_launches()
    assert c1 == c0 + 1
    det(True)
    got, ggot = run(xi, ti, float(n))
    assert torch.equal(ggot, gbase)
    if kind != "bce":
        assert torch.equal(got, base)
        want = (xi - ti).abs().double().sum() if kind == "l1" else ((xi - ti).double() ** 2).sum()
        assert float(got) == float(want)
    # (b) wide data: repeats bit for bit, and is a multiple of 2^-36
    xw, tw = (_wide((n,), 3) * 2.0 ** -6).to(dev()), (_wide((n,), 4) * 2.0 ** -6).to(dev())
    outs = [run(xw, tw, 1.0)[0] for _ in range(3)]      # (scale 1: every workgroup's term is below 2^8, hence rounded)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    v = float(outs[0]) * 2.0 ** 36
    assert v == round(v) and abs(float(outs[0])) < 2.0 ** 17
    # (c) against fp64, the bounds of tests/test_gpu_step_ops.py: 1e-5 of the sum of |terms| (test_l1_mse), BCE_BOUND per unit
    # of 1 + |x| summed (test_bce).  (The rounding adds at most 2^-37 per workgroup, far inside either.)
    from test_gpu_step_ops import BCE_BOUND
    xn, tn = rnd((n,), 5).to(dev()), rnd((n,), 6).to(dev())
    loss = float(run(xn, tn)[0])
    xd, td = xn.double().cpu(), tn.double().cpu()
    w = 100.0 / n
    if kind == "l1":
        want, lim = w * float((xd - td).abs().sum()), 1e-5 * w * float((xd - td).abs().sum())
    elif kind == "mse":
        want, lim = w * float(((xd - td) ** 2).sum()), 1e-5 * w * float(((xd - td) ** 2).sum())
    else:
        want = w * float(F.binary_cross_entropy_with_logits(xd, torch.ones_like(xd), reduction="sum"))
        lim = w * float((BCE_BOUND * (1 + xd.abs())).sum())
    print(f"{kind}: loss {loss!r} fp64 {want!r} err / bound {abs(loss - want) / lim:.3g}")
    assert abs(loss - want) <= lim
    assert ops.order_dependent_launches() == c1


# ---- SSIM / evaluation sums -------------------------------------------------------------------------------------------------
def test_ssim_site(pai, det):
    """ssim_k: two or three fp64 atomics per workgroup.  Under the mode the terms are rounded for exact addition: repeated
    launches agree bit for bit, stay within the rounding of the default mode's value, and meet the fp64 bounds of
    tests/test_gpu_ssim_paths.py (per-image SSIM 5e-6 absolute; squared error 1e-6 relative, its per-image MSE bound)."""
    import oracle
    from test_gpu_ssim_paths import make_pair, ref_metrics
    from thesis_pai_reconstruction_amd import ops
    shape = (2, 3, 96, 80)
    NC, H, W = 6, 96, 80
    a, b = make_pair(shape)
    p, t = b.to(dev()), a.to(dev())

    def run():
        out2 = torch.zeros(2, dtype=torch.float64, device=dev())
        per = torch.zeros(NC, dtype=torch.float64, device=dev())
        ops.ssim_sse(p, t, NC, H, W, False, out2, per)
        torch.cuda.synchronize()
        return out2, per

    c0 = ops.order_dependent_launches()
    base2, basep = run()
    c1 = ops.order_dependent_launches()
    assert c1 == c0 + 1
    det(True)
    outs = [run() for _ in range(3)]
    for o2, pp in outs[1:]:
        assert torch.equal(o2, outs[0][0]) and torch.equal(pp, outs[0][1])
    tiles = 3 * 3 * NC
    assert abs(float(outs[0][0][0] - base2[0])) <= tiles * 2.0 ** -37 + 1e-12 * abs(float(base2[0]))
    assert abs(float(outs[0][0][1] - base2[1])) <= tiles * 2.0 ** -29 + 1e-12 * abs(float(base2[1]))
    assert float((outs[0][1] - basep).abs().max()) <= 9 * 2.0 ** -37 + 1e-12
    # (c) fp64: per-plane crop means against the oracle's, the squared error against the fp64 sum
    ref_per, _ = oracle.ssim_full(b.double().reshape(NC, 1, H, W), a.double().reshape(NC, 1, H, W))
    e_per = float((outs[0][1].cpu() - ref_per.reshape(-1)).abs().max())
    sse = float(((b.double() - a.double()) ** 2).sum())
    e_sse = abs(float(outs[0][0][1]) - sse) / sse
    print(f"ssim under the mode: per-plane max abs err {e_per:.3g} (bound 5e-6), squared error rel err {e_sse:.3g} (bound 1e-6)")
    assert e_per < 5e-6 and e_sse <= 1e-6
    assert abs(float(outs[0][0][0]) - float(ref_per.sum())) < 5e-6 * NC
    assert ops.order_dependent_launches() == c1


def test_eval_planes_site(pai, det):
    """eval_planes_k: the workgroups of a plane add into the plane's two fp64 words (two tile rows, two workgroups per row at
    W = 301).  Under the mode eval_planes_det_k runs: three calls agree bit for bit, the values meet the fp64 bounds of
    tests/test_gpu_ssim_paths.py (test_eval_planes_wide_and_unaligned), the byte outputs are the default mode's."""
    import oracle
    from test_gpu_ssim_paths import make_pair, ref_metrics
    from thesis_pai_reconstruction_amd import functional as PF, ops
    shape = (2, 1, 45, 301)
    a, b = make_pair(shape)
    pred, target = (b * 2.4 - 1.2).to(dev()), (a * 2.4 - 1.2).to(dev())
    assert ops.eval_kernel_name(0) == "eval_planes_k"
    c0 = ops.order_dependent_launches()
    base = PF.eval_images(pred, target, denorm=True, ssim_map=True, hot=True)
    torch.cuda.synchronize()
    c1 = ops.order_dependent_launches()
    assert c1 > c0
    det(True)
    assert ops.eval_kernel_name(0) == "eval_planes_det_k"
    runs = [PF.eval_images(pred, target, denorm=True, ssim_map=True, hot=True) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        for f in ("ssim", "psnr", "mse"):
            assert torch.equal(getattr(r, f), getattr(runs[0], f)), f
    assert torch.equal(runs[0].ssim_map_u8, base.ssim_map_u8) and torch.equal(runs[0].hot_u8, base.hot_u8)
    dp, dt = oracle.denormalize(b * 2.4 - 1.2), oracle.denormalize(a * 2.4 - 1.2)
    for i in range(shape[0]):
        r = ref_metrics(dp[i:i + 1], dt[i:i + 1])
        assert abs(float(runs[0].ssim[i]) - float(r["per"][0])) < 5e-6
        assert abs(float(runs[0].psnr[i]) - float(r["psnr"])) < 2e-5
        assert abs(float(runs[0].mse[i]) - float(r["rmse"]) ** 2) <= 1e-6 * float(r["rmse"]) ** 2
    assert ops.order_dependent_launches() == c1


# ---- first-layer weight gradient in the next layer's input-gradient store ------------------------------------------------
def test_wthin_is_refused_under_the_mode(pai, det):
    """gg_dgrad_wthin_k adds into `workgroup % S` slabs by atomics: counted in default mode; under the mode the predicate
    answers 0, the call itself refuses and writes nothing, and the two-launch path it leaves gives the same bits on integer
    data."""
    import test_gpu_dgrad_wthin as W
    from thesis_pai_reconstruction_amd import ops
    ops.set_tunable("fwd_ksplit", 1)         # as that module's own fixture: the un-split patch kernel for both paths
    try:
        P = W._Problem(ops, 2, 16, 16, 1, True, True)
        ops.ensure_wgrad_workspace([P.d0], dev())
        dw_f, db_f = torch.zeros(64 * 16, device=dev()), torch.zeros(64, device=dev())
        c0 = ops.order_dependent_launches()
        P.fused(dw_f, db_f)
        torch.cuda.synchronize()
        c1 = ops.order_dependent_launches()
        assert c1 == c0 + 1
        det(True)
        ops.ensure_scratch(ops.scratch_bytes_for([P.d0, P.d1]), dev())
        ops.ensure_wgrad_workspace([P.d0], dev())
        assert not ops.conv_dgrad_act_wthin_ok(P.d1, P.d0)
        dw, db = torch.full((64 * 16,), 7.0, device=dev()), torch.full((64,), 9.0, device=dev())
        slabs = torch.zeros(ops.conv_dgrad_act_wthin_slab_bytes(P.d1, P.d0) // 4, device=dev())
        with pytest.raises(ops.PaiError, match="not under the deterministic mode"):
            ops.conv_dgrad_act_wthin(P.d1, P.DY, P.wd, P.A1, ops.ACT_LRELU, P.ADD, ops.ACT_NONE, P.d0, P.X[0], P.X2, dw, db, slabs, 0)
        torch.cuda.synchronize()
        assert bool((dw == 7.0).all()) and bool((db == 9.0).all())
        dw_t, db_t = torch.zeros(64 * 16, device=dev()), torch.zeros(64, device=dev())
        P.two_launch(dw_t, db_t)
        torch.cuda.synchronize()
        assert torch.equal(dw_t, dw_f) and torch.equal(db_t, db_f)
        assert ops.order_dependent_launches() == c1
    finally:
        ops.set_tunable("fwd_ksplit")


# ---- attention gate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_gate_site(pai, det, dtype):
    """gate_hidden_bwd_k: d w_a / d b_a by atomics beside the part_i / part_s partial rows; under the mode a partial row like
    its neighbours.  300 rows = five workgroups.  Bound: tests/test_gpu_gate.py (_sum_ok: 1e-5 of the sum of |terms|)."""
    from thesis_pai_reconstruction_amd import ops
    from test_gpu_gate import ref_gate_hidden_bwd, _sum_ok
    K, M = 16, 300
    lib = pai.lib.load()
    rows = ops.gate_partial_rows(M)
    assert rows == 5

    def inputs(gen, seed):
        h = q(torch.relu(gen((M, K), seed)), dtype)
        ig, sg = q(gen((M, K), seed + 1), dtype), q(gen((M, K), seed + 2), dtype)
        dl, logit = gen((M,), seed + 3), gen((M,), seed + 4)
        return h, ig, sg, dl, logit

    def run(h, ig, sg, dl, logit, exact, init):
        one = lambda v: torch.tensor([v], device=dev())
        vec = lambda v: torch.full((K,), v, device=dev())
        # exact: BatchNorm constants that keep integer data integer (mean 0, rstd 1, no sums term, w_a = 1)
        mean_a, rstd_a = one(0.0 if exact else 0.25), one(1.0 if exact else 0.7)
        sums_a = torch.tensor([0.0, 0.0] if exact else [0.3 * M, -0.2 * M], device=dev())
        w_a = vec(1.0) if exact else rnd((K,), 77, 0.4).to(dev())
        dsum = torch.empty(M * K, dtype=dtype, device=dev())
        part_i, part_s = torch.empty(rows * 2 * K, device=dev()), torch.empty(rows * 2 * K, device=dev())
        dw, db = torch.full((K,), float(init), device=dev()), torch.full((1,), float(init), device=dev())
        dd = lambda v: v.to(dev()).to(dtype).contiguous()
        ops.gate_hidden_bwd(dtype, dl.to(dev()), logit.to(dev()), dd(h), dd(ig), dd(sg), M, K, mean_a, rstd_a, None, sums_a, w_a,
                            vec(0.0), vec(1.0), vec(0.0), vec(1.0), dsum, part_i, part_s, dw, db)
        torch.cuda.synchronize()
        return dw, db, (mean_a, rstd_a, sums_a, w_a)

    xi = inputs(lambda s, seed: _ints(s, seed), 1)
    c0 = ops.order_dependent_launches()
    dw_def, db_def, _ = run(*xi, True, 3)
    c1 = ops.order_dependent_launches()
    assert c1 == c0 + 1
    det(True)
    dw_det, db_det, _ = run(*xi, True, 3)
    assert torch.equal(dw_det, dw_def) and torch.equal(db_det, db_def)
    h, ig, sg, dl, logit = xi
    assert torch.equal(dw_det.cpu().double(), (dl.double()[:, None] * h.double()).sum(0) + 3)
    assert float(db_det) == float(dl.double().sum()) + 3
    xw = inputs(_wide, 11)
    outs = [run(*xw, False, 0)[:2] for _ in range(3)]
    for dw, db in outs[1:]:
        assert torch.equal(dw, outs[0][0]) and torch.equal(db, outs[0][1])
    xn = inputs(rnd, 21)
    dw, db, (mean_a, rstd_a, sums_a, w_a) = run(*xn, False, 0)
    h, ig, sg, dl, logit = xn
    z, o = torch.zeros(K), torch.ones(K)
    ref = ref_gate_hidden_bwd(dl, logit, h, ig, sg, mean_a.cpu(), rstd_a.cpu(), None, sums_a.cpu(), w_a.cpu(), z, o, z, o)
    _sum_ok(dw.cpu(), ref["dw"], ref["dw_abs"], "dw_a")
    _sum_ok(db.cpu(), ref["db"].reshape(1), ref["db_abs"].reshape(1), "db_a")
    assert ops.order_dependent_launches() == c1
    # (e) without scratch: refused before any launch
    hd = ops.handle_for(dev())
    assert lib.pai_handle_set_scratch(hd._h, None, 0) == 0
    try:
        assert hd.scratch_head >= lib.pai_gate_scratch_bytes(M, K)       # (reserved by the launches above: the wrapper re-registers nothing)
        with pytest.raises(ops.PaiError, match="deterministic mode needs [0-9]+ bytes of scratch"):
            run(*xi, True, 3)
    finally:
        _reregister(pai, ops)
