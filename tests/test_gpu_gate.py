"""The four attention-gate row kernels of csrc/gate.hip on their own, against fp64 restatements of each kernel's contract
(the header comment of gate.hip), at the launch edges the Attention U-Net fixtures do not reach: 1, 2, 8 and 64 lanes per
row, K = 512 (the combine loop of gate_hidden_bwd_k runs twice), C = 1024 (two passes per row in gate_apply_bwd_k),
single rows, ragged last blocks, the GATE_MAX_BLOCKS cap with 65 rows per block and empty trailing blocks, the wrapped
grid-stride loop of gate_apply_k, relu_out, absent b_a / db_a / gamma_a -- in fp32 and in bf16 storage.

Every reference is computed from exactly the tensors handed to the kernel (in bf16: the bf16-rounded values).  Two
quantities are DEFINED on a stored bf16 output: gate_hidden's logit is the dot product of h "as stored", and
gate_hidden_bwd's BatchNorm sums are formed from dsum "as stored".  Their references therefore take the h / dsum the
kernel wrote (which is checked elementwise on its own): rounding the fp64 h to bf16 on the host instead would disagree with
the device on the few elements that sit within fp32 noise of a bf16 rounding boundary, by 2^-8 of one term each -- far
outside the fp32 bounds below although nothing is wrong.  A kernel that used the un-rounded value would be off by
2^-9 relative in EVERY term and fails them.

Bounds:
  fp32 elementwise outputs      max |got - ref| < 1e-5 * max |ref|        (the bar of tests/test_gpu_ops.py for row kernels)
  bf16 stored outputs           |got - ref| <= 2^-8 |ref| + 1e-6 max |ref|  (one rounding of an fp32 value + fp32 noise at 0)
  fp32 sums and accumulators    |got - ref| <= 1e-5 * sum |terms|          (n u of a few hundred sequential fp32 additions)
  att                           ATT_BOUND, see test_gate_apply
The accumulators dw_a / db_a start from small non-zero values (1e-3: small against the increments, so that the rounding
of start + increment stays inside the sum bound) and the increment is what is compared."""
import numpy as np
import pytest
import torch

from _gpu_util import dev, max_err, q, rel_err, rnd

GUARD = 64
BIG_M = 64 * 2048 + 77          # GATE_MAX_BLOCKS reached, 65 rows per block, ragged last block, 30 empty trailing blocks
WRAP_M = 8192 * 256 // 2 + 77   # C = 16: M * C / 8 threads' worth of work above the 8192 x 256 grid of gate_apply_k
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
# measured on an MI355X over every case of test_gate_apply: max |att - fp64 sigmoid| = 9.7e-8 (torch's own fp32 CPU sigmoid
# on the same arguments: 9.6e-8); the bound is four times the measured value, and never above 1e-5
ATT_BOUND = min(4 * 9.7e-8, 1e-5)


# ---- fp64 references: plain host functions, one per kernel contract ----------------------------------------------------
def ref_gate_hidden(ig, sg, sc_i, sh_i, sc_s, sh_s, w_a, b_a, h_stored=None):
    """h = ReLU(BN_i(ig) + BN_s(sg)) with the BatchNorms as scale / shift; logit = <h, w_a> + b_a (from ``h_stored`` when
    the storage rounds h); (sum, sum^2) of logit and the sums of the absolute terms."""
    d = torch.float64
    h = torch.relu((ig.to(d) * sc_i.to(d) + sh_i.to(d)) + (sg.to(d) * sc_s.to(d) + sh_s.to(d)))
    hl = h if h_stored is None else h_stored.to(d)
    logit = (hl * w_a.to(d)).sum(1) + (0.0 if b_a is None else b_a.to(d)[0])
    return {"h": h, "logit": logit, "sums": torch.stack([logit.sum(), (logit * logit).sum()]),
            "abs": torch.stack([logit.abs().sum(), (logit * logit).sum()])}


def ref_gate_apply(x, logit, sc_a, sh_a):
    """att = sigmoid(logit * sc + sh), out = x * att."""
    d = torch.float64
    att = torch.sigmoid(logit.to(d) * sc_a.to(d)[0] + sh_a.to(d)[0])
    return {"out": x.to(d) * att[:, None], "att": att}


def ref_gate_apply_bwd(dout, x, att, logit, mean_a, rstd_a, relu_out):
    """dx_skip = dout * att (dout masked by x > 0 when the consumer read ReLU(out)), dl = <dout, x> att (1 - att),
    (sum dl, sum dl * xhat) with xhat = (logit - mean) * rstd."""
    d = torch.float64
    g, xx, a = dout.to(d), x.to(d), att.to(d)
    if relu_out:
        g = torch.where(xx > 0, g, torch.zeros_like(g))
    dl = (g * xx).sum(1) * a * (1 - a)
    xh = (logit.to(d) - mean_a.to(d)[0]) * rstd_a.to(d)[0]
    return {"dx_skip": g * a[:, None], "dl": dl, "sums": torch.stack([dl.sum(), (dl * xh).sum()]),
            "abs": torch.stack([dl.abs().sum(), (dl * xh).abs().sum()])}


def ref_gate_hidden_bwd(dl, logit, h, ig, sg, mean_a, rstd_a, gamma_a, sums_a, w_a, mean_i, rstd_i, mean_s, rstd_s,
                        dsum_stored=None):
    """BatchNorm(1) backward of the logit, d h through w_a and the ReLU mask of h, the increments of dw_a / db_a, and
    the BatchNorm-backward partial sums of BN_i / BN_s (from ``dsum_stored`` when the storage rounds dsum)."""
    d = torch.float64
    M = dl.numel()
    mu, rs = mean_a.to(d)[0], rstd_a.to(d)[0]
    ga = 1.0 if gamma_a is None else gamma_a.to(d)[0]
    xh = (logit.to(d) - mu) * rs
    dlog = ga * rs * (dl.to(d) - sums_a.to(d)[0] / M - xh * sums_a.to(d)[1] / M)
    hh = h.to(d)
    dsum = torch.where(hh > 0, dlog[:, None] * w_a.to(d), torch.zeros_like(hh))
    dd = dsum if dsum_stored is None else dsum_stored.to(d)
    ti = dd * (ig.to(d) - mean_i.to(d)) * rstd_i.to(d)
    ts = dd * (sg.to(d) - mean_s.to(d)) * rstd_s.to(d)
    tw = dlog[:, None] * hh
    return {"dsum": dsum, "dlog": dlog,
            "p0": dd.sum(0), "p0_abs": dd.abs().sum(0), "pi1": ti.sum(0), "pi1_abs": ti.abs().sum(0),
            "ps1": ts.sum(0), "ps1_abs": ts.abs().sum(0), "dw": tw.sum(0), "dw_abs": tw.abs().sum(0),
            "db": dlog.sum(), "db_abs": dlog.abs().sum()}


def _bn_train(z, gamma, beta, eps=1e-5):
    mean, var = z.mean(0), z.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (z - mean) * rstd * gamma + beta, mean, rstd


def ref_gate_core(x, ig_pre, sg_pre, p):
    """The gate behind its two pointwise convolutions, rows [M][C] / [M][K], training-mode BatchNorms, differentiable."""
    ui, _, _ = _bn_train(ig_pre, p["g_i"], p["be_i"])
    us, _, _ = _bn_train(sg_pre, p["g_s"], p["be_s"])
    h = torch.relu(ui + us)
    logit = h @ p["w_a"] + p["b_a"]
    a, _, _ = _bn_train(logit[:, None], p["g_a"], p["be_a"])
    return x * torch.sigmoid(a)


def ref_gate_block(x, signal, p):
    """AttentionBlock.forward as oracle/attention_ref.py states it, on rows."""
    return ref_gate_core(x, x @ p["w_i"].T + p["b_i"], signal @ p["w_s"].T + p["b_s"], p)


def ref_gate_chain(x, ig_pre, sg_pre, dout, p, eps=1e-5):
    """Forward and backward of ref_gate_core composed from the per-kernel references above plus textbook BatchNorm
    finalisation -- the order models' attention executor calls the kernels in.  No autograd."""
    M = x.shape[0]
    one = lambda v: v.reshape(1)
    _, mi, ri = _bn_train(ig_pre, p["g_i"], p["be_i"], eps)
    _, ms, rs_ = _bn_train(sg_pre, p["g_s"], p["be_s"], eps)
    sc_i, sc_s = p["g_i"] * ri, p["g_s"] * rs_
    hid = ref_gate_hidden(ig_pre, sg_pre, sc_i, p["be_i"] - mi * sc_i, sc_s, p["be_s"] - ms * sc_s, p["w_a"], one(p["b_a"]))
    ma = hid["sums"][0] / M
    ra = 1.0 / torch.sqrt(hid["sums"][1] / M - ma * ma + eps)
    sc_a = p["g_a"] * ra
    app = ref_gate_apply(x, hid["logit"], one(sc_a), one(p["be_a"] - ma * sc_a))
    ab = ref_gate_apply_bwd(dout, x, app["att"], hid["logit"], one(ma), one(ra), False)
    hb = ref_gate_hidden_bwd(ab["dl"], hid["logit"], hid["h"], ig_pre, sg_pre, one(ma), one(ra), one(p["g_a"]), ab["sums"],
                             p["w_a"], mi, ri, ms, rs_)
    xi, xs = (ig_pre - mi) * ri, (sg_pre - ms) * rs_
    dig = p["g_i"] * ri * (hb["dsum"] - hb["p0"] / M - xi * hb["pi1"] / M)
    dsg = p["g_s"] * rs_ * (hb["dsum"] - hb["p0"] / M - xs * hb["ps1"] / M)
    return {"out": app["out"], "dx_skip": ab["dx_skip"], "dig": dig, "dsg": dsg, "dw_a": hb["dw"], "db_a": hb["db"],
            "db_a_abs": hb["db_abs"],
            "dg_a": ab["sums"][1], "dbe_a": ab["sums"][0], "dg_i": hb["pi1"], "dbe_i": hb["p0"], "dg_s": hb["ps1"],
            "dbe_s": hb["p0"]}


def _chain_inputs(M, C, K, seed):
    d = torch.float64
    p = {"w_i": rnd((K, C), seed, 0.3), "b_i": rnd((K,), seed + 1, 0.1), "w_s": rnd((K, C), seed + 2, 0.3),
         "b_s": rnd((K,), seed + 3, 0.1), "g_i": 1 + 0.2 * rnd((K,), seed + 4), "be_i": 0.2 * rnd((K,), seed + 5),
         "g_s": 1 + 0.2 * rnd((K,), seed + 6), "be_s": 0.2 * rnd((K,), seed + 7), "w_a": rnd((K,), seed + 8, 0.4),
         "b_a": rnd((1,), seed + 9, 0.3)[0], "g_a": 1 + 0.2 * rnd((1,), seed + 10)[0], "be_a": 0.2 * rnd((1,), seed + 11)[0]}
    p = {k: v.to(d) for k, v in p.items()}
    return rnd((M, C), seed + 20).to(d), rnd((M, C), seed + 21).to(d), rnd((M, C), seed + 22).to(d), p


def _autograd_of(fn, leaves, dout):
    leaves = {k: v.clone().requires_grad_(True) for k, v in leaves.items()}
    out = fn(leaves)
    grads = torch.autograd.grad((out * dout).sum(), list(leaves.values()), allow_unused=True)
    return out.detach(), dict(zip(leaves, grads))


def test_references_compose_to_the_oracle_gate():
    """No GPU: ref_gate_block equals oracle.attention_ref.attention_block (values and every gradient), and the per-kernel
    references composed in the executor's order (ref_gate_chain) equal autograd of it."""
    from oracle.attention_ref import attention_block
    N, H, W, C, K = 2, 3, 5, 16, 8
    M = N * H * W
    x, signal, dout, p = _chain_inputs(M, C, K, 5)
    nchw = lambda t: t.view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, -1)

    def oracle_fn(L):
        st = {}
        for name, w, b, g, be in (("input_gate", "w_i", "b_i", "g_i", "be_i"), ("signal_gate", "w_s", "b_s", "g_s", "be_s")):
            st[f"g.{name}.0.weight"], st[f"g.{name}.0.bias"] = L[w][:, :, None, None], L[b]
            st[f"g.{name}.1.weight"], st[f"g.{name}.1.bias"] = L[g], L[be]
        st["g.attention.0.weight"], st["g.attention.0.bias"] = L["w_a"][None, :, None, None], L["b_a"].reshape(1)
        st["g.attention.1.weight"], st["g.attention.1.bias"] = L["g_a"].reshape(1), L["be_a"].reshape(1)
        for name, n in (("input_gate", K), ("signal_gate", K), ("attention", 1)):
            st[f"g.{name}.1.running_mean"] = torch.zeros(n, dtype=torch.float64)
            st[f"g.{name}.1.running_var"] = torch.ones(n, dtype=torch.float64)
            st[f"g.{name}.1.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
        return rows(attention_block(st, "g", nchw(L["x"]), nchw(L["signal"]), True))

    leaves = dict(p, x=x, signal=signal)
    want, gwant = _autograd_of(oracle_fn, leaves, dout)
    got, ggot = _autograd_of(lambda L: ref_gate_block(L["x"], L["signal"], L), leaves, dout)
    assert max_err(got, want) < 1e-12
    zero = ("b_i", "b_s", "b_a")        # a bias in front of a BatchNorm: analytically zero gradient, cancellation noise
    for k in gwant:
        if k in zero:
            assert float(ggot[k].abs().max()) < 1e-12 and float(gwant[k].abs().max()) < 1e-12, k
        else:
            assert max_err(ggot[k], gwant[k]) < 1e-10, k

    ig_pre, sg_pre = x @ p["w_i"].T + p["b_i"], signal @ p["w_s"].T + p["b_s"]
    core, gcore = _autograd_of(lambda L: ref_gate_core(L["x"], L["ig"], L["sg"], L), dict(p, x=x, ig=ig_pre, sg=sg_pre), dout)
    ch = ref_gate_chain(x, ig_pre, sg_pre, dout, p)
    assert max_err(ch["out"], core) < 1e-12 and max_err(core, want) < 1e-12
    for a, b in (("dx_skip", "x"), ("dig", "ig"), ("dsg", "sg"), ("dw_a", "w_a"), ("dg_a", "g_a"),
                 ("dbe_a", "be_a"), ("dg_i", "g_i"), ("dbe_i", "be_i"), ("dg_s", "g_s"), ("dbe_s", "be_s")):
        assert max_err(ch[a], gcore[b]) < 1e-9, (a, b)
    assert abs(float(ch["db_a"])) < 1e-12 * float(ch["db_a_abs"]) and abs(float(gcore["b_a"])) < 1e-12


# ---- device helpers -------------------------------------------------------------------------------------------------------
def _d(t, dtype=torch.float32):
    return None if t is None else t.to(dev()).to(dtype).contiguous()


def _poisoned(n, dtype=torch.float32):
    """An output buffer of n elements followed by GUARD guard elements, all NaN."""
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev())


def _written(full, n, what):
    """Nothing beyond the n elements was touched, every one of them was written; returns them on the host."""
    assert bool(torch.isnan(full[n:]).all()), f"{what}: wrote past its {n} elements"
    got = full[:n].float().cpu() if full.dtype != torch.float32 else full[:n].cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: elements left unwritten"
    return got


def _elem_ok(got, ref, dtype, what):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    print(f"{what}: max_err {max_err(got, ref):.3g}")
    if dtype == torch.float32:
        assert max_err(got, ref) < 1e-5, what
    else:
        lim = 2.0 ** -8 * ref.abs() + 1e-6 * float(ref.abs().max())
        bad = (got - ref).abs() > lim
        assert not bool(bad.any()), (what, int(bad.sum()), float(((got - ref).abs() - lim).max()))


def _sum_ok(got, ref, abs_terms, what):
    got, ref, abs_terms = got.double().reshape(-1), ref.double().reshape(-1), abs_terms.double().reshape(-1)
    err = (got - ref).abs()
    print(f"{what}: max err / sum|terms| {float((err / abs_terms.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= 1e-5 * abs_terms).all()), (what, float((err - 1e-5 * abs_terms).max()))


def _partial_rows(ops, M, full, width, what):
    """The [rows][2][width] partial buffer of a gate launch over M rows: written exactly, rows of blocks that have no
    row exactly zero.  Returns the host tensor [rows, 2, width]."""
    rows = ops.gate_partial_rows(M)
    assert rows == min(2048, max(1, (M + 63) // 64))
    part = _written(full, rows * 2 * width, what).view(rows, 2, width)
    rpb = (M + rows - 1) // rows
    used = (M + rpb - 1) // rpb
    if used < rows:
        assert bool((part[used:] == 0).all()), f"{what}: empty trailing blocks must write zeros"
    return part


# ---- gate_hidden ----------------------------------------------------------------------------------------------------------
HIDDEN_CASES = [(K, M) for K in (8, 16, 64, 512) for M in (1, 63, 65, 300)] + [(16, BIG_M)]


def _hidden_inputs(K, M, dtype, seed):
    ig, sg = q(rnd((M, K), seed), dtype), q(rnd((M, K), seed + 1) * 0.8 - 0.1, dtype)
    sc_i, sh_i = 1 + 0.2 * rnd((K,), seed + 2), 0.2 * rnd((K,), seed + 3)
    sc_s, sh_s = 0.9 + 0.2 * rnd((K,), seed + 4), 0.2 * rnd((K,), seed + 5)
    w_a = rnd((K,), seed + 6, 0.4)
    return ig, sg, sc_i, sh_i, sc_s, sh_s, w_a


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bias", [True, False], ids=["b_a", "no_b_a"])
@pytest.mark.parametrize("K,M", HIDDEN_CASES, ids=lambda v: str(v))
def test_gate_hidden(pai, K, M, bias, dtype):
    from thesis_pai_reconstruction_amd import ops
    ig, sg, sc_i, sh_i, sc_s, sh_s, w_a = _hidden_inputs(K, M, dtype, 100 + K)
    b_a = torch.tensor([0.3]) if bias else None
    rows = ops.gate_partial_rows(M)
    h = _poisoned(M * K, dtype)
    logit = _poisoned(M)
    part = _poisoned(ops.bn_stats_buffer_rows(rows) * 2)         # as the executor sizes it: scratch rows behind the partials
    ops.gate_hidden(dtype, _d(ig, dtype), _d(sg, dtype), M, K, _d(sc_i), _d(sh_i), _d(sc_s), _d(sh_s), _d(w_a), _d(b_a),
                    h[:M * K], logit[:M], part[:rows * 2])
    torch.cuda.synchronize()
    got_h = _written(h, M * K, "h").view(M, K)
    got_l = _written(logit, M, "logit")
    got_p = _partial_rows(ops, M, part, 1, "partials")
    ref = ref_gate_hidden(ig, sg, sc_i, sh_i, sc_s, sh_s, w_a, b_a, None if dtype == torch.float32 else got_h)
    _elem_ok(got_h, ref["h"], dtype, "h")
    _elem_ok(got_l, ref["logit"], torch.float32, "logit")
    _sum_ok(got_p.double().sum(0).view(2), ref["sums"], ref["abs"], "(sum l, sum l^2)")


# ---- gate_apply -----------------------------------------------------------------------------------------------------------
APPLY_CASES = [(C, M) for C in (16, 64, 512) for M in (1, 65, 300)] + [(16, WRAP_M)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C,M", APPLY_CASES, ids=lambda v: str(v))
def test_gate_apply(pai, C, M, dtype):
    """att goes through __expf: its reference point is the fp64 sigmoid, its floor the error of torch's own fp32 CPU
    sigmoid on the same arguments (printed).  Measured on an MI355X over all cases of this test: max |att - ref| =
    9.7e-8 (floor 9.6e-8); ATT_BOUND is four times that, 3.9e-7.  Logits are planted whose sigmoid argument is +12 and -12."""
    from thesis_pai_reconstruction_amd import ops
    assert M * (C // 8) > 8192 * 256 or M != WRAP_M
    x = q(rnd((M, C), 200 + C), dtype)
    logit = rnd((M,), 201 + C, 2.0)
    sc_a, sh_a = torch.tensor([1.3]), torch.tensor([-0.2])
    if M == 1:
        logit[0] = (-12.0 + 0.2) / 1.3
    else:
        logit[0], logit[M - 1] = (12.0 + 0.2) / 1.3, (-12.0 + 0.2) / 1.3
    out = _poisoned(M * C, dtype)
    att = _poisoned(M)
    ops.gate_apply(dtype, _d(x, dtype), _d(logit), M, C, _d(sc_a), _d(sh_a), out[:M * C], att[:M])
    torch.cuda.synchronize()
    got_out, got_att = _written(out, M * C, "out"), _written(att, M, "att")
    ref = ref_gate_apply(x, logit, sc_a, sh_a)
    err = float((got_att.double() - ref["att"]).abs().max())
    floor = float((torch.sigmoid(logit * sc_a[0] + sh_a[0]).double() - ref["att"]).abs().max())
    print(f"att: max abs err {err:.3g} (torch fp32 sigmoid: {floor:.3g})")
    assert err < ATT_BOUND
    _elem_ok(got_out, ref["out"], dtype, "out")


# ---- gate_apply_bwd -------------------------------------------------------------------------------------------------------
APPLY_BWD_CASES = [(C, M) for C in (8, 64, 512, 1024) for M in (1, 65, 300)] + [(16, BIG_M)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("relu_out", [0, 1], ids=["plain", "relu_out"])
@pytest.mark.parametrize("C,M", APPLY_BWD_CASES, ids=lambda v: str(v))
def test_gate_apply_bwd(pai, C, M, relu_out, dtype):
    from thesis_pai_reconstruction_amd import ops
    x = rnd((M, C), 300 + C)
    x[:, ::5] = 0.0                                   # exact zeros (masked by relu_out like the negatives)
    x[:, 1::5] = -x[:, 1::5].abs() - 0.1
    x, dout = q(x, dtype), q(rnd((M, C), 301 + C), dtype)
    assert bool((x == 0).any()) and bool((x < 0).any())
    att = torch.sigmoid(rnd((M,), 302 + C, 1.5))
    logit = rnd((M,), 303 + C, 2.0)
    mean_a, rstd_a = torch.tensor([0.25]), torch.tensor([0.7])
    rows = ops.gate_partial_rows(M)
    dxs = _poisoned(M * C, dtype)
    dl = _poisoned(M)
    part = _poisoned(rows * 2)
    ops.gate_apply_bwd(dtype, _d(dout, dtype), _d(x, dtype), _d(att), _d(logit), M, C, _d(mean_a), _d(rstd_a), dxs[:M * C],
                       dl[:M], part[:rows * 2], bool(relu_out))
    torch.cuda.synchronize()
    ref = ref_gate_apply_bwd(dout, x, att, logit, mean_a, rstd_a, bool(relu_out))
    _elem_ok(_written(dxs, M * C, "dx_skip"), ref["dx_skip"], dtype, "dx_skip")
    _elem_ok(_written(dl, M, "dl"), ref["dl"], torch.float32, "dl")
    got_p = _partial_rows(ops, M, part, 1, "partials")
    _sum_ok(got_p.double().sum(0).view(2), ref["sums"], ref["abs"], "(sum dl, sum dl xhat)")


# ---- gate_hidden_bwd ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_db,with_gamma", [(True, False), (False, True)], ids=["db_a", "gamma_a"])
@pytest.mark.parametrize("K,M", HIDDEN_CASES, ids=lambda v: str(v))
def test_gate_hidden_bwd(pai, K, M, with_db, with_gamma, dtype):
    from thesis_pai_reconstruction_amd import ops
    s = 400 + K
    h = q(torch.relu(rnd((M, K), s)), dtype)                    # a ReLU output: about half exact zeros
    ig, sg = q(rnd((M, K), s + 1), dtype), q(rnd((M, K), s + 2), dtype)
    dl, logit = rnd((M,), s + 3), rnd((M,), s + 4, 2.0)
    mean_a, rstd_a = torch.tensor([0.25]), torch.tensor([0.7])
    gamma_a = torch.tensor([1.2]) if with_gamma else None
    sums_a = torch.tensor([0.3 * M, -0.2 * M])
    w_a = rnd((K,), s + 5, 0.4)
    mean_i, rstd_i = 0.1 * rnd((K,), s + 6), 0.8 + 0.2 * rnd((K,), s + 7).abs()
    mean_s, rstd_s = 0.1 * rnd((K,), s + 8), 0.8 + 0.2 * rnd((K,), s + 9).abs()
    dw0, db0 = 1e-3 * (1 + rnd((K,), s + 10).abs()), torch.tensor([1e-3])
    rows = ops.gate_partial_rows(M)
    dsum = _poisoned(M * K, dtype)
    part_i, part_s = _poisoned(rows * 2 * K), _poisoned(rows * 2 * K)
    dw = torch.cat([_d(dw0), _poisoned(0)])
    db = torch.cat([_d(db0), _poisoned(0)])
    ops.gate_hidden_bwd(dtype, _d(dl), _d(logit), _d(h, dtype), _d(ig, dtype), _d(sg, dtype), M, K, _d(mean_a), _d(rstd_a),
                        _d(gamma_a), _d(sums_a), _d(w_a), _d(mean_i), _d(rstd_i), _d(mean_s), _d(rstd_s), dsum[:M * K],
                        part_i[:rows * 2 * K], part_s[:rows * 2 * K], dw[:K], db[:1] if with_db else None)
    torch.cuda.synchronize()
    got_d = _written(dsum, M * K, "dsum").view(M, K)
    ref = ref_gate_hidden_bwd(dl, logit, h, ig, sg, mean_a, rstd_a, gamma_a, sums_a, w_a, mean_i, rstd_i, mean_s, rstd_s,
                              None if dtype == torch.float32 else got_d)
    _elem_ok(got_d, ref["dsum"], dtype, "dsum")
    pi, ps = _partial_rows(ops, M, part_i, K, "part_i"), _partial_rows(ops, M, part_s, K, "part_s")
    assert torch.equal(pi[:, 0], ps[:, 0]), "row 0 (sum of dsum) is the same bits in both partial buffers"
    _sum_ok(pi.double().sum(0)[0], ref["p0"], ref["p0_abs"], "part row 0")
    _sum_ok(pi.double().sum(0)[1], ref["pi1"], ref["pi1_abs"], "part_i row 1")
    _sum_ok(ps.double().sum(0)[1], ref["ps1"], ref["ps1_abs"], "part_s row 1")
    got_dw = _written(dw, K, "dw_a")
    _sum_ok(got_dw.double() - dw0.double(), ref["dw"], ref["dw_abs"], "dw_a increment")
    got_db = _written(db, 1, "db_a")
    if with_db:
        _sum_ok(got_db.double() - db0.double(), ref["db"].reshape(1), ref["db_abs"].reshape(1), "db_a increment")
    else:
        assert torch.equal(got_db, db0)


# ---- the four kernels and the BatchNorm finalisation entry points, chained as the executor does ----------------------------
@pytest.mark.gpu
def test_gate_chain_fp32_against_autograd(pai):
    """M = 300 rows, C = 64, K = 32, fp32: forward and backward through gate_hidden -> bn_finalize -> gate_apply and
    gate_apply_bwd -> bn_bwd_finalize -> gate_hidden_bwd -> bn_bwd_finalize x 2 -> bn_bwd_apply x 2, the order of
    AttentionUnetEngine._gate_forward / gate_backward, against fp64 autograd of the gate as oracle/attention_ref.py states it
    (ref_gate_core; test_references_compose_to_the_oracle_gate ties the two).  The two C -> K pointwise convolutions are
    not part of gate.hip: their outputs are computed on the host and their batch statistics handed over as three partial
    rows, as a convolution epilogue would.  Bound: 1e-4 relative, the project's fp32 parity bar for a chain of kernels
    (tests/test_gpu_ops.py::test_batchnorm_forward_backward)."""
    from thesis_pai_reconstruction_amd import ops
    M, C, K, eps = 300, 64, 32, 1e-5
    f32 = torch.float32
    x, signal, dout, p = _chain_inputs(M, C, K, 11)
    # everything the device sees is fp32: the reference starts from those values
    x, dout = x.float().double(), dout.float().double()
    p = {k: v.float().double() for k, v in p.items()}
    ig_pre = (x @ p["w_i"].T + p["b_i"]).float().double()
    sg_pre = (signal @ p["w_s"].T + p["b_s"]).float().double()
    want, g = _autograd_of(lambda L: ref_gate_core(L["x"], L["ig"], L["sg"], L), dict(p, x=x, ig=ig_pre, sg=sg_pre), dout)

    def bn_state(z, gamma, beta, width):
        parts = torch.zeros(3, 2, width, dtype=torch.float64)
        for r, chunk in enumerate(torch.chunk(z.view(M, width), 3, dim=0)):
            parts[r, 0], parts[r, 1] = chunk.sum(0), (chunk * chunk).sum(0)
        stats = torch.zeros(ops.bn_stats_buffer_rows(3) * 2 * width, dtype=f32, device=dev())
        stats[:3 * 2 * width] = parts.float().reshape(-1).to(dev())
        st = {k: torch.empty(width, device=dev()) for k in ("mean", "rstd", "scale", "shift")}
        st["sums"] = torch.empty(2 * width, device=dev())
        ops.bn_finalize(stats, 3, width, M, _d(gamma.reshape(width)), _d(beta.reshape(width)), eps, 0.1, 1, None, None, None,
                        st["mean"], st["rstd"], st["scale"], st["shift"])
        return st

    bi, bs = bn_state(ig_pre, p["g_i"], p["be_i"], K), bn_state(sg_pre, p["g_s"], p["be_s"], K)
    IG, SG, X, DOUT = _d(ig_pre.reshape(-1)), _d(sg_pre.reshape(-1)), _d(x.reshape(-1)), _d(dout.reshape(-1))
    WA, BA, GA, BEA = _d(p["w_a"]), _d(p["b_a"].reshape(1)), _d(p["g_a"].reshape(1)), _d(p["be_a"].reshape(1))
    rows = ops.gate_partial_rows(M)
    h, logit, att, out = (torch.empty(n, device=dev()) for n in (M * K, M, M, M * C))
    stats = torch.empty(ops.bn_stats_buffer_rows(rows) * 2, device=dev())
    ops.gate_hidden(f32, IG, SG, M, K, bi["scale"], bi["shift"], bs["scale"], bs["shift"], WA, BA, h, logit, stats)
    ba = {k: torch.empty(1, device=dev()) for k in ("mean", "rstd", "scale", "shift")}
    ba["sums"] = torch.empty(2, device=dev())
    ops.bn_finalize(stats, rows, 1, M, GA, BEA, eps, 0.1, 1, None, None, None, ba["mean"], ba["rstd"], ba["scale"], ba["shift"])
    ops.gate_apply(f32, X, logit, M, C, ba["scale"], ba["shift"], out, att)

    part, part2 = torch.empty(rows * 2 * K, device=dev()), torch.empty(rows * 2 * K, device=dev())
    dxs, dl, dsum, dig, dsg = (torch.empty(n, device=dev()) for n in (M * C, M, M * K, M * K, M * K))
    acc = {k: torch.zeros(n, device=dev()) for k, n in (("dg_a", 1), ("dbe_a", 1), ("dw_a", K), ("db_a", 1), ("dg_i", K),
                                                        ("dbe_i", K), ("dg_s", K), ("dbe_s", K))}
    ops.gate_apply_bwd(f32, DOUT, X, att, logit, M, C, ba["mean"], ba["rstd"], dxs, dl, part, False)
    ops.bn_bwd_finalize(part, rows, 1, ba["sums"], acc["dg_a"], acc["dbe_a"])
    ops.gate_hidden_bwd(f32, dl, logit, h, IG, SG, M, K, ba["mean"], ba["rstd"], GA, ba["sums"], WA, bi["mean"], bi["rstd"],
                        bs["mean"], bs["rstd"], dsum, part, part2, acc["dw_a"], acc["db_a"])
    ops.bn_bwd_finalize(part, rows, K, bi["sums"], acc["dg_i"], acc["dbe_i"])
    ops.bn_bwd_finalize(part2, rows, K, bs["sums"], acc["dg_s"], acc["dbe_s"])
    ops.bn_bwd_apply(f32, dsum, IG, M, K, bi["mean"], bi["rstd"], _d(p["g_i"]), bi["sums"], dig)
    ops.bn_bwd_apply(f32, dsum, SG, M, K, bs["mean"], bs["rstd"], _d(p["g_s"]), bs["sums"], dsg)
    torch.cuda.synchronize()

    got = dict(acc, out=out, dx_skip=dxs, dig=dig, dsg=dsg)
    refs = {"out": want, "dx_skip": g["x"], "dig": g["ig"], "dsg": g["sg"], "dw_a": g["w_a"],
            "dg_a": g["g_a"], "dbe_a": g["be_a"], "dg_i": g["g_i"], "dbe_i": g["be_i"], "dg_s": g["g_s"], "dbe_s": g["be_s"]}
    for k, r in refs.items():
        e = rel_err(got[k].cpu().reshape(-1), r.reshape(-1))
        print(f"chain {k}: rel_err {e:.3g}")
        assert e < 1e-4, k
    # d b_a is analytically zero (a bias in front of BN_a): held against the size of its terms
    db_abs = float(ref_gate_chain(x, ig_pre, sg_pre, dout, p)["db_a_abs"])
    print(f"chain db_a: {float(acc['db_a']):.3g} (autograd {float(g['b_a']):.3g}, sum |terms| {db_abs:.3g})")
    assert abs(float(acc["db_a"]) - float(g["b_a"])) <= 1e-4 * db_abs
