"""fp64 host references of the spatial attention of the Palette levels (QKVAttentionLegacy, reference
models/guided_diffusion/unet.py:265-297) and its backward as pai_sattn_bwd defines it: on the tensors it is handed.

Layouts (include/pai_hip.h): qkv [N][T][heads][q | k | v][ch], out / dout [N][T][heads * ch], lse / delta [N][heads][T].
Everything here is double precision; tests/test_sattn_ref_host.py ties it to the fixture of the reference's own autograd and to
torch's double autograd.
"""
import math

import torch


def _f(t):
    return t.detach().double().cpu()


def split_qkv(qkv, heads, ch):
    """qkv [N, T, heads * 3 * ch] -> q, k, v [N, heads, T, ch] (fp64)."""
    n, t, _ = qkv.shape
    x = _f(qkv).view(n, t, heads, 3, ch).permute(3, 0, 2, 1, 4)
    return x[0], x[1], x[2]


def _heads(x, heads, ch):
    """[N, T, heads * ch] -> [N, heads, T, ch] (fp64)."""
    n, t, _ = x.shape
    return _f(x).view(n, t, heads, ch).permute(0, 2, 1, 3)


def _rows(x):
    """[N, heads, T, ch] -> [N, T, heads, ch]."""
    return x.permute(0, 2, 1, 3)


def scores(qkv, heads, ch):
    """scale2 q.k [N, heads, T, T], scale2 = ch ** -0.5."""
    q, k, _ = split_qkv(qkv, heads, ch)
    return torch.einsum("nhic,nhjc->nhij", q, k) / math.sqrt(ch)


def forward(qkv, heads, ch):
    """out [N, T, heads * ch] and lse [N, heads, T], exact fp64."""
    n, t, _ = qkv.shape
    s = scores(qkv, heads, ch)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    v = split_qkv(qkv, heads, ch)[2]
    out = _rows(torch.einsum("nhij,nhjc->nhic", p, v)).reshape(n, t, heads * ch)
    return out, lse


def score_abs_max(qkv, heads, ch):
    """max_ij sum_d |q_id k_jd| over the whole tensor: the factor of e_s = ch u scale2 max_ij sum_d |q_id k_jd|."""
    q, k, _ = split_qkv(qkv, heads, ch)
    return float(torch.einsum("nhic,nhjc->nhij", q.abs(), k.abs()).max())


def backward(dout, qkv, out, lse, heads, ch):
    """The formulas of pai_sattn_bwd from exactly these tensors:
        P_ij = exp(scale2 s_ij - lse_i), dP_ij = dO_i . V_j, delta_i = sum_c dO_ic O_ic, dS_ij = P_ij (dP_ij - delta_i),
        dV_j = sum_i P_ij dO_i, dK_j = scale2 sum_i dS_ij Q_i, dQ_i = scale2 sum_j dS_ij K_j.
    Returns a dict, gradients packed like qkv [N, T, heads * 3 * ch]:
        dqkv     the gradient
        abs      A: the fp64 sum of the absolute terms of every element (dQ: scale2 sum_j |dS_ij| |K_jd|, dK: scale2 sum_i
                 |dS_ij| |Q_id|, dV: sum_i P_ij |dO_id|), as in the docstring of tests/test_gpu_vit_ops.py
        cancel   C: what the subtraction dP - delta can lose, C_ij = P_ij (sum_c |dO_ic V_jc| + sum_c |dO_ic O_ic|), carried
                 through the dQ / dK products like A (zero for dV)
        delta, delta_abs   [N, heads, T]: delta_i and sum_c |dO_ic O_ic|
        p        P [N, heads, T, T]"""
    n, t, _ = qkv.shape
    q, k, v = split_qkv(qkv, heads, ch)
    do, o = _heads(dout, heads, ch), _heads(out, heads, ch)
    scale2 = 1.0 / math.sqrt(ch)
    p = torch.exp(torch.einsum("nhic,nhjc->nhij", q, k) * scale2 - _f(lse)[..., None])
    dp = torch.einsum("nhic,nhjc->nhij", do, v)
    delta = (do * o).sum(-1)
    delta_abs = (do * o).abs().sum(-1)
    ds = p * (dp - delta[..., None])
    parts = [scale2 * torch.einsum("nhij,nhjc->nhic", ds, k), scale2 * torch.einsum("nhij,nhic->nhjc", ds, q),
             torch.einsum("nhij,nhic->nhjc", p, do)]
    absum = [scale2 * torch.einsum("nhij,nhjc->nhic", ds.abs(), k.abs()),
             scale2 * torch.einsum("nhij,nhic->nhjc", ds.abs(), q.abs()),
             torch.einsum("nhij,nhic->nhjc", p, do.abs())]
    c = p * (torch.einsum("nhic,nhjc->nhij", do.abs(), v.abs()) + delta_abs[..., None])
    cancel = [scale2 * torch.einsum("nhij,nhjc->nhic", c, k.abs()), scale2 * torch.einsum("nhij,nhic->nhjc", c, q.abs()),
              torch.zeros_like(parts[2])]
    pack = lambda ts: torch.stack([_rows(x) for x in ts], dim=3).reshape(n, t, heads * 3 * ch)
    return {"dqkv": pack(parts), "abs": pack(absum), "cancel": pack(cancel), "delta": delta, "delta_abs": delta_abs, "p": p}


# ---- exact integer data for the lane maps (the construction of test_mha_lane_maps in this layout) ----------------------------
def lane_map_data(N, T, heads, ch, paired):
    """Small-integer q, k, v, dO, every value and every intermediate of the five products exact in bf16 / fp32.
    Key j carries 16 on the two channels c(j) (lower half of the head) and b(j) (upper half), a different pair for every key,
    and query i carries 16 on the two channels of key sigma(i) = (7 i + 2) % T: the matching score is 512 / sqrt(ch) >= 64
    and a key that shares one of the two channels scores half of it (T may exceed ch, so one channel cannot tell the keys
    apart).
    onehot: every query copies ONE row of the asymmetric v, dV_j is ONE row of the asymmetric dO; dS vanishes.
    paired: keys 2 m and 2 m + 1 share both channels and differ in a channel no query looks at, so P = 1/2, 1/2 and
    dS = -+ 1/2 (dP difference) for the pair: dQ = dS K and dK = dS^T Q are whole multiples of 16 scale2 / 2."""
    half = ch // 2
    unit = 2 if paired else 1
    groups = (T + unit - 1) // unit                 # distinct (c, b) addresses needed
    lo_n = half - 2 if paired else half             # paired: the two top channels of the lower half stay free for the tags
    assert groups <= lo_n * half, "not enough (c, b) pairs"
    sigma = lambda i: (7 * i + 2) % T
    assert math.gcd(7, T) == 1 and ch + 2 * 95 + N * heads <= 257
    mult = next(m for m in (5, 7, 11, 13) if math.gcd(m, lo_n) == 1)
    grp = lambda j: j // unit
    cj = lambda j: (mult * grp(j) + 3) % lo_n
    bj = lambda j: half + (grp(j) // lo_n) % half
    assert len({(cj(j), bj(j)) for j in range(T)}) == groups
    qkv = torch.zeros(N, T, heads, 3, ch)
    dout = torch.zeros(N, T, heads, ch)
    d = torch.arange(ch, dtype=torch.float32)
    for n in range(N):
        for h in range(heads):
            for i in range(T):
                s = sigma(i)
                qkv[n, i, h, 0, cj(s)] = 16.0
                qkv[n, i, h, 0, bj(s)] = 16.0
                qkv[n, i, h, 1, cj(i)] = 16.0
                qkv[n, i, h, 1, bj(i)] = 16.0
                if paired:                          # a tag channel no query looks at: 16, 32, 48 by key
                    qkv[n, i, h, 1, half - 2 + (i // 2) % 2] = 16.0 * (i % 3 + 1)
                qkv[n, i, h, 2] = d + 2 * (i % 96) + (n * heads + h)     # at most 256: exact in bf16
                dout[n, i, h] = ((2 * i + 3 * d + n + 2 * h) % 7) - 3
                dout[n, i, h, i % ch] += (i % 4) + 1
    return qkv.reshape(N, T, heads * 3 * ch), dout.reshape(N, T, heads * ch)
