"""Host checks of the block references (tests/_block_ref.py): the emulator without rounding IS the block, the rounding
Function does what it says, the three yardsticks the GPU tests compute again are finite and ordered, and the exclusion
list is what the container layout says.  No GPU."""
import pytest
import torch

import _block_ref as br

# (kind, source channels, output channels): both skip kinds of every block kind that has two
CASES = [("18", (64,), 64), ("18", (64,), 128), ("18", (64, 64), 64),
         ("50", (64,), 64), ("50", (128,), 256), ("50", (64, 64), 64),
         ("next", (64,), 128), ("next", (128,), 128), ("next", (64, 64), 128), ("next", (128, 64), 64),
         ("v2", (64,), 64), ("v2", (64,), 128), ("v2", (64, 64), 128),
         ("tenc", (64,), 128), ("tenc", (128,), 128),
         ("tdec", (64, 64), 64)]


def _case(pai, kind, cins, cout, shape, seed=11, rounded=True):
    torch.manual_seed(seed)
    block = br.init_block(br.make_block(kind, sum(cins), cout), seed, round_weights=rounded)
    n, h, w = shape
    xs, g = br.make_io(seed + 1, n, h, w, cins, cout, br.out_hw(kind, h, w), rounded)
    containers, layout = br.describe(block)
    return containers, layout, (xs[0] if len(xs) == 1 else tuple(xs)), g


@pytest.mark.parametrize("kind,cins,cout", CASES, ids=[f"{k}-{'+'.join(map(str, c))}-{o}" for k, c, o in CASES])
def test_emulator_without_rounding_is_the_block(pai, kind, cins, cout):
    """Every formula the emulator writes out by hand (BatchNorm backward from saved statistics, the fork sums, the strided
    forms, the tails) against autograd on the stock containers: fp64 noise."""
    containers, layout, x, g = _case(pai, kind, cins, cout, (2, 6, 10), rounded=False)
    want = br.ref_block(containers, layout, x, g)
    skip = br.bias_before_bn(containers)
    for fused_tail in (True, False):
        for dgrad_bn in (True, False):
            got = br.emu_block(containers, layout, x, g, dict(br.EXACT, fused_tail=fused_tail, dgrad_bn=dgrad_bn))
            for k, (l2, mx) in br.distances(got, want, skip).items():
                assert l2 <= 1e-12 and mx <= 1e-12, (k, l2, mx)
            assert got["running"].keys() == want["running"].keys()
            for k, v in want["running"].items():
                assert br.rel_l2(got["running"][k], v) <= 1e-12, k
            for k in skip:      # noise in both: absolute, against the block's largest gradient
                top = max(float(v.abs().max()) for v in want["grads"].values())
                assert float(got["grads"][k].abs().max()) <= 1e-9 * top


def test_rounding_function():
    torch.manual_seed(0)
    t = torch.randn(1000, dtype=torch.float64, requires_grad=True)
    r = br.RoundST.apply(t)
    assert torch.equal(r, t.detach().bfloat16().double())
    assert torch.equal(br.RoundST.apply(r), r)                  # idempotent
    g = torch.randn(1000, dtype=torch.float64)
    r.backward(g)
    assert torch.equal(t.grad, g.bfloat16().double())           # the backward rounds
    assert not torch.equal(t.grad, g)
    t2 = t.detach().clone().requires_grad_(True)
    y = br.RoundGrad.apply(t2)
    assert torch.equal(y, t2)
    y.backward(g)
    assert torch.equal(t2.grad, g.bfloat16().double())


def test_fused_dgrad_store_moves_no_bit_for_relu(pai):
    """du = relu' * dgrad stored in bf16 (fused pai_conv_dgrad_bn) against relu' * bf16(dgrad) (two passes): the same bits."""
    containers, layout, x, g = _case(pai, "next", (64,), 128, (2, 6, 10))
    a = br.emu_block(containers, layout, x, g, br.path_flags(dgrad_bn=True))
    b = br.emu_block(containers, layout, x, g, br.path_flags(dgrad_bn=False))
    for k, (l2, _) in br.distances(a, b).items():
        assert l2 == 0.0, (k, l2)


YARD = [("18", (64,), 128, (3, 12, 20)), ("18", (64,), 128, (1, 72, 64)), ("next", (64,), 128, (3, 12, 20)),
        ("next", (64,), 128, (1, 72, 64)), ("next", (64,), 128, (1, 128, 128)), ("50", (64,), 64, (1, 128, 128)),
        ("v2", (64,), 128, (3, 12, 20)), ("tenc", (64,), 128, (3, 12, 20)), ("tdec", (64, 64), 64, (3, 12, 20))]


@pytest.mark.parametrize("kind,cins,cout,shape", YARD, ids=[f"{k}-{s[0]}x{s[1]}x{s[2]}" for k, _, _, s in YARD])
def test_yardsticks_are_finite_and_ordered(pai, kind, cins, cout, shape):
    """The three distances the GPU tests are built on, from the references alone (largest relative L2 over the tensors):
    arithmetic spread (emulator in fp32 against fp64) < statistics-source spread (statistics of the stored z against
    those of the unrounded accumulators) < distance of the emulator from the exact fp64 block."""
    containers, layout, x, g = _case(pai, kind, cins, cout, shape)
    skip = br.bias_before_bn(containers)
    ref = br.ref_block(containers, layout, x, g)
    e64 = br.emu_block(containers, layout, x, g, br.path_flags())
    e32 = br.emu_block(containers, layout, x, g, br.path_flags(), dtype=torch.float32)
    stored = br.emu_block(containers, layout, x, g, dict(br.path_flags(), stats_of_stored=True))
    arith = max(v[0] for v in br.distances(e32, e64, skip).values())
    stats = max(v[0] for v in br.distances(stored, e64, skip).values())
    dist = max(v[0] for v in br.distances(e64, ref, skip).values())
    fwd = br.distances(e64, ref, skip)["out"][0]
    print(f"\n{kind} {cins}->{cout} at {shape}: arithmetic {arith:.3e}  statistics source {stats:.3e}  "
          f"from fp64 {dist:.3e} (forward {fwd:.3e})")
    for v in (arith, stats, dist, fwd):
        assert v == v and v < float("inf")
    assert 0 < arith < dist
    if kind != "v2":        # (the pre-activation block has no convolution epilogue in front of a BatchNorm: nothing moves)
        assert arith < stats < dist
    else:
        assert stats == 0.0


EXCLUDED = {"18": ["conv_block.0.bias", "conv_block.3.bias", "conv_skip.0.bias"],
            "50": ["conv_block.0.bias", "conv_block.3.bias", "conv_block.6.bias", "conv_skip.0.bias"],
            "next": ["conv_block.0.bias", "conv_block.3.bias", "conv_block.6.bias", "conv_skip.0.bias"],
            "v2": ["conv_block.2.bias"],        # the first convolution feeds conv_block.3, a BatchNorm; the other two feed the sum
            "tenc": [],         # bias=False throughout
            "tdec": ["decode.0.bias", "decode.3.bias"]}


@pytest.mark.parametrize("kind,cins,cout", [("18", (64,), 128), ("50", (128,), 256), ("next", (64,), 128), ("v2", (64,), 128),
                                            ("tenc", (64,), 128), ("tdec", (64, 64), 64), ("next", (128,), 128)],
                         ids=["18", "50", "next", "v2", "tenc", "tdec", "next-ident"])
def test_exclusion_list_by_name(pai, kind, cins, cout):
    """Conv biases directly in front of a BatchNorm, from the container layout -- and in the fp64 reference exactly those
    parameter gradients are cancellation noise (below 1e-9 of the block's largest gradient), nothing else."""
    containers, layout, x, g = _case(pai, kind, cins, cout, (3, 12, 20))
    want = [k for k in EXCLUDED[kind] if not (k.startswith("conv_skip") and sum(cins) == cout)]
    assert br.bias_before_bn(containers) == sorted(want)
    ref = br.ref_block(containers, layout, x, g)
    assert br.negligible_by_rule(ref) == sorted(want)
