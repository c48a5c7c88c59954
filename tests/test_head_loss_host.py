"""CPU: the library built for gfx950 exports pai_head_loss with a head_loss_k code object, and its eligibility predicate
(host logic, asked as the *_kernel_name queries are) takes the bf16 bias-free C -> 1 k4 s1 p1 head up to the LDS bound only."""
import torch


def test_library_exports_head_loss_for_gfx950(pai):
    lib = pai.lib.load()
    for name in ("pai_head_loss", "pai_head_loss_ok", "pai_conv_dgrad_f32add", "pai_conv_dgrad_f32add_ok"):
        assert hasattr(lib, name) and name in pai.lib.SIGNATURES, name
    assert lib.pai_version() >= 140
    blob = open(pai.lib.load()._name, "rb").read()
    assert b"head_loss_k" in blob and b"gfx950" in blob


def test_head_loss_predicate(pai):
    from thesis_pai_reconstruction_amd import ops
    bf, f32 = torch.bfloat16, torch.float32
    head = lambda dtype=bf, h=16, w=16, c=512, cout=1, **kw: ops.make_desc(dtype, 0, 4, h, w, c, 0, cout, 1, 0, 0, ops.ACT_NONE, **kw)
    assert ops.head_loss_ok(head())                              # the benchmark's 16 x 16 pixels at 512 channels
    assert ops.head_loss_ok(head(h=32, w=32))                    # 89 KB of the 96 KB asked for
    assert ops.head_loss_ok(head(h=2, w=2)) and ops.head_loss_ok(head(h=3, w=4, c=64))
    assert not ops.head_loss_ok(head(dtype=f32))                 # fp32 storage
    assert not ops.head_loss_ok(head(), has_bias=True)           # a bias
    assert not ops.head_loss_ok(head(cout=2)) and not ops.head_loss_ok(head(cout=64))
    assert not ops.head_loss_ok(head(h=48, w=48))                # 2304 pixels: 157 KB of tap values
    assert not ops.head_loss_ok(head(h=32, w=40))                # just above the bound
    assert not ops.head_loss_ok(head(c=96)) and not ops.head_loss_ok(head(c=48))     # C / 32 no power of two
    assert not ops.head_loss_ok(ops.make_desc(bf, 0, 4, 16, 16, 512, 0, 1, 2))       # stride 2
    assert not ops.head_loss_ok(ops.make_desc(bf, 0, 4, 16, 16, 512, 0, 1, 1, 1))    # ReLU on load
    assert not ops.head_loss_ok(ops.make_desc(bf, 0, 4, 16, 16, 512, 0, 1, 1, 0, 0, ops.ACT_NONE, kernel=3))
    ops.set_tunable("head_fused", 0)
    try:
        assert not ops.head_loss_ok(head())
    finally:
        ops.set_tunable("head_fused")
    assert ops.head_loss_ok(head())


def test_f32add_predicate(pai):
    from thesis_pai_reconstruction_amd import ops
    bf = torch.bfloat16
    d0 = lambda dtype=bf, h=256, c=1: ops.make_desc(dtype, 0, 4, h, h, c, c, 64, 2, 0, 0, ops.ACT_LRELU)
    assert ops.conv_dgrad_f32add_ok(d0()) and ops.conv_dgrad_f32add_ok(d0(h=32))
    assert not ops.conv_dgrad_f32add_ok(d0(dtype=torch.float32))
    assert not ops.conv_dgrad_f32add_ok(d0(h=48))                # thin_up_k works on 16 x 16 source tiles
    assert not ops.conv_dgrad_f32add_ok(d0(c=3))
    assert not ops.conv_dgrad_f32add_ok(ops.make_desc(bf, 0, 4, 64, 64, 64, 0, 128, 2))
