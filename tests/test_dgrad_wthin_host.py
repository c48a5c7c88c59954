"""CPU: the host side of pai_conv_dgrad_act_wthin -- ABI number, exports, the predicate's refusals, the selection's name
and slab bytes, and the argument checks of the ops wrapper.  Nothing here launches a kernel."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pai_hip.h")
BF = torch.bfloat16
NAMES = ("pai_conv_dgrad_act_wthin", "pai_conv_dgrad_act_wthin_ok", "pai_conv_dgrad_act_wthin_slab_bytes",
         "pai_conv_dgrad_act_wthin_kernel_name")


def _pair(ops, N=4, H=64, W=64, T=2, dtype=BF, c_mid=64, stride1=2, stride0=2):
    """(descriptor of the layer behind, descriptor of the thin layer) for H x W images."""
    d1 = ops.make_desc(dtype, 0, N, H // 2, W // 2, c_mid, 0, 128, stride1, 0, 0, ops.ACT_LRELU)
    d0 = ops.make_desc(dtype, 0, N, H, W, 1, T - 1, c_mid, stride0, 0, 0, ops.ACT_LRELU)
    return d1, d0


def test_abi_number_exports_and_header(pai):
    """The entry points are additions under the number the library already reported (tests pinned to 141 stay as they
    are): the history in front of pai_version() still ends at the reported number and names the additions."""
    lib = pai.lib.load()
    src = open(HEADER).read()
    block = src[src.index("/* 100: round 1."):src.index("int pai_version(void);")]
    listed = [int(n) for n in re.findall(r"(?m)^(?:/\*| \*) (\d{3}):", block)]
    assert listed[-1] == lib.pai_version() >= 141, listed
    assert "pai_conv_dgrad_act_wthin" in block[block.index(" * %d:" % listed[-1]):]
    for name in NAMES:
        assert hasattr(lib, name) and name in pai.lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, src), name


def test_predicate_takes_the_two_first_layer_pairs(pai):
    from thesis_pai_reconstruction_amd import ops
    for N, T in ((128, 2), (64, 1)):                 # D block 1 -> block 0 at 2N images; encoders[1] -> encoders[0]
        d1, d0 = _pair(ops, N, 256, 256, T)
        assert ops.conv_dgrad_act_wthin_ok(d1, d0)
        assert ops.conv_dgrad_act_wthin_kernel_name(d1, d0) == "gg_dgrad_wthin_k<%d>" % T
        assert ops.conv_kernel_name(d1, 1) == "gg_fwd_patch_k<128, 64, false>"     # the plain input gradient keeps its kernel
        assert ops.conv_dgrad_act_wthin_slab_bytes(d1, d0) == 128 * (16 * T + 1) * 64 * 4
    d1, d0 = _pair(ops, 2, 32, 64, 2)                 # one 8 x 16 tile per image and phase: the smallest problem
    assert ops.conv_dgrad_act_wthin_ok(d1, d0)
    ops.set_tunable("wthin_slabs", 7)
    try:
        assert ops.conv_dgrad_act_wthin_slab_bytes(d1, d0) == 7 * 33 * 64 * 4
    finally:
        ops.set_tunable("wthin_slabs")


def test_predicate_refusals(pai):
    from thesis_pai_reconstruction_amd import ops
    ok = ops.conv_dgrad_act_wthin_ok
    d1, d0 = _pair(ops)
    assert ok(d1, d0) and ok(d1, d0, need_dx=False)
    assert not ok(d1, d0, need_dx=True)                                  # the G-phase pass through D: du[0] has a second reader
    assert not ok(*_pair(ops, c_mid=128))                                # thin layer with Cout != 64
    assert not ok(*_pair(ops, c_mid=32))
    assert not ok(*_pair(ops, stride1=1)) and not ok(*_pair(ops, stride0=1))      # stride != 2 on either layer
    assert not ok(*_pair(ops, dtype=torch.float32))
    assert not ok(*_pair(ops, H=32, W=32))                               # 8 x 8 pixels per phase: no 8 x 16 patch tile
    assert not ok(d1, _pair(ops, N=2)[1])                                # another batch
    assert not ok(d1, _pair(ops, H=128, W=128)[1])                       # the thin layer's output is not d1's input
    assert not ok(ops.make_desc(BF, 0, 4, 32, 32, 32, 32, 128, 2), d0)   # two source tensors
    assert not ok(ops.make_desc(BF, 1, 4, 32, 32, 64, 0, 128, 2), d0)    # a transposed convolution
    three = ops.make_desc(BF, 0, 4, 64, 64, 3, 0, 64, 2)
    assert not ok(d1, three)                                             # not a (1 | 1)-channel first layer
    ops.set_tunable("dgrad_wthin", 0)
    try:
        assert not ok(d1, d0)
    finally:
        ops.set_tunable("dgrad_wthin")
    ops.set_tunable("fwd_patch", 0)                                      # the input gradient on the tile kernels: no such store
    try:
        assert not ok(d1, d0)
    finally:
        ops.set_tunable("fwd_patch")
    assert ok(d1, d0)
    bad = _pair(ops, c_mid=128)
    with pytest.raises(ops.PaiError):
        ops.conv_dgrad_act_wthin_slab_bytes(*bad)
    with pytest.raises(ops.PaiError):
        ops.conv_dgrad_act_wthin_kernel_name(*bad)


def test_call_refuses_before_it_touches_a_pointer(pai):
    """The C entry point answers a pair the predicate refuses, a null pointer and a slab buffer without room with an error
    code and a message; the pointers here are never dereferenced."""
    from thesis_pai_reconstruction_amd import ops
    lib = pai.lib.load()
    fake = ctypes.c_void_p(0x10000)
    d1, d0 = _pair(ops)

    def call(d1, d0, x2=fake, slabs=fake, slab_bytes=1 << 20, dy=fake, overwrite=0):
        return lib.pai_conv_dgrad_act_wthin(ctypes.byref(d1), dy, fake, fake, ops.ACT_LRELU, None, ops.ACT_NONE,
                                            ctypes.byref(d0), fake, x2, fake, fake, overwrite, slabs, slab_bytes, None)
    assert call(*_pair(ops, c_mid=128)) != 0 and b"pai_conv_dgrad_act_wthin_ok" in lib.pai_last_error()
    assert call(d1, d0, dy=None) != 0 and b"null" in lib.pai_last_error()
    assert call(d1, d0, x2=None) != 0 and b"x2" in lib.pai_last_error()
    assert call(d1, d0, x2=ctypes.c_void_p(0x10008)) != 0 and b"16-B" in lib.pai_last_error()
    assert call(d1, d0, overwrite=3) != 0 and b"overwrite" in lib.pai_last_error()
    assert call(d1, d0, slab_bytes=100) != 0 and b"slab" in lib.pai_last_error()


def test_ops_argument_checks(pai):
    from thesis_pai_reconstruction_amd import ops
    d1, d0 = _pair(ops, N=2, H=32, W=64, T=2)
    bf = lambda n: torch.zeros(n, dtype=BF)
    f32 = lambda n: torch.zeros(n)
    dy, wd, a1 = bf(2 * 128 * 8 * 16), bf(128 * 16 * 64), bf(2 * 64 * 16 * 32)
    x1, x2 = bf(2 * 32 * 64), bf(2 * 32 * 64)
    dw, db, slabs = f32(64 * 16 * 2), f32(64), f32(33 * 64 * 4)
    args = lambda **kw: {**dict(d=d1, dy=dy, w_dgrad=wd, a1=a1, act1=ops.ACT_LRELU, add=None, act2=ops.ACT_NONE, d_thin=d0,
                                x1=x1, x2=x2, dw=dw, dbias=db, slabs=slabs), **kw}
    with pytest.raises(ops.PaiError, match="HIP device"):                 # no CPU path
        ops.conv_dgrad_act_wthin(**args())
    with pytest.raises(ops.PaiError, match="descriptors"):
        ops.conv_dgrad_act_wthin(**args(d_thin=None))
    with pytest.raises(ops.PaiError, match="slabs"):
        ops.conv_dgrad_act_wthin(**args(slabs=None))
    with pytest.raises(ops.PaiError, match="slabs"):
        ops.conv_dgrad_act_wthin(**args(slabs=bf(64)))
    with pytest.raises(ops.PaiError, match="x2"):
        ops.conv_dgrad_act_wthin(**args(x2=None))
    with pytest.raises(ops.PaiError, match="x2"):
        ops.conv_dgrad_act_wthin(**args(d_thin=_pair(ops, N=2, H=32, W=64, T=1)[1]))
    with pytest.raises(ops.PaiError, match="shape"):
        ops.conv_dgrad_act_wthin(**args(dw=f32(64 * 16)))
    with pytest.raises(ops.PaiError, match="shape"):
        ops.conv_dgrad_act_wthin(**args(dbias=f32(32)))
