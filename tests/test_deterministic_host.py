"""CPU: the host side of the deterministic mode -- the tunable, the order-free query over the weight-gradient launches of
the BASELINE step and of the Palette defaults, workspace sizes that never shrink under the mode, the launch counter, and
header / bindings / exports.  Nothing here launches a kernel; no query needs a device (without one no workspace is
registered, which is what makes the default-mode answers the un-slabbed ones)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pai_hip.h")
BF, F32 = torch.bfloat16, torch.float32
NAMES = ("pai_conv_wgrad_order_free", "pai_conv_dgrad_act_wthin_order_free", "pai_order_dependent_launches",
         "pai_get_tunable", "pai_colsum_scratch_bytes", "pai_gate_scratch_bytes")


@pytest.fixture
def mode(pai):
    """set(flag) switches the mode; whatever the test leaves, the built-in default comes back."""
    from thesis_pai_reconstruction_amd import ops
    yield pai.set_deterministic
    ops.set_tunable("deterministic")


def baseline_descs(ops, dtype=BF, N=64, size=256):
    """(name, descriptor, has a bias gradient) of every weight-gradient launch of BASELINE configs[1]: the generator
    (channel_mults 1,2,4,8,8,8,8,8; a conv bias in front of a BatchNorm gets no gradient pass) and the PatchGAN
    discriminator at N and at 2N images (real and generated halves in one batch)."""
    enc_c = [64 * m for m in (1, 2, 4, 8, 8, 8, 8, 8)]
    dec_c = [512, 512, 512, 512, 256, 128, 64, 1]
    L = len(enc_c)
    out = []
    cin = 1
    for i in range(L):
        out.append((f"encoders[{i}]", ops.make_desc(dtype, 0, N, size >> i, size >> i, cin, 0, enc_c[i], 2, 0, 0,
                                                    ops.ACT_LRELU if i == 0 else ops.ACT_NONE), i in (0, L - 1)))
        cin = enc_c[i]
    for j in range(L):
        h = size >> (L - j)
        c1, c2, r1, r2 = (enc_c[L - 1], 0, 1, 0) if j == 0 else (dec_c[j - 1], enc_c[L - 1 - j], 0, 1)
        act = ops.ACT_NONE
        if j == L - 1:
            r1, r2, act = 0, 0, ops.ACT_TANH
        out.append((f"decoders[{j}]", ops.make_desc(dtype, 1, N, h, h, c1, c2, dec_c[j], 2, r1, r2, act), j == L - 1))
    chans = [64, 128, 256, 512]
    for n in (N, 2 * N):
        out.append((f"D block 0 x{n}", ops.make_desc(dtype, 0, n, size, size, 1, 1, chans[0], 2, 0, 0, ops.ACT_LRELU), True))
        for k in range(1, 4):
            out.append((f"D block {k} x{n}", ops.make_desc(dtype, 0, n, size >> k, size >> k, chans[k - 1], 0, chans[k], 2,
                                                         0, 0, ops.ACT_LRELU), False))
        out.append((f"D head x{n}", ops.make_desc(dtype, 0, n, size >> 4, size >> 4, chans[3], 0, 1, 1, 0, 0, ops.ACT_NONE),
                    True))
    return out


def palette_descs(pai, ops, dtype, N=2, size=256):
    """Every Conv2d of the class-default Palette U-Net at every resolution the network has (a superset of the launches: the
    module list says which layers exist, not where), plus its nn.Linear layers as the pointwise rows nnops runs them as."""
    net = pai.Palette(in_channels=1, out_channels=1).unet
    convs = {(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0]) for m in net.modules()
             if isinstance(m, torch.nn.Conv2d)}
    lins = {(m.in_features, m.out_features) for m in net.modules() if isinstance(m, torch.nn.Linear)}
    assert convs and all(k in (1, 3) for _, _, k, _ in convs), convs
    out = []
    for cin, cout, k, _ in sorted(convs):
        for lvl in range(6):
            h = size >> lvl
            out.append((f"conv{k} {cin}->{cout} @{h}", ops.make_desc(dtype, 0, N, h, h, cin, 0, cout, 1, 0, 0, ops.ACT_NONE,
                                                                    kernel=k), True))
    for fin, fout in sorted(lins):
        out.append((f"linear {fin}->{fout}", ops.make_desc(dtype, 0, 1, 1, N, fin, 0, fout, 1, 0, 0, ops.ACT_NONE, kernel=1),
                    True))
    return out


def test_abi_number_exports_and_header(pai):
    """Additions under the number the library already reports: the history still ends there and names them; header,
    ctypes table and exports agree on every new entry point."""
    lib = pai.lib.load()
    src = open(HEADER).read()
    block = src[src.index("/* 100: round 1."):src.index("int pai_version(void);")]
    listed = [int(n) for n in re.findall(r"(?m)^(?:/\*| \*) (\d{3}):", block)]
    assert listed[-1] == lib.pai_version() == 141, listed
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert name in block, name
        assert hasattr(lib, name) and name in pai.lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name


def test_switch_reads_like_the_other_tunables(pai, mode):
    from thesis_pai_reconstruction_amd import ops
    assert not pai.is_deterministic() and ops.get_tunable("deterministic", 0) == 0        # off by default
    mode(True)
    assert pai.is_deterministic() and ops.get_tunable("deterministic", 0) == 1
    mode(False)
    assert not pai.is_deterministic()
    ops.set_tunable("deterministic", 1)
    assert pai.is_deterministic()
    ops.set_tunable("deterministic")
    assert not pai.is_deterministic()
    assert ops.get_tunable("no_such_switch", 7) == 7


def test_environment_default(pai):
    """PAI_TUNE_deterministic=1 is the switch for whole runs (bench.py --set uses pai_set_tunable): a fresh process reads it."""
    import subprocess
    import sys
    code = ("import pai_bootstrap; pai = pai_bootstrap.load(); "
            "from thesis_pai_reconstruction_amd import ops; print(int(pai.is_deterministic()), ops.order_dependent_launches())")
    env = dict(os.environ, PAI_TUNE_deterministic="1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["1", "0"], out


def test_counter_exists_and_starts_at_zero(pai):
    """No launch has happened in this (GPU-less) process: queries and selections do not count."""
    from thesis_pai_reconstruction_amd import ops
    d = ops.make_desc(BF, 0, 64, 64, 64, 128, 0, 256, 2, 0, 0)
    ops.conv_wgrad_order_free(d, True)
    ops.conv_kernel_name(d, 2)
    assert ops.order_dependent_launches() == 0


def test_baseline_step_is_order_free_under_the_mode(pai, mode):
    from thesis_pai_reconstruction_amd import ops
    for dtype in (BF, F32):
        descs = baseline_descs(ops, dtype)
        base = [(ops.conv_wgrad_workspace_bytes(d), ops.conv_scratch_bytes(d, 2), ops.conv_wgrad_order_free(d, b),
                 ops.conv_kernel_name(d, 2)) for _, d, b in descs]
        mode(True)
        try:
            for (name, d, b), (ws, sc, _, _) in zip(descs, base):
                assert ops.conv_wgrad_order_free(d, b) and ops.conv_wgrad_order_free(d, False), (name, dtype)
                assert ops.conv_wgrad_workspace_bytes(d) >= ws and ops.conv_scratch_bytes(d, 2) >= sc, (name, dtype)
                assert ops.conv_kernel_name(d, 2) != "gg_rowdot", (name, dtype)      # its lanes meet by LDS atomics
        finally:
            mode(False)
        # default mode, nothing registered: the query reports today's paths honestly -- every converted family has a layer
        # that answers 0
        zero = {}
        for (name, d, b), (_, _, free, kname) in zip(descs, base):
            if not free:
                zero.setdefault(kname.split("<")[0], name)
        want = {"gg_wgrad_patch3_k", "thin_mfma_bf16"} if dtype == BF else {"gg_simt", "gg_rowdot"}
        assert want <= set(zero), (dtype, zero)
        # the un-split launches are order-free today and say so (the bottleneck layers)
        if dtype == BF:
            free_names = {name for (name, _, _), (_, _, free, _) in zip(descs, base) if free}
            assert {"encoders[6]", "decoders[1]"} <= free_names, free_names


def test_tile_and_patch_kernels_answer_zero_when_split(pai, mode):
    """gg_wgrad_mfma_k / gg_wgrad_patch_k split over the pixels add with atomics: 0 in default mode; under the mode the same
    layers report an un-split launch (1) on the same kernel family."""
    from thesis_pai_reconstruction_amd import ops
    cases = [ops.make_desc(BF, 0, 2, 64, 64, 64, 0, 64, 1, 0, 0, ops.ACT_NONE, kernel=3),
             ops.make_desc(BF, 0, 2, 64, 64, 64, 0, 64, 1, 0, 0, ops.ACT_NONE, kernel=1),
             ops.make_desc(BF, 1, 2, 32, 32, 64, 0, 64, 2, 0, 0, ops.ACT_NONE)]
    seen = set()
    for d in cases:
        name = ops.conv_kernel_name(d, 2)
        assert name.startswith(("gg_wgrad_mfma_k", "gg_wgrad_patch_k")), name
        seen.add(name.split("<")[0])
        assert not ops.conv_wgrad_order_free(d, False) and not ops.conv_wgrad_order_free(d, True)
        mode(True)
        try:
            assert ops.conv_wgrad_order_free(d, True) and ops.conv_kernel_name(d, 2).split("<")[0] == name.split("<")[0]
        finally:
            mode(False)
    assert seen == {"gg_wgrad_mfma_k", "gg_wgrad_patch_k"}, seen


def test_palette_defaults_are_order_free_under_the_mode(pai, mode):
    from thesis_pai_reconstruction_amd import ops
    for dtype in (BF, F32):
        descs = palette_descs(pai, ops, dtype)
        base = [(ops.conv_wgrad_workspace_bytes(d), ops.conv_scratch_bytes(d, 2), ops.conv_wgrad_order_free(d, b))
                for _, d, b in descs]
        assert not all(free for _, _, free in base), dtype        # some launch of today's Palette step is order-dependent
        mode(True)
        try:
            for (name, d, b), (ws, sc, _) in zip(descs, base):
                assert ops.conv_wgrad_order_free(d, b), (name, dtype)
                assert ops.conv_wgrad_workspace_bytes(d) >= ws and ops.conv_scratch_bytes(d, 2) >= sc, (name, dtype)
        finally:
            mode(False)


def test_wthin_is_not_selected_under_the_mode(pai, mode):
    from thesis_pai_reconstruction_amd import ops
    lib = pai.lib.load()
    import ctypes
    d1 = ops.make_desc(BF, 0, 64, 128, 128, 64, 0, 128, 2, 0, 0, ops.ACT_LRELU)
    d0 = ops.make_desc(BF, 0, 64, 256, 256, 1, 0, 64, 2, 0, 0, ops.ACT_LRELU)
    assert ops.conv_dgrad_act_wthin_ok(d1, d0)
    assert lib.pai_conv_dgrad_act_wthin_order_free(ctypes.byref(d1), ctypes.byref(d0)) == 0
    mode(True)
    try:
        assert not ops.conv_dgrad_act_wthin_ok(d1, d0)          # the two-launch path runs
        assert ops.conv_wgrad_order_free(d0, True)
    finally:
        mode(False)
    assert ops.conv_dgrad_act_wthin_ok(d1, d0)


def test_partial_row_queries(pai):
    lib = pai.lib.load()
    assert lib.pai_colsum_scratch_bytes(1000, 96) == 4 * 96 * 4           # four row blocks of 250 rows
    assert lib.pai_colsum_scratch_bytes(32, 16384) == 16384 * 4           # one row block
    assert lib.pai_colsum_scratch_bytes(0, 8) < 0
    assert lib.pai_gate_scratch_bytes(4096, 16) == lib.pai_gate_partial_rows(4096) * 17 * 4


def test_cli_flags_exist():
    import importlib.util
    import sys
    sys.path.insert(0, ROOT)
    for path, argv in ((os.path.join(ROOT, "main.py"), ["x", "--deterministic"]),
                       (os.path.join(ROOT, "scripts", "train_palette.py"), ["x", "--synthetic", "4", "--deterministic"])):
        spec = importlib.util.spec_from_file_location("_cli_under_test", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert mod.build_parser().parse_args(argv).deterministic is True
        assert mod.build_parser().parse_args(argv[:-1]).deterministic is False
