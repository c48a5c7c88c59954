"""Host side of the device-generator Dropout2d of the GAN families: the two entry points in the header (under ABI 141), in
lib.SIGNATURES, in the built library and in ops; the stream constant; the command-line switches; ``pai.DeviceRNG`` as the class
``UnetWrapper`` takes; the composition of the counter word ``sub``; the generator's state in a trainer checkpoint and the two
refused mismatches.  No GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pai_dropout2d_rng", "pai_dropout2d_rng_dev")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_entry_points_declared_listed_exported(pai):
    from thesis_pai_reconstruction_amd import lib, ops
    header = _read("include", "pai_hip.h")
    history = header[:header.index("int pai_version(void);")]
    entry_141 = history[history.rindex(" * 141:"):]
    for name in NEW:
        assert re.search(r"\b%s\b" % name, entry_141), f"{name} is not listed under 141 in the header history"
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in lib.SIGNATURES
        assert hasattr(lib.load(), name)
    assert lib.load().pai_version() == 141
    assert callable(ops.dropout2d_rng) and callable(ops.dropout2d_rng_dev)
    # same arguments but for the step: by value against a pointer
    a, b = lib.SIGNATURES[NEW[0]][1], lib.SIGNATURES[NEW[1]][1]
    assert len(a) == len(b) == 13 and [i for i in range(13) if a[i] is not b[i]] == [8]


def test_stream_constant_documented(pai):
    from thesis_pai_reconstruction_amd import ops, rng
    assert re.search(r"PHILOX_STREAM_DROPOUT2D\s*=\s*4096", _read("thesis-pai-reconstruction_amd", "csrc", "philox.h"))
    header = _read("include", "pai_hip.h")
    assert "PHILOX_STREAM_DROPOUT2D" in header and "4096 + j" in header
    assert ops.STREAM_DROPOUT2D == rng.DROPOUT2D_STREAM == 4096
    assert ops.STREAM_DROPOUT2D >= ops.STREAM_DROPOUT + 1024       # clear of the 16 + i of any ResBlock count in use


def test_null_pointers_refused_without_a_device(pai):
    """The refusals come before any launch, so they answer on a box without a GPU (the GPU test covers the rest)."""
    from thesis_pai_reconstruction_amd import lib
    L = lib.load()
    assert L.pai_dropout2d_rng(lib.F32, None, 1, 1, 8, 0, 0, 0, 0, 0, 1.0, None, None) != 0
    assert b"pai_dropout2d_rng" in L.pai_last_error()
    assert L.pai_dropout2d_rng_dev(lib.F32, None, 1, 1, 8, 0, 0, 0, None, 0, 1.0, None, None) != 0
    assert b"pai_dropout2d_rng_dev" in L.pai_last_error()


def test_cli_switches(pai):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_main_for_rng_test", os.path.join(ROOT, "main.py"))
    main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(main)
    p = main.build_parser()
    a = p.parse_args(["run"])
    assert a.device_rng is False and a.rng_seed == 0
    a = p.parse_args(["run", "--device-rng", "--rng-seed", "41"])
    assert a.device_rng is True and a.rng_seed == 41


def test_device_rng_is_the_class_the_wrapper_takes(pai):
    from thesis_pai_reconstruction_amd import rng
    from thesis_pai_reconstruction_amd.models import palette
    assert pai.DeviceRNG is rng.DeviceRNG is palette.DeviceRNG
    assert pai.UnetWrapper.device_rng is None                      # the opt-in, off by default
    for m in (pai.Pix2Pix(1, 1, (1, 2, 2, 4), 0.5, "gan"), pai.AttentionUnetGAN(1, 1, (1, 2, 2, 4), 0.5, "gan"),
              pai.ResUnetGAN(1, 1, "18", (1, 2, 2, 4), 0.5, "gan")):
        assert isinstance(m, pai.UnetWrapper) and m.device_rng is None and m.unet.device_rng is None
        m.device_rng = pai.DeviceRNG(7)
        assert isinstance(m.device_rng, rng.DeviceRNG) and "device_rng" not in m.state_dict()


def test_plan_refusal_strings(pai):
    """Without a generator the refusals are the parent's, word for word; with one Dropout2d passes and the ViT's dropout stays."""
    from thesis_pai_reconstruction_amd import plan

    class OnDevice(torch.Tensor):          # _why_not asks the batch only whether it is on the device
        is_cuda = property(lambda self: True)

    def why(m):
        m.train()
        m._all_optimizers = lambda: []      # no optimizer is built on the host
        return plan.PlannedStep(m)._why_not((torch.zeros(1).as_subclass(OnDevice),))

    res = pai.ResUnetGAN(1, 1, "18", (1, 2, 2, 2), 0.5, "gan")
    assert sum(isinstance(x, torch.nn.Dropout2d) for x in res.modules()) >= 1
    assert why(res) == "Dropout2d masks are drawn per step outside the C ABI"
    res.device_rng = pai.DeviceRNG(1)
    assert why(res) is None
    p2p = pai.Pix2Pix(1, 1, (1, 4, 4, 4), 0.5, "gan")
    assert sum(isinstance(x, torch.nn.Dropout2d) for x in p2p.modules()) == 2
    assert why(p2p) == "dropout > 0"        # Unet.dropout is met before the first Dropout2d module: the parent's answer
    p2p.device_rng = pai.DeviceRNG(1)
    assert why(p2p) is None
    tu = pai.TransUnetGAN(1, 1, patch_size=4, channel_mults=(1, 2, 2), dropout=0.5, loss_type="gan")
    tu.device_rng = pai.DeviceRNG(1)
    assert why(tu) == "dropout > 0"
    assert why(pai.Pix2Pix(1, 1, (1, 2, 2, 4), 0.0, "gan")) is None


@pytest.mark.parametrize("rank,k,want", [(0, 0, 0), (0, 1, 1), (3, 0, 3 << 16), (3, 1, (3 << 16) | 1)])
def test_sub_composition(pai, rank, k, want):
    from thesis_pai_reconstruction_amd import rng
    assert rng.dropout_sub(rank, k) == want
    r = pai.DeviceRNG(5)
    r.rank = rank
    seen = [rng.dropout_sub(r.rank, r.next_forward()) for _ in range(k + 1)]
    assert seen[-1] == want and seen[0] == rank << 16
    r.advance()                                                    # the next step counts its forwards from 0 again
    assert r.next_forward() == 0 and r.step == 1 and r._mirrors == {}


def test_sub_refuses_what_does_not_fit(pai):
    from thesis_pai_reconstruction_amd import rng
    for rank, k in ((1 << 16, 0), (0, 1 << 16), (-1, 0)):
        with pytest.raises(pai.PaiError):
            rng.dropout_sub(rank, k)


def test_checkpoint_round_trip_and_mismatches(pai, tmp_path):
    """Trainer.save_checkpoint writes the two integers; restoring puts them back; a generator on one side only is refused."""
    from thesis_pai_reconstruction_amd import rng
    seed, step = (1 << 64) - 3, (1 << 32) - 2
    m = pai.Pix2Pix(1, 1, (1, 2, 2, 4), 0.5, "gan")
    m.device_rng = pai.DeviceRNG(seed, step)
    tr = pai.Trainer(max_epochs=1, logger=False, enable_progress_bar=False)
    tr.model = m
    path = tmp_path / "with.ckpt"
    tr.save_checkpoint(path)
    ckpt = torch.load(str(path), map_location="cpu", weights_only=False)
    assert ckpt["device_rng"] == {"seed": seed, "step": step}

    fresh = pai.Pix2Pix(1, 1, (1, 2, 2, 4), 0.5, "gan")
    fresh.device_rng = pai.DeviceRNG(1)
    fresh.device_rng.next_forward()
    rng.restore_checkpoint_state(fresh, ckpt)
    assert (fresh.device_rng.seed, fresh.device_rng.step) == (seed, step) and fresh.device_rng.next_forward() == 0

    bare = pai.Pix2Pix(1, 1, (1, 2, 2, 4), 0.5, "gan")
    with pytest.raises(pai.PaiError, match="device_rng"):
        rng.restore_checkpoint_state(bare, ckpt)                   # the checkpoint has a generator, the model has none
    with pytest.raises(pai.PaiError, match="device_rng"):
        pai.Trainer(max_epochs=1, logger=False, enable_progress_bar=False).restore(bare, path)

    tr.model = bare
    path2 = tmp_path / "without.ckpt"
    tr.save_checkpoint(path2)
    assert "device_rng" not in torch.load(str(path2), map_location="cpu", weights_only=False)
    with pytest.raises(pai.PaiError, match="device_rng"):
        pai.Trainer(max_epochs=1, logger=False, enable_progress_bar=False).restore(fresh, path2)
    assert (fresh.device_rng.seed, fresh.device_rng.step) == (seed, step)      # a refused restore changed nothing
