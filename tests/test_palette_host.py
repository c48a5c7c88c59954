"""CPU: the host side of pai.Palette against the fixtures recorded from the reference (tests/golden/ref_palette_*.npz,
scripts/gen_palette_golden.py): module tree (state-dict keys and shapes), schedule buffers, the per-step scalar table of the
sampler, checkpoint loading, and the refusals (host tensors, training)."""
import numpy as np
import pytest
import torch

import _palette_util as U
from oracle import golden


@pytest.fixture(scope="module")
def recs(golden_dir):
    return {name: golden.load(golden_dir, f"ref_palette_{name}") for name in U.CONFIGS}


@pytest.mark.parametrize("learn_var", [False, True])
@pytest.mark.parametrize("name", list(U.CONFIGS))
def test_state_dict_matches_reference(pai, recs, name, learn_var):
    rec = recs[name]
    kw = dict(U.palette_kwargs(name), learn_var=learn_var)
    sd = pai.Palette(**kw).state_dict()
    want = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(rec["keys"], rec["shapes"])}
    if learn_var != bool(rec["meta_learn_var"]):      # the variance head doubles / halves the last convolution, nothing else
        co = 2 if learn_var else 1
        want["unet.out.2.weight"] = (co,) + want["unet.out.2.weight"][1:]
        want["unet.out.2.bias"] = (co,)
    assert list(sd) == list(want)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want


@pytest.mark.parametrize("name", list(U.CONFIGS))
def test_schedule_buffers(pai, recs, name):
    m = pai.Palette(**U.palette_kwargs(name))
    assert m.diffusion.timesteps == 2000 and m.diffusion_inf.timesteps == 100
    for dm in ("diffusion", "diffusion_inf"):
        for b in ("alphas", "gammas", "gammas_prev"):
            got, want = getattr(getattr(m, dm), b).numpy(), recs[name][f"{dm}.{b}"]
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.abs(got.astype(np.float64) - want).max() <= 1e-7, (dm, b)


def test_step_table_matches_reference_expressions(pai, recs):
    """The six scalars of every step against the expressions of reference palette.py:271-306, evaluated as the reference
    evaluates them (fp32 tensor arithmetic) on the recorded buffers."""
    rec = recs["a"]
    a, g, gp = (torch.from_numpy(rec[f"diffusion_inf.{b}"]) for b in ("alphas", "gammas", "gammas_prev"))
    lower = torch.clamp((1 - a) * (1 - gp) / (1 - g), min=1e-20)
    want = torch.stack([torch.sqrt(1 - g), 1 / torch.sqrt(g), torch.sqrt(gp) * (1 - a) / (1 - g),
                        torch.sqrt(a) * (1 - gp) / (1 - g), torch.log(lower), torch.log(1 - a)], 1).double().numpy()
    table = np.array(pai.Palette(**U.palette_kwargs("a")).diffusion_inf.step_table(), dtype=np.float64)
    assert table.shape == (100, 6)
    assert np.all(np.abs(table - want) <= 1e-6 * np.abs(want)), np.abs(table - want).max(0)
    assert abs(table[99, 1] - 1 / np.sqrt(float(g[99]))) < 1e-3 * table[99, 1] and table[99, 1] > 700     # the 800 of step 99
    assert table[0, 3] == 0.0 and abs(table[0, 4] - np.log(1e-20)) < 1e-4        # step 0: variance at its clamp


def test_reference_checkpoint_without_inference_steps(pai, tmp_path):
    """A checkpoint that carries only the reference's hyper-parameters loads, with the reference's 100 steps."""
    src = U.init_portable(pai.Palette(**U.palette_kwargs("b")), 5)
    hp = dict(U.palette_kwargs("b"))
    assert "inference_steps" not in hp and src.hparams["inference_steps"] == 100
    path = tmp_path / "ref.ckpt"
    torch.save({"hyper_parameters": hp, "state_dict": src.state_dict()}, path)
    m = pai.Palette.load_from_checkpoint(path)
    assert m.diffusion_inf.timesteps == 100 and m.hparams["inference_steps"] == 100 and m.learn_var
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    short = pai.Palette(**hp, inference_steps=4)
    assert short.diffusion_inf.timesteps == 4 and len(short.diffusion_inf.step_table()) == 4


def test_host_tensors_and_training_are_refused(pai):
    m = pai.Palette(**U.palette_kwargs("a"))
    x = torch.zeros(1, 1, 16, 16)
    m.eval()
    with pytest.raises(pai.PaiError):
        m(x)
    with pytest.raises(pai.PaiError):
        m.unet(x, x, torch.ones(1))
    with pytest.raises(NotImplementedError, match="sampling only"):
        m.training_step((x, x), 0)
    with pytest.raises(NotImplementedError, match="sampling only"):
        m.configure_optimizers()
    assert hasattr(m.unet, "compute_dtype")
    m.set_precision("bf16-mixed")
    assert m.unet.compute_dtype == torch.bfloat16


def test_main_still_refuses_palette_and_says_why(pai):
    import main as cli
    args = cli.build_parser().parse_args(["run", "-m", "palette", "--synthetic", "4"])
    with pytest.raises(NotImplementedError, match="training"):
        cli.main(args)


def test_mac_count_of_one_sampling_call(pai):
    """report.py counts inference_steps U-Net passes; the U-Net count includes the two attention products."""
    import report
    m = pai.Palette(**U.palette_kwargs("a"), inference_steps=3)
    per_pass = m.unet.macs(256, 256)
    assert report.count_macs(m) == 3 * per_pass
    att = [b for b in m.unet.modules() if type(b).__name__ == "AttentionBlock"]
    assert len(att) == 6 and per_pass > sum(2 * (128 * 128) ** 2 * b.channels for b in att)
