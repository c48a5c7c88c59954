"""GPU: the eval-mode guided-diffusion U-Net of pai.Palette against the reference's own forward pass (fixtures
tests/golden/ref_palette_*.npz, recorded on the CPU with the weights of tests/_palette_util.py).

fp32 mode: 1e-4 of the largest value, the project's forward bound (the fixtures' own fp32-vs-fp64 floor is about 1e-6), for
the output and for the recorded intermediates (every 8th channel behind the first convolution, the first ResBlock, the
first AttentionBlock and the middle block), which place a failure.  bf16 mode: relative L2 distance at most twice
``bf16_dev``, the distance of the reference's own output under bf16 autocast from its fp32 output; the factor 2 because
this path also stores the activations in bf16 between the layers.  The intermediates are printed there, not bounded: the
reference records no bf16 yardstick for them.

The second gamma vector runs on the same model right after the first: FiLM coefficients left over from the first call
would show, because the two recorded outputs differ by far more than the bound."""
import pytest
import torch

import _palette_util as U
from _gpu_util import dev, max_err, rel_err
from oracle import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recs(golden_dir):
    return {name: golden.load(golden_dir, f"ref_palette_{name}") for name in U.CONFIGS}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(U.CONFIGS))
def test_unet_forward_matches_reference(pai, recs, name, dtype):
    rec = recs[name]
    m = U.init_portable(pai.Palette(**U.palette_kwargs(name)), U.CONFIGS[name][4]).to(dev())
    m.freeze()
    m.set_precision("32" if dtype == torch.float32 else "bf16-mixed")
    x, y_t = (torch.from_numpy(rec[k]).to(dev()) for k in ("x", "y_t"))
    want = [torch.from_numpy(rec[f"out{i}"]) for i in (0, 1)]
    assert max_err(want[1], want[0]) > 1e-3          # the two gamma vectors are told apart by the fp32 bound
    for i in (0, 1):
        m.unet.debug_capture = cap = {} if i == 0 else None
        got = m.unet(x, y_t, torch.from_numpy(rec[f"gammas{i}"]).to(dev())).cpu()
        assert got.shape == want[i].shape and got.dtype == torch.float32
        if i == 0:
            for key in U.first_modules(m.unet):
                a_got, a_want = cap[key][:, ::U.CROP].cpu(), torch.from_numpy(rec["act:" + key])
                e = max_err(a_got, a_want)
                print(f"palette {name} {dtype} {key}: max err / max {e:.3e}")
                if dtype == torch.float32:
                    assert e <= 1e-4, key
        if dtype == torch.float32:
            e = max_err(got, want[i])
            print(f"palette {name} fp32 gammas{i}: max err / max {e:.3e}")
            assert e <= 1e-4
        else:
            e, yard = rel_err(got, want[i]), float(rec[f"bf16_dev{i}"])
            print(f"palette {name} bf16 gammas{i}: rel L2 {e:.3e}, reference under autocast {yard:.3e}")
            assert e <= 2 * yard


def test_unet_refuses_training_mode(pai):
    m = pai.Palette(**U.palette_kwargs("a")).to(dev())
    m.train()
    x = torch.zeros(1, 1, 16, 16, device=dev())
    with pytest.raises(pai.PaiError, match="eval"):
        m.unet(x, x, torch.ones(1, device=dev()))
    with pytest.raises(pai.PaiError, match="eval"):
        m(x)
