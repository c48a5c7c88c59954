"""CPU: the host restatement of the device generator (tests/_philox_ref.py) against the published known answers of
Philox4x32-10, the statistics of its derived kinds, the ABI surface of the device generator and the host-side refusals.

Known answers: the three Philox4x32-10 vectors of the Random123 distribution (kat_vectors).  Statistics at one fixed seed
(SEED below, the first one tried; every figure was inside its bound), n = 2^20: the keep rate within 5 sqrt(p (1 - p) / n) of
1 - thr / 65536, the normal mean within 5 / sqrt(n), its variance within 5 sqrt(2 / n), the integers all in [0, 2000)."""
import io
import os
import re

import numpy as np
import pytest
import torch

import _philox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x9E3779B97F4A7C15
N = 1 << 20
NEW = ("pai_philox_fill", "pai_film_norm_fwd_rng", "pai_film_norm_bwd_rng", "pai_palette_noise_rng", "pai_palette_step_rng")


def _hex(block):
    return " ".join(f"{int(w):08x}" for w in np.asarray(block).reshape(-1))


def test_known_answers():
    assert _hex(R.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(R.philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_counter_layout():
    """blocks() puts the block index in counter word 0, sub / stream / step in words 1 .. 3 and the seed halves in the key."""
    seed, sub, stream, step = 0x299F31D0A4093822, 0x85A308D3, 0x13198A2E, 0x03707344
    b = R.blocks(9, seed, sub, stream, step)
    for i in (0, 3, 8):
        assert _hex(b[i]) == _hex(R.philox4x32_10((i, sub, stream, step), (0xA4093822, 0x299F31D0)))
    assert R.raw(7, seed, sub, stream, step).tolist() == [int(v) for v in b.reshape(-1)[:7]]


def test_abi_surface(pai):
    """The new names are declared in the header, listed in lib.SIGNATURES and exported; the version stays 141."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pai_hip.h")).read(), flags=re.S)
    lib = pai.lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in pai_hip.h"
        assert name in pai.lib.SIGNATURES, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.pai_version() == 141
    from thesis_pai_reconstruction_amd import ops
    assert (ops.PHILOX_RAW, ops.PHILOX_UNIFORM, ops.PHILOX_NORMAL, ops.PHILOX_INT, ops.PHILOX_KEEP) == \
        (R.RAW, R.UNIFORM, R.NORMAL, R.INT, R.KEEP)
    assert (ops.STREAM_T, ops.STREAM_U, ops.STREAM_Z, ops.STREAM_SAMPLER, ops.STREAM_DROPOUT) == \
        (R.STREAM_T, R.STREAM_U, R.STREAM_Z, R.STREAM_SAMPLER, R.STREAM_DROPOUT)
    for p in (0.0, 0.1, 0.25, 0.5):
        assert ops.dropout_thr(p) == R.thr_of(p)


def test_distinct_streams():
    """Changing any one of seed low, seed high, sub, stream or step changes the block."""
    base = dict(seed=0x0123456789ABCDEF, sub=5, stream=17, step=9)
    ref = R.blocks(2, **base)
    for change in (dict(seed=base["seed"] ^ 1), dict(seed=base["seed"] ^ (1 << 32)), dict(sub=6), dict(stream=18), dict(step=10)):
        other = R.blocks(2, **dict(base, **change))
        assert (other != ref).any(axis=1).all(), change
    assert (ref[0] != ref[1]).any()


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_rate(p):
    thr = R.thr_of(p)
    rate = float(R.keep(N, thr, SEED, 0, R.STREAM_DROPOUT, 7).mean())
    want, lim = 1 - thr / 65536, 5 * np.sqrt(p * (1 - p) / N)
    print(f"keep rate p={p}: {rate:.6f} want {want:.6f} (|diff| / bound {abs(rate - want) / lim:.3f})")
    assert abs(rate - want) <= lim
    assert R.keep(64, 0, SEED, 0, R.STREAM_DROPOUT, 7).all()                 # p = 0 keeps all


def test_normal_moments():
    z, r = R.normal(N, SEED, 0, R.STREAM_Z, 7)
    mean, var = float(z.mean()), float(z.var())
    print(f"normal: mean {mean:.3e} (bound {5 / np.sqrt(N):.3e}), var - 1 {var - 1:.3e} (bound {5 * np.sqrt(2 / N):.3e})")
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1) <= 5 * np.sqrt(2 / N)
    assert np.isfinite(z).all() and (np.abs(z) <= r + 1e-12).all()
    assert np.allclose(z[0::2] ** 2 + z[1::2] ** 2, r[0::2] ** 2, rtol=1e-12, atol=1e-300)


def test_integers_and_uniforms_in_range():
    t = R.integer(N, 2000, SEED, 0, R.STREAM_T, 7)
    assert t.dtype == np.int32 and int(t.min()) >= 0 and int(t.max()) < 2000
    assert int(t.min()) == 0 and int(t.max()) == 1999                        # 2^20 draws reach both ends
    assert not R.integer(64, 1, SEED, 0, R.STREAM_T, 7).any()
    u = R.uniform(N, SEED, 0, R.STREAM_U, 7)
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    w = R.raw(16, SEED, 0, R.STREAM_U, 7)
    assert np.array_equal(u[:16].astype(np.float64) * 2.0 ** 24, (w >> np.uint32(8)).astype(np.float64))


# ---- refusals before any launch (no GPU here) ---------------------------------------------------------------------------------
def test_dropout_rng_excludes_dropout_mask(pai):
    from thesis_pai_reconstruction_amd import functional as PF
    x = torch.zeros(2, 4, 8)
    w, b = torch.ones(8), torch.zeros(8)
    with pytest.raises(pai.PaiError, match="exclude"):
        PF.film_norm_act(x, w, b, p=0.25, dropout_mask=torch.ones(2, 4, 8, dtype=torch.uint8), dropout_rng=(1, 16, 0))


def test_host_tensors_are_refused(pai):
    from thesis_pai_reconstruction_amd import functional as PF
    from thesis_pai_reconstruction_amd import ops
    x = torch.zeros(2, 4, 8)
    with pytest.raises(pai.PaiError, match="device"):
        PF.film_norm_act(x, torch.ones(8), torch.zeros(8), p=0.25, dropout_rng=(1, 16, 0))
    with pytest.raises(pai.PaiError, match="device"):
        PF.philox_fill("normal", (8,), 1, device="cpu")
    with pytest.raises(pai.PaiError, match="device"):
        PF.philox_fill("normal", None, 1, out=torch.zeros(8))
    with pytest.raises(pai.PaiError, match="kind"):
        PF.philox_fill("gauss", (8,), 1, device="cpu")
    with pytest.raises(pai.PaiError, match="device"):
        ops.philox_fill(ops.PHILOX_RAW, torch.zeros(8, dtype=torch.int32), 1, 0, 0, 0)
    m = pai.DiffusionModel("linear", 2000)
    with pytest.raises(pai.PaiError, match="device"):
        PF.palette_noise_rng(torch.zeros(2, 1, 4, 4), 1, 0, m)
    with pytest.raises(pai.PaiError, match="64-bit"):
        ops._u64(1 << 64)
    with pytest.raises(pai.PaiError, match="32-bit"):
        ops._u32(-1, "step")


def test_device_rng_state_round_trip(pai):
    a = pai.DeviceRNG(0xFEDCBA9876543210)
    assert (a.seed, a.step) == (0xFEDCBA9876543210, 0)
    assert a.advance() == 1 and a.advance() == 2
    state = a.state_dict()
    assert state == {"seed": 0xFEDCBA9876543210, "step": 2}
    b = pai.DeviceRNG(1)
    b.load_state_dict(state)
    assert (b.seed, b.step) == (a.seed, a.step)
    assert b.advance() == 3 and a.step == 2
    buf = io.BytesIO()                 # plain integers: the state survives torch.save / torch.load as part of a checkpoint
    torch.save({"rng": state}, buf)
    buf.seek(0)
    assert torch.load(buf)["rng"] == state
    with pytest.raises(pai.PaiError):
        pai.DeviceRNG(-1)
    with pytest.raises(pai.PaiError):
        pai.DeviceRNG(1 << 64)
    c = pai.DeviceRNG(3, step=0xFFFFFFFF)
    assert c.advance() == 0                                                  # the 32-bit counter wraps
    assert pai.Palette(1, 1, (1, 2), (2,), 0.0).device_rng is None                # off by default
