"""CPU: the host side of the planned Palette sampler: the five C entry points it adds (declared, exported, bound, ABI still
141) and their refusals, the opt-in switch, and ``DeviceRNG`` with its device mirror -- which on a box without a GPU must
never come into being."""
import ctypes
import os
import re

import pytest

import _palette_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pai_counter_set", "pai_counter_add", "pai_philox_fill_dev", "pai_palette_step_dev", "pai_palette_step_rng_dev")


def test_new_entries_under_abi_141(pai):
    src = open(os.path.join(ROOT, "include", "pai_hip.h")).read()
    decl = set(re.findall(r"\b(pai_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = pai.lib.load()
    for name in NEW:
        assert name in decl and name in pai.lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pai_version() == 141
    from thesis_pai_reconstruction_amd import ops
    for name in ("counter_set", "counter_add", "philox_fill_dev", "palette_step_dev", "palette_step_rng_dev"):
        assert callable(getattr(ops, name)), name


def test_sampler_plan_switch(pai, monkeypatch):
    monkeypatch.delenv("PAI_PALETTE_PLAN", raising=False)
    m = pai.Palette(**U.palette_kwargs("a"))
    assert m.sampler_plan is False
    info = m.sampler_plan_info()
    assert info == {"plans": 0, "records": 0, "replays": 0, "disabled": None, "launches_per_step": None}
    monkeypatch.setenv("PAI_PALETTE_PLAN", "1")
    assert pai.Palette(**U.palette_kwargs("a")).sampler_plan is True
    assert m.sampler_plan is False                      # the default of NEW objects only
    monkeypatch.setenv("PAI_PALETTE_PLAN", "0")
    assert pai.Palette(**U.palette_kwargs("a")).sampler_plan is False
    # the switch is no parameter, buffer or hyper-parameter: checkpoints do not change
    assert not any("plan" in k for k in m.state_dict())


def test_device_rng_host_semantics(pai):
    from thesis_pai_reconstruction_amd.models.palette import DeviceRNG
    r = DeviceRNG(seed=(1 << 64) - 1, step=(1 << 32) - 2)
    assert r.advance() == (1 << 32) - 1 and r.advance() == 0 and r.advance(5) == 5      # 32 bits, wraps
    assert r.state_dict() == {"seed": (1 << 64) - 1, "step": 5}
    q = DeviceRNG()
    q.load_state_dict(r.state_dict())
    assert (q.seed, q.step) == (r.seed, r.step) and repr(q) == f"DeviceRNG(seed={r.seed}, step=5)"
    q.step = 9                                                                              # direct assignment stays possible
    assert q.advance() == 10 and q.state_dict()["step"] == 10
    for bad in (dict(seed=-1), dict(seed=1 << 64), dict(step=-1), dict(step=1 << 32)):
        with pytest.raises(pai.PaiError):
            DeviceRNG(**bad)
    with pytest.raises(pai.PaiError):
        q.load_state_dict({"seed": 0, "step": 1 << 32})
    # nothing above touched a device: no mirror exists, and the state holds the two integers only
    assert r._mirrors == {} and q._mirrors == {}
    assert set(r.state_dict()) == {"seed", "step"}
    with pytest.raises(pai.PaiError, match="HIP device"):
        r.device_step("cpu")
    assert r._mirrors == {}


def test_refusals_come_before_any_launch(pai):
    """Every refusal returns an error with its message in pai_last_error and never touches a pointer (there is no GPU here)."""
    lib = pai.lib.load()
    fake = ctypes.c_void_p(0x100000)          # aligned, never dereferenced
    odd = ctypes.c_void_p(0x100002)
    F32 = pai.lib.F32

    def cset(c=fake):
        return lib.pai_counter_set(c, 1, None)

    def cadd(c=fake):
        return lib.pai_counter_add(c, 1, None)

    def fill(kind=2, out=fake, n=7, step=fake, param=0):
        return lib.pai_philox_fill_dev(kind, out, n, 1, 0, 3, step, param, None)

    def step(dtype=F32, mo=fake, y_t=fake, stack=fake, pixels=37, C=1, table=fake, T=5, pos=fake, gammas=fake, N=2, gnext=fake,
             y_next=fake):
        return lib.pai_palette_step_dev(dtype, mo, y_t, stack, pixels, C, 0, table, T, pos, gammas, N, gnext, y_next, None, None)

    def srng(dtype=F32, mo=fake, y_t=fake, pixels=37, C=1, table=fake, T=5, pos=fake, gammas=fake, N=2, gnext=fake, rstep=fake,
             y_next=fake):
        return lib.pai_palette_step_rng_dev(dtype, mo, y_t, pixels, C, 0, table, T, pos, gammas, N, gnext, 1, rstep, y_next, None,
                                            None)

    cases = [(cset, dict(c=None), b"null"), (cadd, dict(c=None), b"null"), (cset, dict(c=odd), b"aligned"),
             (cadd, dict(c=odd), b"aligned"),
             (fill, dict(out=None), b"null"), (fill, dict(step=None), b"null"), (fill, dict(n=0), b"n=0"),
             (fill, dict(kind=5), b"kind=5"), (fill, dict(kind=3, param=0), b"T=0"), (fill, dict(kind=4, param=65537), b"thr=65537")]
    for fn in (step, srng):
        cases += [(fn, dict(T=0), b"T=0"), (fn, dict(C=0), b"C=0"), (fn, dict(pixels=0), b"pixels=0"), (fn, dict(N=0), b"N=0"),
                  (fn, dict(dtype=2), b"dtype=2")]
        for ptr in ("mo", "y_t", "table", "pos", "gammas", "gnext", "y_next"):
            cases.append((fn, {ptr: None}, b"null"))
    cases += [(step, dict(stack=None), b"null"), (srng, dict(rstep=None), b"null"),
              (step, dict(pixels=1 << 40, C=1 << 20), b"too large"), (srng, dict(pixels=1 << 40), b"too large")]
    for call, kw, word in cases:
        assert call(**kw) != 0, (call.__name__, kw)
        assert word in lib.pai_last_error(), (call.__name__, kw, lib.pai_last_error())
