"""``DeviceRNG``: the host-side state of the device generator (csrc/philox.h), shared by Palette and by the Dropout2d sites of
the GAN families.  Two Python integers and, for consumers replayed from a launch plan, a uint32 mirror in device memory."""
import torch

from . import ops
from .ops import PaiError

DROPOUT2D_STREAM = ops.STREAM_DROPOUT2D      # + j: the Dropout2d behind decoder j (PHILOX_STREAM_DROPOUT2D)


def dropout_sub(rank: int, k: int) -> int:
    """Counter word ``sub`` of a Dropout2d site: ``(rank << 16) | k``.  ``k`` is the index of the train-mode forward of the
    network within the step (a GAN step: 0 the D-phase forward, 1 the G-phase forward), ``rank`` the data-parallel rank."""
    rank, k = int(rank), int(k)
    if not 0 <= rank < 1 << 16 or not 0 <= k < 1 << 16:
        raise PaiError(f"dropout_sub: rank={rank} and k={k} must each fit 16 bits")
    return (rank << 16) | k


class DeviceRNG:
    """The state of the device generator (csrc/philox.h): a 64-bit ``seed`` and a ``step`` counter, two Python integers.  Every
    random value of a step is a pure function of (seed, step, site, element index), so a run resumes reproducibly
    from ``state_dict()``.  ``step`` is the training step or the index of the sampling call: each consumer calls ``advance()``
    once per call.  The two integers are the truth (``state_dict`` / ``load_state_dict`` / ``--resume``), and nothing is ever
    read back from the device.

    A consumer whose launches are replayed from a recorded plan (the planned sampler, the planned GAN step) cannot take ``step``
    by value: it asks ``device_step(device)`` for a uint32 device scalar that mirrors it.  The mirror of a device is created on
    that first request; from then on ``advance()`` moves it with ``pai_counter_add`` in stream order, and the next request
    rewrites it with ``pai_counter_set`` whenever the host value is not the one the mirror was last given (first use,
    ``load_state_dict``, an assignment to ``step``).  Without such a consumer no mirror exists and nothing is launched.  A
    mirror follows the host in the order of ONE stream: consumers on different streams need generators of their own.

    The Dropout2d sites of a ``UnetWrapper`` family (``model.device_rng = DeviceRNG(seed)``) also use ``rank`` (the
    data-parallel rank, set by the Trainer; not part of the state) and ``next_forward()``, the count of train-mode forwards since
    the last ``advance()``: the two halves of ``dropout_sub``."""

    def __init__(self, seed: int = 0, step: int = 0):
        self.seed, self.step = self._check(seed, 64, "seed"), self._check(step, 32, "step")
        self._mirrors = {}          # device index -> [int32 device scalar (the bits of the uint32), the value it holds]
        self.rank = 0
        self._forwards = 0

    @staticmethod
    def _check(v, bits, what):
        v = int(v)
        if not 0 <= v < 1 << bits:
            raise PaiError(f"DeviceRNG: {what}={v} is not an unsigned {bits}-bit integer")
        return v

    def advance(self, n: int = 1) -> int:
        """The step the next call uses; the counter is 32 bits wide and wraps."""
        old = self.step
        self.step = (old + int(n)) & 0xFFFFFFFF
        self._forwards = 0
        for m in self._mirrors.values():
            if m[1] == old:                     # in step with the host: stays so; otherwise the next request rewrites it
                with torch.cuda.device(m[0].device):
                    ops.counter_add(m[0], int(n) & 0xFFFFFFFF)
                m[1] = self.step
        return self.step

    def replayed(self, n: int) -> int:
        """A replayed launch plan held the ``pai_counter_add`` of an ``advance(n)``: the mirrors that were in step have moved on the
        device already, so only the host side follows -- no launch."""
        old = self.step
        self.step = (old + int(n)) & 0xFFFFFFFF
        self._forwards = 0
        for m in self._mirrors.values():
            if m[1] == old:
                m[1] = self.step
        return self.step

    def next_forward(self) -> int:
        """k of ``dropout_sub``: 0 for the first train-mode forward since ``advance()``, 1 for the second, ..."""
        k = self._forwards
        self._forwards = k + 1
        return k

    def device_step(self, device) -> torch.Tensor:
        """The device scalar (int32 storage, uint32 bits) that holds ``step`` in the order of the current stream of ``device``."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise PaiError("DeviceRNG.device_step needs a HIP device")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        m = self._mirrors.get(idx)
        if m is None:
            m = self._mirrors[idx] = [torch.empty(1, dtype=torch.int32, device=torch.device("cuda", idx)), None]
        step = self._check(self.step, 32, "step")
        if m[1] != step:
            with torch.cuda.device(m[0].device):
                ops.counter_set(m[0], step)
            m[1] = step
        return m[0]

    def state_dict(self) -> dict:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state) -> None:
        self.seed, self.step = self._check(state["seed"], 64, "seed"), self._check(state["step"], 32, "step")
        self._forwards = 0

    def __repr__(self):
        return f"DeviceRNG(seed={self.seed}, step={self.step})"


def checkpoint_state(model) -> dict:
    """The entry a trainer's checkpoint carries for ``model.device_rng`` ({} without one)."""
    rng = getattr(model, "device_rng", None)
    return {} if rng is None else {"device_rng": rng.state_dict()}


def restore_checkpoint_state(model, ckpt) -> None:
    """Restore ``model.device_rng`` from a checkpoint dictionary; a mismatch between the two is refused (the run could not
    continue with the masks it would have drawn)."""
    rng = getattr(model, "device_rng", None)
    state = ckpt.get("device_rng")
    if state is not None and rng is None:
        raise PaiError("the checkpoint was written with a device generator (device_rng): set model.device_rng (--device-rng) "
                       "before restoring it")
    if state is None and rng is not None:
        raise PaiError("the checkpoint holds no device generator state: it was written without device_rng (--device-rng)")
    if rng is not None:
        rng.load_state_dict(state)
