"""Fixture files of tests/golden.

A fixture is ``<name>.npz``.  A committed file stays under ``LIMIT`` bytes, so an array whose compressed form would take
the file past it is stored instead in part files ``<name>.part<k>.npz`` (k = 1, 2, ...), split along its first axis
long enough for the pieces: piece i along axis a is ``<key>#<a>.<i>``.  ``load`` joins the pieces again and returns
every array under its own key.

TEST INFRASTRUCTURE ONLY.
"""
import io
import os

import numpy as np

LIMIT = 1 << 20


class Fixture(dict):
    """The arrays of one fixture by key; ``files`` lists the keys, as on the ``NpzFile`` that ``np.load`` returns."""

    @property
    def files(self):
        return list(self)


def load(golden_dir: str, name: str) -> Fixture:
    rec = Fixture(np.load(os.path.join(golden_dir, name + ".npz")))
    k = 1
    while os.path.exists(os.path.join(golden_dir, f"{name}.part{k}.npz")):
        rec.update(np.load(os.path.join(golden_dir, f"{name}.part{k}.npz")))
        k += 1
    pieces = {}
    for key in [key for key in rec if "#" in key]:
        base, where = key.rsplit("#", 1)
        axis, i = (int(v) for v in where.split("."))
        pieces.setdefault((base, axis), {})[i] = rec.pop(key)
    for (base, axis), parts in pieces.items():
        rec[base] = np.concatenate([parts[i] for i in sorted(parts)], axis=axis)
    return rec


def _compressed_size(arrays: dict) -> int:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return len(buf.getvalue())


def save(golden_dir: str, name: str, rec: dict) -> None:
    """``np.savez_compressed(<name>.npz, **rec)``, with the arrays too large for one file split into part files."""
    budget = LIMIT * 7 // 8                 # headroom for the zip directory and the arrays that stay in the main file
    main, parts = {}, []
    for key, v in rec.items():
        v = np.asarray(v)
        size = _compressed_size({key: v})
        if size <= budget // 8:
            main[key] = v
            continue
        n = -(-size // budget)
        axis = next((a for a, extent in enumerate(v.shape) if extent >= n), None)
        if axis is None:
            raise ValueError(f"{name}: {key} {v.shape} has no axis to split into {n} pieces")
        parts += [{f"{key}#{axis}.{i}": p} for i, p in enumerate(np.array_split(v, n, axis=axis))]
    for k in range(1, 1 << 10):             # part files of an earlier write of the same fixture
        stale = os.path.join(golden_dir, f"{name}.part{k}.npz")
        if not os.path.exists(stale):
            break
        os.remove(stale)
    files = [(os.path.join(golden_dir, name + ".npz"), main)]
    files += [(os.path.join(golden_dir, f"{name}.part{k}.npz"), p) for k, p in enumerate(parts, 1)]
    for path, arrays in files:
        np.savez_compressed(path, **arrays)
        if os.path.getsize(path) >= LIMIT:
            raise ValueError(f"{path}: {os.path.getsize(path)} bytes, over the {LIMIT}-byte limit of a committed fixture")
