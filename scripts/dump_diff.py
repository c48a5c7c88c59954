"""|difference| between `bench.py --dump-outputs` directories, pair by pair.

    python scripts/dump_diff.py label=DIR [label=DIR ...]

Prints, for every pair of directories, each logged scalar's |a - b| and max / mean |a - b| of the two state vectors.  Pairs
of runs of ONE tree give the run-to-run spread (fp32 atomics) that a pair across two trees is to be read against."""
import itertools
import os
import sys

import numpy as np


def main(specs):
    runs = [s.split("=", 1) for s in specs]
    for (la, da), (lb, db) in itertools.combinations(runs, 2):
        parts = []
        for f in sorted(os.listdir(da)):
            if not f.endswith(".npy") or not os.path.exists(os.path.join(db, f)):
                continue
            a, b = np.load(os.path.join(da, f)), np.load(os.path.join(db, f))
            d = np.abs(a - b)
            parts.append(f"{f[:-4]} {float(d):.1e}" if d.ndim == 0 else f"{f[:-4]} max {d.max():.1e} mean {d.mean():.1e}")
        print(f"{la} - {lb}: " + " | ".join(parts))


if __name__ == "__main__":
    main(sys.argv[1:])
