"""Golden stage times of the fixed-grid methods: the times the REFERENCE's euler, midpoint, heun2, heun3 and rk4 hand to
`func` on grids chosen for their edges (tests/_fixed_grid_cases.py: a negative time, steps that end and start on zero, a
float32 subnormal, the smallest normal, a one-ulp interval, a time with x + 1 == x in float32, double times that are no
float32 numbers), for every (state type, grid type, perturb, direction).  The field records the time and returns zeros.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fixed_grid.py      (build container only: /root/reference)

-> tests/golden/fixed_grid_times.npz: the grids and the recorded times, nothing else.  Pins
`OracleKernels.grid_advance_stages` / `grid_advance` (tests/test_fixed_grid_oracle.py), which in turn is what the kernels
behind tdeq_grid_advance_stages / tdeq_grid_advance are compared with bit for bit on the GPU
(tests/test_fixed_grid_kernels_gpu.py).  The archive is written with fixed member dates: a second run gives the same bytes.
"""
import io
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(1, os.path.dirname(HERE))

from torchdiffeq import odeint  # noqa: E402

from _fixed_grid_cases import DT, GRIDS, METHODS, golden_cases  # noqa: E402

torch.set_num_threads(1)


class SeenTimes:
    """The user's `func`: records the time it is called with, returns zeros."""

    def __init__(self):
        self.seen = []

    def __call__(self, t, y):
        self.seen.append(t.detach().clone())
        return torch.zeros_like(y)


def write_npz(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01, in sorted order: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    arrays = {"grid_" + name: np.asarray(g, dtype=np.float64) for name, g in GRIDS.items()}
    for key, gname, state, gtype, perturb, rev in golden_cases():
        t = torch.tensor(GRIDS[gname], dtype=torch.float64).to(DT[gtype])
        assert t.double().tolist() == list(GRIDS[gname])            # the grid type holds every entry exactly
        if rev:
            t = t.flip(0)
        y0 = torch.zeros(3, dtype=DT[state])
        for method in METHODS:
            func = SeenTimes()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sol = odeint(func, y0, t, method=method, options=dict(perturb=perturb))
            assert sol.shape == (len(t), 3) and not bool(sol.any())  # the reference accepts the grid
            assert all(s.dtype == DT[state] and s.dim() == 0 for s in func.seen), (key, method)
            times = torch.stack(func.seen).numpy()
            assert times.size % (len(t) - 1) == 0
            arrays["{}_{}".format(method, key)] = times
    path = os.path.join(HERE, "fixed_grid_times.npz")
    write_npz(path, arrays)
    print("fixed_grid_times.npz", len(arrays), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
