#!/usr/bin/env python3
"""Generate tests/golden/focal_binary.npz: 301 one-logit inputs with 0/1 float targets and what the REFERENCE's
`utils.FocalLoss_binary(focusing_param, balance_param, reduction='none')` (utils.py:695-724) makes of them in fp64, for
(gamma 5, balance 0.9), its defaults, and (gamma 2, balance 0.25), those of Lin et al.

Runs only in the build container (needs /root/reference).  Imports the reference's utils.py *unmodified*; the third-party
packages it imports at module level but which are not installed here are satisfied by the placeholders under
tests/golden/_standin (the class uses none of them).  The tests read the file and need no reference.

    python tests/golden/make_golden_focal.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MTMC_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, "_standin"))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import utils as ref_utils  # noqa: E402  (the reference, unmodified)

SETTINGS = [(5, 0.9), (2, 0.25)]


def inputs():
    g = torch.Generator().manual_seed(20240)
    x = torch.randn(301, generator=g) * 3
    t = (torch.rand(301, generator=g) < 0.3).float()
    x[5::29], x[7::31], x[::17] = 80.0, -80.0, 0.0             # confident rows of either sign and ties, under both targets
    t[5], t[7], t[0] = 1.0, 1.0, 1.0
    t[34], t[38], t[17] = 0.0, 0.0, 0.0
    return x, t


def main():
    x, t = inputs()
    out = {"x": x.numpy(), "t": t.numpy(), "settings": np.array(SETTINGS, dtype=np.float64), "torch": np.array(torch.__version__)}
    for gamma, balance in SETTINGS:
        rows = ref_utils.FocalLoss_binary(gamma, balance, reduction="none")(x.double(), t.double())
        assert rows.dtype == torch.float64 and rows.shape == x.shape and torch.isfinite(rows).all()
        out[f"rows_g{gamma}"] = rows.numpy()
    path = os.path.join(HERE, "focal_binary.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {x.numel()} rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
