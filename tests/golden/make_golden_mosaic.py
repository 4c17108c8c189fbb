#!/usr/bin/env python
"""Record what the REAL reference computes for demosaicing: its `Inpainting(channels, img_dim, missing_indices, device)`
(functions/svd_operators.py:324-439) built with the entries a colour filter array does NOT sample, at d = 16, B = 2, for
the `rggb` and `xtrans` arrays.  Run once where the reference tree is present (DDNM_REFERENCE_ROOT):

    python tests/golden/make_golden_mosaic.py

Writes tests/golden/mosaic.npz: per array `<name>_missing` (the indices handed to the reference, from the plain-loop
construction of tests/test_mosaic_host.py), `_A`, `_A_pinv`, `_Vt`, `_V`, `_U`, `_Ut`, `_add_zeros`, `_singulars`, `_At`,
`_A_pinv_eta` (eta = 0.3) and `_Lambda_<k>` / `_Lambda_noise_<k>` at sigma_y = 0.4, eta = 0.85 for the two (a, sigma_t) pairs
of PLUS_CASES, one on each side of the threshold sigma_t = a * sigma_y.  The inputs are `golden_inputs()` of that module.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests.test_mosaic_host import (ETA, ETA_REG, GOLDEN_B, GOLDEN_D, GOLDEN_PATTERNS, PLUS_CASES, SIGMA_Y,  # noqa: E402
                                    golden_inputs, numpy_cfa, numpy_tables)


def main():
    R = ref_import.load().svd_operators
    d, B = GOLDEN_D, GOLDEN_B
    inp = golden_inputs(d, B)
    out = {}
    for name in GOLDEN_PATTERNS:
        _, _, missing = numpy_tables(numpy_cfa(name), d)
        ref = R.Inpainting(3, d, torch.from_numpy(missing), "cpu")
        put = lambda key, t: out.__setitem__(f"{name}_{key}", t.reshape(B, -1).numpy().copy())      # noqa: E731
        out[f"{name}_missing"] = missing
        out[f"{name}_singulars"] = ref.singulars().numpy().copy()
        put("A", ref.A(inp["x"].clone()))
        put("A_pinv", ref.A_pinv(inp["y"].clone()))
        put("Vt", ref.Vt(inp["x"].clone()))
        put("V", ref.V(inp["v"].clone()))
        put("U", ref.U(inp["y"].clone()))
        put("Ut", ref.Ut(inp["y"].clone()))
        put("add_zeros", ref.add_zeros(inp["y"].clone()))
        put("At", ref.At(inp["y"].clone()))
        put("A_pinv_eta", ref.A_pinv_eta(inp["y"].clone(), ETA_REG))
        for k, (a, sigma_t) in enumerate(PLUS_CASES):
            put(f"Lambda_{k}", ref.Lambda(inp["v"].clone(), a, SIGMA_Y, sigma_t, ETA))
            put(f"Lambda_noise_{k}", ref.Lambda_noise(inp["v"].clone(), a, SIGMA_Y, sigma_t, ETA, inp["eps"].clone()))
    path = os.path.join(HERE, "mosaic.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
