"""Writes tests/golden/sensitivity_blocks.npz: the per-Gaussian 6 x 6 blocks of the golden scene of tests/sensitivity_common.py by the
project's own dense twin (J^T J of its Jacobian with respect to (means3D, scales), colours constant), in float64 and in float32, per view
and summed -- so that no GPU test pays for the twin (the float64 pass takes some ten seconds on a CPU).

    python tests/golden/make_golden_sensitivity.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sensitivity_common as sc  # noqa: E402
import torch  # noqa: E402


def main():
    g, colors, cams = sc.golden_scene()
    out = {}
    for dd, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        views = np.stack([sc.twin_blocks(sc.scene_kw(g, colors, cam, 32, 32, sc.GOLDEN_BG), dd) for cam in cams])
        out[f"views_{name}"] = sc.tri(views)                 # [2, 24, 21]
        out[f"sum_{name}"] = sc.tri(views.sum(0))            # [24, 21]
    out["views"] = np.asarray(sc.GOLDEN_VIEWS, np.int32)
    np.savez_compressed(sc.GOLDEN, **out)
    ref, r32 = sc.full(out["sum_f64"]), sc.full(out["sum_f32"])
    ld, ld32 = sc.logdet(ref), sc.logdet(r32)
    print(f"{sc.GOLDEN}: {os.path.getsize(sc.GOLDEN)} bytes")
    print(f"positive definite {int(np.isfinite(ld).sum())} of {len(ld)}, kappa <= {sc.kappa(ref).max():.3g}, log det {ld.min():.3g} .. {ld.max():.3g}")
    print(f"float32 twin: entries within {sc.scaled_err(r32, ref).max():.3g}, log det within {np.abs(ld32 - ld).max():.3g}")


if __name__ == "__main__":
    main()
