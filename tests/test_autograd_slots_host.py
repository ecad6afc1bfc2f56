"""The positional hand-off of the per-Gaussian gradient buffers: rasterizer._GradSet.SLOTS against include/lightgaussian.h.

The three backward entry points take their nine dL_d* output pointers by position, and the Python side passes `_GradSet.ptrs()`
in SLOTS order: a slot out of place would be a silently wrong gradient, not an error.  No GPU needed.
"""
import os
import re

import pytest

import common
from lightgaussian_amd import rasterizer

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")
INPUTS_AND_EXTRAS = {"dL_dcolor", "dL_dout", "dL_dalpha", "dL_dfeatures"}      # (the gradients that come IN, and lg_backward_features' own row)


def _gradient_parameters(function):
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    params = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % function, text)
    assert params, f"{function} not declared in include/lightgaussian.h"
    names = [p.split()[-1].lstrip("*") for p in params.group(1).split(",")]
    return [n[len("dL_d"):] for n in names if n.startswith("dL_d") and n not in INPUTS_AND_EXTRAS]


@pytest.mark.parametrize("function", ["lg_backward", "lg_backward_chunked", "lg_backward_features"])
def test_slot_order_is_the_headers(function):
    declared = _gradient_parameters(function)
    assert len(declared) == 9
    assert list(rasterizer._GradSet.SLOTS) == declared


def test_hook_names_map_onto_their_slots():
    """What set_grad_chunk_hook's callback receives: the rasterizer's argument names on the literal path, GaussianModel's parameter
    names on the fused one (parallel.OverlappedGradAllReduce looks its buckets up by them)."""
    assert dict(rasterizer._GradSet.HOOK_NAMES[False]) == {
        "means3D": "means3D", "shs": "shs", "colors_precomp": "colors", "opacities": "opacity", "scales": "scales", "rotations": "rotations",
        "cov3D_precomp": "cov3D"}
    assert dict(rasterizer._GradSet.HOOK_NAMES[True]) == {
        "_xyz": "means3D", "_features_dc": "shs", "_features_rest": "shs_rest", "_opacity": "opacity", "_scaling": "scales",
        "_rotation": "rotations"}
    for names in rasterizer._GradSet.HOOK_NAMES.values():
        assert {slot for _name, slot in names} <= set(rasterizer._GradSet.SLOTS)
