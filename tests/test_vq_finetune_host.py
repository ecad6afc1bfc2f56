"""No GPU: the C ABI of the compressed model's backward (declared, bound, ABI still 7) and the host side of
vectree.TrainableCompressed -- repack() of an untouched trainable() is the dict it came from, and nothing runs on CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import common
import vq_finetune_common as fc
from lightgaussian_amd import _lib, vectree

NEW = ("lg_vq_code_index_bytes", "lg_vq_code_index", "lg_vq_colors_bwd")


def test_the_new_entry_points_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(common.ROOT, "include", "lightgaussian.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW + ("lg_vq_code_index_scratch_bytes", "lg_vq_colors_bwd_scratch_bytes"):
        assert re.search(r"^\s*(?:int|size_t)\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define\s+LG_ABI_VERSION\s+7\b", src) and _lib.ABI_VERSION == 7 and lib.lg_abi_version() == 7
    assert len(lib.lg_vq_colors_bwd.argtypes) == 17 and len(lib.lg_vq_code_index.argtypes) == 6
    # the size queries are pure functions of their arguments: linear in N, 0 for what the calls refuse
    a, b = lib.lg_vq_code_index_bytes(1000, 8192), lib.lg_vq_code_index_bytes(3000000, 8192)
    assert 0 < a < b and b >= 4 * 3000000 + 8 * 8192 and b < 5 * 3000000 + 16 * 8192
    assert lib.lg_vq_code_index_bytes(-1, 16) == 0 and lib.lg_vq_code_index_bytes(10, 0) == 0
    assert lib.lg_vq_code_index_scratch_bytes(3000000, 8192) >= 16 * 3000000
    assert lib.lg_vq_colors_bwd_scratch_bytes(3000000, 16, 8192) >= (3000000 // 256 + 8192) * 48 * 4
    assert lib.lg_vq_colors_bwd_scratch_bytes(10, 17, 16) == 0
    # refused before any launch: a bad degree, a table shorter than the codebook, a missing buffer
    assert lib.lg_vq_colors_bwd(10, 16, 4, 16, 20, *([None] * 4), 96, *([None] * 5), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_vq_colors_bwd(10, 16, 3, 16, 8, *([None] * 4), 96, *([None] * 5), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert lib.lg_vq_colors_bwd(10, 16, 3, 16, 20, *([None] * 4), 96, *([None] * 5), 0, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert b"missing buffer" in lib.lg_last_error()
    assert lib.lg_vq_code_index(10, 16, None, None, None, None) == _lib.LG_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("N,deg,how", [(3001, 3, 0.6), (2113, 2, "hand"), (515, 2, 1.0), (515, 3, 0.0)])
def test_repack_of_an_untouched_trainable_is_the_input(N, deg, how, tmp_path):
    packed = fc.packed_case(N, deg, how)
    cg = vectree.CompressedGaussians.from_packed(packed, "cpu")
    for params in (("rows",), fc.ALL_PARAMS, ()):
        tc = cg.trainable(params)
        assert isinstance(tc, vectree.TrainableCompressed) and isinstance(tc, vectree.CompressedGaussians)
        assert len(tc.parameters()) == len(params) and all(isinstance(p, torch.nn.Parameter) for p in tc.parameters())
        d, K = tc.sh_dim, tc.codebook_size
        assert tc._rows.dtype == torch.float32 and tuple(tc._rows.shape) == (K + int((cg._slot >= K).sum()), d)
        assert isinstance(tc._rows, torch.nn.Parameter) == ("rows" in params)
        assert isinstance(tc._opacity, torch.nn.Parameter) == ("opacity" in params) and tuple(tc._rotation.shape) == (N, 4)
        again = tc.repack()
        assert fc.np_equal_packed(again, packed)
    vectree.save(str(tmp_path / "m"), again)
    loaded = vectree.load(str(tmp_path / "m"))
    assert fc.np_equal_packed(loaded, packed)
    assert torch.equal(vectree.unpack(loaded), vectree.unpack(packed))
    # a changed master shows in the repacked rows only, rounded to float16; the table the forward reads follows sync_rows()
    tc = cg.trainable(("rows",))
    with torch.no_grad():
        tc._rows[0, 0] += 0.25
    changed = tc.repack()
    assert changed["codebook"][0, 0] == np.float16(np.float32(packed["codebook"][0, 0]) + np.float32(0.25))
    assert np.array_equal(changed["vq_indexs"], packed["vq_indexs"]) and np.array_equal(changed["non_vq_feats"], packed["non_vq_feats"])
    tc.sync_rows()
    assert tc.rows[0, 0].item() == float(changed["codebook"][0, 0]) and not tc.rows[:, d:].any()
    assert cg.rows[0, 0].item() == float(packed["codebook"][0, 0])        # the source model keeps its own table
    with pytest.raises(ValueError):
        cg.trainable(("rows", "colour"))


def test_no_cpu_fallback():
    cg = vectree.CompressedGaussians.from_packed(fc.packed_case(515, 2, 0.6), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cg.colors(torch.zeros(3))
    tc = cg.trainable()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tc.colors(torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tc._build_index()
    assert tc._index is None
