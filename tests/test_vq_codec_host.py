"""CPU: the VecTree model codec (lightgaussian_amd/vectree.py) against tests/golden/reference_vq_codec.npz, which
tests/golden/make_golden_vq_codec.py produced with the reference's own fully_vq_reformat (writer) and load_vqgaussian (reader):
pack() reproduces every stored array byte for byte, unpack() the dequantised table bit for bit, and CompressedGaussians
(on the CPU; its colour kernel is covered by tests/test_gpu_vq_render.py) the tensors GaussianModel.load_vq builds."""
import os

import numpy as np
import pytest
import torch

import common
from lightgaussian_amd import vectree

GOLD = os.path.join(common.ROOT, "tests", "golden", "reference_vq_codec.npz")
CASES = ("deg2_k32", "deg3_k64", "deg2_k8192", "deg3_all_vq")
ARRAYS = ("vq_indexs", "codebook", "non_vq_mask", "non_vq_feats", "other_attribute", "xyz")


def _case(name):
    z = np.load(GOLD)
    N, C, K, d = (int(v) for v in z[f"{name}_meta"])
    stored = {"metadata": {"input_pc_num": N, "input_pc_dim": C, "codebook_size": K, "codebook_dim": d}}
    for a in ARRAYS:
        stored[a] = z[f"{name}_{a}"]
    feats = z[f"{name}_in_feats"].astype(np.float32)
    mask = np.unpackbits(z[f"{name}_in_mask"])[:N].astype(bool)
    ind = z[f"{name}_in_indices"].astype(np.int64)
    return stored, feats, mask, ind, z[f"{name}_table"].astype(np.float32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_packed_equal(p, q):
    assert p["metadata"] == q["metadata"] and all(type(v) is int for v in p["metadata"].values())
    for a in ARRAYS:
        assert _same(np.asarray(p[a]), np.asarray(q[a])), a


def test_the_golden_file_holds_the_cases_the_format_needs():
    seen_bits, dims = set(), set()
    for name in CASES:
        stored, feats, mask, ind, table = _case(name)
        m = stored["metadata"]
        assert m["input_pc_num"] % 8 != 0
        seen_bits.add(m["codebook_size"].bit_length() - 1)
        dims.add(m["codebook_dim"])
    assert 13 in seen_bits and any(b % 8 and 8 % b for b in seen_bits) and dims == {27, 48}
    assert _case("deg3_all_vq")[2].sum() == 0 and _case("deg3_all_vq")[0]["non_vq_feats"].shape == (0, 48)
    N = _case("deg2_k32")[0]["metadata"]["input_pc_num"]
    assert _case("deg2_k32")[2].sum() == int(N * (1 - 0.6))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("as_torch", [False, True])
def test_pack_reproduces_the_reference_files_byte_for_byte(name, as_torch):
    stored, feats, mask, ind, _ = _case(name)
    cb = stored["codebook"].astype(np.float32)
    args = (feats, mask, cb, ind)
    if as_torch:
        args = tuple(torch.from_numpy(a) for a in args)
    _assert_packed_equal(vectree.pack(*args), stored)


@pytest.mark.parametrize("name", CASES)
def test_unpack_of_a_reference_directory_is_the_reference_table(name, tmp_path):
    stored, _, _, _, table = _case(name)
    # the directory as the reference leaves it: numpy.savez_compressed per file, positional arrays, the dict pickled
    for a in ARRAYS:
        np.savez_compressed(tmp_path / f"{a}.npz", stored[a])
    np.savez_compressed(tmp_path / "metadata.npz", metadata=stored["metadata"])
    got = vectree.unpack(vectree.load(str(tmp_path)), "cpu")
    assert got.dtype == torch.float32 and tuple(got.shape) == table.shape
    assert np.array_equal(got.numpy().view(np.uint32), table.view(np.uint32))
    assert not got[:, 3:6].any()


@pytest.mark.parametrize("name", CASES)
def test_save_load_round_trip_and_directory_layout(name, tmp_path):
    stored, feats, mask, ind, _ = _case(name)
    packed = vectree.pack(feats, mask, stored["codebook"], ind)
    folder = str(tmp_path / "extreme_saving")
    vectree.save(folder, packed)
    assert sorted(os.listdir(folder)) == sorted(f"{a}.npz" for a in ARRAYS + ("metadata",))
    for a in ARRAYS:
        with np.load(os.path.join(folder, f"{a}.npz")) as z:
            assert z.files == ["arr_0"]
    with np.load(os.path.join(folder, "metadata.npz"), allow_pickle=True) as z:
        assert z.files == ["metadata"] and z["metadata"].item() == stored["metadata"]
    _assert_packed_equal(vectree.load(folder), packed)


def test_float32_way_keeps_rows_and_attributes_wide():
    stored, feats, mask, ind, _ = _case("deg2_k32")
    p = vectree.pack(feats, mask, stored["codebook"], ind, vq_way="float")
    assert p["non_vq_feats"].dtype == np.float32 and p["other_attribute"].dtype == np.float32 and p["codebook"].dtype == np.float16
    assert np.array_equal(p["non_vq_feats"], feats[mask, 6:33]) and np.array_equal(p["other_attribute"], feats[:, -8:])
    assert np.array_equal(vectree.unpack(p)[:, -8:].numpy(), feats[:, -8:])
    with pytest.raises(ValueError):
        vectree.CompressedGaussians.from_packed(p, "cpu")


def test_malformed_input_is_rejected():
    stored, feats, mask, ind, _ = _case("deg2_k32")
    cb = stored["codebook"].astype(np.float32)
    with pytest.raises(ValueError):
        vectree.pack(feats, mask, cb[:24], ind % 24)                          # K not a power of two
    with pytest.raises(ValueError):
        vectree.pack(feats, mask, np.zeros((131072, 27), np.float32), ind)    # K > 65536
    with pytest.raises(ValueError):
        vectree.pack(feats[:, :-1], mask, cb, ind)                            # wrong column count
    with pytest.raises(ValueError):
        vectree.pack(feats, mask, np.zeros((32, 30), np.float32), ind)        # ... on the codebook's side
    with pytest.raises(ValueError):
        vectree.pack(feats, mask[:-1], cb, ind)                               # mask length
    with pytest.raises(ValueError):
        vectree.pack(feats, mask, cb, ind[:-3])                               # index length
    with pytest.raises(ValueError):
        vectree.pack(feats, mask, cb, ind + 32 * (~mask))                     # a code beyond the codebook
    for key, bad in (("vq_indexs", stored["vq_indexs"][:-1]), ("non_vq_mask", stored["non_vq_mask"][:-1]),
                     ("non_vq_feats", stored["non_vq_feats"][:-1]), ("codebook", stored["codebook"][:16]),
                     ("other_attribute", stored["other_attribute"][:-1]), ("xyz", stored["xyz"][:, :2])):
        broken = dict(stored)
        broken[key] = bad
        for fn in (lambda p: vectree.unpack(p), lambda p: vectree.CompressedGaussians.from_packed(p, "cpu")):
            with pytest.raises(ValueError):
                fn(broken)
    broken = dict(stored, metadata=dict(stored["metadata"], codebook_size=48))
    with pytest.raises(ValueError):
        vectree.unpack(broken)
    with pytest.raises(ValueError):
        vectree.unpack({k: v for k, v in stored.items() if k != "xyz"})
    with pytest.raises(RuntimeError):
        vectree.quantize_model(torch.zeros(10, 41), torch.ones(10))          # GPU only


@pytest.mark.parametrize("name", CASES)
def test_compressed_gaussians_against_the_load_vq_column_rule(name):
    stored, feats, mask, ind, table = _case(name)
    N, K, d = stored["metadata"]["input_pc_num"], stored["metadata"]["codebook_size"], stored["metadata"]["codebook_dim"]
    cg = vectree.CompressedGaussians.from_packed(stored, "cpu")
    M = d // 3
    assert cg.max_sh_degree == {27: 2, 48: 3}[d] and cg.active_sh_degree == cg.max_sh_degree and cg.num == N
    # slot: the code of a VQ row, K + rank of a non-VQ row; the table rows behind it are the Gaussian's SH row
    slot = cg.slot
    assert slot.dtype == torch.uint32 and tuple(slot.shape) == (N,)
    s = slot.view(torch.int32).long().numpy()
    assert np.array_equal(s[~mask], ind[~mask]) and np.array_equal(s[mask], K + np.arange(int(mask.sum())))
    n_nv = int(mask.sum())
    stride = cg.row_stride
    assert stride % 16 == 0 and stride == {27: 64, 48: 96}[d] and cg.rows.dtype == torch.float16
    assert tuple(cg.rows.shape) == (K + n_nv, stride // 2) and cg.rows.is_contiguous() and cg.rows.data_ptr() % 16 == 0
    assert np.array_equal(cg.rows[s, :d].float().numpy(), table[:, 6:6 + d]) and not cg.rows[:, d:].any()
    assert cg.nbytes() == N * (12 + 32 + 4) + (K + n_nv) * stride
    # the getters: what GaussianModel's return after load_vq (activations of the float16 -> float32 attributes)
    t = torch.from_numpy(table)
    assert torch.equal(cg.get_xyz, t[:, 0:3]) and cg.get_xyz.dtype == torch.float32
    # (load_vq makes each parameter a tensor of its own, i.e. contiguous, before the getters activate it)
    assert torch.equal(cg.get_opacity, torch.sigmoid(t[:, -8:-7].contiguous())) and torch.equal(cg.get_scaling, torch.exp(t[:, -7:-4].contiguous()))
    assert torch.equal(cg.get_rotation, torch.nn.functional.normalize(t[:, -4:].contiguous()))
    assert not any(x.requires_grad for x in (cg.get_xyz, cg.get_opacity, cg.get_scaling, cg.get_rotation))
    # to_dense(): scene/gaussian_model.py:420-461 applied to the reference's table
    dense = cg.to_dense()
    sh_rest = 3 * M - 3
    assert torch.equal(dense._xyz, t[:, 0:3])
    assert torch.equal(dense._features_dc, t[:, 6:9].reshape(N, 3, 1).transpose(1, 2).contiguous())
    assert torch.equal(dense._features_rest, t[:, 9:9 + sh_rest].reshape(N, 3, sh_rest // 3).transpose(1, 2).contiguous())
    assert torch.equal(dense._opacity, t[:, -8:-7]) and torch.equal(dense._scaling, t[:, -7:-4]) and torch.equal(dense._rotation, t[:, -4:])
    assert tuple(dense._features_dc.shape) == (N, 1, 3) and tuple(dense._features_rest.shape) == (N, M - 1, 3)
    assert dense.max_sh_degree == cg.max_sh_degree and dense.active_sh_degree == cg.active_sh_degree
    assert torch.equal(dense.get_opacity, cg.get_opacity) and torch.equal(dense.get_rotation, cg.get_rotation) and torch.equal(dense.get_scaling, cg.get_scaling)
    with pytest.raises(RuntimeError):
        cg.colors(torch.zeros(3))                                             # the colour kernel is HIP only, no fallback


def test_compressed_render_refuses_the_python_side_alternates():
    from lightgaussian_amd import synthetic as syn
    from lightgaussian_amd.gaussian_renderer import render, render_compressed
    cg = vectree.CompressedGaussians.from_packed(_case("deg2_k32")[0], "cpu")
    cam = syn.orbit_camera(0, 4, 64, 48)
    for pipe in (syn.PipelineParams(convert_SHs_python=True), syn.PipelineParams(compute_cov3D_python=True)):
        for fn in (render, render_compressed):
            with pytest.raises(NotImplementedError, match="to_dense"):
                fn(cam, cg, pipe, torch.zeros(3))
