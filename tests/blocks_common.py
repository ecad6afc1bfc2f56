"""Shared by tests/test_blocks_host.py and tests/test_gpu_blocks.py (test infrastructure): the g++ build of
tests/cpu_harness/lg_blocks_harness.cpp, the two input sets of DESIGN section 10.15, and the float64 twin of the touch rule.

Inputs come from mesh_common: FIRST = sphere_views(6) under volume_spec((24, 20, 16)) (voxel 3/23, trunc 4 voxels; 49 blocks with
coordinates -1 .. 2), SECOND = sphere_views(6, sizes=((70, 45), (160, 90))) under volume_spec((48, 40, 32)) (151 blocks).

The twin.  twin_touch() is the touch rule in numpy float64 on the float32 inputs: per pixel its lattice box, whether it is skipped, and
whether an end of the box lies within NEAR (1e-3 voxel) of a block face, where float32 may decide otherwise."""
import ctypes as C

import numpy as np

import common
import mesh_common as mc
from common import bits, f32, ptr  # noqa: F401

NEAR = 1e-3
BIAS = 1 << 20
FIRST_DIMS, SECOND_DIMS = (24, 20, 16), (48, 40, 32)
SECOND_SIZES = ((70, 45), (160, 90))


def harness():
    P, F, I, L = C.c_void_p, C.c_float, C.c_int, C.c_int64
    return common.build_harness("blocks", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_blocks_touch": (L, [P, F, F, I, P, P, P, P, P, L, P, P, P]),
        "h_blocks_integrate": (None, [I, P, P, F, F, P, P, P, I, P, P, P, P, P, P]),
        "h_blocks_mesh": (None, [I, P, P, F, P, P, P, F, F, P, P, P, P, P, P, P])})


def input_set(which):
    """(origin, voxel, trunc, views) of the first or second input set."""
    if which == 0:
        return mc.volume_spec(FIRST_DIMS) + (mc.sphere_views(6),)
    return mc.volume_spec(SECOND_DIMS) + (mc.sphere_views(6, sizes=SECOND_SIZES),)


def keys_of(coords):
    c = np.asarray(coords, np.int64).reshape(-1, 3) + BIAS
    return (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def coords_of(keys):
    k = np.asarray(keys, np.int64)
    return np.stack([(k & 0x1FFFFF) - BIAS, ((k >> 21) & 0x1FFFFF) - BIAS, ((k >> 42) & 0x1FFFFF) - BIAS], axis=1)


def _view_args(views, alpha_min, depth_max, z_min, use_alpha, color):
    n = len(views)
    wh = np.array([[v["W"], v["H"]] for v in views], np.int32).reshape(-1, 2)
    cam = np.array([[v["tanfov"][0], v["tanfov"][1], depth_max, z_min, alpha_min] for v in views], np.float32).reshape(-1, 5)
    vms = np.ascontiguousarray(np.stack([v["vm"] for v in views]) if n else np.zeros((0, 16)), np.float32)
    arr = lambda key, on=True: (C.c_void_p * max(n, 1))(*[v[key].ctypes.data if on else None for v in views])  # noqa: E731
    return wh, cam, vms, arr("depth"), arr("color", color), arr("alpha", use_alpha)


# ---- the harness --------------------------------------------------------------------------------------------------------------------
def harness_touch(origin, voxel, trunc, views, *, use_alpha=False, alpha_min=0.5, depth_max=0.0, pixels=False):
    """(keys ascending, skipped pixels[, per-pixel (status, lo[3], n[3])]) of the harness."""
    wh, cam, vms, depth, _c, alpha = _view_args(views, alpha_min, depth_max, 0.05, use_alpha, False)
    npix = int(sum(v["W"] * v["H"] for v in views))
    room = 64 * max(npix, 1)
    keys = np.zeros(min(room, 1 << 22), np.int64)
    pix = np.zeros((npix, 7), np.int32) if pixels else None
    stats = np.zeros(2, np.int64)
    n = harness().h_blocks_touch(ptr(f32(np.array(origin))), voxel, trunc, len(views), ptr(wh), ptr(cam), ptr(vms), depth, alpha, len(keys), ptr(keys), ptr(pix), ptr(stats))
    assert n <= len(keys)
    return (keys[:n].copy(), int(stats[1])) + ((pix,) if pixels else ())


def fresh_pools(n, color=True):
    return (np.ones((n, 8, 8, 8), np.float32), np.zeros((n, 8, 8, 8), np.float32), np.zeros((n, 8, 8, 8, 3), np.float32) if color else None)


def harness_integrate(keys, origin, voxel, trunc, state, views, *, use_alpha=False, alpha_min=0.5, depth_max=0.0, z_min=0.05):
    """state = (tsdf, weight, color or None) [n,8,8,8(,3)] is copied; returns the new state."""
    keys = np.ascontiguousarray(keys, np.int64)
    tsdf, weight = state[0].copy(), state[1].copy()
    color = None if state[2] is None else state[2].copy()
    wh, cam, vms, depth, image, alpha = _view_args(views, alpha_min, depth_max, z_min, use_alpha, color is not None)
    harness().h_blocks_integrate(len(keys), ptr(keys), ptr(f32(np.array(origin))), voxel, trunc, ptr(tsdf), ptr(weight), ptr(color), len(views), ptr(wh), ptr(cam), ptr(vms),
                                 depth, image, alpha)
    return tsdf, weight, color


def harness_extract(keys, tsdf, weight, color, origin, voxel, iso=0.0, min_weight=1.0):
    """dict(vertices, faces, colors, cell_of_face, used [6,16], nbr [n,8]) of the harness."""
    keys = np.ascontiguousarray(keys, np.int64)
    n = len(keys)
    tsdf, weight, color = f32(tsdf), f32(weight), f32(color)
    o = f32(np.array(origin))
    counts = np.zeros(2, np.int64)
    harness().h_blocks_mesh(n, ptr(keys), ptr(o), voxel, ptr(tsdf), ptr(weight), ptr(color), iso, min_weight, ptr(counts), None, None, None, None, None, None)
    nv, nf = int(counts[0]), int(counts[1])
    out = dict(vertices=np.full((nv, 3), np.nan, np.float32), faces=np.full((nf, 3), -1, np.int32), colors=None if color is None else np.full((nv, 3), np.nan, np.float32),
               cell_of_face=np.full(nf, -1, np.int64), used=np.zeros((6, 16), np.int64), nbr=np.full((n, 8), -2, np.int32))
    again = np.zeros(2, np.int64)
    harness().h_blocks_mesh(n, ptr(keys), ptr(o), voxel, ptr(tsdf), ptr(weight), ptr(color), iso, min_weight, ptr(again), ptr(out["vertices"]), ptr(out["colors"]),
                            ptr(out["faces"]), ptr(out["cell_of_face"]), ptr(out["used"]), ptr(out["nbr"]))
    assert np.array_equal(again, counts)
    return out


# ---- the float64 twin of the touch rule -----------------------------------------------------------------------------------------------
def twin_touch(origin, voxel, trunc, views, *, use_alpha=False, alpha_min=0.5, depth_max=0.0, grow=0.0):
    """Per pixel of all views, back to back: dict(take [N] bool: passes the gates and is not skipped, skipped [N] bool, lo, hi [N,3] int64
    block ranges, near [N] bool).  grow: the boxes enlarged by that many voxels on every side."""
    o = np.asarray(origin, np.float32).astype(np.float64)
    vx, tr = float(np.float32(voxel)), float(np.float32(trunc))
    out = dict(take=[], skipped=[], lo=[], hi=[], near=[])
    for v in views:
        W, H = v["W"], v["H"]
        tx, ty = float(np.float32(v["tanfov"][0])), float(np.float32(v["tanfov"][1]))
        vm = v["vm"].astype(np.float64).reshape(4, 4)
        d = v["depth"].astype(np.float64)
        ok = (d > 0) & np.isfinite(d)
        if depth_max > 0:
            ok &= ~(d > float(np.float32(depth_max)))
        if use_alpha:
            ok &= ~(v["alpha"].astype(np.float64) < float(np.float32(alpha_min)))
        rx = np.broadcast_to((((2 * np.arange(W) + 1) / W - 1) * tx)[None, :], (H, W))
        ry = np.broadcast_to((((2 * np.arange(H) + 1) / H - 1) * ty)[:, None], (H, W))
        r = np.stack([rx, ry, np.ones((H, W))], axis=-1)
        R, t = vm[:3, :3], vm[3, :3]                                   # p_v = p R + t
        pa = (r * (d - tr)[..., None] - t) @ R.T
        pb = (r * (d + tr)[..., None] - t) @ R.T
        pad = vx + (d + tr) * np.hypot(tx / W, ty / H)
        lo = (np.minimum(pa, pb) - pad[..., None] - o) / vx - grow
        hi = (np.maximum(pa, pb) + pad[..., None] - o) / vx + grow
        with np.errstate(invalid="ignore"):
            flo, fhi = np.floor(lo), np.floor(hi)
            inside = ((flo >= -2.0 ** 23) & (fhi < 2.0 ** 23)).all(axis=-1)
            blo = np.floor(np.where(inside[..., None], flo, 0) / 8).astype(np.int64)
            bhi = np.floor(np.where(inside[..., None], fhi, 0) / 8).astype(np.int64)
            skipped = ok & (~inside | ((bhi - blo + 1) > 4).any(axis=-1))
            # an end of the box within NEAR voxels of a block face (a multiple of 8 in index units)
            dist = lambda x: np.abs(x / 8 - np.round(x / 8)) * 8  # noqa: E731
            near = ok & ((dist(lo) < NEAR) | (dist(hi) < NEAR)).any(axis=-1)
        for key, val in (("take", ok & ~skipped), ("skipped", skipped), ("lo", blo), ("hi", bhi), ("near", near)):
            out[key].append(val.reshape(-1, 3) if val.ndim == 3 else val.reshape(-1))
    return {k: np.concatenate(v) for k, v in out.items()}


def twin_keys(tw, which):
    """The sorted set of keys of the pixels tw['take'] & which."""
    sel = tw["take"] & which
    lo, hi = tw["lo"][sel], tw["hi"][sel]
    found = set()
    for l, h in {(tuple(a), tuple(b)) for a, b in zip(lo.tolist(), hi.tolist())}:
        for z in range(l[2], h[2] + 1):
            for y in range(l[1], h[1] + 1):
                for x in range(l[0], h[0] + 1):
                    found.add(int(keys_of([[x, y, z]])[0]))
    return np.array(sorted(found), np.int64)


# ---- dense grids aligned with the lattice ---------------------------------------------------------------------------------------------
def dense_box(keys, margin_blocks=0):
    """(base index [3], dims (nx, ny, nz)) of the dense lattice-aligned grid over the blocks, margin_blocks more on every side."""
    c = coords_of(keys)
    lo, hi = c.min(axis=0) - margin_blocks, c.max(axis=0) + margin_blocks
    return (lo * 8).astype(np.int64), tuple(int(v) for v in (hi - lo + 1) * 8)


def lattice_origin(origin, voxel, base):
    """The float32 position of lattice point `base`: lg_tsdf_coord per axis."""
    return tuple(float(np.float32(o) + np.float32(voxel) * np.float32(b)) for o, b in zip(origin, base))


def block_index(keys, base, dims):
    """[n,8,8,8] linear index into the dense grid (base, dims) of every point of every block."""
    c = coords_of(keys)
    g = c[:, :, None] * 8 + np.arange(8)[None, None, :] - np.asarray(base)[None, :, None]
    return (g[:, 2][:, :, None, None] * dims[1] + g[:, 1][:, None, :, None]) * dims[0] + g[:, 0][:, None, None, :]


def scattered_field(seed=0, missing=1 / 3):
    """(keys, tsdf, weight, colour [n,8,8,8(,3)], dense (tsdf, weight, colour) [32,32,32(,3)]) of mesh_common.random_field over a random
    subset of the 3 x 3 x 3 block region at block coordinates 1 .. 3 (lattice indices 8 .. 31).  The dense copy starts at lattice point 0,
    so that its index is the global index, and has weight 0 outside the chosen blocks."""
    rs = np.random.RandomState(40 + seed)
    f, w, c = mc.random_field((32, 32, 32), seed=seed, observed=0.93)
    assert not (f == 0).any()
    chosen = rs.uniform(0, 1, (3, 3, 3)) >= missing                      # [bz, by, bx]
    coords = np.array([(x + 1, y + 1, z + 1) for z in range(3) for y in range(3) for x in range(3) if chosen[z, y, x]])
    keys = np.sort(keys_of(coords))
    at = block_index(keys, (0, 0, 0), (32, 32, 32))
    mask = np.zeros(32 ** 3, bool); mask[at.reshape(-1)] = True
    wd = np.where(mask.reshape(32, 32, 32), w, 0).astype(np.float32)
    return keys, f.reshape(-1)[at], w.reshape(-1)[at], c.reshape(-1, 3)[at], (f, wd, c)


def dense_vertex_owners(tsdf, weight, iso=0.0, min_weight=1.0):
    """(point linear index, slot) of every vertex of a dense grid, in the dense order (point, slot): the vertex rule in numpy."""
    nz, ny, nx = tsdf.shape
    obs, ins = weight >= min_weight, tsdf < iso
    carry = np.zeros((nz, ny, nx, 7), bool)
    for k, m in enumerate(mc.SLOT_MASKS):
        ox, oy, oz = m & 1, (m >> 1) & 1, (m >> 2) & 1
        a = (slice(0, nz - oz), slice(0, ny - oy), slice(0, nx - ox))
        b = (slice(oz, nz), slice(oy, ny), slice(ox, nx))
        carry[a + (k,)] = obs[a] & obs[b] & (ins[a] != ins[b])
    p, k = np.nonzero(carry.reshape(-1, 7))
    return p, k


def sparse_rank_of(keys, lin, dims, base=(0, 0, 0)):
    """rank 512 + local index of the dense points `lin` (linear indices in the grid (base, dims)); -1 for a point outside the blocks."""
    nx, ny, _nz = dims
    x, y, z = lin % nx + base[0], (lin // nx) % ny + base[1], lin // (nx * ny) + base[2]
    k = keys_of(np.stack([x >> 3, y >> 3, z >> 3], axis=1))
    r = np.searchsorted(keys, k)
    ok = (r < len(keys)) & (np.asarray(keys)[np.minimum(r, len(keys) - 1)] == k)
    return np.where(ok, r * 512 + ((z & 7) * 8 + (y & 7)) * 8 + (x & 7), -1)


def match_meshes(sparse, dense):
    """Sparse and dense meshes as sets: the permutation perm with dense vertex perm[i] = sparse vertex i by position bits; asserts colours
    bit for bit and faces as matched triples."""
    sv, dv = bits(sparse["vertices"]), bits(dense["vertices"])
    assert sv.shape == dv.shape, (sv.shape, dv.shape)
    so, do = np.lexsort(sv.T[::-1]), np.lexsort(dv.T[::-1])
    assert np.array_equal(sv[so], dv[do]), "vertex positions differ as sets"
    assert len(np.unique(sv, axis=0)) == len(sv), "two vertices share a position"
    perm = np.empty(len(sv), np.int64); perm[so] = do
    if sparse["colors"] is not None:
        assert np.array_equal(bits(sparse["colors"]), bits(dense["colors"])[perm]), "colours differ"
    sf = perm[sparse["faces"].astype(np.int64)]
    df = dense["faces"].astype(np.int64)
    assert sf.shape == df.shape
    assert np.array_equal(sf[np.lexsort(sf.T[::-1])], df[np.lexsort(df.T[::-1])]), "faces differ as sets of triples"
    return perm
