"""A block-sparse TSDF volume for unbounded scenes: the fusion and the marching tetrahedra of lightgaussian_amd.mesh over 8 x 8 x 8 blocks
that are allocated from the depth maps themselves, so that a thin surface shell in a very large box costs memory for the shell alone.

    BlockTSDFVolume(voxel_size, origin=(0, 0, 0), trunc=None, color=True, device="cuda", backend="hip")
        .keys [n] int64   .coords() [n,3] int32   .points() [n,8,8,8,3]   .tsdf .weight [n,8,8,8]   .color [n,8,8,8,3] or None   .n_blocks
        .allocate(views) -> dict(blocks, new_blocks, skipped_pixels)        .allocate_blocks(coords) -> the same dict
        .integrate(depth, camera, ...) / .integrate_many(views, allocate=True)      the view dicts of mesh.TSDFVolume
        .extract_mesh(iso=0.0, min_weight=1.0, drop_unreferenced=True)              the return of mesh.TSDFVolume.extract_mesh
        .reset() (values fresh, blocks kept)   .clear() (no blocks)
        .to_dense(margin=0) -> mesh.TSDFVolume over the blocks' bounding box (refused at 2^29 points)
    mesh.fuse_views(cameras, model, pipe, volume) takes a BlockTSDFVolume as it takes a TSDFVolume.

The contract (include/lightgaussian_blocks.h), in float32.  Lattice point (i, j, k) lies at origin + voxel_size (i, j, k),
the dense volume's expression with the global index; block b = floor(i / 8) per axis, b in [-2^20, 2^20); key = (bz + 2^20) << 42 | (by + 2^20)
<< 21 | (bx + 2^20).  The volume is its keys in ascending order and storage follows that order, so no result depends on the order in which
blocks were allocated.  0 < trunc <= 4 voxel_size and n 512 < 2^29.  A pixel whose depth d passes the gates of the integration (d > 0 and
finite, not above depth_max > 0, alpha not below alpha_min) touches the blocks of the lattice box about the world segment of its centre
ray between d - trunc and d + trunc, padded by voxel_size + (d + trunc) sqrt((tanfovx / W)^2 + (tanfovy / H)^2); it is skipped and counted
(skipped_pixels, one warning per volume) when that box spans more than 4 blocks along an axis or leaves the lattice indices [-2^23, 2^23).
Integration is mesh.TSDFVolume's per-point rule at every point of every block; points outside the blocks do not exist, so free space far in
front of a surface is not carved.  Extraction is its marching tetrahedra across block borders: a missing neighbour block is unobserved,
vertex ids count (block rank, point in block, slot), faces (block rank, cell in block, tetrahedron, triangle).

backend="torch" is the same contract in torch ops: the path CPU tensors take, and the comparand of tools/blocks_bench.py.  It meshes through
the dense bounding box of the blocks and reorders.  backend="hip" takes contiguous float32 tensors on the GPU.  set_profile(True) records the
launches under "blocks_touch", "blocks_regrid", "blocks_integrate", "blocks_mesh_count", "blocks_mesh_scan", "blocks_mesh_emit"."""
import ctypes as C
import math
import warnings

import numpy as np
import torch

from . import _lib, mesh, model_rows
from .mesh import lg_tsdf_view
from .model_rows import check_backend

BLOCK = 8
BLOCK_POINTS = 512
BIAS = 1 << 20
MAX_BLOCKS = 1 << 20                # n 512 < 2^29
INDEX_LIMIT = float(1 << 23)
MAX_SPAN = 4
MAX_TOUCH_PIXELS = 1 << 26          # LG_BLK_TOUCH_MAX_PIXELS: per lg_blocks_touch call


class lg_block_volume(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("voxel_size", C.c_float), ("trunc", C.c_float), ("n_blocks", C.c_int32), ("keys", C.c_void_p),
                ("tsdf", C.c_void_p), ("weight", C.c_void_p), ("color", C.c_void_p)]


# The C ABI of include/lightgaussian_blocks.h, in header order: name -> (restype, argtypes).  tests/test_blocks_host.py holds every entry
# against the header.
i32, i64, u32, f32, sz, vp, P = C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_size_t, C.c_void_p, C.POINTER
PROTOTYPES = {
    "lg_blocks_touch_scratch_bytes": (sz, (i32, P(lg_tsdf_view))),
    "lg_blocks_touch": (C.c_int, (P(lg_block_volume), i32, P(lg_tsdf_view), i64, vp, vp, vp, u32, vp)),
    "lg_blocks_merge_scratch_bytes": (sz, (i64,)),
    "lg_blocks_merge": (C.c_int, (i64, vp, i64, vp, vp, vp, vp, u32, vp)),
    "lg_blocks_regrid": (C.c_int, (P(lg_block_volume), P(lg_block_volume), u32, vp)),
    "lg_blocks_integrate": (C.c_int, (P(lg_block_volume), i32, P(lg_tsdf_view), u32, vp)),
    "lg_blocks_mesh_scratch_bytes": (sz, (i32,)),
    "lg_blocks_mesh_count": (C.c_int, (P(lg_block_volume), f32, f32, vp, vp, u32, vp)),
    "lg_blocks_mesh_emit": (C.c_int, (P(lg_block_volume), f32, f32, vp, i64, i64, vp, vp, vp, u32, vp)),
}

set_profile, _flags = model_rows.profile_switch()
def load():
    """The library object of _lib.load() with the prototypes of include/lightgaussian_blocks.h set on it."""
    return _lib.bind(_lib.load(), PROTOTYPES)


# ---- keys ----------------------------------------------------------------------------------------------------------------------------
def keys_of(coords):
    """[n] int64 keys of block coordinates [n,3] (bx, by, bz), each in [-2^20, 2^20)."""
    c = coords.to(torch.int64) + BIAS
    return (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def coords_of(keys):
    """[n,3] int32 block coordinates (bx, by, bz) of keys."""
    k = keys.to(torch.int64)
    return torch.stack([(k & 0x1FFFFF) - BIAS, ((k >> 21) & 0x1FFFFF) - BIAS, ((k >> 42) & 0x1FFFFF) - BIAS], dim=1).to(torch.int32)


# ---- the torch backend ---------------------------------------------------------------------------------------------------------------
def _touch_torch(vol, depth, vm, tx, ty, alpha, alpha_min, depth_max):
    """(keys the view touches, unique and ascending; skipped pixels): lg_math.h's lg_blk_touch, operation by operation, in float32."""
    dev, dt = depth.device, torch.float32
    H, W = (int(v) for v in depth.shape)
    one = np.float32
    m = [float(v) for v in vm.reshape(-1).tolist()]
    d = depth
    ok = (d > 0) & torch.isfinite(d)
    if depth_max > 0:
        ok = ok & ~(d > depth_max)
    if alpha is not None:
        ok = ok & ~(alpha < alpha_min)
    rx = (((2 * torch.arange(W, device=dev) + 1).to(dt) / float(W) - 1.0) * tx)[None, :]
    ry = (((2 * torch.arange(H, device=dev) + 1).to(dt) / float(H) - 1.0) * ty)[:, None]
    za, zb = d - vol.trunc, d + vol.trunc
    fw, fh = one(tx) / one(W), one(ty) / one(H)
    foot = float(np.sqrt(fw * fw + fh * fh, dtype=np.float32))
    pad = vol.voxel_size + zb * foot
    ax, ay, az = rx * za - m[12], ry * za - m[13], za - m[14]
    bx, by, bz = rx * zb - m[12], ry * zb - m[13], zb - m[14]
    skipped = torch.zeros_like(ok)
    lo_b, n_b = [], []
    for a in range(3):
        wa = ax * m[4 * a] + ay * m[4 * a + 1] + az * m[4 * a + 2]
        wb = bx * m[4 * a] + by * m[4 * a + 1] + bz * m[4 * a + 2]
        lo, hi = torch.minimum(wa, wb) - pad, torch.maximum(wa, wb) + pad
        flo, fhi = torch.floor((lo - vol.origin[a]) / vol.voxel_size), torch.floor((hi - vol.origin[a]) / vol.voxel_size)
        inside = (flo >= -INDEX_LIMIT) & (fhi < INDEX_LIMIT) & (flo <= fhi)
        zero = torch.zeros((), dtype=dt, device=dev)
        blo = torch.div(torch.where(inside, flo, zero).to(torch.int64), BLOCK, rounding_mode="floor")
        bhi = torch.div(torch.where(inside, fhi, zero).to(torch.int64), BLOCK, rounding_mode="floor")
        skipped = skipped | (ok & ~skipped & (~inside | (bhi - blo + 1 > MAX_SPAN)))
        lo_b.append(blo); n_b.append(bhi - blo + 1)
    take = ok & ~skipped
    lo3 = torch.stack([b[take] for b in lo_b], dim=1)
    n3 = torch.stack([b[take] for b in n_b], dim=1)
    found = [torch.zeros(0, dtype=torch.int64, device=dev)]
    for dz in range(MAX_SPAN):
        for dy in range(MAX_SPAN):
            for dx in range(MAX_SPAN):
                sel = (n3[:, 0] > dx) & (n3[:, 1] > dy) & (n3[:, 2] > dz)
                if bool(sel.any()):
                    found.append(torch.unique(keys_of(lo3[sel] + torch.tensor([dx, dy, dz], device=dev))))
    return torch.unique(torch.cat(found)), int(skipped.sum())


# ---- the volume -----------------------------------------------------------------------------------------------------------------------
class BlockTSDFVolume:
    """A block-sparse TSDF volume: see the module docstring.  origin: three floats (world position of lattice point (0, 0, 0)); trunc
    defaults to 4 voxel_size, the widest band; color=False keeps no colour.  keys [n], tsdf, weight [n,8,8,8] and color [n,8,8,8,3] (or
    None) are public; allocate replaces them by new tensors when the key list grows."""

    def __init__(self, voxel_size, origin=(0.0, 0.0, 0.0), trunc=None, color=True, device="cuda", backend="hip"):
        check_backend(backend, "BlockTSDFVolume")
        self.origin = tuple(model_rows.f32(v) for v in origin)
        self.voxel_size = model_rows.f32(voxel_size)
        self.trunc = model_rows.f32(4.0 * self.voxel_size if trunc is None else trunc)
        if len(self.origin) != 3:
            raise ValueError("BlockTSDFVolume: origin has three entries")
        if not (self.voxel_size > 0 and math.isfinite(self.voxel_size)):
            raise ValueError(f"BlockTSDFVolume: voxel_size must be positive and finite, not {self.voxel_size}")
        if not (0 < self.trunc <= model_rows.f32(4.0 * self.voxel_size)):
            raise ValueError(f"BlockTSDFVolume: trunc must lie in (0, 4 voxel_size], not {self.trunc} at voxel_size {self.voxel_size}")
        if not all(math.isfinite(v) for v in self.origin):
            raise ValueError("BlockTSDFVolume: origin must be finite")
        self.backend = backend
        self.device = torch.device(device)
        self.keep_color = bool(color)
        self._warned = False
        self.clear()

    # -- storage --
    def _pools(self, n):
        dev = self.device
        return (torch.empty((n, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=dev), torch.empty((n, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=dev),
                torch.empty((n, BLOCK, BLOCK, BLOCK, 3), dtype=torch.float32, device=dev) if self.keep_color else None)

    def clear(self):
        """No blocks."""
        self.keys = torch.empty(0, dtype=torch.int64, device=self.device)
        self.tsdf, self.weight, self.color = self._pools(0)

    def reset(self):
        """Fresh values in every block; the blocks are kept."""
        self.tsdf.fill_(1.0)
        self.weight.fill_(0.0)
        if self.color is not None:
            self.color.fill_(0.0)

    @property
    def n_blocks(self):
        return int(self.keys.shape[0])

    def coords(self):
        """[n,3] int32 block coordinates (bx, by, bz), in key order."""
        return coords_of(self.keys)

    def _global_index(self):
        """[n,3,8] int64 lattice indices of the points of every block per axis."""
        return self.coords().to(torch.int64)[:, :, None] * BLOCK + torch.arange(BLOCK, device=self.keys.device)[None, None, :]

    def _points(self):
        """(px, py, pz): the world coordinates of the points per axis, from the global index, shaped to broadcast over [n,8,8,8]."""
        g = self._global_index()
        ax = [self.origin[a] + self.voxel_size * g[:, a].to(torch.float32) for a in range(3)]
        return ax[0][:, None, None, :], ax[1][:, None, :, None], ax[2][:, :, None, None]

    def points(self):
        """[n,8,8,8,3] float32 world positions of the points, [block, z, y, x, (x y z)]."""
        shape = (self.n_blocks, BLOCK, BLOCK, BLOCK)
        return torch.stack([a.expand(shape) for a in self._points()], dim=-1)

    def nbytes(self):
        """Bytes of the keys and the pools."""
        return sum(t.numel() * t.element_size() for t in (self.keys, self.tsdf, self.weight, self.color) if t is not None)

    def _resolve(self, what, tensors):
        return mesh._resolve_backend(self.backend, self.tsdf, what, tensors)

    def _own(self):
        return [("keys", self.keys), ("tsdf", self.tsdf), ("weight", self.weight)] + ([] if self.color is None else [("color", self.color)])

    def _struct(self, keys=None, pools=None):
        keys = self.keys if keys is None else keys
        tsdf, weight, color = (self.tsdf, self.weight, self.color) if pools is None else pools
        n = int(keys.shape[0])
        return lg_block_volume((C.c_float * 3)(*self.origin), self.voxel_size, self.trunc, n, keys.data_ptr() if n else None, tsdf.data_ptr() if n else None,
                               weight.data_ptr() if n else None, color.data_ptr() if (n and color is not None) else None)

    # -- allocation --
    def _grow(self, new_keys, backend):
        """The pools under new_keys (a superset of self.keys, ascending): old blocks keep their bits, new ones are fresh."""
        n_old, n_new = self.n_blocks, int(new_keys.shape[0])
        if n_new * BLOCK_POINTS >= mesh.MAX_POINTS:
            raise ValueError(f"BlockTSDFVolume: {n_new} blocks: n 512 must stay below 2^29")
        if n_new == n_old:
            return
        pools = self._pools(n_new)
        if backend == "torch":
            at = torch.searchsorted(new_keys, self.keys)
            for new, old, fresh in zip(pools, (self.tsdf, self.weight, self.color), (1.0, 0.0, 0.0)):
                if new is not None:
                    new.fill_(fresh)
                    new[at] = old
        else:
            dev = self.device
            a, b = self._struct(), self._struct(new_keys, pools)
            with torch.cuda.device(dev):
                _lib.check(load().lg_blocks_regrid(C.byref(a), C.byref(b), _flags(), _lib.stream(dev)))
        self.keys = new_keys
        self.tsdf, self.weight, self.color = pools

    def _report(self, n_before, skipped):
        if skipped > 0 and not self._warned:
            self._warned = True
            warnings.warn(f"BlockTSDFVolume: {skipped} pixels were skipped by the allocation: their band spans more than {MAX_SPAN} blocks along an axis "
                          f"(a footprint far above {MAX_SPAN} voxels) or leaves the lattice; choose a larger voxel_size or a depth_max", RuntimeWarning, stacklevel=3)
        return dict(blocks=self.n_blocks, new_blocks=self.n_blocks - n_before, skipped_pixels=int(skipped))

    def _merge_hip(self, add_keys, stats):
        """lg_blocks_merge of self.keys and add_keys: the merged buffer; its length goes to stats[0] on the device."""
        dev, lib = self.device, load()
        n_old, n_add = self.n_blocks, int(add_keys.shape[0])
        merged = torch.empty(max(n_old + n_add, 1), dtype=torch.int64, device=dev)
        scratch = _lib.scratch(lib.lg_blocks_merge_scratch_bytes(n_old + n_add), dev)
        _lib.check(lib.lg_blocks_merge(n_old, _lib.ptr(self.keys) if n_old else None, n_add, _lib.ptr(add_keys) if n_add else None, _lib.ptr(merged), _lib.ptr(stats),
                                       _lib.ptr(scratch), _flags(), _lib.stream(dev)))
        return merged

    @staticmethod
    def _capacity(pixels):
        """Candidate keys the first lg_blocks_touch call of a chunk has room for: a wave of 8 x 8 pixels leaves some 8 to 75 keys."""
        return max(4096, pixels // 2)

    def _allocate_checked(self, checked, backend):
        n_before, skipped = self.n_blocks, 0
        if backend == "torch":
            with torch.no_grad():
                found = [self.keys]
                for depth, vm, tx, ty, _color, alpha, alpha_min, depth_max, _z_min in checked:
                    k, s = _touch_torch(self, depth, vm, model_rows.f32(tx), model_rows.f32(ty), alpha, model_rows.f32(alpha_min), model_rows.f32(depth_max))
                    found.append(k); skipped += s
                self._grow(torch.unique(torch.cat(found)), backend)
            return self._report(n_before, skipped)
        # chunks of views below LG_BLK_TOUCH_MAX_PIXELS; one read-back per chunk: (blocks, candidates the views produced, skipped pixels)
        dev, lib = self.device, load()
        first = 0
        while first < len(checked):
            last, pixels = first, 0
            while last < len(checked) and (last == first or pixels + checked[last][0].numel() < MAX_TOUCH_PIXELS):
                pixels += checked[last][0].numel(); last += 1
            part = checked[first:last]
            arr = mesh._view_array(part)
            capacity = self._capacity(pixels)
            with torch.cuda.device(dev):
                scratch = _lib.scratch(lib.lg_blocks_touch_scratch_bytes(len(part), arr), dev)
                stats = torch.empty(4, dtype=torch.int64, device=dev)
                vol = self._struct()
                while True:
                    cand = torch.empty(capacity, dtype=torch.int64, device=dev)
                    _lib.check(lib.lg_blocks_touch(C.byref(vol), len(part), arr, capacity, _lib.ptr(cand), _lib.ptr(stats), _lib.ptr(scratch), _flags(), _lib.stream(dev)))
                    merged = self._merge_hip(cand, stats)
                    n_new, needed, skip = stats.tolist()[:3]
                    if needed <= capacity:
                        break
                    capacity = int(needed)          # the wave-level de-duplication left more keys than the buffer holds: once more, exactly
            if n_new < 0:
                raise RuntimeError("BlockTSDFVolume.allocate: the radix sort of the block keys gave up; the key list is void")
            skipped += skip
            self._grow(merged[:n_new].clone(), backend)
            first = last
        return self._report(n_before, skipped)

    def allocate(self, views):
        """Allocate the blocks the views touch (dicts of integrate's arguments; depth, alpha, alpha_min, depth_max and the camera matter).
        Returns dict(blocks, new_blocks, skipped_pixels)."""
        what = "BlockTSDFVolume.allocate"
        checked, tensors = mesh._check_views(what, list(views), self.tsdf, False)
        return self._allocate_checked(checked, self._resolve(what, self._own() + tensors))

    def allocate_blocks(self, coords):
        """Add the blocks of the coordinates [m,3] (bx, by, bz), each in [-2^20, 2^20), by the same sorted union."""
        what = "BlockTSDFVolume.allocate_blocks"
        c = torch.as_tensor(coords)
        if c.dim() != 2 or c.shape[1] != 3 or c.dtype.is_floating_point or c.dtype == torch.bool:
            raise ValueError(f"{what}: coords must be an integer [m, 3] tensor")
        c = c.to(device=self.device, dtype=torch.int64)
        if c.numel() and (int(c.min()) < -BIAS or int(c.max()) >= BIAS):
            raise ValueError(f"{what}: block coordinates must lie in [-2^20, 2^20)")
        backend = self._resolve(what, self._own())
        n_before = self.n_blocks
        add = keys_of(c).contiguous()
        if backend == "torch":
            self._grow(torch.unique(torch.cat([self.keys, add])), backend)
        else:
            dev = self.device
            with torch.cuda.device(dev):
                stats = torch.empty(4, dtype=torch.int64, device=dev)
                merged = self._merge_hip(add, stats)
                n_new = int(stats[0])
            if n_new < 0:
                raise RuntimeError(f"{what}: the radix sort of the block keys gave up; the key list is void")
            self._grow(merged[:n_new].clone(), backend)
        return self._report(n_before, 0)

    # -- integration --
    def integrate(self, depth, camera, color=None, alpha=None, alpha_min=0.5, depth_max=0.0, z_min=0.05, allocate=True):
        """One view into the volume: mesh.TSDFVolume.integrate's arguments; allocate=False integrates into the blocks that exist."""
        self.integrate_many([dict(depth=depth, camera=camera, color=color, alpha=alpha, alpha_min=alpha_min, depth_max=depth_max, z_min=z_min)], allocate=allocate)

    def integrate_many(self, views, allocate=True):
        """The views, dicts of integrate's arguments, in order: the blocks they touch are allocated first (allocate=True), then one library
        call integrates them, 8 views per pass over the blocks."""
        what = "BlockTSDFVolume.integrate_many"
        checked, tensors = mesh._check_views(what, list(views), self.tsdf, self.color is not None)
        backend = self._resolve(what, self._own() + tensors)
        if not checked:
            return
        if allocate:
            self._allocate_checked(checked, backend)
        if self.n_blocks == 0:
            return
        if backend == "torch":
            mesh._integrate_checked_torch(self, self._points(), checked)
            return
        arr = mesh._view_array(checked)
        dev, vol = self.device, self._struct()
        with torch.cuda.device(dev):
            _lib.check(load().lg_blocks_integrate(C.byref(vol), len(checked), arr, _flags(), _lib.stream(dev)))

    # -- extraction --
    def _bounding_box(self, margin, what):
        c = self.coords().to(torch.int64)
        lo, hi = c.min(dim=0).values, c.max(dim=0).values
        base = [int(v) * BLOCK - margin for v in lo.tolist()]
        dims = [(int(h) - int(l) + 1) * BLOCK + 2 * margin for l, h in zip(lo.tolist(), hi.tolist())]
        if dims[0] * dims[1] * dims[2] >= mesh.MAX_POINTS:
            raise ValueError(f"{what}: the bounding box of the blocks has {dims[0]} x {dims[1]} x {dims[2]} points, 2^29 or more")
        return base, dims

    def _dense_index(self, base, dims):
        """[n,8,8,8] linear index of every point of every block in the dense grid (base, dims)."""
        g = self._global_index()
        x, y, z = (g[:, a] - base[a] for a in range(3))
        return (z[:, :, None, None] * dims[1] + y[:, None, :, None]) * dims[0] + x[:, None, None, :]

    def _scatter_dense(self, base, dims, tsdf, weight, color):
        """The blocks' values into the tensors [nz,ny,nx] (color [nz,ny,nx,3]; ignored by a volume without colour) of the dense grid
        (base, dims), by the one index both to_dense and the torch extraction use; the other points keep what they hold."""
        at = self._dense_index(base, dims).reshape(-1)
        tsdf.view(-1)[at] = self.tsdf.reshape(-1)
        weight.view(-1)[at] = self.weight.reshape(-1)
        if self.color is not None:
            color.view(-1, 3)[at] = self.color.reshape(-1, 3)

    def to_dense(self, margin=0):
        """A mesh.TSDFVolume over the bounding box of the blocks, `margin` points wider on every side, holding the blocks' values and fresh
        values elsewhere.  Its points lie at its own origin + voxel_size index: where the sparse origin is not the lattice point itself
        the coordinates may differ from the sparse ones in the last bit."""
        what = "BlockTSDFVolume.to_dense"
        margin = int(margin)
        if margin < 0 or self.n_blocks == 0:
            raise ValueError(f"{what}: margin must not be negative and the volume must hold a block")
        base, dims = self._bounding_box(margin, what)
        origin = tuple(float(np.float32(o) + np.float32(self.voxel_size) * np.float32(b)) for o, b in zip(self.origin, base))
        dense = mesh.TSDFVolume(origin, dims, self.voxel_size, trunc=self.trunc, color=self.color is not None, device=self.device, backend=self.backend)
        self._scatter_dense(base, dims, dense.tsdf, dense.weight, dense.color)
        return dense

    def _extract_torch(self, iso, min_weight):
        dev = self.device
        if self.n_blocks == 0:
            return (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev),
                    None if self.color is None else torch.zeros((0, 3), dtype=torch.float32, device=dev))
        base, dims = self._bounding_box(0, "BlockTSDFVolume.extract_mesh (backend='torch' meshes through the dense bounding box)")
        nx, ny, nz = dims
        tsdf, weight = torch.ones((nz, ny, nx), dtype=torch.float32, device=dev), torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
        color = None if self.color is None else torch.zeros((nz, ny, nx, 3), dtype=torch.float32, device=dev)
        self._scatter_dense(base, dims, tsdf, weight, color)
        v, f, c, p, k, cell = mesh._extract_grid(tsdf, weight, color, self.origin, self.voxel_size, iso, min_weight, base=base)

        def sparse_index(lin):          # dense linear index of a point of an allocated block -> rank 512 + local index
            x, y, z = lin % nx + base[0], (lin // nx) % ny + base[1], lin // (nx * ny) + base[2]
            b = torch.stack([torch.div(a, BLOCK, rounding_mode="floor") for a in (x, y, z)], dim=1)
            rank = torch.searchsorted(self.keys, keys_of(b))
            return rank * BLOCK_POINTS + ((z & 7) * BLOCK + (y & 7)) * BLOCK + (x & 7)
        order = torch.argsort(sparse_index(p) * 7 + k)
        new_id = torch.empty_like(order)
        new_id[order] = torch.arange(order.numel(), device=dev)
        forder = torch.sort(sparse_index(cell), stable=True).indices
        return v[order], new_id[f[forder]].to(torch.int32).reshape(-1, 3), None if c is None else c[order]

    def extract_mesh(self, iso=0.0, min_weight=1.0, drop_unreferenced=True):
        """(vertices [Nv,3] float32 in world space, faces [Nf,3] int32, colors [Nv,3] or None) of the surface tsdf = iso over the points with
        weight >= min_weight, across block borders, normals toward larger tsdf; drop_unreferenced as mesh.TSDFVolume.extract_mesh."""
        what = "BlockTSDFVolume.extract_mesh"
        iso, min_weight = mesh._check_extract_args(what, iso, min_weight)
        if self._resolve(what, self._own()) == "torch":
            with torch.no_grad():
                vertices, faces, colors = self._extract_torch(iso, min_weight)
        else:
            lib = load()
            vertices, faces, colors = mesh._extract_hip(lib.lg_blocks_mesh_scratch_bytes(self.n_blocks), lib.lg_blocks_mesh_count, lib.lg_blocks_mesh_emit,
                                                        self._struct(), self.color is not None, self.device, iso, min_weight, _flags())
        if drop_unreferenced:
            vertices, faces, colors = mesh.drop_unreferenced_vertices(vertices, faces, colors)
        return vertices, faces, colors
