"""TSDF fusion of rendered depth maps and extraction of a triangle mesh by marching tetrahedra: the surface 2DGS, GOF, PGSR and RaDe-GS
publish, from the maps gaussian_renderer.render_geometry returns.

    TSDFVolume(origin, dims, voxel_size, trunc=None, color=True, device="cuda", backend="hip")
        .integrate(depth, camera, color=None, alpha=None, alpha_min=0.5, depth_max=0.0, z_min=0.05)        one view
        .integrate_many(views)             views = dicts of integrate's arguments: ONE lg_tsdf_integrate call, BATCH (8) views per launch
        .extract_mesh(iso=0.0, min_weight=1.0, drop_unreferenced=True) -> (vertices [Nv,3], faces [Nf,3] int32, colors [Nv,3] or None)
        .reset()
    fuse_views(cameras, model, pipe, volume, depth="median_depth", options=None)       render_geometry per camera, BATCH views per pass
    bounds_from_cameras(cameras, voxel_size, scale=1.0, multiple=4) -> (origin, dims)   a cube about the cameras' centre
    save_ply(path, vertices, faces, colors=None)                                        binary little-endian PLY

The contract (include/lightgaussian_mesh.h), in float32.  The volume is nx x ny x nz points, point (x, y, z) at
origin + voxel_size (x, y, z); tsdf [nz,ny,nx] starts at 1, weight at 0, color [nz,ny,nx,3] at 0.  One point under one view:
    p_v = point vm                                   skip when !(p_v.z > z_min)
    fx = (p_v.x / (p_v.z tanfovx) + 1) (0.5 W)       px = floor(fx), py likewise; skip outside the image
    d = depth[py, px]                                skip when !(d > 0), not finite, above depth_max > 0, or alpha[py, px] < alpha_min
    sdf = d - p_v.z                                  skip when sdf < -trunc
    t = min(1, sdf / trunc)    w' = w + 1    tsdf = (tsdf w + t) / w'    color = (color w + image[:, py, px]) / w'    weight = w'
One call with n views gives the bits of n calls with one view.  The mesh: a point is observed when weight >= min_weight and inside when
tsdf < iso; an edge of the seven a point owns (to p + offset(m), m = 1, 2, 4, 3, 5, 6, 7) carries a vertex iff both ends are observed and
exactly one is inside, at t = f0 / (f0 - f1) along it; vertex ids count these edges by (point, slot).  A cell whose eight corners are
observed is cut into six tetrahedra (one per permutation of the axes, corners 0, 1<<a, 1<<a | 1<<b, 7), each gives 0, 1 or 2 triangles by
its inside mask; normals point toward larger tsdf; faces are ordered by cell, tetrahedron, triangle.  The six-tetrahedra split has no
ambiguous case: over a fully observed region the mesh is closed and manifold.

backend="torch" is the same contract as vectorised torch ops, with the same vertex and face order: the path CPU tensors take, and the
comparand of tools/mesh_bench.py.  backend="hip" takes contiguous float32 tensors on the GPU and raises for anything else on the GPU.
set_profile(True) records the launches under "tsdf_integrate", "mesh_count", "mesh_scan", "mesh_emit" (_lib.profile_read)."""
import ctypes as C
import itertools
import math
import struct

import torch

from . import _lib, model_rows
from .model_rows import check_backend

BATCH = 8                   # LG_TSDF_BATCH: views per launch of lg_tsdf_integrate
MAX_POINTS = 1 << 29
MAX_DIM = 32768
SLOT_MASKS = (1, 2, 4, 3, 5, 6, 7)          # the offset mask of edge slot k
PERMUTATIONS = tuple(itertools.permutations(range(3)))


class lg_tsdf_volume(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3), ("voxel_size", C.c_float),
                ("trunc", C.c_float), ("tsdf", C.c_void_p), ("weight", C.c_void_p), ("color", C.c_void_p)]


class lg_tsdf_view(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("viewmatrix", C.c_void_p),
                ("depth", C.c_void_p), ("color", C.c_void_p), ("alpha", C.c_void_p), ("alpha_min", C.c_float), ("depth_max", C.c_float),
                ("z_min", C.c_float)]


# The C ABI of include/lightgaussian_mesh.h, in header order: name -> (restype, argtypes).  tests/test_mesh_host.py holds every entry
# against the header.
i32, i64, u32, f32, sz, vp, P = C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_size_t, C.c_void_p, C.POINTER
PROTOTYPES = {
    "lg_tsdf_integrate": (C.c_int, (P(lg_tsdf_volume), i32, P(lg_tsdf_view), u32, vp)),
    "lg_mesh_scratch_bytes": (sz, (i32, i32, i32)),
    "lg_mesh_count": (C.c_int, (P(lg_tsdf_volume), f32, f32, vp, vp, u32, vp)),
    "lg_mesh_emit": (C.c_int, (P(lg_tsdf_volume), f32, f32, vp, i64, i64, vp, vp, vp, u32, vp)),
}

set_profile, _flags = model_rows.profile_switch()
def load():
    """The library object of _lib.load() with the prototypes of include/lightgaussian_mesh.h set on it."""
    return _lib.bind(_lib.load(), PROTOTYPES)


def tanfov(camera):
    """(tanfovx, tanfovy) of a camera, as the renderer evaluates them."""
    return math.tan(camera.FoVx * 0.5), math.tan(camera.FoVy * 0.5)


# ---- the triangle table of the six tetrahedra, derived from the rule ----------------------------------------------------------------
def _offset(m):
    return (m & 1, (m >> 1) & 1, (m >> 2) & 1)


def tet_corners(t):
    """The cell corners (offset masks) of the four local corners of tetrahedron t."""
    a, b, _c = PERMUTATIONS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def _triangles(t, mask):
    """The triangles of tetrahedron t under the inside mask, as triples of edges (lo, hi) of local corners, winding applied."""
    inside = [i for i in range(4) if (mask >> i) & 1]
    outside = [i for i in range(4) if not (mask >> i) & 1]
    edge = lambda u, v: (min(u, v), max(u, v))  # noqa: E731
    if len(inside) in (0, 4):
        return []
    if len(inside) == 2:
        (a, b), (c, d) = inside, outside
        q = [edge(a, c), edge(a, d), edge(b, d), edge(b, c)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        a = inside[0] if len(inside) == 1 else outside[0]
        tris = [[edge(a, o) for o in range(4) if o != a]]
    pos = [_offset(m) for m in tet_corners(t)]
    mid = lambda e: [(pos[e[0]][k] + pos[e[1]][k]) / 2 for k in range(3)]  # noqa: E731
    centre = lambda idx: [sum(pos[i][k] for i in idx) / len(idx) for k in range(3)]  # noqa: E731
    toward_inside = [ci - co for ci, co in zip(centre(inside), centre(outside))]
    out = []
    for tri in tris:
        v0, v1, v2 = (mid(e) for e in tri)
        u, w = [v1[k] - v0[k] for k in range(3)], [v2[k] - v0[k] for k in range(3)]
        n = (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])
        flip = sum(n[k] * toward_inside[k] for k in range(3)) > 0              # the normal must point toward the outside corners
        out.append([tri[0], tri[2], tri[1]] if flip else tri)
    return out


def _build_tables():
    """count [6,16]; c0, slot [6,16,2,3]: per (tetrahedron, inside mask, triangle, vertex) the cell corner that owns the edge and its slot."""
    count = torch.zeros((6, 16), dtype=torch.int64)
    c0 = torch.zeros((6, 16, 2, 3), dtype=torch.int64)
    slot = torch.zeros((6, 16, 2, 3), dtype=torch.int64)
    for t in range(6):
        cm = tet_corners(t)
        for mask in range(16):
            tris = _triangles(t, mask)
            count[t, mask] = len(tris)
            for j, tri in enumerate(tris):
                for v, (lo, hi) in enumerate(tri):
                    c0[t, mask, j, v] = cm[lo]
                    slot[t, mask, j, v] = SLOT_MASKS.index(cm[hi] ^ cm[lo])
    return count, c0, slot


_TABLES = _build_tables()


# ---- the torch backend ---------------------------------------------------------------------------------------------------------------
def _integrate_torch(vol, px, py, pz, depth, vm, tx, ty, color, alpha, alpha_min, depth_max, z_min):
    """One view into vol.tsdf, vol.weight (and vol.color, one more axis of 3 at the end) in place: px, py, pz are the world coordinates
    of the points, float32 tensors that broadcast to the shape of vol.tsdf.  Both volumes' torch backend."""
    dev, dt = vol.tsdf.device, torch.float32
    H, W = (int(v) for v in depth.shape)
    vx = vm[0, 0] * px + vm[1, 0] * py + vm[2, 0] * pz + vm[3, 0]
    vy = vm[0, 1] * px + vm[1, 1] * py + vm[2, 1] * pz + vm[3, 1]
    vz = vm[0, 2] * px + vm[1, 2] * py + vm[2, 2] * pz + vm[3, 2]
    ok = vz > z_min
    flx = torch.floor((vx / (vz * tx) + 1.0) * (0.5 * W))
    fly = torch.floor((vy / (vz * ty) + 1.0) * (0.5 * H))
    ok = ok & (flx >= 0) & (flx < W) & (fly >= 0) & (fly < H)
    zero = torch.zeros((), dtype=dt, device=dev)
    pix = torch.where(ok, fly, zero).long() * W + torch.where(ok, flx, zero).long()
    d = depth.reshape(-1)[pix]
    ok = ok & (d > 0) & torch.isfinite(d)
    if depth_max > 0:
        ok = ok & ~(d > depth_max)
    if alpha is not None:
        ok = ok & ~(alpha.reshape(-1)[pix] < alpha_min)
    sdf = d - vz
    ok = ok & ~(sdf < -vol.trunc)
    t = torch.clamp_max(sdf / vol.trunc, 1.0)
    w = vol.weight
    w1 = w + 1.0
    vol.tsdf.copy_(torch.where(ok, (vol.tsdf * w + t) / w1, vol.tsdf))
    if vol.color is not None:
        img = torch.movedim(color.reshape(3, -1)[:, pix], 0, -1)
        vol.color.copy_(torch.where(ok[..., None], (vol.color * w[..., None] + img) / w1[..., None], vol.color))
    vol.weight.copy_(torch.where(ok, w1, w))


def _shifted(t, m, fill):
    """t[p + offset(m)] per point p, `fill` where that leaves the grid."""
    ox, oy, oz = _offset(m)
    nz, ny, nx = t.shape
    out = torch.full_like(t, fill)
    out[:nz - oz, :ny - oy, :nx - ox] = t[oz:, oy:, ox:]
    return out


def _extract_grid(tsdf, weight, color, origin, voxel, iso, min_weight, base=(0, 0, 0)):
    """The mesh of the contract over a dense grid whose point (0, 0, 0) is the lattice point `base` (positions come from the lattice
    index), every vertex kept, in the contract's order; the dtype of tsdf.  Returns (vertices, faces int64, colors, p, k, cell_of_face):
    p, k = the (point, slot) of every vertex and cell_of_face the cell of every face, as linear indices of the grid."""
    nz, ny, nx = (int(v) for v in tsdf.shape)
    dev, dt = tsdf.device, tsdf.dtype
    obs, ins = weight >= min_weight, tsdf < iso
    carry = torch.stack([obs & _shifted(obs, m, False) & (ins != _shifted(ins, m, False)) for m in SLOT_MASKS], dim=-1).reshape(-1)
    ids = torch.cumsum(carry, 0) - carry.long()                     # vertex id of (point, slot), flat [P * 7]
    sel = carry.nonzero().squeeze(1)
    p, k = sel // 7, sel % 7
    m = torch.tensor(SLOT_MASKS, device=dev)[k]
    off = torch.stack([m & 1, (m >> 1) & 1, (m >> 2) & 1], dim=1)
    q = p + off[:, 0] + off[:, 1] * nx + off[:, 2] * (nx * ny)
    flat = tsdf.reshape(-1)
    f0, f1 = flat[p] - iso, flat[q] - iso
    t = f0 / (f0 - f1)
    grid = torch.stack([p % nx + base[0], (p // nx) % ny + base[1], p // (nx * ny) + base[2]], dim=1).to(dt)
    org = torch.tensor([float(v) for v in origin], dtype=dt, device=dev)
    vertices = org + voxel * (grid + t[:, None] * off.to(dt))
    colors = None
    if color is not None:
        c = color.reshape(-1, 3)
        colors = c[p] + t[:, None] * (c[q] - c[p])
    faces = torch.zeros(0, dtype=torch.int64, device=dev)
    cell_of_face = torch.zeros(0, dtype=torch.int64, device=dev)
    if min(nx, ny, nz) >= 2:
        valid = obs.clone()
        for cm in range(1, 8):
            valid &= _shifted(obs, cm, False)
        cells = valid.reshape(-1).nonzero().squeeze(1)
        corner = torch.stack([_shifted(ins, cm, False).reshape(-1)[cells] for cm in range(8)], dim=1).long()        # [Nc, 8]
        count, c0, slot = (x.to(dev) for x in _TABLES)
        tris, keep = [], []
        for tt in range(6):
            m4 = sum(corner[:, cm] << i for i, cm in enumerate(tet_corners(tt)))
            a, s = c0[tt][m4], slot[tt][m4]                                                                     # [Nc, 2, 3]
            owner = cells[:, None, None] + (a & 1) + ((a >> 1) & 1) * nx + ((a >> 2) & 1) * (nx * ny)
            tris.append(ids[owner * 7 + s])
            keep.append(torch.arange(2, device=dev)[None, :] < count[tt][m4][:, None])
        keep = torch.stack(keep, dim=1)
        faces = torch.stack(tris, dim=1)[keep]
        cell_of_face = cells[:, None, None].expand(-1, 6, 2)[keep]
    return vertices, faces.reshape(-1, 3), colors, p, k, cell_of_face


def _extract_torch(tsdf, weight, color, origin, voxel, iso, min_weight):
    """(vertices, faces, colors) of the contract, every vertex kept, in the contract's order; the dtype of tsdf."""
    vertices, faces, colors = _extract_grid(tsdf, weight, color, origin, voxel, iso, min_weight)[:3]
    return vertices, faces.to(torch.int32), colors


def drop_unreferenced_vertices(vertices, faces, colors=None):
    """The mesh without the vertices no face names, renumbered; the order of the rest is kept."""
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[faces.reshape(-1).long()] = True
    new_id = torch.cumsum(used, 0) - 1
    return vertices[used], new_id[faces.long()].to(torch.int32), None if colors is None else colors[used]


# ---- the volume -----------------------------------------------------------------------------------------------------------------------
def _check_map(what, name, t, shape, like):
    if not torch.is_tensor(t):
        raise ValueError(f"{what}: {name} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, not {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must have shape {list(shape)}, not {list(t.shape)}")
    if t.device != like.device:
        raise ValueError(f"{what}: {name} is on {t.device}, not on {like.device}")


def _check_views(what, views, like, keep_color):
    """The checks of a list of view dicts (integrate's arguments) for a volume whose tensors live where `like` does: [(depth, vm, tx, ty,
    color, alpha, alpha_min, depth_max, z_min)] and the named tensors a backend may ask to be contiguous.  keep_color: the volume keeps
    colour, so every view needs one; otherwise a colour given is ignored."""
    checked, tensors = [], []
    for i, v in enumerate(views):
        unknown = set(v) - {"depth", "camera", "color", "alpha", "alpha_min", "depth_max", "z_min"}
        if unknown:
            raise ValueError(f"{what}: views[{i}] has unknown entries {sorted(unknown)}")
        depth, camera, color, alpha = v["depth"], v["camera"], v.get("color"), v.get("alpha")
        if not torch.is_tensor(depth) or depth.dim() != 2:
            raise ValueError(f"{what}: views[{i}]: depth must be a [H, W] tensor")
        H, W = (int(s) for s in depth.shape)
        if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
            raise ValueError(f"{what}: views[{i}]: H and W must lie in [1, {MAX_DIM}], not {H} x {W}")
        _check_map(what, f"views[{i}].depth", depth, (H, W), like)
        if keep_color:
            if color is None:
                raise ValueError(f"{what}: views[{i}]: the volume keeps colour and the view has no color")
            _check_map(what, f"views[{i}].color", color, (3, H, W), like)
        else:
            color = None
        if alpha is not None:
            _check_map(what, f"views[{i}].alpha", alpha, (H, W), like)
        vm = camera.world_view_transform.detach().to(device=like.device, dtype=torch.float32)
        if tuple(vm.shape) != (4, 4):
            raise ValueError(f"{what}: views[{i}]: camera.world_view_transform must be [4, 4]")
        tx, ty = tanfov(camera)
        scal = tuple(float(v.get(n, dflt)) for n, dflt in (("alpha_min", 0.5), ("depth_max", 0.0), ("z_min", 0.05)))
        if any(math.isnan(s) for s in scal + (tx, ty)):
            raise ValueError(f"{what}: views[{i}]: tanfov, alpha_min, depth_max and z_min must not be NaN")
        checked.append((depth.detach(), vm.contiguous(), tx, ty, None if color is None else color.detach(), None if alpha is None else alpha.detach()) + scal)
        tensors += [(f"views[{i}].depth", depth)] + ([] if color is None else [(f"views[{i}].color", color)]) + \
            ([] if alpha is None else [(f"views[{i}].alpha", alpha)])
    return checked, tensors


def _view_array(checked):
    """The lg_tsdf_view array of checked views (at least one element long: ctypes has no empty array to point at)."""
    arr = (lg_tsdf_view * max(len(checked), 1))()
    for a, (depth, vm, tx, ty, color, alpha, alpha_min, depth_max, z_min) in zip(arr, checked):
        a.H, a.W = (int(s) for s in depth.shape)
        a.tanfovx, a.tanfovy, a.alpha_min, a.depth_max, a.z_min = tx, ty, alpha_min, depth_max, z_min
        a.viewmatrix, a.depth = vm.data_ptr(), depth.data_ptr()
        a.color = None if color is None else color.data_ptr()
        a.alpha = None if alpha is None else alpha.data_ptr()
    return arr


def _integrate_checked_torch(vol, points, checked):
    """The checked views into vol, in order, by _integrate_torch; points = (px, py, pz)."""
    with torch.no_grad():
        for depth, vm, tx, ty, color, alpha, alpha_min, depth_max, z_min in checked:
            _integrate_torch(vol, *points, depth, vm, model_rows.f32(tx), model_rows.f32(ty), color, alpha, model_rows.f32(alpha_min),
                             model_rows.f32(depth_max), model_rows.f32(z_min))


def _resolve_backend(backend, like, what, tensors):
    """The backend a call takes: a CPU volume (`like` is one of its tensors) takes the torch path; on the GPU backend="hip" asks for
    contiguous tensors."""
    if backend == "hip" and not like.is_cuda:
        return "torch"
    if backend == "hip":
        for name, t in tensors:
            if not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous for backend='hip' (call .contiguous())")
    return backend


def _check_extract_args(what, iso, min_weight):
    """(iso, min_weight) of an extract_mesh call as float32 values, or a ValueError."""
    iso, min_weight = model_rows.f32(iso), model_rows.f32(min_weight)
    if not math.isfinite(iso) or not (min_weight > 0 and math.isfinite(min_weight)):
        raise ValueError(f"{what}: iso must be finite and min_weight positive and finite")
    return iso, min_weight


def _extract_hip(scratch_bytes, count, emit, vol, keeps_color, dev, iso, min_weight, flags):
    """The extraction of either volume by the library: scratch of scratch_bytes, `count` (lg_mesh_count, or a sparse volume's counterpart) on the
    volume struct `vol`, the one read-back, the outputs, `emit`; flags: the calling module's profile switch.  Returns (vertices, faces, colors), every vertex kept."""
    with torch.cuda.device(dev):
        scratch = _lib.scratch(scratch_bytes, dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(count(C.byref(vol), iso, min_weight, _lib.ptr(scratch), _lib.ptr(counts), flags, _lib.stream(dev)))
        nv, nf = (int(c) for c in counts.tolist())                     # the one read-back: the caller allocates the outputs
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        colors = torch.empty((nv, 3), dtype=torch.float32, device=dev) if keeps_color else None
        _lib.check(emit(C.byref(vol), iso, min_weight, _lib.ptr(scratch), nv, nf, _lib.ptr(vertices), _lib.ptr(colors), _lib.ptr(faces), flags, _lib.stream(dev)))
    return vertices, faces, colors


class TSDFVolume:
    """A dense TSDF volume: see the module docstring.  origin: three floats (world position of point (0, 0, 0)); dims = (nx, ny, nz);
    trunc defaults to 4 voxel_size; color=False keeps no colour.  The tensors tsdf, weight [nz,ny,nx] and color [nz,ny,nx,3] (or None) are
    public; nx a multiple of 4 keeps every run of the integration on whole 16-byte words."""

    def __init__(self, origin, dims, voxel_size, trunc=None, color=True, device="cuda", backend="hip"):
        check_backend(backend, "TSDFVolume")
        self.origin = tuple(model_rows.f32(v) for v in origin)
        self.dims = tuple(int(v) for v in dims)
        self.voxel_size = model_rows.f32(voxel_size)
        self.trunc = model_rows.f32(4.0 * float(voxel_size) if trunc is None else trunc)
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise ValueError("TSDFVolume: origin and dims have three entries")
        nx, ny, nz = self.dims
        if min(self.dims) < 1 or nx * ny * nz >= MAX_POINTS:
            raise ValueError(f"TSDFVolume: every dimension must be at least 1 and nx ny nz below 2^29, not {self.dims}")
        for name, v in (("voxel_size", self.voxel_size), ("trunc", self.trunc)):
            if not (v > 0 and math.isfinite(v)):
                raise ValueError(f"TSDFVolume: {name} must be positive and finite, not {v}")
        if not all(math.isfinite(v) for v in self.origin):
            raise ValueError("TSDFVolume: origin must be finite")
        self.backend = backend
        self.tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=device)
        self.weight = torch.empty((nz, ny, nx), dtype=torch.float32, device=device)
        self.color = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=device) if color else None
        self.reset()

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.fill_(0.0)
        if self.color is not None:
            self.color.fill_(0.0)

    def _resolve(self, what, tensors):
        return _resolve_backend(self.backend, self.tsdf, what, tensors)

    def _struct(self):
        nx, ny, nz = self.dims
        return lg_tsdf_volume(nx, ny, nz, (C.c_float * 3)(*self.origin), self.voxel_size, self.trunc, self.tsdf.data_ptr(), self.weight.data_ptr(),
                              None if self.color is None else self.color.data_ptr())

    def _own(self):
        return [("tsdf", self.tsdf), ("weight", self.weight)] + ([] if self.color is None else [("color", self.color)])

    def _points(self):
        """(px, py, pz): the world coordinates of the points per axis, shaped to broadcast over [nz,ny,nx]."""
        nx, ny, nz = self.dims
        dev, dt = self.tsdf.device, torch.float32
        o = [model_rows.f32(v) for v in self.origin]
        return ((o[0] + self.voxel_size * torch.arange(nx, dtype=dt, device=dev))[None, None, :],
                (o[1] + self.voxel_size * torch.arange(ny, dtype=dt, device=dev))[None, :, None],
                (o[2] + self.voxel_size * torch.arange(nz, dtype=dt, device=dev))[:, None, None])

    def integrate(self, depth, camera, color=None, alpha=None, alpha_min=0.5, depth_max=0.0, z_min=0.05):
        """One view into the volume: depth [H,W] (view-space z, 0 = nothing), camera (world_view_transform, FoVx, FoVy), color [3,H,W]
        (required by a volume that keeps colour), alpha [H,W] with alpha_min, depth_max (0: none), z_min."""
        self.integrate_many([dict(depth=depth, camera=camera, color=color, alpha=alpha, alpha_min=alpha_min, depth_max=depth_max, z_min=z_min)])

    def integrate_many(self, views):
        """The views, dicts of integrate's arguments, in order: one library call, BATCH views per pass over the volume."""
        what = "TSDFVolume.integrate_many"
        checked, tensors = _check_views(what, list(views), self.tsdf, self.color is not None)
        backend = self._resolve(what, self._own() + tensors)
        if not checked:
            return
        if backend == "torch":
            _integrate_checked_torch(self, self._points(), checked)
            return
        dev = self.tsdf.device
        vol = self._struct()
        with torch.cuda.device(dev):
            _lib.check(load().lg_tsdf_integrate(C.byref(vol), len(checked), _view_array(checked), _flags(), _lib.stream(dev)))

    def extract_mesh(self, iso=0.0, min_weight=1.0, drop_unreferenced=True):
        """(vertices [Nv,3] float32 in world space, faces [Nf,3] int32, colors [Nv,3] or None) of the surface tsdf = iso over the points
        with weight >= min_weight, normals toward larger tsdf.  drop_unreferenced removes the vertices no face names (they lie on edges
        none of whose cells is fully observed) with torch ops and renumbers."""
        what = "TSDFVolume.extract_mesh"
        iso, min_weight = _check_extract_args(what, iso, min_weight)
        if self._resolve(what, self._own()) == "torch":
            with torch.no_grad():
                vertices, faces, colors = _extract_torch(self.tsdf, self.weight, self.color, self.origin, self.voxel_size, iso, min_weight)
        else:
            lib = load()
            vertices, faces, colors = _extract_hip(lib.lg_mesh_scratch_bytes(*self.dims), lib.lg_mesh_count, lib.lg_mesh_emit, self._struct(),
                                                   self.color is not None, self.tsdf.device, iso, min_weight, _flags())
        if drop_unreferenced:
            vertices, faces, colors = drop_unreferenced_vertices(vertices, faces, colors)
        return vertices, faces, colors


# ---- on top of the renderer -----------------------------------------------------------------------------------------------------------
def fuse_views(cameras, model, pipe, volume, depth="median_depth", options=None, alpha_min=0.5, depth_max=0.0, z_min=0.05):
    """Render every camera with gaussian_renderer.render_geometry (no gradients) and integrate its `depth` map ("median_depth", the z of
    the Gaussian that carries the transmittance across one half, or "depth", the expected depth), its colour and its alpha into `volume`,
    BATCH views per pass over the volume.  Returns the number of views."""
    from .gaussian_renderer import render_geometry
    if depth not in ("median_depth", "depth"):
        raise ValueError(f"fuse_views: depth must be 'median_depth' or 'depth', not {depth!r}")
    cameras = list(cameras)
    with torch.no_grad():
        for first in range(0, len(cameras), BATCH):
            views = []
            for cam in cameras[first:first + BATCH]:
                pkg = render_geometry(cam, model, pipe, options=options, distortion=(depth == "median_depth"), geometry_grad=False)
                views.append(dict(depth=pkg[depth].contiguous(), camera=cam, color=pkg["render"].contiguous() if volume.color is not None else None,
                                  alpha=pkg["alpha"].contiguous(), alpha_min=alpha_min, depth_max=depth_max, z_min=z_min))
            volume.integrate_many(views)
    return len(cameras)


def bounds_from_cameras(cameras, voxel_size, scale=1.0, multiple=4):
    """(origin, dims) of a cube about the centroid of the camera centres whose half side is `scale` times the largest distance of a
    camera from it -- cameras that look inward from around a scene enclose it; scale < 1 leaves the cameras outside.  Every dimension is
    rounded up to a multiple of `multiple` (4: whole 16-byte runs)."""
    centres = torch.stack([c.camera_center.detach().double().cpu() for c in cameras])
    mid = centres.mean(dim=0)
    half = float(scale) * float((centres - mid).norm(dim=1).max())
    n = max(2, int(math.ceil(2.0 * half / float(voxel_size))) + 1)
    n = (n + multiple - 1) // multiple * multiple
    origin = tuple(float(m) - 0.5 * (n - 1) * float(voxel_size) for m in mid)
    return origin, (n, n, n)


def save_ply(path, vertices, faces, colors=None):
    """A binary little-endian PLY: float x, y, z (and uchar red, green, blue from colours in [0, 1]) per vertex, one int32 triple per face."""
    v = vertices.detach().cpu().to(torch.float32).numpy()
    f = faces.detach().cpu().to(torch.int32).numpy()
    c = None if colors is None else (colors.detach().cpu().clamp(0, 1) * 255 + 0.5).to(torch.uint8).numpy()
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if c is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        if c is None:
            out.write(v.astype("<f4").tobytes())
        else:
            out.write(b"".join(struct.pack("<3f3B", *row, *col) for row, col in zip(v.tolist(), c.tolist())))
        out.write(b"".join(struct.pack("<B3i", 3, *tri) for tri in f.tolist()))
