"""Shared by tests/test_mesh_host.py and tests/test_gpu_mesh.py (test infrastructure): the g++ build of
tests/cpu_harness/lg_tsdf_harness.cpp, the inputs, and the float64 twin of the contract of DESIGN section 10.13.

Inputs.  sphere_views(): analytic z-depth maps of the unit sphere at the pixel centres (0 where the ray misses) under
syn.orbit_camera(k, 6, W, H, radius=4.0, height_y=-1.5 or 0.8), the sizes alternating 33 x 17 and 70 x 45, with random colour images and a
random alpha map.  volume_spec(): a grid centred on the origin that spans 3 units along its longest axis, moved by a small
irrational-looking offset so that nothing is lattice-aligned by accident.

The twin.  twin_integrate() is section 2 of the contract in numpy float64 and also returns, per (point, view), whether the view updated the
point and the distance to the nearest decision: |fx - round(fx)| and |fy - round(fy)| in pixels, |sdf + trunc| / trunc, |z - z_min| in world
units.  A pair within MARGIN (1e-4) of one of them is left out of the comparisons, and a point's values when one of its pairs is; the
float32 loop decides every other pair as float64 does.  twin_extract() is section 3 in numpy, any dtype, with its own derivation of the
triangle table from the rule (tet_table)."""
import ctypes as C
import itertools

import numpy as np

import common
from common import bits, f32, ptr, syn  # noqa: F401

MARGIN = 1e-4
MAX_LEFT_OUT = 0.01
B = 8                                   # LG_TSDF_BATCH
GRIDS = ((1, 1, 1), (2, 2, 2), (3, 2, 2), (5, 4, 3), (65, 3, 2), (67, 5, 3), (24, 20, 16))
IMAGES = ((1, 1), (33, 17), (70, 45))
SLOT_MASKS = (1, 2, 4, 3, 5, 6, 7)
PERMS = tuple(itertools.permutations(range(3)))


def harness():
    P, F, I = C.c_void_p, C.c_float, C.c_int
    return common.build_harness("tsdf", headers=(common.LG_MATH_H,), flags=common.STRICT_FP_FMA, signatures={
        "h_tsdf_integrate": (None, [I, I, I, P, F, F, P, P, P, I, P, P, P, P, P, P, P]),
        "h_mesh_count": (None, [I, I, I, P, P, F, F, P]),
        "h_mesh_extract": (None, [I, I, I, P, F, P, P, P, F, F, P, P, P, P, P])})


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def volume_spec(dims, span=3.0):
    """(origin, voxel_size, trunc) of a grid of dims = (nx, ny, nz) points about the origin."""
    voxel = span / max(max(dims) - 1, 1)
    off = np.array([0.0123456, -0.0071234, 0.0049871])
    origin = -0.5 * voxel * (np.array(dims) - 1) + off
    return tuple(np.float32(origin).tolist()), float(np.float32(voxel)), float(np.float32(4.0 * np.float32(voxel)))


def sphere_depth(cam, W, H, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """z-depth [H,W] (float64) of the sphere under the camera at the pixel centres; 0 where the ray misses."""
    import math
    vm = cam.world_view_transform.double().numpy()
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    c = np.append(np.asarray(centre, np.float64), 1.0) @ vm                 # the centre in view space
    rx = ((2 * np.arange(W) + 1) / W - 1) * tx
    ry = ((2 * np.arange(H) + 1) / H - 1) * ty
    d = np.stack([np.broadcast_to(rx[None, :], (H, W)), np.broadcast_to(ry[:, None], (H, W)), np.ones((H, W))], axis=-1)     # the ray with z = 1
    a, b, cc = (d * d).sum(-1), -2 * (d @ c[:3]), c[:3] @ c[:3] - radius * radius
    disc = b * b - 4 * a * cc
    s = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
    return np.where((disc > 0) & (s > 0), s, 0.0)


_VIEWS = {}


def sphere_views(n, sizes=((33, 17), (70, 45)), seed=0):
    """n views: dict(cam, W, H, tanfov, vm [16], depth, color [3,H,W], alpha [H,W]) in float32 numpy; view k uses sizes[k % len(sizes)].
    Computed once per key and shared."""
    import math
    key = (n, tuple(sizes), seed)
    if key not in _VIEWS:
        rs = np.random.RandomState(100 + seed)
        out = []
        for k in range(n):
            W, H = sizes[k % len(sizes)]
            cam = syn.orbit_camera(k % 6, 6, W, H, radius=4.0, height_y=-1.5 if (k // 6 + k) % 2 == 0 else 0.8)
            out.append(dict(cam=cam, W=W, H=H, tanfov=(math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)),
                            vm=np.ascontiguousarray(cam.world_view_transform.numpy(), np.float32).reshape(16),
                            depth=sphere_depth(cam, W, H).astype(np.float32), color=rs.uniform(0, 1, (3, H, W)).astype(np.float32),
                            alpha=rs.uniform(0.3, 1.0, (H, W)).astype(np.float32)))
        _VIEWS[key] = out
    return _VIEWS[key]


def seeded_volume(dims, color=True, seed=0):
    """A volume that has seen things: random tsdf in [-1, 1], integer weights 0 .. 5, random colours."""
    nx, ny, nz = dims
    rs = np.random.RandomState(7 + seed + nx * 131 + ny * 17 + nz)
    return (rs.uniform(-1, 1, (nz, ny, nx)).astype(np.float32), rs.randint(0, 6, (nz, ny, nx)).astype(np.float32),
            rs.uniform(0, 1, (nz, ny, nx, 3)).astype(np.float32) if color else None)


def fresh_volume(dims, color=True):
    nx, ny, nz = dims
    return (np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx, 3), np.float32) if color else None)


# ---- the harness --------------------------------------------------------------------------------------------------------------------
def harness_integrate(dims, origin, voxel, trunc, state, views, *, use_alpha=False, alpha_min=0.5, depth_max=0.0, z_min=0.05, decided=False):
    """state = (tsdf, weight, color or None) is copied; returns the new state (and the decisions [n, P] when asked)."""
    nx, ny, nz = dims
    tsdf, weight = state[0].copy(), state[1].copy()
    color = None if state[2] is None else state[2].copy()
    n = len(views)
    wh = np.array([[v["W"], v["H"]] for v in views], np.int32).reshape(-1, 2)
    cam = np.array([[v["tanfov"][0], v["tanfov"][1], depth_max, z_min, alpha_min] for v in views], np.float32).reshape(-1, 5)
    vms = np.ascontiguousarray(np.stack([v["vm"] for v in views]) if n else np.zeros((0, 16)), np.float32)
    arr = lambda key, on=True: (C.c_void_p * max(n, 1))(*[v[key].ctypes.data if on else None for v in views])  # noqa: E731
    dec = np.zeros((n, nx * ny * nz), np.uint8) if decided else None
    harness().h_tsdf_integrate(nx, ny, nz, ptr(f32(np.array(origin))), voxel, trunc, ptr(tsdf), ptr(weight), ptr(color), n, ptr(wh), ptr(cam), ptr(vms),
                               arr("depth"), arr("color", color is not None), arr("alpha", use_alpha), ptr(dec))
    return ((tsdf, weight, color), dec) if decided else (tsdf, weight, color)


def harness_counts(tsdf, weight, iso=0.0, min_weight=1.0):
    nz, ny, nx = tsdf.shape
    counts = np.zeros(2, np.int64)
    harness().h_mesh_count(nx, ny, nz, ptr(f32(tsdf)), ptr(f32(weight)), iso, min_weight, ptr(counts))
    return int(counts[0]), int(counts[1])


def harness_extract(tsdf, weight, color, origin, voxel, iso=0.0, min_weight=1.0):
    """dict(vertices, faces, colors, cell_of_face, used [6,16]) of the harness."""
    nz, ny, nx = tsdf.shape
    tsdf, weight, color = f32(tsdf), f32(weight), f32(color)
    nv, nf = harness_counts(tsdf, weight, iso, min_weight)
    out = dict(vertices=np.full((nv, 3), np.nan, np.float32), faces=np.full((nf, 3), -1, np.int32), colors=None if color is None else np.full((nv, 3), np.nan, np.float32),
               cell_of_face=np.full(nf, -1, np.int64), used=np.zeros((6, 16), np.int64))
    harness().h_mesh_extract(nx, ny, nz, ptr(f32(np.array(origin))), voxel, ptr(tsdf), ptr(weight), ptr(color), iso, min_weight, ptr(out["vertices"]),
                             ptr(out["colors"]), ptr(out["faces"]), ptr(out["cell_of_face"]), ptr(out["used"]))
    return out


# ---- the float64 twin: integration --------------------------------------------------------------------------------------------------
def twin_integrate(dims, origin, voxel, trunc, state, views, *, use_alpha=False, alpha_min=0.5, depth_max=0.0, z_min=0.05, dtype=np.float64):
    """(state, decided [n, P] bool, near [n, P] bool): the contract in `dtype` on the float32 inputs; near = the pair lies within MARGIN of
    one of its decisions."""
    nx, ny, nz = dims
    dt = dtype
    tsdf, weight = state[0].astype(dt), state[1].astype(dt)
    color = None if state[2] is None else state[2].astype(dt)
    o = np.asarray(origin, np.float32).astype(dt)
    vx_, tr = dt(np.float32(voxel)), dt(np.float32(trunc))
    px = (o[0] + vx_ * np.arange(nx).astype(dt))[None, None, :]
    py = (o[1] + vx_ * np.arange(ny).astype(dt))[None, :, None]
    pz = (o[2] + vx_ * np.arange(nz).astype(dt))[:, None, None]
    decided, near = [], []
    with np.errstate(all="ignore"):
        for v in views:
            vm = v["vm"].astype(dt).reshape(4, 4)
            W, H = v["W"], v["H"]
            tx, ty = dt(np.float32(v["tanfov"][0])), dt(np.float32(v["tanfov"][1]))
            zmin, dmax, amin = dt(np.float32(z_min)), dt(np.float32(depth_max)), dt(np.float32(alpha_min))
            x = vm[0, 0] * px + vm[1, 0] * py + vm[2, 0] * pz + vm[3, 0]
            y = vm[0, 1] * px + vm[1, 1] * py + vm[2, 1] * pz + vm[3, 1]
            z = vm[0, 2] * px + vm[1, 2] * py + vm[2, 2] * pz + vm[3, 2]
            nr = np.abs(z - zmin) < MARGIN
            ok = z > zmin
            fx = (x / (z * tx) + 1) * (dt(0.5) * W)
            fy = (y / (z * ty) + 1) * (dt(0.5) * H)
            nr |= ok & ((np.abs(fx - np.round(fx)) < MARGIN) | (np.abs(fy - np.round(fy)) < MARGIN))
            flx, fly = np.floor(fx), np.floor(fy)
            ok = ok & (flx >= 0) & (flx < W) & (fly >= 0) & (fly < H)
            pix = np.where(ok, fly, 0).astype(np.int64) * W + np.where(ok, flx, 0).astype(np.int64)
            d = v["depth"].astype(dt).reshape(-1)[pix]
            ok = ok & (d > 0) & np.isfinite(d)
            if depth_max > 0:
                ok = ok & ~(d > dmax)
            if use_alpha:
                ok = ok & ~(v["alpha"].astype(dt).reshape(-1)[pix] < amin)
            sdf = d - z
            nr |= ok & (np.abs(sdf + tr) / tr < MARGIN)
            ok = ok & ~(sdf < -tr)
            t = np.minimum(dt(1), sdf / tr)
            w1 = weight + 1
            tsdf = np.where(ok, (tsdf * weight + t) / w1, tsdf)
            if color is not None:
                img = np.moveaxis(v["color"].astype(dt).reshape(3, -1)[:, pix], 0, -1)
                color = np.where(ok[..., None], (color * weight[..., None] + img) / w1[..., None], color)
            weight = np.where(ok, w1, weight)
            decided.append(ok.reshape(-1)); near.append(nr.reshape(-1))
    P = nx * ny * nz
    return (tsdf, weight, color), np.array(decided).reshape(len(views), P), np.array(near).reshape(len(views), P)


# ---- the float64 twin: marching tetrahedra --------------------------------------------------------------------------------------------
def offset(m):
    return np.array([m & 1, (m >> 1) & 1, (m >> 2) & 1])


def tet_corners(t):
    a, b, _c = PERMS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def tet_table():
    """{(t, mask): [triangle, ...]}, a triangle = three edges (lo, hi) of local corners, from the rule of the contract: the listed order,
    with the 2nd and 3rd swapped where the normal on the unit cube (edge midpoints) points from the outside corners to the inside ones."""
    table = {}
    for t in range(6):
        pos = [offset(m).astype(np.float64) for m in tet_corners(t)]
        for mask in range(16):
            ins = [i for i in range(4) if (mask >> i) & 1]
            out = [i for i in range(4) if not (mask >> i) & 1]
            e = lambda u, v: (min(u, v), max(u, v))  # noqa: E731
            if len(ins) in (0, 4):
                tris = []
            elif len(ins) == 2:
                q = [e(ins[0], out[0]), e(ins[0], out[1]), e(ins[1], out[1]), e(ins[1], out[0])]
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            else:
                a = ins[0] if len(ins) == 1 else out[0]
                tris = [[e(a, o) for o in range(4) if o != a]]
            done = []
            for tri in tris:
                v = [(pos[lo] + pos[hi]) / 2 for lo, hi in tri]
                n = np.cross(v[1] - v[0], v[2] - v[0])
                toward_inside = np.mean([pos[i] for i in ins], axis=0) - np.mean([pos[i] for i in out], axis=0)
                done.append([tri[0], tri[2], tri[1]] if n @ toward_inside > 0 else list(tri))
            table[(t, mask)] = done
    return table


_TABLE = tet_table()


def twin_extract(tsdf, weight, color, origin, voxel, iso=0.0, min_weight=1.0, dtype=np.float64):
    """dict(vertices, faces, colors, cell_of_face, used [6,16]) of the contract in `dtype`: loops over slots and tetrahedra, numpy over points."""
    dt = dtype
    nz, ny, nx = tsdf.shape
    f, w = np.asarray(tsdf).astype(dt), np.asarray(weight).astype(dt)
    P = nx * ny * nz
    obs, ins = (w >= dt(min_weight)).reshape(-1), (f < dt(iso)).reshape(-1)
    lin = np.arange(P)
    X, Y, Z = lin % nx, (lin // nx) % ny, lin // (nx * ny)

    def neighbour(m):           # (index of p + offset(m), it exists)
        o = offset(m)
        return lin + o[0] + o[1] * nx + o[2] * nx * ny, (X + o[0] < nx) & (Y + o[1] < ny) & (Z + o[2] < nz)

    carry = np.zeros((P, 7), bool)
    for k, m in enumerate(SLOT_MASKS):
        q, exists = neighbour(m)
        qq = np.where(exists, q, 0)
        carry[:, k] = exists & obs & obs[qq] & (ins != ins[qq])
    ids = (np.cumsum(carry.reshape(-1)) - carry.reshape(-1)).reshape(P, 7)
    p, k = np.nonzero(carry)                         # row-major: by point, then slot
    m = np.array(SLOT_MASKS)[k]
    off = np.stack([m & 1, (m >> 1) & 1, (m >> 2) & 1], axis=1)
    q = p + off[:, 0] + off[:, 1] * nx + off[:, 2] * nx * ny
    ff = f.reshape(-1) - dt(iso)
    with np.errstate(all="ignore"):
        t = ff[p] / (ff[p] - ff[q])
    grid = np.stack([X[p], Y[p], Z[p]], axis=1).astype(dt)
    vertices = np.asarray(origin, np.float32).astype(dt) + dt(np.float32(voxel)) * (grid + t[:, None] * off.astype(dt))
    colors = None
    if color is not None:
        c = np.asarray(color).astype(dt).reshape(-1, 3)
        colors = c[p] + t[:, None] * (c[q] - c[p])
    faces, cell_of_face, used = [], [], np.zeros((6, 16), np.int64)
    if min(nx, ny, nz) >= 2:
        valid = (X < nx - 1) & (Y < ny - 1) & (Z < nz - 1)
        corner_idx = []
        for cm in range(8):
            qc, exists = neighbour(cm)
            qc = np.where(exists, qc, 0)
            valid &= exists & obs[qc]
            corner_idx.append(qc)
        cells = np.nonzero(valid)[0]
        per_cell = [[] for _ in range(len(cells))]
        for t_ in range(6):
            cm = tet_corners(t_)
            m4 = sum(ins[corner_idx[c][cells]].astype(np.int64) << i for i, c in enumerate(cm))
            for mask in range(16):
                hit = np.nonzero(m4 == mask)[0]
                used[t_, mask] = len(hit)
                for tri in _TABLE[(t_, mask)]:
                    vid = np.stack([ids[corner_idx[cm[lo]][cells[hit]], SLOT_MASKS.index(cm[hi] ^ cm[lo])] for lo, hi in tri], axis=1)
                    for j, c in enumerate(hit):
                        per_cell[c].append(vid[j])
        for c, tris in enumerate(per_cell):          # appended by tetrahedron, then mask (one per tetrahedron), then triangle: the contract's order
            faces += tris
            cell_of_face += [cells[c]] * len(tris)
    return dict(vertices=vertices, faces=np.array(faces, np.int64).reshape(-1, 3), colors=colors, cell_of_face=np.array(cell_of_face, np.int64), used=used)


# ---- fields and mesh properties -----------------------------------------------------------------------------------------------------
def grid_points(dims, origin, voxel):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.asarray(origin, np.float64) + voxel * np.stack([x, y, z], axis=-1)


def sphere_field(dims, origin, voxel, radius, centre=(0.0, 0.0, 0.0), trunc=None):
    """(tsdf, weight = 1) of a sphere, clipped to [-1, 1] in units of trunc (default 4 voxels)."""
    trunc = 4 * voxel if trunc is None else trunc
    d = np.linalg.norm(grid_points(dims, origin, voxel) - np.asarray(centre), axis=-1) - radius
    return np.clip(d / trunc, -1, 1).astype(np.float32), np.ones(d.shape, np.float32)


def torus_field(dims, origin, voxel, R, r):
    pts = grid_points(dims, origin, voxel)
    d = np.sqrt((np.sqrt(pts[..., 0] ** 2 + pts[..., 2] ** 2) - R) ** 2 + pts[..., 1] ** 2) - r
    return np.clip(d / (4 * voxel), -1, 1).astype(np.float32), np.ones(d.shape, np.float32)


def random_field(dims, seed=0, observed=0.8):
    """Random signs with a random observed mask: meets every entry of the triangle table."""
    nx, ny, nz = dims
    rs = np.random.RandomState(900 + seed)
    return (rs.uniform(-1, 1, (nz, ny, nx)).astype(np.float32), (rs.uniform(0, 1, (nz, ny, nx)) < observed).astype(np.float32) * 2,
            rs.uniform(0, 1, (nz, ny, nx, 3)).astype(np.float32))


def mesh_properties(vertices, faces):
    """dict(closed, euler, volume): every directed edge once with its reverse once; V - E + F over the referenced vertices; the signed
    volume (positive for outward normals)."""
    faces = np.asarray(faces, np.int64)
    v = np.asarray(vertices, np.float64)
    directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    keys = directed[:, 0] * (len(v) + 1) + directed[:, 1]
    rev = directed[:, 1] * (len(v) + 1) + directed[:, 0]
    uniq, counts = np.unique(keys, return_counts=True)
    closed = bool((counts == 1).all() and np.isin(rev, uniq).all() and len(faces) > 0)
    und = np.unique(np.sort(directed, axis=1), axis=0)
    euler = len(np.unique(faces)) - len(und) + len(faces)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return dict(closed=closed, euler=int(euler), volume=float((a * np.cross(b, c)).sum() / 6.0))
