"""Seeded synthetic meshes for builder / traversal parity tests (positions, normals|None, tex|None, triangles)."""
import numpy as np


def _soup(n, seed, extent=4.0, size=0.25):
    rng = np.random.default_rng(seed)
    c = (rng.random((n, 1, 3), dtype=np.float32) - 0.5) * extent
    pos = (c + (rng.random((n, 3, 3), dtype=np.float32) - 0.5) * size).reshape(-1, 3).astype(np.float32)
    tri = np.arange(n * 3, dtype=np.uint32).reshape(n, 3)
    return pos, None, None, tri


def _grid(n, seed):
    """Height field n x n quads -> 2 n^2 triangles with smooth normals and uv."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.linspace(-2, 2, n + 1, dtype=np.float32), np.linspace(-2, 2, n + 1, dtype=np.float32))
    z = (0.3 * np.sin(2.1 * xs) * np.cos(1.7 * ys) + 0.02 * rng.random(xs.shape, dtype=np.float32)).astype(np.float32)
    pos = np.stack([xs, z, ys], -1).reshape(-1, 3).astype(np.float32)
    nrm = np.stack([-0.63 * np.cos(2.1 * xs) * np.cos(1.7 * ys), np.ones_like(xs), 0.51 * np.sin(2.1 * xs) * np.sin(1.7 * ys)], -1)
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).reshape(-1, 3).astype(np.float32)
    tex = np.stack([(xs + 2) / 4, (ys + 2) / 4, np.zeros_like(xs)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange((n + 1) * (n + 1), dtype=np.uint32).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    tri = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)]).astype(np.uint32)
    return pos, nrm, tex, tri


def _sphere(n):
    th = np.linspace(0, np.pi, n + 1, dtype=np.float32)
    ph = np.linspace(0, 2 * np.pi, 2 * n + 1, dtype=np.float32)
    T, P = np.meshgrid(th, ph, indexing="ij")
    pos = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], -1).reshape(-1, 3).astype(np.float32)
    nrm = pos.copy()
    tex = np.stack([P / (2 * np.pi), T / np.pi, np.zeros_like(T)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(pos.shape[0], dtype=np.uint32).reshape(n + 1, 2 * n + 1)
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    tri = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)]).astype(np.uint32)
    # drop degenerate pole triangles (two identical positions) -- keeps the set non-trivial but valid
    return pos, nrm, tex, tri


def _walls(n, seed, extent=8.0, snap=0.0):
    """n axis-aligned rectangles (two triangles each) in a cube of side `extent`: leaf and inner boxes with zero thickness along
    the rectangle's normal, so triangles lie ON box faces -- where a box's floating-point slab entry can exceed the distance of a
    triangle it holds (include/minipath_hip.h, consequence 4 of the bounded queries)."""
    rng = np.random.default_rng(seed)
    c = (rng.random((n, 3), dtype=np.float32) - 0.5) * np.float32(extent)
    half = 0.1 + rng.random((n, 2), dtype=np.float32) * 0.9
    axis = rng.integers(0, 3, n)
    if snap:  # walls on the planes of a lattice: many of them end up exactly on a face of their node's box
        c[np.arange(n), axis] = np.round(c[np.arange(n), axis] / np.float32(snap)) * np.float32(snap)
    corners = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float32)
    pos = np.repeat(c[:, None, :], 4, axis=1)
    for k in range(n):
        a, b = [x for x in range(3) if x != axis[k]]
        pos[k, :, a] += corners[:, 0] * half[k, 0]
        pos[k, :, b] += corners[:, 1] * half[k, 1]
    base = (np.arange(n, dtype=np.uint32) * 4)[:, None]
    tri = np.concatenate([base + np.array([0, 1, 2], np.uint32), base + np.array([0, 2, 3], np.uint32)], axis=1).reshape(-1, 3)
    return pos.reshape(-1, 3).astype(np.float32), None, None, tri.astype(np.uint32)


def make(name):
    if name == "walls_600":
        return _walls(600, 17, snap=2.0)
    if name == "soup_300":
        return _soup(300, 11)
    if name == "soup_5000":
        return _soup(5000, 12, extent=10.0, size=0.2)
    if name == "grid_40":
        return _grid(40, 13)
    if name == "sphere_24":
        return _sphere(24)
    if name == "flat_plane":
        # axis-aligned plane: the root box has zero extent in y (NaN path of compress, compressed_geometry.rs:25-46)
        # 50 triangles = a single leaf (a larger planar mesh is unbuildable: see flat_plane_big)
        pos, nrm, tex, tri = _grid(5, 14)
        pos = pos.copy()
        pos[:, 1] = 0.5
        return pos, None, tex, tri
    if name == "flat_plane_big":
        # zero-volume centroid box -> bin_size 0 -> the reference's BinGrid panics (building.rs:424-429)
        pos, nrm, tex, tri = _grid(12, 14)
        pos = pos.copy()
        pos[:, 1] = 0.5
        return pos, None, tex, tri
    if name == "two_clusters":
        p1, _, _, t1 = _soup(200, 15, extent=1.0, size=0.1)
        p2, _, _, t2 = _soup(150, 16, extent=1.0, size=0.1)
        p2 = p2 + np.array([50.0, 3.0, -20.0], np.float32)
        return np.concatenate([p1, p2]).astype(np.float32), None, None, np.concatenate([t1, t2 + p1.shape[0]]).astype(np.uint32)
    if name == "sliver_fan":
        # long thin triangles sharing an apex: many coincident centroids per bin, exact-tie candidates on shared edges
        n = 400
        ang = np.linspace(0, 2 * np.pi, n + 1, dtype=np.float32)
        rim = np.stack([3 * np.cos(ang), 0.4 * np.sin(3 * ang), 3 * np.sin(ang)], -1)
        pos = np.concatenate([np.array([[0, 1.5, 0]], np.float32), rim]).astype(np.float32)
        tri = np.stack([np.zeros(n, np.uint32), np.arange(1, n + 1, dtype=np.uint32), np.arange(2, n + 2, dtype=np.uint32)], -1)
        nrm = np.tile(np.array([[0, 1, 0]], np.float32), (pos.shape[0], 1))
        return pos, nrm, None, tri.astype(np.uint32)
    raise KeyError(name)


def doubled(name, seed=5, keep=None):
    """make(name) with every triangle twice: a second copy of the triangle list (same vertex indices, same order) appended and
    the 2n rows permuted.  Returns (pos, nrm, tex, tri2, copy_id, source): copy_id[i] in {0, 1} = the copy row i came from,
    source[i] = its triangle of make(name).  Twins share a centroid, so the builder bins them together; where both land in one
    packet they decode to the same f32 vertices and every ray that hits one hits the other with the same t, u and v, bit for bit.
    keep = n cuts the mesh down to its first n source triangles before it is doubled (2 n rows)."""
    pos, nrm, tex, tri = make(name)
    if keep is not None:
        tri = tri[:keep]
    n = tri.shape[0]
    perm = np.random.default_rng(seed).permutation(2 * n)
    tri2 = np.ascontiguousarray(np.concatenate([tri, tri])[perm], np.uint32)
    return pos, nrm, tex, tri2, (perm >= n).astype(np.uint32), (perm % n).astype(np.uint32)


STACK_SIZES = (2, 8, 9, 16)


def stack(k):
    """One fixed triangle, oblique to every axis, k times over (k in STACK_SIZES): a whole packet, and a packet plus one, of
    the same triangle.  Returns (pos, None, None, tri)."""
    assert k in STACK_SIZES
    pos = np.array([[-1.25, 0.5, 0.75], [1.5, -0.25, 0.375], [0.125, 1.75, -1.0]], np.float32)
    return pos, None, None, np.tile(np.arange(3, dtype=np.uint32), (k, 1))


def stack_rays(n=32):
    """n x n parallel rays through stack(k)'s triangle, on a grid over its barycentric square (so about half of them hit, and
    some run along its edges), from a point off its plane."""
    pos = stack(2)[0].astype(np.float64)
    e1, e2 = pos[1] - pos[0], pos[2] - pos[0]
    a, b = np.meshgrid(np.linspace(0.0, 1.0, n), np.linspace(0.0, 1.0, n), indexing="ij")
    tgt = pos[0] + a.reshape(-1, 1) * e1 + b.reshape(-1, 1) * e2
    d = np.cross(e1, e2) + 0.3 * e1 - 0.2 * e2
    o = tgt - 1.5 * d
    return o.astype(np.float32), np.tile(d.astype(np.float32), (n * n, 1))


def random_rays(n, seed, bmin, bmax):
    """Rays aimed at random points of the (slightly enlarged) box from random outside/inside origins."""
    rng = np.random.default_rng(seed)
    bmin, bmax = np.asarray(bmin, np.float32), np.asarray(bmax, np.float32)
    ext = bmax - bmin
    ctr = (bmin + bmax) / 2
    o = (ctr + (rng.random((n, 3), dtype=np.float32) - 0.5) * ext * 4.0).astype(np.float32)
    tgt = (bmin - 0.05 * ext + rng.random((n, 3), dtype=np.float32) * ext * 1.1).astype(np.float32)
    d = (tgt - o).astype(np.float32)
    # a few axis-parallel and zero-component directions (inv_direction = +inf path, geometry/mod.rs:47)
    k = max(1, n // 50)
    d[:k, 0] = 0.0
    d[k : 2 * k, 1] = -0.0
    d[2 * k : 3 * k, :2] = 0.0
    d[2 * k : 3 * k, 2] = 1.0
    return o, d
