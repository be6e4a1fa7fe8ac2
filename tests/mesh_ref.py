"""CPU restatement of the surface-nets definition in include/nsr.h ("Mesh export"), NumPy only, for tests/test_mesh_cpu.py and
tests/test_gpu_mesh.py.

surface_nets_ref(vol, iso, lo, hi)                  the definition in f32, the same edge order and the same operation order as
                                                    the kernel: every NumPy ufunc rounds once, so the vertices are the kernel's
                                                    bits where its divide is IEEE and nothing is contracted
surface_nets_ref(vol, iso, lo, hi, np.float64)      the same definition from the same f32 volume, f32 iso and f32 step,
                                                    evaluated in fp64
surface_nets_loop(vol, iso, lo, hi)                 the definition once more as plain loops over cells and edges (small volumes):
                                                    written apart from the vectorised one, the CPU tests compare the two
plus the mesh properties the tests ask for (edge use, signed volume, Euler characteristic) and the test volumes."""
import functools

import numpy as np

EDGES = ((0, 4), (1, 5), (2, 6), (3, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 1), (2, 3), (4, 5), (6, 7))
EPS32 = float(np.finfo(np.float32).eps)


def _box(lo, hi, shape):
    lo32 = np.broadcast_to(np.asarray(lo, np.float32), (3,)).copy()
    hi32 = np.broadcast_to(np.asarray(hi, np.float32), (3,)).copy()
    step = ((hi32 - lo32) / np.asarray([s - 1 for s in shape], np.float32)).astype(np.float32)
    return lo32, step


def vertex_tolerance(lo, hi):
    """the issue's bound on |vertex - fp64 restatement| per coordinate"""
    return 32.0 * EPS32 * max(float(np.abs(np.asarray(lo, np.float64)).max()), float(np.abs(np.asarray(hi, np.float64)).max()), 1.0)


def surface_nets_ref(vol, iso, lo, hi, dtype=np.float32):
    """-> (verts dtype [V,3], faces int32 [F,3])"""
    vol = np.ascontiguousarray(vol, np.float32)
    R0, R1, R2 = vol.shape
    ft = np.dtype(dtype).type
    lo32, step32 = _box(lo, hi, vol.shape)
    lo_t, step_t, iso_t = lo32.astype(ft), step32.astype(ft), ft(np.float32(iso))
    inside = vol > np.float32(iso)                              # a NaN compares False: outside
    n = (R0 - 1, R1 - 1, R2 - 1)

    def corner(a, q):
        dx, dy, dz = q >> 2, (q >> 1) & 1, q & 1
        return a[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]]

    n_in = sum(corner(inside, q).astype(np.uint8) for q in range(8))
    cells = np.flatnonzero(((n_in > 0) & (n_in < 8)).ravel())   # ascending linear cell index: the vertex ids
    ci = np.unravel_index(cells, n)
    vals = [corner(vol, q)[ci].astype(ft) for q in range(8)]
    ins = [corner(inside, q)[ci] for q in range(8)]
    coord = [[lo_t[a] + (ci[a] + d).astype(ft) * step_t[a] for d in (0, 1)] for a in range(3)]
    total = [np.zeros(cells.size, ft) for _ in range(3)]
    count = np.zeros(cells.size, np.int64)
    half = ft(0.5)
    with np.errstate(all='ignore'):
        for e, (qa, qb) in enumerate(EDGES):
            axis = e >> 2
            ia, ib = ins[qa], ins[qb]
            cross = ia != ib
            va, vb = np.where(ia, vals[qb], vals[qa]), np.where(ia, vals[qa], vals[qb])      # a: the outside end
            t = (iso_t - va) / (vb - va)
            t = np.where((t >= 0) & (t <= 1), t, half)
            p = [coord[a][(qa >> (2 - a)) & 1] for a in range(3)]
            pa, pb = np.where(ia, coord[axis][1], coord[axis][0]), np.where(ia, coord[axis][0], coord[axis][1])
            p[axis] = pa + t * (pb - pa)
            for a in range(3):
                total[a] = np.where(cross, total[a] + p[a], total[a])
            count += cross
        verts = np.stack([total[a] / count.astype(ft) for a in range(3)], axis=1).astype(ft) if cells.size else np.zeros((0, 3), ft)

    # faces
    ncells = n[0] * n[1] * n[2]
    cell_vertex = np.full(ncells, -1, np.int64)
    cell_vertex[cells] = np.arange(cells.size)
    in0 = inside[:-1, :-1, :-1]
    ends = (inside[1:, :-1, :-1], inside[:-1, 1:, :-1], inside[:-1, :-1, 1:])
    idx = np.ogrid[0:n[0], 0:n[1], 0:n[2]]
    strides = (n[1] * n[2], n[2], 1)
    owners, axes = [], []
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3
        own = np.flatnonzero(((in0 != ends[a]) & (idx[u] >= 1) & (idx[w] >= 1)).ravel())
        owners.append(own)
        axes.append(np.full(own.size, a, np.int64))
    owners, axes = np.concatenate(owners), np.concatenate(axes)
    order = np.argsort(owners * 3 + axes, kind='stable')
    c, a = owners[order], axes[order]
    su, sw = np.asarray(strides)[(a + 1) % 3], np.asarray(strides)[(a + 2) % 3]
    v0, v1, v2, v3 = cell_vertex[c - su - sw], cell_vertex[c - sw], cell_vertex[c], cell_vertex[c - su]
    keep = in0.ravel()[c]
    w1, w3 = np.where(keep, v1, v3), np.where(keep, v3, v1)
    faces = np.stack([v0, w1, v2, v0, v2, w3], axis=1).reshape(-1, 3)
    assert faces.size == 0 or faces.min() >= 0
    return verts, faces.astype(np.int32)


def surface_nets_loop(vol, iso, lo, hi):
    """The definition as loops, f32; for small volumes."""
    f = np.float32
    vol = np.asarray(vol, np.float32)
    R0, R1, R2 = vol.shape
    lo32, step = _box(lo, hi, vol.shape)
    iso = f(iso)

    def inside(i, j, k):
        return bool(vol[i, j, k] > iso)

    def point(i, j, k):
        return [lo32[0] + f(i) * step[0], lo32[1] + f(j) * step[1], lo32[2] + f(k) * step[2]]

    ids, verts = {}, []
    with np.errstate(all='ignore'):
        for cx in range(R0 - 1):
            for cy in range(R1 - 1):
                for cz in range(R2 - 1):
                    corners = [(cx + (q >> 2), cy + ((q >> 1) & 1), cz + (q & 1)) for q in range(8)]
                    flags = [inside(*p) for p in corners]
                    if all(flags) or not any(flags):
                        continue
                    total, count = [f(0), f(0), f(0)], 0
                    for e, (qa, qb) in enumerate(EDGES):
                        if flags[qa] == flags[qb]:
                            continue
                        out_q, in_q = (qb, qa) if flags[qa] else (qa, qb)
                        va, vb = vol[corners[out_q]], vol[corners[in_q]]
                        t = (iso - va) / (vb - va)
                        if not (t >= 0 and t <= 1):
                            t = f(0.5)
                        pa, pb = point(*corners[out_q]), point(*corners[in_q])
                        axis = e >> 2
                        p = list(pa)
                        p[axis] = pa[axis] + t * (pb[axis] - pa[axis])
                        total = [total[a] + p[a] for a in range(3)]
                        count += 1
                    ids[(cx, cy, cz)] = len(verts)
                    verts.append([total[a] / f(count) for a in range(3)])
    faces = []
    for cx in range(R0 - 1):
        for cy in range(R1 - 1):
            for cz in range(R2 - 1):
                c = (cx, cy, cz)
                for a in range(3):
                    u, w = (a + 1) % 3, (a + 2) % 3
                    far = list(c)
                    far[a] += 1
                    if inside(*c) == inside(*far) or c[u] < 1 or c[w] < 1:
                        continue

                    def back(du, dw):
                        n = list(c)
                        n[u] -= du
                        n[w] -= dw
                        return ids[tuple(n)]
                    quad = [back(1, 1), back(0, 1), back(0, 0), back(1, 0)]
                    if not inside(*c):
                        quad = [quad[0], quad[3], quad[2], quad[1]]
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)


# ---- mesh properties -----------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_use(faces):
    """-> (counts of every undirected edge, the largest count of a directed edge)"""
    d = directed_edges(faces)
    _, cd = np.unique(d, axis=0, return_counts=True)
    _, cu = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    return cu, int(cd.max()) if cd.size else 0


def is_closed(faces):
    """every undirected edge in exactly two triangles, once in each direction"""
    cu, dmax = edge_use(faces)
    return bool(cu.size) and bool((cu == 2).all()) and dmax == 1


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


def euler_characteristic(verts, faces):
    cu, _ = edge_use(faces)
    return int(len(verts)) - int(cu.size) + int(len(faces))


# ---- test volumes --------------------------------------------------------------------------------------------------------
LO, HI = (-1.0, -0.5, 0.25), (1.5, 2.0, 3.0)                    # three different extents: a swapped axis shows


def grid(shape):
    """index coordinates scaled to [-1, 1] an axis"""
    return np.meshgrid(*[np.linspace(-1.0, 1.0, s) for s in shape], indexing='ij')


def sphere(shape, centre=(0.0, 0.0, 0.0), radius=0.6):
    x, y, z = grid(shape)
    return (radius ** 2 - ((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def torus(shape, R=0.6, r=0.25):
    x, y, z = grid(shape)
    return (r ** 2 - ((np.sqrt(x * x + y * y) - R) ** 2 + z * z)).astype(np.float32)


def smooth_random(shape, seed):
    rng = np.random.default_rng(seed)
    x, y, z = grid(shape)
    out = np.zeros(shape, np.float64)
    for _ in range(5):
        k = rng.uniform(1.0, 7.0, 3)
        ph = rng.uniform(0.0, 2 * np.pi, 3)
        out += rng.uniform(0.5, 1.0) * np.sin(k[0] * x + ph[0]) * np.sin(k[1] * y + ph[1]) * np.sin(k[2] * z + ph[2])
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (vol f32, iso, lo, hi): the volumes of the issue"""
    out = {}
    v = np.zeros((2, 2, 2), np.float32)
    v[1, 0, 1] = 1.0
    out['one_corner_2'] = (v, 0.25, LO, HI)
    v = np.zeros((3, 3, 3), np.float32)
    v[1, 1, 1] = 2.0
    out['centre_3'] = (v, 0.5, LO, HI)
    out['all_outside'] = (np.full((4, 5, 6), -1.0, np.float32), 0.0, LO, HI)
    out['all_inside'] = (np.full((4, 5, 6), 1.0, np.float32), 0.0, LO, HI)
    out['all_iso'] = (np.full((4, 5, 6), 0.75, np.float32), 0.75, LO, HI)
    v = sphere((12, 12, 12), radius=0.7)
    rng = np.random.default_rng(3)
    v.reshape(-1)[rng.choice(v.size, 60, replace=False)] = np.nan
    v[6, 6, 2], v[2, 6, 6], v[6, 9, 6] = np.nan, np.nan, np.nan      # on and beside the surface
    out['sphere_nan'] = (v, 0.0, LO, HI)
    out['sphere_567'] = (sphere((5, 6, 7), centre=(0.2, -0.1, 0.15), radius=0.55), 0.0, LO, HI)
    a, b = sphere((9, 9, 9), (-0.4, 0.0, 0.0), 0.4), sphere((9, 9, 9), (0.4, 0.0, 0.0), 0.4)
    out['two_spheres_9'] = (np.maximum(a, b), 0.0, LO, HI)
    x, y, z = grid((9, 9, 9))
    out['plane_9'] = ((0.31 * x + 0.47 * y + z + 0.013).astype(np.float32), 0.0, LO, HI)
    out['sphere_17_9_9'] = (sphere((17, 9, 9), radius=0.7), 0.0, LO, HI)
    out['random_33'] = (smooth_random((33, 33, 33), 1), 0.1, LO, HI)
    out['random_65_65_33'] = (smooth_random((65, 65, 33), 2), -0.05, LO, HI)
    # 32^3 cells in blocks of 256: the last block is cx = 31, cy >= 24; the first cx = 0, cy < 8.  A point on the x = 32 (x = 0)
    # plane makes cells of cx = 31 (cx = 0) only active, and its x-edge a quad whose four cells lie in that block
    v = np.zeros((33, 33, 33), np.float32)
    v[32, 28, 16] = v[32, 32, 32] = 1.0
    out['last_block_33'] = (v, 0.5, LO, HI)
    v = np.zeros((33, 33, 33), np.float32)
    v[0, 3, 5] = v[0, 0, 0] = 1.0
    out['first_block_33'] = (v, 0.5, LO, HI)
    out['sphere_33'] = (sphere((33, 33, 33), centre=(0.1, -0.05, 0.0), radius=0.62), 0.0, LO, HI)
    for vol, _, _, _ in out.values():
        vol.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(f32 restatement, fp64 restatement) of a case, computed once and shared"""
    vol, iso, lo, hi = cases()[name]
    return surface_nets_ref(vol, iso, lo, hi), surface_nets_ref(vol, iso, lo, hi, np.float64)
