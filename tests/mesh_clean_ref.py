"""CPU restatement of the mesh-cleaning definition in include/nsr.h ("Mesh cleaning"), NumPy only, for
tests/test_mesh_clean_cpu.py and tests/test_gpu_mesh_clean.py.

labels_union_find(faces, V)       the components as a sequential union-find over the faces (plain loops)
labels_propagation(faces, V)      the same definition written apart from it: label = min over the face's vertices, iterated to
                                  a fixed point (vectorised; a pointer jump label = label[label] a round only shortens the way)
component_stats(verts, faces, labels), keep_rule(stats, ...), filter_components(verts, faces, ...)
plus the synthetic meshes the tests run (cases()) and the thresholds of the surface-nets cases."""
import functools

import numpy as np

import mesh_ref


def good_faces(faces, V):
    """the faces whose three indices all lie in [0, V), as int64, and the number of the others"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(axis=1)
    return f[ok], int((~ok).sum())


def labels_union_find(faces, V):
    f, _ = good_faces(faces, V)
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f.tolist():
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)                   # the root is the tree's smallest id
    return np.asarray([find(v) for v in range(V)], np.int32).reshape(V)


def labels_propagation(faces, V):
    f, _ = good_faces(faces, V)
    label = np.arange(V, dtype=np.int64)
    while True:
        new = label.copy()
        m = label[f].min(axis=1) if len(f) else np.zeros(0, np.int64)
        for k in range(3):
            np.minimum.at(new, f[:, k], m)
        new = new[new]                                              # label[v] is a vertex of v's component: so is its label
        if np.array_equal(new, label):
            return label.astype(np.int32)
        label = new


def _key(x):
    """f32 -> uint32 in the floats' order, -0 below +0"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def component_stats(verts, faces, labels):
    """-> dict(roots int32 [C] ascending, n_verts, n_faces int32 [C], lo, hi f32 [C,3])"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    V = len(verts)
    labels = np.asarray(labels, np.int64)
    roots = np.flatnonzero(labels == np.arange(V))
    f, _ = good_faces(faces, V)
    n_verts = np.bincount(labels, minlength=V)[roots]
    n_faces = np.bincount(labels[f[:, 0]], minlength=V)[roots]
    keys = _key(verts)
    lo = np.full((V, 3), 0xffffffff, np.uint32)
    hi = np.zeros((V, 3), np.uint32)
    for a in range(3):
        np.minimum.at(lo[:, a], labels, keys[:, a])
        np.maximum.at(hi[:, a], labels, keys[:, a])
    return dict(roots=roots.astype(np.int32), n_verts=n_verts.astype(np.int32), n_faces=n_faces.astype(np.int32),
                lo=_unkey(lo[roots]).reshape(-1, 3), hi=_unkey(hi[roots]).reshape(-1, 3))


def diagonal2(stats):
    """dx^2 + dy^2 + dz^2 of every component's box, f32, in this written order"""
    d = (stats['hi'] - stats['lo']).astype(np.float32)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32) + d[:, 2] * d[:, 2]).astype(np.float32)


def keep_rule(stats, min_faces=0, min_diagonal=0.0, keep_largest=None):
    """-> bool [C]"""
    thr = np.float32(min_diagonal) * np.float32(min_diagonal)
    ok = (stats['n_faces'] >= min_faces) & (diagonal2(stats) >= thr)
    if keep_largest is not None:
        order = sorted(np.flatnonzero(ok).tolist(), key=lambda i: (-int(stats['n_faces'][i]), int(stats['roots'][i])))
        ok = np.zeros_like(ok)
        ok[order[:keep_largest]] = True
    return ok


def filter_components(verts, faces, min_faces=0, min_diagonal=0.0, keep_largest=None, labels=None):
    """-> (verts [Vk,3], faces int32 [Fk,3], index_map int32 [V])"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(verts)
    if labels is None:
        labels = labels_propagation(faces, V)
    stats = component_stats(verts, faces, labels)
    keep_root = np.zeros(V, bool)
    keep_root[stats['roots']] = keep_rule(stats, min_faces, min_diagonal, keep_largest)
    keep_v = keep_root[labels]
    index_map = np.where(keep_v, np.cumsum(keep_v) - 1, -1).astype(np.int32)
    f, _ = good_faces(faces, V)
    f = f[keep_v[f[:, 0]]]
    return verts[keep_v], index_map[f].astype(np.int32).reshape(-1, 3), index_map


# ---- synthetic meshes --------------------------------------------------------------------------------------------------------
def _positions(V, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (V, 3)).astype(np.float32)


def strip(n, order, seed=0):
    """n triangles (i, i+1, i+2) over n + 2 vertices whose ids are ascending, descending or a seeded permutation"""
    V = n + 2
    ids = {'ascending': np.arange(V), 'descending': np.arange(V)[::-1], 'permuted': np.random.default_rng(seed).permutation(V)}[order]
    i = np.arange(n)
    return _positions(V, seed + 1), ids[np.stack([i, i + 1, i + 2], 1)].astype(np.int32)


def fan(n):
    """n triangles around one hub whose id is V - 1"""
    V = n + 2
    i = np.arange(n)
    return _positions(V, 7), np.stack([np.full(n, V - 1), i, i + 1], 1).astype(np.int32)


def disjoint_triangles(n, seed=11):
    """n triangles over 3 n shuffled ids; every third one is joined to the next by one more face"""
    ids = np.random.default_rng(seed).permutation(3 * n)
    tri = ids.reshape(n, 3)
    t = np.arange(0, n - 1, 3)
    bridge = np.stack([tri[t, 0], tri[t + 1, 0], tri[t + 1, 1]], 1)
    faces = np.concatenate([tri, bridge])
    faces = faces[np.random.default_rng(seed + 1).permutation(len(faces))]
    return _positions(3 * n, seed + 2), faces.astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (verts f32 [V,3], faces int32 [F,3]): the synthetic meshes of the issue"""
    out = {}
    e = np.zeros((0, 3), np.int32)
    out['no_vertices'] = (np.zeros((0, 3), np.float32), e)
    out['five_singletons'] = (_positions(5, 1), e)
    out['one_triangle'] = (_positions(3, 2), np.asarray([[0, 1, 2]], np.int32))
    out['two_disjoint'] = (_positions(6, 3), np.asarray([[3, 1, 5], [0, 4, 2]], np.int32))
    out['shared_edge'] = (_positions(4, 4), np.asarray([[0, 1, 2], [2, 1, 3]], np.int32))
    out['shared_vertex'] = (_positions(5, 5), np.asarray([[4, 1, 2], [2, 0, 3]], np.int32))
    out['degenerate_face'] = (_positions(5, 6), np.asarray([[3, 3, 1], [0, 2, 4]], np.int32))
    out['duplicate_face'] = (_positions(6, 8), np.asarray([[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 4, 5]], np.int32))
    out['unreferenced_between'] = (_positions(7, 9), np.asarray([[0, 1, 2], [4, 5, 6], [2, 0, 1]], np.int32))   # vertex 3 is in no face
    for order in ('permuted', 'ascending', 'descending'):
        out['strip_' + order] = strip(5000, order)
    out['fan'] = fan(10000)
    out['disjoint_1000'] = disjoint_triangles(1000)
    for v, f in out.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return out


# keep rules every synthetic case is filtered with; the disjoint triangles tie in their face counts
RULES = (dict(), dict(min_faces=1), dict(min_faces=2), dict(keep_largest=1), dict(keep_largest=3), dict(keep_largest=10),
         dict(min_diagonal=1.0), dict(min_faces=2, min_diagonal=1.5, keep_largest=3))

# The issue's volumes, and one of this file's: mesh_ref's two random fields turn out to be one sheet each beside a handful of
# small pieces and unreferenced boundary vertices (7 and 10 components), so `blobs_33` -- 60 balls of radii 0.04 .. 0.3 at seeded
# places, 14 components of 0 .. 11 554 faces, two of them tied at 60 -- is what gives the thresholds something to cut.
SURFACE_CASES = ('two_spheres_9', 'sphere_33', 'random_33', 'random_65_65_33', 'blobs_33')


@functools.lru_cache(maxsize=None)
def surface_volumes():
    """name -> (vol f32, iso, lo, hi)"""
    out = {n: mesh_ref.cases()[n] for n in SURFACE_CASES if n in mesh_ref.cases()}
    rng = np.random.default_rng(4)
    vol = np.full((33, 33, 33), -1.0, np.float32)
    for _ in range(60):
        centre, radius = rng.uniform(-0.9, 0.9, 3), rng.uniform(0.04, 0.3)
        vol = np.maximum(vol, mesh_ref.sphere(vol.shape, tuple(centre), radius))
    vol.setflags(write=False)
    out['blobs_33'] = (vol, 0.0, mesh_ref.LO, mesh_ref.HI)
    return out


@functools.lru_cache(maxsize=None)
def surface_mesh(name):
    """the f32 restatement of the case's surface-nets mesh (the extractor's bits: tests/test_gpu_mesh.py)"""
    return mesh_ref.surface_nets_ref(*surface_volumes()[name])


def lattice_unit(name):
    """the lattice step min_diagonal is counted in: the longest of the case's three steps"""
    vol, _, lo, hi = surface_volumes()[name]
    return float(mesh_ref._box(lo, hi, vol.shape)[1].max())


def surface_rules(name):
    """the keep rules of a surface-nets case: min_faces 2, 8, 64 and min_diagonal 1.5, 3.5 lattice steps"""
    u = lattice_unit(name)
    return tuple(dict(min_faces=m) for m in (2, 8, 64)) + tuple(dict(min_diagonal=k * u) for k in (1.5, 3.5)) + (
        dict(min_faces=8, min_diagonal=3.5 * u, keep_largest=2), dict(keep_largest=1))


def diagonal_margin(stats, min_diagonal):
    """the smallest relative distance of a component's squared diagonal from the threshold"""
    thr = float(np.float32(min_diagonal) * np.float32(min_diagonal))
    d2 = diagonal2(stats).astype(np.float64)
    return float((np.abs(d2 - thr) / thr).min()) if len(d2) and thr > 0 else np.inf
