"""Mesh export: the density field's iso-surface as an indexed triangle mesh (torch-ngp's / instant-ngp's `save_mesh`, which the
reference predates).  The extractor is naive surface nets on the device (csrc/surface_nets.hip; include/nsr.h, "Mesh export",
states the definition): one vertex per sign-changing cell, one quad per sign-changing lattice edge, vertex ids and face order a
pure function of the volume, no atomics.

    mesh = renderer.extract_mesh(resolution=256, iso=10.0)     # verts, faces, colours, normals, region labels
    mesh.save_ply('scene.ply')

or by hand: `density_volume` samples sigma on a lattice with the fused sigma-only forward, `surface_nets` turns any device volume
into (verts, faces).  NOT capture-legal: the sizes of the outputs are known only after a count, so `surface_nets` reads two
integers back on the host between its two launches (and nsr_surface_nets_emit checks them once more).  Opt-in: nothing else in
the package calls it.

Mesh cleaning (csrc/mesh_clean.hip; include/nsr.h, "Mesh cleaning"): `connected_components` labels every vertex with the smallest
vertex id of its component (a lock-free union-find on the device whose result does not depend on the interleaving),
`component_stats` gives each component's vertex and face counts and its box, `filter_components` / `Mesh.clean` /
`extract_mesh(min_faces=..., min_diagonal=..., keep_largest=...)` drop whole components -- the floaters of a NeRF density --
and re-index what stays, order preserved, bit for bit a function of the input.  The same host reads, so not capture-legal
either."""
import ctypes
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L

MAX_RESOLUTION = 1024


def _triple(x, what, dtype):
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError('{} must be a scalar or three values; got {}'.format(what, a.size))
    return a.astype(dtype)


def lattice_step(lo, hi, shape):
    """(lo, step) as f32 [3] arrays: step = (hi - lo) / (R - 1), formed in f32 (the definition's host arithmetic)."""
    lo32, hi32 = _triple(lo, 'lo', np.float32), _triple(hi, 'hi', np.float32)
    r = np.asarray([int(s) - 1 for s in shape], np.float32)
    return lo32, ((hi32 - lo32) / r).astype(np.float32)


def surface_nets(volume, iso, lo, hi):
    """Iso-surface of a device volume [R0,R1,R2] (f32, 2 <= R <= 1024 an axis) whose lattice point (i,j,k) sits at
    lo + (i,j,k) * (hi - lo) / (R - 1)  ->  (verts f32 [V,3], faces int32 [F,3]).  Inside is volume > iso (a NaN is outside);
    the faces' right-hand normals point from inside to outside.  Empty results are [0,3] tensors.  One host read of the two
    counts between the launches: not legal while a graph is captured.  CPU tensors are refused."""
    if volume.dim() != 3 or volume.dtype != torch.float32:
        raise ValueError('surface_nets: volume must be a float32 [R0,R1,R2] tensor; got {} {}'.format(volume.dtype, tuple(volume.shape)))
    volume = volume.detach().contiguous()
    vol_p = L.p(volume)
    R = [int(s) for s in volume.shape]
    if min(R) < 2 or max(R) > MAX_RESOLUTION:
        raise ValueError('surface_nets: every axis needs 2 .. {} lattice points; got {}'.format(MAX_RESOLUTION, R))
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('surface_nets reads its counts on the host: it cannot be captured into a graph')
    lo32, step = lattice_step(lo, hi, R)
    dev = volume.device
    nbytes = int(L.lib().nsr_surface_nets_workspace_bytes(*R))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    L.check(L.lib().nsr_surface_nets_count(vol_p, R[0], R[1], R[2], float(iso), L.p(ws), L.p(counts), L.stream()), 'surface_nets_count')
    V, Q = (int(c) & 0xffffffff for c in counts.cpu().tolist())          # the host read
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(2 * Q, 3, dtype=torch.int32, device=dev)
    if V:
        fp = ctypes.POINTER(ctypes.c_float)
        L.check(L.lib().nsr_surface_nets_emit(vol_p, R[0], R[1], R[2], float(iso), lo32.ctypes.data_as(fp), step.ctypes.data_as(fp),
                                              L.p(ws), V, Q, L.p(verts), L.p(faces) if Q else None, L.stream()), 'surface_nets_emit')
    return verts, faces


# ---- mesh cleaning -----------------------------------------------------------------------------------------------------------
ComponentStats = namedtuple('ComponentStats', 'roots n_verts n_faces lo hi')


def _check_faces(faces, who):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError('{}: faces must be an int32 [F,3] tensor; got {} {}'.format(
            who, getattr(faces, 'dtype', type(faces)), tuple(getattr(faces, 'shape', ()))))
    return faces.detach().contiguous()


def _check_verts(verts, who):
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError('{}: verts must be a float32 [V,3] tensor; got {} {}'.format(
            who, getattr(verts, 'dtype', type(verts)), tuple(getattr(verts, 'shape', ()))))
    return verts.detach().contiguous()


def _check_keep_rule(min_faces, min_diagonal, keep_largest, who):
    if int(min_faces) != min_faces or not 0 <= min_faces < 2 ** 31:
        raise ValueError('{}: min_faces must be an integer in 0 .. 2^31 - 1; got {}'.format(who, min_faces))
    if not float(min_diagonal) >= 0.0:
        raise ValueError('{}: min_diagonal must be >= 0; got {}'.format(who, min_diagonal))
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 1):
        raise ValueError('{}: keep_largest must be None or an integer >= 1; got {}'.format(who, keep_largest))


def _no_capture(who):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('{} reads its counts on the host: it cannot be captured into a graph'.format(who))


def connected_components(faces, num_verts):
    """labels int32 [V] of the mesh (faces int32 [F,3] on the device, V = num_verts): labels[v] is the smallest vertex id of v's
    component; a vertex in no face is its own.  A face with an index outside [0, V) joins nothing and raises ValueError after the
    host read of the device's bad-face count.  Not legal while a graph is captured.  CPU tensors are refused."""
    faces = _check_faces(faces, 'connected_components')
    V, F = int(num_verts), int(faces.shape[0])
    if not 0 <= V < 2 ** 31 or F >= 2 ** 31:
        raise ValueError('connected_components: V and F must be below 2^31; got {} and {}'.format(V, F))
    faces_p = L.p(faces)
    _no_capture('connected_components')
    labels = torch.empty(V, dtype=torch.int32, device=faces.device)
    bad = torch.empty(1, dtype=torch.int32, device=faces.device)
    L.check(L.lib().nsr_mesh_components(faces_p, V, F, L.p(labels), L.p(bad), L.stream()), 'mesh_components')
    n_bad = int(bad.item())                                               # the host read
    if n_bad:
        raise ValueError('connected_components: {} of {} faces hold a vertex index outside [0, {})'.format(n_bad, F, V))
    return labels


def _stats_arrays(verts, faces, labels):
    """n_verts, n_faces [V] int32 and lo, hi [V,3] f32, indexed by vertex id and meaningful at the roots"""
    V, F = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    n_verts = torch.empty(V, dtype=torch.int32, device=dev)
    n_faces = torch.empty(V, dtype=torch.int32, device=dev)
    lo = torch.empty(V, 3, dtype=torch.float32, device=dev)
    hi = torch.empty(V, 3, dtype=torch.float32, device=dev)
    L.check(L.lib().nsr_mesh_component_stats(L.p(verts), L.p(faces), L.p(labels), V, F, L.p(n_verts), L.p(n_faces), L.p(lo), L.p(hi),
                                             L.stream()), 'mesh_component_stats')
    return n_verts, n_faces, lo, hi


def component_stats(verts, faces, labels):
    """ComponentStats(roots, n_verts, n_faces, lo, hi) of the mesh's components, one row a component in ascending order of the
    root (its label, the smallest vertex id): roots, n_verts, n_faces int32 [C]; lo, hi f32 [C,3], the exact box of the
    component's vertices.  `labels` as connected_components returns them.  All on the device; one host read (C)."""
    verts, faces = _check_verts(verts, 'component_stats'), _check_faces(faces, 'component_stats')
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.shape != (verts.shape[0],):
        raise ValueError('component_stats: labels must be an int32 [V] tensor; got {} {}'.format(
            getattr(labels, 'dtype', type(labels)), tuple(getattr(labels, 'shape', ()))))
    labels = labels.detach().contiguous()
    for t in (verts, faces, labels):
        L.p(t)
    _no_capture('component_stats')
    n_verts, n_faces, lo, hi = _stats_arrays(verts, faces, labels)
    V = int(verts.shape[0])
    roots = torch.nonzero(labels == torch.arange(V, dtype=torch.int32, device=labels.device)).reshape(-1)     # ascending
    return ComponentStats(roots.to(torch.int32), n_verts[roots], n_faces[roots], lo[roots], hi[roots])


def keep_components(stats, num_verts, min_faces=0, min_diagonal=0.0, keep_largest=None):
    """The keep rule on ComponentStats -> keep uint8 [V], set at the roots of the kept components.  A component is kept iff
    n_faces >= min_faces, dx^2 + dy^2 + dz^2 >= min_diagonal^2 (d = hi - lo; f32, in this written order) and, with keep_largest
    = k, it is among the k of the most faces of those that passed (ties to the smaller label).  Elementwise work over the
    roots: torch on the device."""
    _check_keep_rule(min_faces, min_diagonal, keep_largest, 'keep_components')
    d = stats.hi - stats.lo
    diag2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    threshold = float(np.float32(min_diagonal) * np.float32(min_diagonal))
    ok = (stats.n_faces >= int(min_faces)) & (diag2 >= threshold)
    roots = stats.roots.to(torch.int64)
    if keep_largest is not None:
        cand = torch.nonzero(ok).reshape(-1)
        key = (0x7fffffff - stats.n_faces[cand].to(torch.int64)) * (1 << 32) + roots[cand]       # most faces first, then the label
        first = cand[torch.argsort(key)[:int(keep_largest)]]
        ok = torch.zeros_like(ok)
        ok[first] = True
    keep = torch.zeros(int(num_verts), dtype=torch.uint8, device=roots.device)
    keep[roots] = ok.to(torch.uint8)
    return keep


def filter_components(verts, faces, min_faces=0, min_diagonal=0.0, keep_largest=None):
    """Drops the components the keep rule (keep_components) refuses -> (verts [Vk,3], faces [Fk,3], index_map int32 [V]).  The
    survivors keep their relative order; a surviving vertex's new id is its rank among them, index_map[v] is that id or -1, and
    the faces are re-indexed.  Bit for bit a function of the input.  Raises ValueError on a face index outside [0, V).  Host
    reads of the counts: not legal while a graph is captured.  CPU tensors are refused."""
    verts, faces = _check_verts(verts, 'filter_components'), _check_faces(faces, 'filter_components')
    _check_keep_rule(min_faces, min_diagonal, keep_largest, 'filter_components')
    L.p(verts)
    labels = connected_components(faces, verts.shape[0])
    stats = component_stats(verts, faces, labels)
    keep = keep_components(stats, verts.shape[0], min_faces, min_diagonal, keep_largest)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    nbytes = int(L.lib().nsr_mesh_filter_workspace_bytes(V, F))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    L.check(L.lib().nsr_mesh_filter_count(L.p(faces), L.p(labels), L.p(keep), V, F, L.p(ws), L.p(counts), L.stream()), 'mesh_filter_count')
    Vk, Fk = (int(c) for c in counts.cpu().tolist())                      # the host read
    index_map = torch.empty(V, dtype=torch.int32, device=dev)
    verts_out = torch.empty(Vk, 3, dtype=torch.float32, device=dev)
    faces_out = torch.empty(Fk, 3, dtype=torch.int32, device=dev)
    L.check(L.lib().nsr_mesh_filter_emit(L.p(verts), L.p(faces), L.p(labels), L.p(keep), V, F, L.p(ws), Vk, Fk, L.p(index_map),
                                         L.p(verts_out), L.p(faces_out), L.stream()), 'mesh_filter_emit')
    return verts_out, faces_out, index_map


def lattice_points(lo32, step, shape, start, end, device):
    """World positions [end - start, 3] of the lattice points with C-order linear indices start .. end - 1: coordinate a of
    point i is lo_a + (float)i * step_a, a product and a sum in f32, the formula the extractor places its vertices with."""
    R0, R1, R2 = shape
    idx = torch.arange(start, end, dtype=torch.int64, device=device)
    ijk = (idx // (R1 * R2), (idx // R2) % R1, idx % R2)
    cols = [float(lo32[a]) + ijk[a].to(torch.float32) * float(step[a]) for a in range(3)]
    return torch.stack(cols, dim=1)


@torch.no_grad()
def density_volume(model, lo, hi, resolution, density_scale=1.0, chunk=1 << 24):
    """sigma of `model` on the lattice lo .. hi with `resolution` points an axis (an int or a triple) -> [R0,R1,R2] f32 on the
    model's device: model.field(pts, sigma_only=True, density_scale=...) over chunks of `chunk` points, no grad."""
    res = np.asarray(resolution, np.int64).reshape(-1)
    shape = tuple(int(r) for r in (np.repeat(res, 3) if res.size == 1 else res))
    if len(shape) != 3 or min(shape) < 2 or max(shape) > MAX_RESOLUTION:
        raise ValueError('density_volume: resolution must be an int or a triple in 2 .. {}; got {}'.format(MAX_RESOLUTION, resolution))
    lo32, step = lattice_step(lo, hi, shape)
    dev = model.arena.device
    n = shape[0] * shape[1] * shape[2]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    chunk = max(int(chunk), 1)
    for start in range(0, n, chunk):
        end = min(start + chunk, n)
        out[start:end] = model.field(lattice_points(lo32, step, shape, start, end, dev), sigma_only=True, density_scale=density_scale)
    return out.view(shape)


_PLY_HEAD = 'ply\nformat binary_little_endian 1.0\ncomment nerfstyle_amd mesh export\n'


@dataclass
class Mesh:
    """verts f32 [V,3], faces int32 [F,3]; per vertex and optional: colors uint8 [V,3], normals f32 [V,3], labels int32 [V]
    (the region label: the argmax of the model's class channels)."""
    verts: torch.Tensor
    faces: torch.Tensor
    colors: Optional[torch.Tensor] = None
    normals: Optional[torch.Tensor] = None
    labels: Optional[torch.Tensor] = None

    def save_ply(self, path):
        """Binary little-endian PLY: vertex properties x y z [nx ny nz] [red green blue] [label], faces as
        `list uchar int vertex_indices`.  Plain host code."""
        def host(t, dtype, shape):
            a = np.ascontiguousarray((t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype, copy=False))
            if a.shape != shape:
                raise ValueError('Mesh.save_ply: expected shape {}, got {}'.format(shape, a.shape))
            return a
        V, F = int(self.verts.shape[0]), int(self.faces.shape[0])
        fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
        cols = list(host(self.verts, np.float32, (V, 3)).T)
        props = ['property float x', 'property float y', 'property float z']
        if self.normals is not None:
            fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
            cols += list(host(self.normals, np.float32, (V, 3)).T)
            props += ['property float nx', 'property float ny', 'property float nz']
        if self.colors is not None:
            fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
            cols += list(host(self.colors, np.uint8, (V, 3)).T)
            props += ['property uchar red', 'property uchar green', 'property uchar blue']
        if self.labels is not None:
            fields += [('label', '<i4')]
            cols += [host(self.labels, np.int32, (V,))]
            props += ['property int label']
        vrec = np.empty(V, dtype=np.dtype(fields))             # packed: no padding between the fields
        for (name, _), col in zip(fields, cols):
            vrec[name] = col
        frec = np.empty(F, dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
        frec['n'] = 3
        frec['v'] = host(self.faces, np.int32, (F, 3))
        head = (_PLY_HEAD + 'element vertex {}\n'.format(V) + ''.join(p + '\n' for p in props)
                + 'element face {}\nproperty list uchar int vertex_indices\nend_header\n'.format(F))
        with open(path, 'wb') as f:
            f.write(head.encode('ascii'))
            f.write(vrec.tobytes())
            f.write(frec.tobytes())

    def clean(self, min_faces=0, min_diagonal=0.0, keep_largest=None):
        """-> a new Mesh without the components filter_components drops; colors, normals and labels follow the vertices."""
        verts, faces, index_map = filter_components(self.verts, self.faces, min_faces, min_diagonal, keep_largest)
        kept = index_map >= 0                                             # a boolean mask keeps the order
        pick = lambda t: None if t is None else t[kept]
        return Mesh(verts, faces, pick(self.colors), pick(self.normals), pick(self.labels))


def colors_uint8(rgb):
    """sigmoid colours in [0,1] -> uint8, round to nearest"""
    return torch.round(rgb * 255.0).clamp_(0.0, 255.0).to(torch.uint8)


@torch.no_grad()
def extract_mesh(renderer, resolution=256, iso=10.0, aabb=None, colors=True, normals=True, labels=True, chunk=1 << 24,
                 min_faces=0, min_diagonal=0.0, keep_largest=None):
    """Renderer.extract_mesh (its docstring states the interface)."""
    _check_keep_rule(min_faces, min_diagonal, keep_largest, 'extract_mesh')
    model = renderer.model
    if aabb is None:
        mn, sz = model._bbox()
        lo, hi = np.asarray(mn, np.float32), np.asarray(mn, np.float32) + np.asarray(sz, np.float32)
    else:
        box = _triple(aabb[:3], 'aabb', np.float32), _triple(aabb[3:], 'aabb', np.float32)
        lo, hi = box
    vol = density_volume(model, lo, hi, resolution, density_scale=renderer.cfg.density_scale, chunk=chunk)
    verts, faces = surface_nets(vol, iso, lo, hi)
    del vol
    if min_faces != 0 or min_diagonal != 0.0 or keep_largest is not None:
        verts, faces, _ = filter_components(verts, faces, min_faces, min_diagonal, keep_largest)     # dropped vertices are never shaded
    mesh = Mesh(verts, faces)
    want_field = colors or (labels and model.class_dim > 0)
    nrm = None
    if normals or (want_field and model.use_dir):
        nrm = model.density_gradient(verts, normalize=True)[1]
    if normals:
        mesh.normals = nrm
    if want_field:
        # a view-dependent model is looked at head-on: from outside, along the inward normal
        _, out = model.field(verts, dirs=-nrm if model.use_dir else None)
        if colors:
            mesh.colors = colors_uint8(out[:, :3])
        if labels and model.class_dim > 0:
            mesh.labels = out[:, 3:].argmax(dim=1).to(torch.int32)
    return mesh
