"""No GPU: the surface-nets restatement the GPU tests judge the kernels by (tests/mesh_ref.py) checked on its own -- closed,
outward-oriented surfaces of the right topology, its vectorised and its loop form bit for bit -- the PLY writer read back by a
parser written here, and the argument checks of the new entry points, which answer before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_reference_sphere_is_closed_outward_and_a_sphere():
    verts, faces = R.surface_nets_ref(R.sphere((17, 17, 17)), 0.0, -1.0, 1.0)
    assert len(verts) > 100 and R.is_closed(faces)
    vol = R.signed_volume(verts, faces)
    assert vol > 0 and abs(vol - 4.0 / 3.0 * np.pi * 0.6 ** 3) < 0.1           # outward, and about the ball's volume
    assert R.euler_characteristic(verts, faces) == 2


def test_reference_torus_has_genus_one():
    verts, faces = R.surface_nets_ref(R.torus((24, 24, 24)), 0.0, -1.0, 1.0)
    assert R.is_closed(faces) and R.signed_volume(verts, faces) > 0
    assert R.euler_characteristic(verts, faces) == 0


def test_reference_minimal_cases():
    (v, f), _ = R.reference('one_corner_2')
    assert v.shape == (1, 3) and f.shape == (0, 3)
    (v, f), _ = R.reference('centre_3')
    assert v.shape == (8, 3) and f.shape == (12, 3) and R.is_closed(f) and R.signed_volume(v, f) > 0
    for name in ('all_outside', 'all_inside', 'all_iso'):
        (v, f), _ = R.reference(name)
        assert v.shape == (0, 3) and f.shape == (0, 3), name


def test_reference_open_mesh_reaches_the_boundary():
    (v, f), _ = R.reference('plane_9')
    cu, dmax = R.edge_use(f)
    assert dmax == 1 and set(np.unique(cu)) == {1, 2}            # boundary edges once, inner edges twice, none more often
    # the sheet crosses all six boundary faces of the lattice: vertices in the first and the last cell layer of every axis
    vol, iso, lo, hi = R.cases()['plane_9']
    step = (np.asarray(hi) - np.asarray(lo)) / (np.asarray(vol.shape) - 1)
    for a in range(3):
        assert (v[:, a] < lo[a] + step[a]).any() and (v[:, a] > hi[a] - step[a]).any(), a


def test_reference_nan_is_outside_and_vertices_stay_finite():
    vol, iso, lo, hi = R.cases()['sphere_nan']
    (v, f), (v64, _) = R.reference('sphere_nan')
    assert np.isnan(vol).sum() >= 60 and np.isfinite(v).all() and np.isfinite(v64).all()
    filled = np.where(np.isnan(vol), np.float32(-1e30), vol)      # any value that is outside gives the same faces
    assert np.array_equal(R.surface_nets_ref(filled, iso, lo, hi)[1], f)


@pytest.mark.parametrize('name', ['one_corner_2', 'centre_3', 'sphere_nan', 'sphere_567', 'two_spheres_9', 'plane_9', 'sphere_17_9_9'])
def test_vectorised_and_loop_restatement_agree_bit_for_bit(name):
    vol, iso, lo, hi = R.cases()[name]
    (v, f), (v64, f64) = R.reference(name)
    vl, fl = R.surface_nets_loop(vol, iso, lo, hi)
    assert np.array_equal(fl, f) and np.array_equal(f64, f)
    assert np.array_equal(vl.view(np.uint32), v.view(np.uint32))
    assert len(v) == 0 or float(np.abs(v.astype(np.float64) - v64).max()) <= R.vertex_tolerance(lo, hi)


def test_vertices_lie_in_their_cells():
    vol, iso, lo, hi = R.cases()['random_33']
    (v, f), _ = R.reference('random_33')
    assert len(v) > 1000 and f.min() >= 0 and f.max() < len(v)       # (a vertex on the boundary may lie in no face)
    assert (v >= np.asarray(lo, np.float32) - 1e-5).all() and (v <= np.asarray(hi, np.float32) + 1e-5).all()
    assert float(np.abs(v[f[:, 0]] - v[f[:, 1]]).max()) < 2.01 * max((np.asarray(hi) - np.asarray(lo)) / 32)   # neighbours' cells


# ---- PLY -------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {'float': '<f4', 'uchar': 'u1', 'int': '<i4'}


def read_ply(path):
    """-> (vertex property names, vertex records, faces [F,3]) of a binary little-endian PLY with one face list"""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    counts, fields, element, face_list = {}, [], None, None
    for ln in lines[2:]:
        w = ln.split()
        if not w or w[0] in ('comment', 'end_header'):
            continue
        if w[0] == 'element':
            element = w[1]
            counts[element] = int(w[2])
        elif w[0] == 'property' and element == 'vertex':
            fields.append((w[2], _PLY_TYPES[w[1]]))
        elif w[0] == 'property' and element == 'face':
            face_list = ln
    assert face_list == 'property list uchar int vertex_indices'
    vdt = np.dtype(fields)
    V, F = counts['vertex'], counts['face']
    vrec = np.frombuffer(raw, vdt, V, end)
    frec = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), F, end + V * vdt.itemsize)
    assert end + V * vdt.itemsize + F * 13 == len(raw)
    assert (frec['n'] == 3).all()
    return [n for n, _ in fields], vrec, frec['v']


def _mesh(full):
    from nerfstyle_amd.mesh import Mesh
    (v, f), _ = R.reference('sphere_567')
    rng = np.random.default_rng(0)
    V = len(v)
    m = Mesh(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()))
    if full:
        m.colors = torch.from_numpy(rng.integers(0, 256, (V, 3)).astype(np.uint8))
        m.normals = torch.from_numpy(rng.standard_normal((V, 3)).astype(np.float32))
        m.labels = torch.from_numpy(rng.integers(0, 13, V).astype(np.int32))
    return m


def test_ply_round_trip_with_every_block(tmp_path):
    m = _mesh(True)
    path = str(tmp_path / 'full.ply')
    m.save_ply(path)
    names, vrec, faces = read_ply(path)
    assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'label']
    assert len(vrec) == m.verts.shape[0] and len(faces) == m.faces.shape[0]
    assert np.array_equal(np.stack([vrec['x'], vrec['y'], vrec['z']], 1).view(np.uint32), m.verts.numpy().view(np.uint32))
    assert np.array_equal(np.stack([vrec['nx'], vrec['ny'], vrec['nz']], 1).view(np.uint32), m.normals.numpy().view(np.uint32))
    assert np.array_equal(np.stack([vrec['red'], vrec['green'], vrec['blue']], 1), m.colors.numpy())
    assert np.array_equal(vrec['label'], m.labels.numpy())
    assert np.array_equal(faces, m.faces.numpy())


def test_ply_optional_blocks_are_absent_when_none(tmp_path):
    m = _mesh(False)
    path = str(tmp_path / 'bare.ply')
    m.save_ply(path)
    names, vrec, faces = read_ply(path)
    assert names == ['x', 'y', 'z'] and vrec.dtype.itemsize == 12
    assert np.array_equal(faces, m.faces.numpy())
    m.labels = torch.arange(m.verts.shape[0], dtype=torch.int32)
    m.save_ply(path)
    names, vrec, _ = read_ply(path)
    assert names == ['x', 'y', 'z', 'label'] and np.array_equal(vrec['label'], m.labels.numpy())


def test_ply_of_an_empty_mesh(tmp_path):
    from nerfstyle_amd.mesh import Mesh
    path = str(tmp_path / 'empty.ply')
    Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)).save_ply(path)
    names, vrec, faces = read_ply(path)
    assert names == ['x', 'y', 'z'] and len(vrec) == 0 and faces.shape == (0, 3)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(built):
    from nerfstyle_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'nsr.h')).read()
    for name in ('nsr_surface_nets_workspace_bytes', 'nsr_surface_nets_count', 'nsr_surface_nets_emit'):
        assert re.search(r'\b' + name + r'\s*\(', hdr) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.lib().nsr_abi_version() == _lib.ABI_VERSION


def test_workspace_size(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    assert L.nsr_surface_nets_workspace_bytes(1, 8, 8) == 0 and L.nsr_surface_nets_workspace_bytes(8, 8, 1025) == 0
    cells = 1023 ** 3
    for shape, ncell in (((2, 2, 2), 1), ((33, 33, 33), 32 ** 3), ((1024, 1024, 1024), cells)):
        b = L.nsr_surface_nets_workspace_bytes(*shape)
        blocks = -(-ncell // 256)
        assert b % 16 == 0 and 4 * ncell + 8 * blocks <= b <= 4 * ncell + 8 * blocks * 1.01 + 256, (shape, b)


def test_invalid_arguments_answer_before_a_device_is_touched(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    INVALID = -1
    fake = 0x10000                                                  # aligned, never dereferenced: the checks come first
    f3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025), (0, 0, 0)):
        assert L.nsr_surface_nets_count(fake, *shape, 0.0, fake, fake, None) == INVALID, shape
        assert L.nsr_surface_nets_emit(fake, *shape, 0.0, f3, f3, fake, 1, 0, fake, fake, None) == INVALID, shape
    # null pointers
    assert L.nsr_surface_nets_count(None, 8, 8, 8, 0.0, fake, fake, None) == INVALID
    assert L.nsr_surface_nets_count(fake, 8, 8, 8, 0.0, None, fake, None) == INVALID
    assert L.nsr_surface_nets_count(fake, 8, 8, 8, 0.0, fake, None, None) == INVALID
    assert L.nsr_surface_nets_emit(None, 8, 8, 8, 0.0, f3, f3, fake, 1, 0, fake, fake, None) == INVALID
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, None, f3, fake, 1, 0, fake, fake, None) == INVALID
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, f3, None, fake, 1, 0, fake, fake, None) == INVALID
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, f3, f3, None, 1, 0, fake, fake, None) == INVALID
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, f3, f3, fake, 1, 0, None, fake, None) == INVALID       # V > 0 without verts
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, f3, f3, fake, 4, 1, fake, None, None) == INVALID       # Q > 0 without faces
    # misaligned pointers, impossible counts
    assert L.nsr_surface_nets_count(fake + 2, 8, 8, 8, 0.0, fake, fake, None) == INVALID
    assert L.nsr_surface_nets_count(fake, 8, 8, 8, 0.0, fake + 8, fake, None) == INVALID
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, f3, f3, fake, 1, 0, fake + 1, fake, None) == INVALID
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, f3, f3, fake, 7 ** 3 + 1, 0, fake, fake, None) == INVALID
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, f3, f3, fake, 4, 3 * 7 ** 3 + 1, fake, fake, None) == INVALID
    assert L.nsr_surface_nets_emit(fake, 8, 8, 8, 0.0, f3, f3, fake, 0, 2, fake, fake, None) == INVALID


def test_python_layer_refuses_cpu_tensors_and_bad_shapes(built):
    from nerfstyle_amd import mesh
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mesh.surface_nets(torch.zeros(4, 4, 4), 0.5, -1.0, 1.0)
    with pytest.raises(ValueError):
        mesh.surface_nets(torch.zeros(4, 4), 0.5, -1.0, 1.0)
    with pytest.raises(ValueError):
        mesh.surface_nets(torch.zeros(4, 4, 4, dtype=torch.float64), 0.5, -1.0, 1.0)
    lo, step = mesh.lattice_step((-1.0, -0.5, 0.25), (1.5, 2.0, 3.0), (5, 6, 7))
    ref_lo, ref_step = R._box((-1.0, -0.5, 0.25), (1.5, 2.0, 3.0), (5, 6, 7))
    assert lo.dtype == np.float32 and np.array_equal(lo, ref_lo) and np.array_equal(step.view(np.uint32), ref_step.view(np.uint32))
    pts = mesh.lattice_points(lo, step, (5, 6, 7), 0, 5 * 6 * 7, 'cpu').numpy().reshape(5, 6, 7, 3)
    assert np.array_equal(pts[3, 4, 5], np.asarray([lo[a] + np.float32(i) * step[a] for a, i in enumerate((3, 4, 5))], np.float32))
