"""GPU: the surface-nets extractor (nsr_surface_nets_count / _emit, nerfstyle_amd/mesh.py) against the CPU restatement of the
definition (tests/mesh_ref.py), and Renderer.extract_mesh end to end.

For every volume: V and the faces equal the restatement exactly; the vertices are within 32 eps_f32 max(|lo|, |hi|, 1) of its
fp64 form per coordinate (about 20 f32 roundings of values no larger than the box: the lattice coordinates, the interpolation
with a t whose ends straddle iso, up to 12 adds and a divide); a second call gives the same bits.  The f32 form has the kernel's
operation order, so its bits are the expectation too (test_vertices_are_the_f32_restatements_bits)."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_ref as R
from helpers import render_setup

pytestmark = pytest.mark.gpu

CASES = ['one_corner_2', 'centre_3', 'all_outside', 'all_inside', 'all_iso', 'sphere_nan', 'sphere_567', 'two_spheres_9', 'plane_9',
         'sphere_17_9_9', 'random_33', 'random_65_65_33', 'last_block_33', 'first_block_33', 'sphere_33']


def _run(dev, name):
    from nerfstyle_amd.mesh import surface_nets
    vol, iso, lo, hi = R.cases()[name]
    verts, faces = surface_nets(torch.tensor(vol, device=dev), iso, lo, hi)
    assert verts.dtype == torch.float32 and verts.dim() == 2 and verts.shape[1] == 3 and verts.device.type == 'cuda'
    assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3
    return verts.cpu().numpy(), faces.cpu().numpy()


def test_cases_are_the_issues():
    shapes = {n: R.cases()[n][0].shape for n in CASES}
    assert shapes['one_corner_2'] == (2, 2, 2) and shapes['centre_3'] == (3, 3, 3) and shapes['sphere_567'] == (5, 6, 7)
    assert shapes['two_spheres_9'] == shapes['plane_9'] == (9, 9, 9) and shapes['sphere_17_9_9'] == (17, 9, 9)
    assert shapes['random_33'] == (33, 33, 33) and shapes['random_65_65_33'] == (65, 65, 33)
    cells = {n: (s[0] - 1) * (s[1] - 1) * (s[2] - 1) for n, s in shapes.items()}
    assert cells['sphere_17_9_9'] == 1024 and cells['random_65_65_33'] // 256 > 256   # a few blocks; more block totals than one scan pass holds
    assert set(CASES) == set(R.cases())


@pytest.mark.parametrize('name', CASES)
def test_against_the_restatement(dev, name):
    vol, iso, lo, hi = R.cases()[name]
    (v32, f_ref), (v64, _) = R.reference(name)
    verts, faces = _run(dev, name)
    assert verts.shape == v32.shape, (verts.shape, v32.shape)                        # V
    assert faces.shape == f_ref.shape and np.array_equal(faces, f_ref)
    tol = R.vertex_tolerance(lo, hi)
    err = float(np.abs(verts.astype(np.float64) - v64).max()) if len(verts) else 0.0
    bits = bool(np.array_equal(verts.view(np.uint32), v32.view(np.uint32)))
    print('{:18s} V {:6d} F {:6d}  max |v - fp64| {:.2e} (bound {:.2e})  f32 bits equal: {}'.format(name, len(verts), len(faces), err, tol, bits))
    assert np.isfinite(verts).all() and err <= tol
    again_v, again_f = _run(dev, name)
    assert np.array_equal(again_v.view(np.uint32), verts.view(np.uint32)) and np.array_equal(again_f, faces)


@pytest.mark.parametrize('name', ['sphere_nan', 'sphere_567', 'plane_9', 'random_33', 'random_65_65_33'])
def test_vertices_are_the_f32_restatements_bits(dev, name):
    (v32, _), _ = R.reference(name)
    verts, _ = _run(dev, name)
    assert np.array_equal(verts.view(np.uint32), v32.view(np.uint32))


def test_minimal_volumes(dev):
    v, f = _run(dev, 'one_corner_2')
    assert v.shape == (1, 3) and f.shape == (0, 3)
    v, f = _run(dev, 'centre_3')
    assert v.shape == (8, 3) and f.shape == (12, 3) and R.is_closed(f)
    for name in ('all_outside', 'all_inside', 'all_iso'):
        v, f = _run(dev, name)
        assert v.shape == (0, 3) and f.shape == (0, 3), name


def test_open_mesh_boundary_edges_once_inner_edges_twice(dev):
    _, f = _run(dev, 'plane_9')
    cu, dmax = R.edge_use(f)
    assert dmax == 1 and set(np.unique(cu)) == {1, 2}


def test_orientation_points_out_of_the_dense_side(dev):
    vol, iso, lo, hi = R.cases()['sphere_33']
    v, f = _run(dev, 'sphere_33')
    assert R.is_closed(f) and R.euler_characteristic(v, f) == 2
    assert R.signed_volume(v, f) > 0
    # the sphere's centre (0.1, -0.05, 0) of the [-1, 1] index frame, in world coordinates
    centre = np.asarray(lo) + (np.asarray([0.1, -0.05, 0.0]) + 1.0) / 2.0 * (np.asarray(hi) - np.asarray(lo))
    a, b, c = (v[f[:, i]].astype(np.float64) for i in range(3))
    normal = np.cross(b - a, c - a)
    assert (np.einsum('ij,ij->i', normal, (a + b + c) / 3.0 - centre) > 0).all()


def test_three_scan_levels_and_the_largest_axis(dev):
    """1023 x 129 x 129 cells are 66 499 blocks: more than 256^2 block totals, so the scan runs three levels deep, on an axis of
    the largest length allowed.  Isolated points, among them the lattice's first and last, against the restatement."""
    from nerfstyle_amd.mesh import surface_nets
    shape = (1024, 130, 130)
    assert -(-(1023 * 129 * 129) // 256) > 256 * 256
    vol = np.zeros(shape, np.float32)
    rng = np.random.default_rng(5)
    for i, j, k in zip(rng.integers(1, 1023, 40), rng.integers(1, 129, 40), rng.integers(1, 129, 40)):
        vol[i, j, k] = 1.0 + rng.random()
    vol[0, 0, 0] = vol[1023, 129, 129] = vol[1023, 64, 64] = vol[512, 129, 7] = 2.0
    lo, hi = (-1.0, -2.0, 0.5), (3.0, 2.0, 1.5)
    v32, f_ref = R.surface_nets_ref(vol, 0.5, lo, hi)
    v64, _ = R.surface_nets_ref(vol, 0.5, lo, hi, np.float64)
    assert len(v32) > 300 and len(f_ref) > 400
    verts, faces = surface_nets(torch.tensor(vol, device=dev), 0.5, lo, hi)
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    assert verts.shape == v32.shape and np.array_equal(faces, f_ref)
    assert float(np.abs(verts.astype(np.float64) - v64).max()) <= R.vertex_tolerance(lo, hi)


def test_emit_refuses_counts_that_are_not_the_workspaces(dev):
    from nerfstyle_amd import _lib as L
    vol, iso, lo, hi = R.cases()['sphere_567']
    (v32, f_ref), _ = R.reference('sphere_567')
    V, Q = len(v32), len(f_ref) // 2
    shape = vol.shape
    t = torch.tensor(vol, device=dev)
    ws = torch.zeros(int(L.lib().nsr_surface_nets_workspace_bytes(*shape)) // 4, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    L.check(L.lib().nsr_surface_nets_count(L.p(t), *shape, iso, L.p(ws), L.p(counts), L.stream()))
    assert counts.cpu().tolist() == [V, Q]
    verts = torch.full((V + 1, 3), -7.0, device=dev)
    faces = torch.full((2 * Q + 2, 3), -7, dtype=torch.int32, device=dev)
    f3 = ctypes.c_float * 3
    lo3, step3 = f3(*lo), f3(0.1, 0.1, 0.1)

    def emit(shape, V, Q):
        return L.lib().nsr_surface_nets_emit(L.p(t), *shape, iso, lo3, step3, L.p(ws), V, Q, L.p(verts), L.p(faces), L.stream())
    assert emit(shape, V + 1, Q) == -1 and emit(shape, V, Q + 1) == -1 and emit(shape, V - 1, Q) == -1
    assert emit((shape[0], shape[2], shape[1]), V, Q) == -1                           # another shape's workspace
    torch.cuda.synchronize()
    assert bool((verts == -7.0).all()) and bool((faces == -7).all())                  # nothing was written
    assert emit(shape, V, Q) == 0
    torch.cuda.synchronize()
    assert bool((verts[:V] != -7.0).all()) and bool((verts[V:] == -7.0).all()) and bool((faces[2 * Q:] == -7).all())
    assert np.array_equal(faces[:2 * Q].cpu().numpy(), f_ref)


def test_surface_nets_is_refused_under_capture_and_on_bad_input(dev):
    from nerfstyle_amd.mesh import surface_nets
    with pytest.raises(ValueError):
        surface_nets(torch.zeros(1, 4, 4, device=dev), 0.5, -1.0, 1.0)
    # a non-contiguous view is read through a contiguous copy
    vol, iso, lo, hi = R.cases()['sphere_567']
    (_, f_ref), _ = R.reference('sphere_567')
    wide = torch.zeros(5, 6, 9, device=dev)
    wide[:, :, :7] = torch.tensor(vol, device=dev)
    assert np.array_equal(surface_nets(wide[:, :, :7], iso, lo, hi)[1].cpu().numpy(), f_ref)


# ---- end to end ----------------------------------------------------------------------------------------------------------
RES, ISO = 24, 1.0


@pytest.fixture(scope='module')
def scene(dev):
    r, _, _, _, _ = render_setup(dev, contrast=16.0)
    return r


def test_density_volume_is_the_field_on_the_lattice(dev, scene):
    from nerfstyle_amd import mesh
    model = scene.model
    lo, hi = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
    vol = mesh.density_volume(model, lo, hi, (5, 6, 7), density_scale=1.5, chunk=64)          # several chunks, a ragged last one
    assert vol.shape == (5, 6, 7) and vol.dtype == torch.float32
    lo32, step = R._box(lo, hi, (5, 6, 7))
    i, j, k = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing='ij')
    pts = np.stack([lo32[a] + g.astype(np.float32) * step[a] for a, g in enumerate((i, j, k))], -1).reshape(-1, 3)
    with torch.no_grad():
        want = model.field(torch.tensor(pts, device=dev), sigma_only=True, density_scale=1.5)
    assert torch.equal(vol.reshape(-1), want)
    assert torch.equal(mesh.density_volume(model, lo, hi, 6), mesh.density_volume(model, lo, hi, (6, 6, 6), chunk=7))


def test_extract_mesh_end_to_end(dev, scene):
    from nerfstyle_amd import mesh
    model = scene.model
    mn, sz = model._bbox()
    lo, hi = np.asarray(mn, np.float32), np.asarray(mn, np.float32) + np.asarray(sz, np.float32)
    vol = mesh.density_volume(model, lo, hi, RES, density_scale=scene.cfg.density_scale)
    assert float(vol.min()) < ISO < float(vol.max())
    verts, faces = mesh.surface_nets(vol, ISO, lo, hi)
    assert verts.shape[0] > 100 and faces.shape[0] > 100
    m = scene.extract_mesh(resolution=RES, iso=ISO)
    assert torch.equal(m.verts, verts) and torch.equal(m.faces, faces)
    with torch.no_grad():
        _, out = model.field(verts)
    assert m.colors.dtype == torch.uint8 and torch.equal(m.colors, torch.round(out[:, :3] * 255.0).to(torch.uint8))
    assert float(m.colors.float().std()) > 1.0                                        # not one grey
    assert m.labels.dtype == torch.int32 and torch.equal(m.labels, out[:, 3:].argmax(dim=1).to(torch.int32))
    _, nrm = model.density_gradient(verts, normalize=True)
    assert torch.equal(m.normals, nrm)
    assert float((m.normals.norm(dim=1) - 1.0).abs().max()) < 1e-3
    # the same box, spelled out
    m2 = scene.extract_mesh(resolution=(RES, RES, RES), iso=ISO, aabb=[-2.0, -2.0, -2.0, 2.0, 2.0, 2.0], colors=False, labels=False)
    assert torch.equal(m2.verts, verts) and torch.equal(m2.normals, nrm) and m2.colors is None and m2.labels is None


def test_extract_mesh_switches_off_launch_nothing(dev, scene, monkeypatch):
    model = scene.model
    calls = []
    field, grad = model.field, model.density_gradient
    monkeypatch.setattr(model, 'field', lambda *a, **k: (calls.append(('field', bool(k.get('sigma_only', False)))), field(*a, **k))[1])
    monkeypatch.setattr(model, 'density_gradient', lambda *a, **k: (calls.append(('grad', None)), grad(*a, **k))[1])
    m = scene.extract_mesh(resolution=RES, iso=ISO, colors=False, normals=False, labels=False)
    assert m.verts.shape[0] > 100 and m.colors is None and m.normals is None and m.labels is None
    assert calls and all(c == ('field', True) for c in calls)                         # the sigma-only lattice sweep alone
    calls.clear()
    m = scene.extract_mesh(resolution=RES, iso=ISO, colors=False, normals=False, labels=True)
    assert m.labels is not None and m.colors is None and ('grad', None) not in calls and calls.count(('field', False)) == 1


def test_ply_of_an_extracted_mesh(dev, scene, tmp_path):
    from test_mesh_cpu import read_ply
    m = scene.extract_mesh(resolution=RES, iso=ISO)
    path = str(tmp_path / 'scene.ply')
    m.save_ply(path)
    names, vrec, faces = read_ply(path)
    assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'label']
    assert np.array_equal(faces, m.faces.cpu().numpy()) and np.array_equal(vrec['label'], m.labels.cpu().numpy())
    assert np.array_equal(np.stack([vrec['x'], vrec['y'], vrec['z']], 1), m.verts.cpu().numpy())
