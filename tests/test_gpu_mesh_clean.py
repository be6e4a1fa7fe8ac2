"""GPU: mesh cleaning (nsr_mesh_components / _component_stats / _filter_count / _filter_emit, nerfstyle_amd/mesh.py) against the
CPU restatement of the definition (tests/mesh_clean_ref.py).

For every mesh: labels, roots, n_verts, n_faces, index_map and the filtered faces equal the restatement exactly; the boxes and
the filtered vertices equal it bit for bit (they are mins, maxes and copies); a second call gives the same bits."""
import functools

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as R
from helpers import render_setup

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(labels, stats) of a synthetic case, computed once and shared"""
    verts, faces = C.cases()[name]
    labels = C.labels_propagation(faces, len(verts))
    return labels, C.component_stats(verts, faces, labels)


def _labels_and_stats(dev, verts, faces):
    from nerfstyle_amd import mesh
    tv, tf = torch.tensor(verts, device=dev), torch.tensor(faces, device=dev)
    labels = mesh.connected_components(tf, len(verts))
    assert labels.dtype == torch.int32 and labels.shape == (len(verts),) and labels.device.type == 'cuda'
    stats = mesh.component_stats(tv, tf, labels)
    for t, dt in zip(stats, (torch.int32, torch.int32, torch.int32, torch.float32, torch.float32)):
        assert t.dtype == dt and t.device.type == 'cuda' and t.shape[0] == stats.roots.shape[0]
    return labels.cpu().numpy(), [t.cpu().numpy() for t in stats]


def _filter(dev, verts, faces, rule):
    from nerfstyle_amd import mesh
    out = mesh.filter_components(torch.tensor(verts, device=dev), torch.tensor(faces, device=dev), **rule)
    assert out[0].dtype == torch.float32 and out[0].dim() == 2 and out[0].shape[1] == 3
    assert out[1].dtype == torch.int32 and out[1].dim() == 2 and out[1].shape[1] == 3
    assert out[2].dtype == torch.int32 and out[2].shape == (len(verts),)
    return [t.cpu().numpy() for t in out]


def check_mesh(dev, verts, faces, rules, labels_ref, stats_ref):
    """everything the issue lists, for one mesh"""
    labels, stats = _labels_and_stats(dev, verts, faces)
    assert np.array_equal(labels, labels_ref)
    roots, n_verts, n_faces, lo, hi = stats
    assert np.array_equal(roots, stats_ref['roots']) and np.array_equal(n_verts, stats_ref['n_verts'])
    assert np.array_equal(n_faces, stats_ref['n_faces'])
    assert np.array_equal(bits(lo), bits(stats_ref['lo'])) and np.array_equal(bits(hi), bits(stats_ref['hi']))
    labels2, stats2 = _labels_and_stats(dev, verts, faces)
    assert np.array_equal(labels2, labels) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(stats, stats2))
    for rule in rules:
        v_ref, f_ref, m_ref = C.filter_components(verts, faces, labels=labels_ref, **rule)
        v, f, m = _filter(dev, verts, faces, rule)
        assert v.shape == v_ref.shape and f.shape == f_ref.shape, (rule, v.shape, v_ref.shape, f.shape, f_ref.shape)
        assert np.array_equal(m, m_ref) and np.array_equal(f, f_ref) and np.array_equal(bits(v), bits(v_ref)), rule
        v2, f2, m2 = _filter(dev, verts, faces, rule)
        assert np.array_equal(bits(v2), bits(v)) and np.array_equal(f2, f) and np.array_equal(m2, m), rule


# ---- synthetic meshes ------------------------------------------------------------------------------------------------------
def test_cases_are_the_issues():
    cs = C.cases()
    assert len(cs['no_vertices'][0]) == 0 and cs['five_singletons'][1].shape == (0, 3) and len(cs['five_singletons'][0]) == 5
    for order in ('permuted', 'ascending', 'descending'):
        assert cs['strip_' + order][1].shape == (5000, 3)
    assert np.array_equal(cs['strip_ascending'][1][7], [7, 8, 9]) and np.array_equal(cs['strip_descending'][1][0], [5001, 5000, 4999])
    v, f = cs['fan']
    assert f.shape == (10000, 3) and (f[:, 0] == len(v) - 1).all()
    assert len(cs['disjoint_1000'][0]) == 3000 and len(cs['disjoint_1000'][1]) == 1000 + 333
    assert [r.get('keep_largest') for r in C.RULES].count(None) < len(C.RULES) and {1, 3, 10} <= {r.get('keep_largest') for r in C.RULES}


@pytest.mark.parametrize('name', sorted(C.cases()))
def test_against_the_restatement(dev, name):
    verts, faces = C.cases()[name]
    labels_ref, stats_ref = _reference(name)
    check_mesh(dev, verts, faces, C.RULES, labels_ref, stats_ref)


def test_empty_inputs(dev):
    cs = C.cases()
    v, f, m = _filter(dev, *cs['no_vertices'], dict())
    assert v.shape == (0, 3) and f.shape == (0, 3) and m.shape == (0,)
    labels, stats = _labels_and_stats(dev, *cs['five_singletons'])
    assert labels.tolist() == [0, 1, 2, 3, 4] and stats[0].tolist() == [0, 1, 2, 3, 4]
    assert stats[1].tolist() == [1] * 5 and stats[2].tolist() == [0] * 5
    assert np.array_equal(bits(stats[3]), bits(cs['five_singletons'][0])) and np.array_equal(bits(stats[4]), bits(cs['five_singletons'][0]))
    v, f, m = _filter(dev, *cs['five_singletons'], dict(min_faces=1))                 # drops everything
    assert v.shape == (0, 3) and f.shape == (0, 3) and m.tolist() == [-1] * 5
    v, f, m = _filter(dev, *cs['five_singletons'], dict())
    assert np.array_equal(bits(v), bits(cs['five_singletons'][0])) and f.shape == (0, 3) and m.tolist() == [0, 1, 2, 3, 4]


def test_minimal_meshes(dev):
    cs = C.cases()
    lab = lambda n: _labels_and_stats(dev, *cs[n])[0].tolist()
    assert lab('one_triangle') == [0, 0, 0] and lab('two_disjoint') == [0, 1, 0, 1, 0, 1] and lab('shared_edge') == [0, 0, 0, 0]
    assert lab('shared_vertex') == [0, 0, 0, 0, 0] and lab('degenerate_face') == [0, 1, 0, 1, 0]
    assert lab('duplicate_face') == [0, 0, 0, 3, 3, 3] and lab('unreferenced_between') == [0, 0, 0, 3, 4, 4, 4]
    v, f, m = _filter(dev, *cs['unreferenced_between'], dict(min_faces=1))            # the index map has a gap
    assert m.tolist() == [0, 1, 2, -1, 3, 4, 5] and f.tolist() == [[0, 1, 2], [3, 4, 5], [2, 0, 1]]
    v, f, m = _filter(dev, *cs['unreferenced_between'], dict(keep_largest=1))
    assert m.tolist() == [0, 1, 2, -1, -1, -1, -1] and f.tolist() == [[0, 1, 2], [2, 0, 1]]


def test_keep_largest_ties_go_to_the_smaller_label(dev):
    verts, faces = C.cases()['disjoint_1000']
    _, stats_ref = _reference('disjoint_1000')
    three = stats_ref['roots'][stats_ref['n_faces'] == 3]
    labels_ref = _reference('disjoint_1000')[0]
    for k in (1, 3, 10):
        v, f, m = _filter(dev, verts, faces, dict(keep_largest=k))
        assert len(f) == 3 * k and len(v) == 6 * k
        assert np.array_equal(np.unique(labels_ref[m >= 0]), three[:k])


# ---- surface-nets meshes ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def surfaces(dev):
    """name -> the case's mesh, extracted on the device"""
    from nerfstyle_amd.mesh import surface_nets
    out = {}
    for name in C.SURFACE_CASES:
        vol, iso, lo, hi = C.surface_volumes()[name]
        verts, faces = surface_nets(torch.tensor(vol, device=dev), iso, lo, hi)
        out[name] = (verts.cpu().numpy(), faces.cpu().numpy())
    return out


@pytest.mark.parametrize('name', C.SURFACE_CASES)
def test_surface_nets_meshes(dev, surfaces, name):
    verts, faces = surfaces[name]
    v_ref, f_ref = C.surface_mesh(name)
    assert np.array_equal(faces, f_ref) and np.array_equal(bits(verts), bits(v_ref))
    labels_ref = C.labels_propagation(faces, len(verts))
    stats_ref = C.component_stats(verts, faces, labels_ref)
    rules = C.surface_rules(name)
    for rule in rules:                                              # no squared diagonal near a threshold: the f32 compare cannot flip
        if 'min_diagonal' in rule:
            margin = C.diagonal_margin(stats_ref, rule['min_diagonal'])
            print('{:16s} min_diagonal {:.4f}: margin {:.3g}'.format(name, rule['min_diagonal'], margin))
            assert margin > 1e-3, (name, rule)
    check_mesh(dev, verts, faces, rules, labels_ref, stats_ref)


def test_two_spheres_are_two_components_and_the_larger_one_is_closed(dev, surfaces):
    verts, faces = surfaces['two_spheres_9']
    labels, stats = _labels_and_stats(dev, verts, faces)
    assert len(stats[0]) == 2 and len(set(labels.tolist())) == 2
    v, f, m = _filter(dev, verts, faces, dict(keep_largest=1))
    assert 0 < len(f) < len(faces) and R.is_closed(f) and R.euler_characteristic(v, f) == 2


def test_one_component_is_left_as_it_is(dev, surfaces):
    verts, faces = surfaces['sphere_33']
    labels, stats = _labels_and_stats(dev, verts, faces)
    assert len(stats[0]) == 1 and stats[1].tolist() == [len(verts)] and stats[2].tolist() == [len(faces)]
    v, f, m = _filter(dev, verts, faces, dict(min_faces=1))
    assert np.array_equal(bits(v), bits(verts)) and np.array_equal(f, faces) and np.array_equal(m, np.arange(len(verts)))


# ---- scan depths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('triangles,depth', [(100, 1), (30000, 2), (5592500, 3)])
def test_every_scan_depth_on_isolated_triangles(dev, triangles, depth):
    """n isolated triangles, every third one large: the filter keeps those.  A block of the filter owns 256 vertices and 256
    faces, so 3 n vertices are ceil(3 n / 256) block totals, scanned 256 a pass: 1, 2 and 3 levels.  The expectation is closed
    form (np.arange), not the restatement's loops."""
    from nerfstyle_amd import mesh
    n, V = triangles, 3 * triangles
    blocks = -(-V // 256)
    assert {1: blocks <= 256, 2: 256 < blocks <= 256 * 256, 3: blocks > 256 * 256}[depth]
    t = np.arange(V) // 3
    j = np.arange(V) % 3
    big = t % 3 == 0
    size = np.where(big, 2.0, 0.5).astype(np.float32)
    verts = np.stack([size * (j == 1), size * (j == 2), (t % 1024) * 0.25], 1).astype(np.float32)
    faces = np.arange(V, dtype=np.int32).reshape(n, 3)
    tv, tf = torch.tensor(verts, device=dev), torch.tensor(faces, device=dev)
    labels = mesh.connected_components(tf, V)
    assert np.array_equal(labels.cpu().numpy(), 3 * t)
    stats = mesh.component_stats(tv, tf, labels)
    assert np.array_equal(stats.roots.cpu().numpy(), np.arange(0, V, 3))
    assert bool((stats.n_verts == 3).all()) and bool((stats.n_faces == 1).all())
    assert np.array_equal(bits(stats.lo.cpu().numpy()), bits(verts[0::3]))
    hi = verts[0::3].copy()
    hi[:, 0] = hi[:, 1] = size[0::3]
    assert np.array_equal(bits(stats.hi.cpu().numpy()), bits(hi))
    del stats
    # diagonals^2: 8 and 0.5 against 1.5^2
    v, f, m = mesh.filter_components(tv, tf, min_diagonal=1.5)
    nk = -(-n // 3)
    assert v.shape == (3 * nk, 3) and f.shape == (nk, 3)
    assert np.array_equal(m.cpu().numpy(), np.where(big, 3 * (t // 3) + j, -1))
    assert np.array_equal(f.cpu().numpy(), np.arange(3 * nk, dtype=np.int32).reshape(nk, 3))
    assert np.array_equal(bits(v.cpu().numpy()), bits(verts[big]))


# ---- bad faces, refusals ---------------------------------------------------------------------------------------------------
def test_a_bad_face_joins_nothing_and_is_counted(dev):
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import mesh
    verts, good = C.cases()['disjoint_1000']
    V = len(verts)
    faces = np.concatenate([good[:400], [[good[0, 0], V, good[5, 1]]], good[400:900], [[good[7, 2], good[9, 0], -1]], good[900:]]).astype(np.int32)
    tf = torch.tensor(faces, device=dev)
    labels = torch.full((V,), -5, dtype=torch.int32, device=dev)
    bad = torch.full((1,), -5, dtype=torch.int32, device=dev)
    assert L.lib().nsr_mesh_components(L.p(tf), V, len(faces), L.p(labels), L.p(bad), L.stream()) == 0
    assert int(bad.item()) == 2
    assert np.array_equal(labels.cpu().numpy(), _reference('disjoint_1000')[0])       # the mesh without the two faces
    with pytest.raises(ValueError, match='2 of 1335 faces'):
        mesh.connected_components(tf, V)
    with pytest.raises(ValueError):
        mesh.filter_components(torch.tensor(verts, device=dev), tf, min_faces=1)
    # the statistics and the filter skip them too
    tv = torch.tensor(verts, device=dev)
    n_faces = mesh._stats_arrays(tv, tf, labels)[1].cpu().numpy()
    assert np.array_equal(n_faces[_reference('disjoint_1000')[1]['roots']], _reference('disjoint_1000')[1]['n_faces'])
    keep = torch.ones(V, dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(L.lib().nsr_mesh_filter_workspace_bytes(V, len(faces))) // 4, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    assert L.lib().nsr_mesh_filter_count(L.p(tf), L.p(labels), L.p(keep), V, len(faces), L.p(ws), L.p(counts), L.stream()) == 0
    assert counts.cpu().tolist() == [V, len(good)]
    imap = torch.zeros(V, dtype=torch.int32, device=dev)
    vo, fo = torch.zeros(V, 3, device=dev), torch.zeros(len(good), 3, dtype=torch.int32, device=dev)
    assert L.lib().nsr_mesh_filter_emit(L.p(tv), L.p(tf), L.p(labels), L.p(keep), V, len(faces), L.p(ws), V, len(good), L.p(imap),
                                        L.p(vo), L.p(fo), L.stream()) == 0
    assert np.array_equal(fo.cpu().numpy(), good) and np.array_equal(imap.cpu().numpy(), np.arange(V))


def test_emit_refuses_counts_that_are_not_the_workspaces(dev):
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import mesh
    verts, faces = C.cases()['disjoint_1000']
    V, F = len(verts), len(faces)
    tv, tf = torch.tensor(verts, device=dev), torch.tensor(faces, device=dev)
    labels = mesh.connected_components(tf, V)
    keep = mesh.keep_components(mesh.component_stats(tv, tf, labels), V, min_faces=2)
    v_ref, f_ref, m_ref = C.filter_components(verts, faces, min_faces=2)
    Vk, Fk = len(v_ref), len(f_ref)
    ws = torch.zeros(int(L.lib().nsr_mesh_filter_workspace_bytes(V, F)) // 4, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    L.check(L.lib().nsr_mesh_filter_count(L.p(tf), L.p(labels), L.p(keep), V, F, L.p(ws), L.p(counts), L.stream()))
    assert counts.cpu().tolist() == [Vk, Fk] and ws[:4].cpu().tolist() == [Vk, Fk, V, F]
    imap = torch.full((V,), -7, dtype=torch.int32, device=dev)
    vo = torch.full((Vk + 1, 3), -7.0, device=dev)
    fo = torch.full((Fk + 1, 3), -7, dtype=torch.int32, device=dev)

    def emit(V, F, Vk, Fk):
        return L.lib().nsr_mesh_filter_emit(L.p(tv), L.p(tf), L.p(labels), L.p(keep), V, F, L.p(ws), Vk, Fk, L.p(imap), L.p(vo), L.p(fo),
                                            L.stream())
    assert emit(V, F, Vk + 1, Fk) == -1 and emit(V, F, Vk, Fk + 1) == -1 and emit(V, F, Vk - 1, Fk) == -1 and emit(V, F, Vk, Fk - 1) == -1
    assert emit(V - 1, F, Vk, Fk) == -1 and emit(V, F - 1, Vk, Fk) == -1                # another mesh's workspace
    torch.cuda.synchronize()
    assert bool((imap == -7).all()) and bool((vo == -7.0).all()) and bool((fo == -7).all())        # nothing was written
    assert emit(V, F, Vk, Fk) == 0
    torch.cuda.synchronize()
    assert np.array_equal(imap.cpu().numpy(), m_ref) and np.array_equal(fo[:Fk].cpu().numpy(), f_ref)
    assert np.array_equal(bits(vo[:Vk].cpu().numpy()), bits(v_ref)) and bool((vo[Vk:] == -7.0).all()) and bool((fo[Fk:] == -7).all())


def test_python_layer_checks_its_input_on_the_device(dev):
    from nerfstyle_amd import mesh
    verts, faces = (torch.tensor(x, device=dev) for x in C.cases()['shared_edge'])
    with pytest.raises(ValueError, match='faces must be an int32'):
        mesh.connected_components(faces.to(torch.int64), 4)
    with pytest.raises(ValueError, match='verts must be a float32'):
        mesh.filter_components(verts.double(), faces)
    with pytest.raises(ValueError):
        mesh.filter_components(verts, faces, keep_largest=0)
    # a non-contiguous view is read through a contiguous copy
    wide = torch.zeros(2, 5, dtype=torch.int32, device=dev)
    wide[:, :3] = faces
    assert mesh.connected_components(wide[:, :3], 4).tolist() == [0, 0, 0, 0]


# ---- Mesh.clean and extract_mesh -------------------------------------------------------------------------------------------
def test_clean_carries_the_attributes_through_the_index_map(dev, surfaces, tmp_path):
    from nerfstyle_amd.mesh import Mesh
    from test_mesh_cpu import read_ply
    verts, faces = surfaces['blobs_33']
    V = len(verts)
    rng = np.random.default_rng(0)
    colors, normals, labels = rng.integers(0, 256, (V, 3)).astype(np.uint8), rng.standard_normal((V, 3)).astype(np.float32), rng.integers(0, 13, V).astype(np.int32)
    m = Mesh(*(torch.tensor(x, device=dev) for x in (verts, faces, colors, normals, labels)))
    c = m.clean(min_faces=64)
    v_ref, f_ref, m_ref = C.filter_components(verts, faces, min_faces=64)
    kept = m_ref >= 0
    assert 0 < kept.sum() < V
    assert np.array_equal(bits(c.verts.cpu().numpy()), bits(v_ref)) and np.array_equal(c.faces.cpu().numpy(), f_ref)
    assert np.array_equal(c.colors.cpu().numpy(), colors[kept]) and np.array_equal(bits(c.normals.cpu().numpy()), bits(normals[kept]))
    assert np.array_equal(c.labels.cpu().numpy(), labels[kept])
    bare = Mesh(m.verts, m.faces).clean(keep_largest=2)
    assert bare.colors is None and bare.normals is None and bare.labels is None and 0 < bare.verts.shape[0] < V
    path = str(tmp_path / 'clean.ply')
    c.save_ply(path)
    names, vrec, pf = read_ply(path)                                # (it checks the file's length against the header's counts)
    assert len(vrec) == len(v_ref) and np.array_equal(pf, f_ref) and np.array_equal(vrec['label'], labels[kept])


RES, ISO = 24, 1.0                                                  # tests/test_gpu_mesh.py's end-to-end resolution


@pytest.fixture(scope='module')
def scene(dev):
    r, _, _, _, _ = render_setup(dev, contrast=16.0)
    return r


def test_extract_mesh_cleans_before_it_shades(dev, scene, tmp_path, monkeypatch):
    from nerfstyle_amd import mesh
    from test_mesh_cpu import read_ply
    full = scene.extract_mesh(resolution=RES, iso=ISO)
    stats = mesh.component_stats(full.verts, full.faces, mesh.connected_components(full.faces, full.verts.shape[0]))
    sizes = sorted(stats.n_faces.cpu().tolist())
    print('extract_mesh at {}: V {} F {}, components of {} faces'.format(RES, full.verts.shape[0], full.faces.shape[0], sizes))
    for rule in (dict(min_faces=8), dict(keep_largest=1)):
        a, b = full.clean(**rule), scene.extract_mesh(resolution=RES, iso=ISO, **rule)
        assert torch.equal(a.verts, b.verts) and torch.equal(a.faces, b.faces), rule
        assert torch.equal(a.normals, b.normals) and torch.equal(a.colors, b.colors) and torch.equal(a.labels, b.labels), rule
        path = str(tmp_path / 'scene.ply')
        b.save_ply(path)
        names, vrec, pf = read_ply(path)
        assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'label']
        assert len(vrec) == b.verts.shape[0] and np.array_equal(pf, b.faces.cpu().numpy())
    # the vertices handed to the shading launches are the kept ones
    seen = []
    grad = scene.model.density_gradient
    monkeypatch.setattr(scene.model, 'density_gradient', lambda x, **k: (seen.append(int(x.shape[0])), grad(x, **k))[1])
    b = scene.extract_mesh(resolution=RES, iso=ISO, keep_largest=1)
    assert seen == [b.verts.shape[0]]
    # with the defaults none of the new code runs and the bits are the extractor's
    monkeypatch.setattr(mesh, 'filter_components', lambda *a, **k: pytest.fail('filter_components called with the defaults'))
    again = scene.extract_mesh(resolution=RES, iso=ISO)
    mn, sz = scene.model._bbox()
    lo, hi = np.asarray(mn, np.float32), np.asarray(mn, np.float32) + np.asarray(sz, np.float32)
    verts, faces = mesh.surface_nets(mesh.density_volume(scene.model, lo, hi, RES, density_scale=scene.cfg.density_scale), ISO, lo, hi)
    assert torch.equal(again.verts, verts) and torch.equal(again.faces, faces)
    assert torch.equal(again.normals, full.normals) and torch.equal(again.colors, full.colors) and torch.equal(again.labels, full.labels)
