"""No GPU: the mesh-cleaning restatement the GPU tests judge the kernels by (tests/mesh_clean_ref.py) checked on its own -- its
two forms of the components against each other, the filter's algebra --, the union-find core of the kernels run from 16 host
threads (tests/uf_stress.cpp), and the argument checks of the new entry points, which answer before anything touches a
device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('nsr_mesh_components', 'nsr_mesh_component_stats', 'nsr_mesh_filter_workspace_bytes', 'nsr_mesh_filter_count',
         'nsr_mesh_filter_emit')


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def _all_cases():
    out = dict(C.cases())
    for name in C.SURFACE_CASES:
        out[name] = C.surface_mesh(name)
    v, f = C.cases()['strip_permuted']
    out['bad_faces'] = (v, np.concatenate([f[:100], [[3, len(v), 5]], f[100:200], [[7, -1, 9]], f[200:]]).astype(np.int32))
    return out


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(_all_cases()))
def test_the_two_restatements_of_the_components_agree(name):
    verts, faces = _all_cases()[name]
    V = len(verts)
    a, b = C.labels_union_find(faces, V), C.labels_propagation(faces, V)
    assert a.dtype == b.dtype == np.int32 and a.shape == (V,) and np.array_equal(a, b)
    assert (a <= np.arange(V)).all() and np.array_equal(a[a], a)               # a label is a root, and no larger than the vertex
    good, _ = C.good_faces(faces, V)
    assert (a[good] == a[good[:, :1]]).all()                                   # a face lies in one component


def test_known_components():
    cs = C.cases()
    lab = lambda n: C.labels_propagation(cs[n][1], len(cs[n][0])).tolist()
    assert lab('five_singletons') == [0, 1, 2, 3, 4] and lab('one_triangle') == [0, 0, 0]
    assert lab('two_disjoint') == [0, 1, 0, 1, 0, 1] and lab('shared_edge') == [0, 0, 0, 0]
    assert lab('shared_vertex') == [0, 0, 0, 0, 0]                              # one shared vertex joins
    assert lab('degenerate_face') == [0, 1, 0, 1, 0] and lab('unreferenced_between') == [0, 0, 0, 3, 4, 4, 4]
    for n in ('strip_permuted', 'strip_ascending', 'strip_descending', 'fan'):
        assert set(lab(n)) == {0}, n
    s = C.component_stats(*cs['disjoint_1000'], C.labels_propagation(cs['disjoint_1000'][1], 3000))
    assert len(s['roots']) == 667 and sorted(set(s['n_faces'].tolist())) == [1, 3] and s['n_verts'].sum() == 3000
    (v, f) = C.surface_mesh('two_spheres_9')
    assert len(set(C.labels_propagation(f, len(v)).tolist())) == 2
    (v, f) = C.surface_mesh('sphere_33')
    assert len(set(C.labels_propagation(f, len(v)).tolist())) == 1
    for n, comps, sizes in (('random_33', 7, 2), ('random_65_65_33', 10, 4), ('blobs_33', 14, 10)):
        (v, f) = C.surface_mesh(n)
        s = C.component_stats(v, f, C.labels_propagation(f, len(v)))
        assert len(s['roots']) == comps and len(set(s['n_faces'].tolist())) == sizes, n
        kept = [int(C.keep_rule(s, min_faces=m).sum()) for m in (2, 8, 64)]
        assert kept[0] >= kept[1] >= kept[2] >= 1 and (n == 'random_33' or kept[2] < kept[0] < comps), (n, kept)


def test_statistics_by_hand():
    verts = np.asarray([[0, 0, 0], [1, -2, 0.5], [-0.0, 3, 1], [9, 9, 9], [4, 4, 4], [5, 3, 4], [4, 6, -1]], np.float32)
    faces = np.asarray([[0, 1, 2], [4, 5, 6], [2, 0, 1], [0, 7, 1]], np.int32)                    # the last one is a bad face
    labels = C.labels_union_find(faces, 7)
    s = C.component_stats(verts, faces, labels)
    assert s['roots'].tolist() == [0, 3, 4] and s['n_verts'].tolist() == [3, 1, 3] and s['n_faces'].tolist() == [2, 0, 1]
    assert np.array_equal(s['lo'], np.asarray([[-0.0, -2, 0], [9, 9, 9], [4, 3, -1]], np.float32))
    assert np.signbit(s['lo'][0, 0]) and not np.signbit(s['hi'][0, 2])                            # -0 orders below +0
    assert np.array_equal(s['hi'], np.asarray([[1, 3, 1], [9, 9, 9], [5, 6, 4]], np.float32))
    assert C.diagonal2(s).tolist() == [27.0, 0.0, 35.0]
    assert C.keep_rule(s, min_faces=1).tolist() == [True, False, True]
    assert C.keep_rule(s, min_diagonal=5.5).tolist() == [False, False, True]
    assert C.keep_rule(s, keep_largest=1).tolist() == [True, False, False]


@pytest.mark.parametrize('name', sorted(C.cases()))
def test_filter_is_idempotent_and_its_defaults_are_the_identity(name):
    verts, faces = C.cases()[name]
    v0, f0, m0 = C.filter_components(verts, faces)
    assert np.array_equal(v0.view(np.uint32), verts.view(np.uint32)) and np.array_equal(f0, faces)
    assert np.array_equal(m0, np.arange(len(verts)))
    for rule in C.RULES:
        v1, f1, m1 = C.filter_components(verts, faces, **rule)
        v2, f2, m2 = C.filter_components(v1, f1, **rule)
        assert np.array_equal(v2.view(np.uint32), v1.view(np.uint32)) and np.array_equal(f2, f1), rule
        assert np.array_equal(m2, np.arange(len(v1))), rule
        kept = m1 >= 0
        assert np.array_equal(m1[kept], np.arange(kept.sum())) and np.array_equal(v1, verts[kept])
        assert len(f1) == 0 or (f1.min() >= 0 and f1.max() < len(v1))


def test_keep_largest_ties_go_to_the_smaller_label():
    verts, faces = C.cases()['disjoint_1000']
    labels = C.labels_propagation(faces, len(verts))
    s = C.component_stats(verts, faces, labels)
    three = s['roots'][s['n_faces'] == 3]                                      # 333 components tie at three faces
    for k in (1, 3, 10):
        kept = s['roots'][C.keep_rule(s, keep_largest=k)]
        assert np.array_equal(kept, three[:k]), k                              # roots are ascending: the k smallest labels
    kept = s['roots'][C.keep_rule(s, keep_largest=400)]
    one = s['roots'][s['n_faces'] == 1]
    assert np.array_equal(np.sort(kept), np.sort(np.concatenate([three, one[:67]])))
    # the selection comes after the thresholds
    big = s['roots'][C.keep_rule(s, min_diagonal=2.0)]
    assert 3 < len(big) < len(s['roots'])
    top = s['roots'][C.keep_rule(s, min_diagonal=2.0, keep_largest=3)]
    order = sorted(big.tolist(), key=lambda r: (-int(s['n_faces'][s['roots'] == r][0]), r))
    assert sorted(top.tolist()) == sorted(order[:3])


def test_surface_thresholds_keep_clear_of_every_diagonal():
    for name in C.SURFACE_CASES:
        (v, f) = C.surface_mesh(name)
        s = C.component_stats(v, f, C.labels_propagation(f, len(v)))
        for k in (1.5, 3.5):
            assert C.diagonal_margin(s, k * C.lattice_unit(name)) > 1e-3, (name, k)


# ---- the union-find core from many host threads ------------------------------------------------------------------------------
def test_union_find_core_from_sixteen_host_threads(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'uf_stress')
    subprocess.run([cxx, '-O2', '-std=c++17', '-pthread', os.path.join(ROOT, 'tests', 'uf_stress.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe, '16', '3'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith('ok'), r.stdout


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(built):
    from nerfstyle_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'nsr.h')).read()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', hdr) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.lib().nsr_abi_version() == _lib.ABI_VERSION == 6               # additive: the version stays


def test_workspace_size(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    assert L.nsr_mesh_filter_workspace_bytes(2 ** 31, 1) == 0 and L.nsr_mesh_filter_workspace_bytes(1, 2 ** 31) == 0
    for V, F in ((0, 0), (5, 0), (1000, 3000), (2 ** 31 - 1, 7), (9, 2 ** 31 - 1)):
        b = L.nsr_mesh_filter_workspace_bytes(V, F)
        blocks = max(-(-max(V, F) // 256), 1)
        assert b % 16 == 0 and 8 * blocks <= b <= 8 * blocks * 1.01 + 256, (V, F, b)


def test_invalid_arguments_answer_before_a_device_is_touched(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    INVALID = -1
    a = 0x10000                                                     # aligned, never dereferenced: the checks come first
    big = 2 ** 31
    comp = lambda faces=a, V=8, F=4, labels=a, bad=a: L.nsr_mesh_components(faces, V, F, labels, bad, None)
    assert comp(V=big) == INVALID and comp(F=big) == INVALID
    assert comp(faces=None) == INVALID and comp(labels=None) == INVALID and comp(bad=None) == INVALID
    assert comp(faces=a + 2) == INVALID and comp(labels=a + 1) == INVALID and comp(bad=a + 3) == INVALID

    def stats(verts=a, faces=a, labels=a, V=8, F=4, nv=a, nf=a, lo=a, hi=a):
        return L.nsr_mesh_component_stats(verts, faces, labels, V, F, nv, nf, lo, hi, None)
    assert stats(V=big) == INVALID and stats(F=big) == INVALID
    for k in ('verts', 'faces', 'labels', 'nv', 'nf', 'lo', 'hi'):
        assert stats(**{k: None}) == INVALID and stats(**{k: a + 2}) == INVALID, k

    def count(faces=a, labels=a, keep=a, V=8, F=4, ws=a, counts=a):
        return L.nsr_mesh_filter_count(faces, labels, keep, V, F, ws, counts, None)
    assert count(V=big) == INVALID and count(F=big) == INVALID
    for k in ('faces', 'labels', 'keep', 'ws', 'counts'):
        assert count(**{k: None}) == INVALID, k
    for k in ('faces', 'labels', 'counts'):
        assert count(**{k: a + 2}) == INVALID, k
    assert count(ws=a + 8) == INVALID

    def emit(verts=a, faces=a, labels=a, keep=a, V=8, F=4, ws=a, Vk=6, Fk=2, imap=a, vo=a, fo=a):
        return L.nsr_mesh_filter_emit(verts, faces, labels, keep, V, F, ws, Vk, Fk, imap, vo, fo, None)
    assert emit(V=big) == INVALID and emit(F=big) == INVALID
    for k in ('verts', 'faces', 'labels', 'keep', 'ws', 'imap', 'vo', 'fo'):
        assert emit(**{k: None}) == INVALID, k
    for k in ('verts', 'faces', 'labels', 'imap', 'vo', 'fo'):
        assert emit(**{k: a + 1}) == INVALID, k
    assert emit(ws=a + 8) == INVALID
    assert emit(Vk=9) == INVALID and emit(Fk=5) == INVALID and emit(Vk=0, Fk=1) == INVALID        # counts that disagree


def test_python_layer_refuses_cpu_tensors_and_bad_input(built):
    from nerfstyle_amd import mesh
    verts, faces = (torch.from_numpy(np.array(x)) for x in C.cases()['shared_edge'])
    labels = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mesh.connected_components(faces, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mesh.component_stats(verts, faces, labels)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mesh.filter_components(verts, faces, min_faces=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mesh.Mesh(verts, faces).clean(min_faces=1)
    for bad in (faces.to(torch.int64), faces.reshape(-1), faces[:, :2], faces.numpy()):
        with pytest.raises(ValueError, match='faces must be an int32'):
            mesh.connected_components(bad, 4)
        with pytest.raises(ValueError, match='faces must be an int32'):
            mesh.filter_components(verts, bad)
    for bad in (verts.double(), verts.reshape(-1), verts[:, :2]):
        with pytest.raises(ValueError, match='verts must be a float32'):
            mesh.filter_components(bad, faces)
        with pytest.raises(ValueError, match='verts must be a float32'):
            mesh.component_stats(bad, faces, labels)
    with pytest.raises(ValueError, match='labels must be an int32'):
        mesh.component_stats(verts, faces, labels.to(torch.int64))
    with pytest.raises(ValueError, match='labels must be an int32'):
        mesh.component_stats(verts, faces, labels[:3])
    with pytest.raises(ValueError):
        mesh.connected_components(faces, -1)
    for rule in (dict(min_faces=-1), dict(min_faces=1.5), dict(min_diagonal=-0.5), dict(min_diagonal=float('nan')), dict(keep_largest=0),
                 dict(keep_largest=2.5)):
        with pytest.raises(ValueError):
            mesh.filter_components(verts, faces, **rule)
