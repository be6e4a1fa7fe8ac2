"""Region-wise colour transfer, host side: the test's restatement (color_regions_ref.py) against the reference's recorded
per-region outputs (tests/golden/make_color_regions_goldens.py), nerfstyle_amd.color_match.solve_region_transforms against the
restatement, the label rule, and the C ABI's host-only paths."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import color_match_ref as R
import color_regions_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('a_fallbacks', 'b_shared')
KC, KS = 4, 3
# The reference computes in f32, so its own error sets the bar.  Distance of the fp64 restatement from the reference's outputs as
# make_color_regions_goldens.py printed it (max abs over all regions):
#                    A           b           image
#   a_fallbacks      1.085e-05   9.537e-07   1.609e-06
#   b_shared         8.225e-06   1.162e-06   1.192e-06
# Allowed: four times the largest of each column (A and image come out above the global test's figures, so they are not imported
# from there).  tests/test_gpu_color_regions.py holds the device path to the same bars.
TOL_A, TOL_B, TOL_IMAGE = 4 * 1.085e-05, 4 * 1.162e-06, 4 * 1.609e-06


def load_cases():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'color_regions_reference.npz'))
    keys = ('content', 'classes', 'style', 'clusters', 'matching', 'min_rows', 'tfs', 'image')
    return {name: {k: z[name + '_' + k] for k in keys} for name in CASES}


@pytest.fixture(scope='module')
def cases():
    return load_cases()


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def _sides(c):
    rows, srows = c['content'].reshape(-1, 3), c['style'].reshape(-1, 3)
    return rows, G.region_of(c['classes'].reshape(-1), KC), srows, G.region_of(c['clusters'].reshape(-1), KS)


def test_fixture_covers_the_issue_cases(cases):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'color_regions_reference.npz')) < 512 * 1024
    for name, c in cases.items():
        assert c['content'].shape == (3, 33, 47, 3) and c['classes'].shape == (3, 33, 47) and c['style'].shape == (21, 19, 3)
        assert c['clusters'].shape == (21, 19) and c['tfs'].shape == (KC + 1, 4, 4) and c['image'].shape == c['content'].shape
        assert c['tfs'].dtype == np.float32 and c['image'].dtype == np.float32 and int(c['min_rows']) == 64
    a, b = cases['a_fallbacks'], cases['b_shared']
    counts = np.bincount(G.region_of(a['classes'].reshape(-1), KC), minlength=KC + 1)
    assert a['matching'].tolist() == [1, 0, -1, 2] and 0 < counts[3] < 64 <= counts[:3].min() and counts[4] > 0
    assert np.array_equal(a['tfs'][2], a['tfs'][4]) and np.array_equal(a['tfs'][3], a['tfs'][4])       # the fallbacks
    assert not np.array_equal(a['tfs'][0], a['tfs'][4]) and not np.array_equal(a['tfs'][0], a['tfs'][1])
    assert b['matching'].tolist() == [2, 2, 0, 1] and (b['clusters'] == -1).any()


def test_restatement_equals_reference(cases):
    for name, c in cases.items():
        rows, reg, srows, sreg = _sides(c)
        got, tfs = G.match_by_region(rows, reg, KC, srows, sreg, KS, c['matching'].tolist(), int(c['min_rows']), 'global')
        assert got.dtype == np.float32 and tfs.dtype == np.float32 and tfs.shape == (KC + 1, 4, 4)
        dA, db = np.abs(tfs[:, :3, :3] - c['tfs'][:, :3, :3]).max(), np.abs(tfs[:, :3, 3] - c['tfs'][:, :3, 3]).max()
        di = np.abs(got - c['image'].reshape(-1, 3)).max()
        print('{:12s} restatement |dA| {:.3e} |db| {:.3e} |dimage| {:.3e}'.format(name, dA, db, di))
        assert dA <= TOL_A and db <= TOL_B and di <= TOL_IMAGE, name


def _same(got, ref):
    """two fp64 eigen-solvers of the same 3x3 matrices: the same transforms up to rounding of A's size (as the global test)"""
    assert got.dtype == torch.float32 and got.device.type == 'cpu' and tuple(got.shape) == ref.shape
    got = got.numpy()
    for k in range(ref.shape[0]):
        assert np.abs(got[k] - ref[k]).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(ref[k]).max()), k
        assert np.array_equal(got[k, 3], np.array([0, 0, 0, 1], np.float32))


def test_solve_region_transforms_equals_restatement(cases):
    """Host code: runs without a device, takes tensors, arrays or lists.  Cases: matched classes, matching[i] = -1, a class
    below min_rows, a cluster below min_rows, two classes on one cluster, both fallbacks."""
    from nerfstyle_amd.color_match import solve_region_transforms
    for name, c in cases.items():
        rows, reg, srows, sreg = _sides(c)
        mc, ms = G.region_moments(rows, reg, KC), G.region_moments(srows, sreg, KS)
        for matching, min_rows in ((c['matching'].tolist(), 64),       # the golden's: a: -1 and a small class; b: a shared cluster
                                   ([0, 1, 2, 0], 120),                # cluster 2 (100..105 rows) is below min_rows
                                   ([2, 2, 2, 2], 1),                  # every class matched, all on one cluster
                                   ([-1, 3, 7, -5], 1)):               # nothing matched: 3 >= Ks, negative
            for fallback in ('global', 'identity'):
                ref = G.solve_regions(mc, ms, matching, min_rows, fallback)
                _same(solve_region_transforms(torch.from_numpy(mc), ms, matching, min_rows=min_rows, fallback=fallback), ref)
                if fallback == 'identity':
                    assert np.array_equal(ref[KC], np.eye(4, dtype=np.float32))
        # which classes fell back, in the golden's own setting
        ref = G.solve_regions(mc, ms, c['matching'].tolist(), 64, 'global')
        fell = [bool(np.array_equal(ref[i], ref[KC])) for i in range(KC)]
        assert fell == ([False, False, True, True] if name == 'a_fallbacks' else [False, False, False, True])
        if name == 'b_shared':
            assert not np.array_equal(ref[0], ref[1])                   # one cluster, two content regions: two transforms
        ref = G.solve_regions(mc, ms, [0, 1, 2, 0], 120, 'global')
        assert np.array_equal(ref[2], ref[KC]) and not np.array_equal(ref[0], ref[KC])
        got = solve_region_transforms(torch.from_numpy(mc), torch.from_numpy(ms), torch.tensor(c['matching'].tolist()), min_rows=64)
        dA, db = np.abs(got.numpy()[:, :3, :3] - c['tfs'][:, :3, :3]).max(), np.abs(got.numpy()[:, :3, 3] - c['tfs'][:, :3, 3]).max()
        assert dA <= TOL_A and db <= TOL_B, name
    with pytest.raises(ValueError):
        solve_region_transforms(mc, ms, [0, 1, 2])                      # len(matching) != Kc
    with pytest.raises(ValueError):
        solve_region_transforms(mc[:, :9], ms, [0, 1, 2, 0])
    with pytest.raises(ValueError):
        solve_region_transforms(mc, ms, [0, 1, 2, 0], fallback='none')


def test_one_region_equals_the_global_solve(cases):
    """K = 1 with every row in region 0 is the global transfer: color_match_ref.solve of the whole set, in slot 0 and slot 1"""
    from nerfstyle_amd.color_match import solve_region_transforms
    c = cases['a_fallbacks']
    rows, srows = c['content'].reshape(-1, 3), c['style'].reshape(-1, 3)
    mc = G.region_moments(rows, np.zeros(rows.shape[0], np.int64), 1)
    ms = G.region_moments(srows, np.zeros(srows.shape[0], np.int64), 1)
    assert mc[1].tolist() == [0.0] * 10 and mc[0, 0] == rows.shape[0] and np.array_equal(mc[0, 1:], R.moments(rows))
    ref = R.solve(R.moments(rows), rows.shape[0], R.moments(srows), srows.shape[0])
    assert np.array_equal(G.solve_regions(mc, ms, [0], 256, 'global'), np.stack([ref, ref]))
    _same(solve_region_transforms(mc, ms, [0]), np.stack([ref, ref]))
    _same(solve_region_transforms(mc, ms, [0], fallback='identity'), np.stack([ref, np.eye(4, dtype=np.float32)]))


def test_region_of():
    K = 3
    w = np.array([-1, K, 2.5, np.nan, np.inf, -0.0, 0.0, 1.0, 2.0, -np.inf, 1e30, 2.0000002, 1e-45], np.float32)
    assert G.region_of(w, K).tolist() == [K, K, K, K, K, 0, 0, 1, 2, K, K, K, K]
    assert G.region_of(np.array([-1, K, 0, 2, -2 ** 31, 2 ** 31 - 1], np.int32), K).tolist() == [K, K, 0, 2, K, K]
    # rows of each region and nothing else; an empty region is ten zeros
    rng = np.random.default_rng(1)
    rows = rng.random((50, 4)).astype(np.float32)
    reg = G.region_of(rng.integers(-1, 4, 50), 4)
    reg[reg == 2] = 4
    m = G.region_moments(rows, reg, 4)
    assert m[:, 0].sum() == 50 and m[2].tolist() == [0.0] * 10 and np.allclose(m[:, 1:].sum(0), R.moments(rows), rtol=1e-14)
    tfs = np.repeat(np.eye(4, dtype=np.float32)[None], 5, 0)
    tfs[:, :3, 3] = 10.0 * np.arange(5)[:, None]
    out = G.apply_regions(rows, reg, tfs, clamp=False)
    assert np.array_equal(np.rint((out[:, 0] - rows[:, 0]) / 10).astype(np.int64), reg) and np.array_equal(out[:, 3], rows[:, 3])


def _proto(src, name):
    m = re.search(r'\b(?:int|uint64_t)\s+' + name + r'\s*\(([^)]*)\)\s*;', src)
    assert m, name + ' is not declared in include/nsr.h'
    return [a.strip() for a in m.group(1).split(',')]


def test_symbols_signatures_and_host_refusals(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    text = open(os.path.join(ROOT, 'include', 'nsr.h')).read()
    assert re.search(r'#define\s+NSR_COLOR_MAX_REGIONS\s+64\b', text)
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, nargs in (('nsr_color_region_moments_workspace_bytes', 2), ('nsr_color_region_moments', 8), ('nsr_color_region_apply', 9)):
        assert hasattr(so, name), 'libnsr_hip.so does not export ' + name
        declared = _proto(src, name)
        res, args = _lib.SIGNATURES[name]
        assert len(declared) == len(args) == nargs, name
        for a, t in zip(declared, args):
            assert (t is _lib.vp) == ('*' in a or a.startswith('nsr_stream_t')), (name, a)
            assert (t is _lib.u64) == a.startswith('uint64_t') and (t is _lib.u32) == a.startswith('uint32_t'), (name, a)
    assert _lib.ABI_VERSION == 6
    L = _lib.lib()
    assert L.nsr_abi_version() == 6
    # the grid is that of the global pass, a function of n alone; (K + 1) x 10 doubles a block
    assert L.nsr_color_region_moments_workspace_bytes(1, 1) == 2 * 80
    assert L.nsr_color_region_moments_workspace_bytes(1024, 5) == 6 * 80 and L.nsr_color_region_moments_workspace_bytes(1025, 5) == 2 * 6 * 80
    assert L.nsr_color_region_moments_workspace_bytes(35 * 1008 * 756, 64) == 2048 * 65 * 80
    assert L.nsr_color_region_moments_workspace_bytes(1024, 0) == 0 and L.nsr_color_region_moments_workspace_bytes(1024, 65) == 0
    rows, rows2, mom, ws, tfs, lab = (ctypes.c_void_p(a) for a in (4096, 65536, 8192, 12288, 16384, 20480))   # never dereferenced
    M, A = L.nsr_color_region_moments, L.nsr_color_region_apply
    # refused before anything touches a device
    assert M(None, 8, 4, lab, 2, mom, ws, None) == -1 and M(rows, 8, 4, lab, 2, None, ws, None) == -1
    assert M(rows, 8, 4, lab, 2, mom, None, None) == -1
    assert M(rows, 0, 4, lab, 2, mom, ws, None) == -1                                           # n == 0
    assert M(rows, 8, 2, lab, 2, mom, ws, None) == -1 and M(rows, 8, 5, lab, 2, mom, ws, None) == -1
    assert M(rows, 8, 4, lab, 0, mom, ws, None) == -1 and M(rows, 8, 4, lab, 65, mom, ws, None) == -1
    assert M(rows, 8, 3, None, 2, mom, ws, None) == -1                                          # stride 3 carries no label
    assert M(ctypes.c_void_p(4098), 8, 3, lab, 2, mom, ws, None) == -1                          # rows: 4 bytes
    assert M(ctypes.c_void_p(4100), 8, 4, lab, 2, mom, ws, None) == -1                          # stride 4: 16 bytes
    assert M(rows, 8, 4, ctypes.c_void_p(20482), 2, mom, ws, None) == -1                        # labels: 4 bytes
    assert M(rows, 8, 4, lab, 2, ctypes.c_void_p(8196), ws, None) == -1                         # moments, workspace: 8 bytes
    assert M(rows, 8, 4, lab, 2, mom, ctypes.c_void_p(12292), None) == -1
    assert A(None, rows2, 8, 4, lab, 2, tfs, 1, None) == -1 and A(rows, None, 8, 4, lab, 2, tfs, 1, None) == -1
    assert A(rows, rows2, 8, 4, lab, 2, None, 1, None) == -1
    assert A(rows, rows2, 0, 4, lab, 2, tfs, 1, None) == -1
    assert A(rows, rows2, 8, 1, lab, 2, tfs, 1, None) == -1 and A(rows, rows2, 8, 5, lab, 2, tfs, 1, None) == -1
    assert A(rows, rows2, 8, 4, lab, 0, tfs, 1, None) == -1 and A(rows, rows2, 8, 4, lab, 65, tfs, 1, None) == -1
    assert A(rows, rows2, 8, 3, None, 2, tfs, 1, None) == -1
    assert A(ctypes.c_void_p(4098), rows2, 8, 3, lab, 2, tfs, 1, None) == -1 and A(rows, ctypes.c_void_p(65538), 8, 3, lab, 2, tfs, 1, None) == -1
    assert A(ctypes.c_void_p(4100), rows2, 8, 4, lab, 2, tfs, 1, None) == -1 and A(rows, ctypes.c_void_p(65540), 8, 4, lab, 2, tfs, 1, None) == -1
    assert A(rows, rows2, 8, 4, ctypes.c_void_p(20481), 2, tfs, 1, None) == -1
    assert A(rows, rows2, 8, 4, lab, 2, ctypes.c_void_p(16386), 1, None) == -1
    # src and dst that overlap without being equal: 8 rows of 16 B from 4096 reach 4224
    for stride, off in ((4, 16), (4, 112), (3, 12), (3, 84)):
        assert A(rows, ctypes.c_void_p(4096 + off), 8, stride, lab, 2, tfs, 1, None) == -1, (stride, off)
        assert A(ctypes.c_void_p(4096 + off), rows, 8, stride, lab, 2, tfs, 1, None) == -1, (stride, off)


def test_wrappers_refuse_cpu_tensors_and_bad_arguments(built):
    from nerfstyle_amd import color_match as CM
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ResidentDataset
    rows = torch.rand(10, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        CM.region_moments(rows, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        CM.region_moments(rows[:, :3].contiguous(), 2, torch.zeros(10, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        CM.apply_region_transforms(rows, torch.eye(4).repeat(3, 1, 1))

    def dataset(num_classes, seg=True):
        rng = np.random.default_rng(0)
        return ResidentDataset(rng.random((2, 3, 4, 5), np.float32), np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)),
                               Intrinsics(4, 5, 5.0, 5.0, 2.5, 2.0), 1.0, 'cpu',
                               seg_maps=rng.integers(0, 2, (2, 4, 5)).astype(np.float32) if seg else None, num_classes=num_classes)
    style, clusters = torch.rand(3, 6, 7), torch.zeros(6, 7, dtype=torch.int64)
    ds = dataset(2)
    assert ds.region_tf is None and ds.color_tf is None
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ds.match_colors_by_region(style, clusters, [0, 0])
    assert ds.region_tf is None
    with pytest.raises(ValueError, match='segment maps'):
        dataset(0, seg=False).match_colors_by_region(style, clusters, [])
    with pytest.raises(ValueError, match='style_image'):
        ds.match_colors_by_region(torch.rand(6, 7, 3), clusters, [0, 0])
    with pytest.raises(ValueError, match='style_clusters'):
        ds.match_colors_by_region(style, torch.zeros(7, 6, dtype=torch.int64), [0, 0])
    with pytest.raises(ValueError, match='style_clusters'):
        ds.match_colors_by_region(style, torch.zeros(6, 7), [0, 0])                             # not integer
    with pytest.raises(ValueError, match='matching'):
        ds.match_colors_by_region(style, clusters, [0])
    with pytest.raises(ValueError, match='num_classes'):
        dataset(65).match_colors_by_region(style, clusters, [0] * 65)
    with pytest.raises(ValueError, match='clusters'):
        ds.match_colors_by_region(style, clusters + 64, [0, 0])
