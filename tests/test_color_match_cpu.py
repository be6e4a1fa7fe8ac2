"""Colour transfer to a style image (the reference's utils.match_colors_for_image_set, utils/__init__.py:262-295), host side:
the test's restatement (color_match_ref.py) and nerfstyle_amd.color_match.solve_color_transform against the reference's
recorded outputs (tests/golden/make_color_match_goldens.py), the eigenvalue clamp on a grey content set, and the C ABI's
host-only paths."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import color_match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('a_uniform', 'b_photo', 'c_grey_style', 'd_clamped')
# The reference computes in f32 (means, centred matmul, SVD, the map), so its own error sets the bar, and it varies from case to
# case.  Distance of the fp64 restatement from the reference's outputs as make_color_match_goldens.py printed it (max abs):
#                    A           b           image       outputs at the clamp
#   a_uniform        4.768e-07   3.632e-07   4.768e-07    7.30 %
#   b_photo          5.364e-06   2.086e-07   8.643e-07    1.77 %
#   c_grey_style     3.576e-07   8.941e-08   2.384e-07    3.38 %
#   d_clamped        2.384e-06   1.192e-06   6.557e-07   11.04 %
# Allowed: four times the largest of each column.  tests/test_gpu_color_match.py holds the device path to the same bars.
TOL_A, TOL_B, TOL_IMAGE = 4 * 5.364e-06, 4 * 1.192e-06, 4 * 8.643e-07


def load_cases():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'color_match_reference.npz'))
    out = {}
    for name in CASES:
        content = z[('b_photo' if name == 'c_grey_style' else name) + '_content']
        out[name] = (content, z[name + '_style'], z[name + '_image'], z[name + '_tf'])
    return out


@pytest.fixture(scope='module')
def cases():
    return load_cases()


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def test_fixture_covers_the_issue_cases(cases):
    shapes = {n: (c.shape, s.shape) for n, (c, s, _, _) in cases.items()}
    assert shapes == {'a_uniform': ((3, 5, 7, 3), (6, 9, 3)), 'b_photo': ((4, 33, 47, 3), (21, 19, 3)),
                      'c_grey_style': ((4, 33, 47, 3), (8, 8, 3)), 'd_clamped': ((2, 16, 20, 3), (12, 10, 3))}
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'color_match_reference.npz')) < 512 * 1024
    # b: one large and two small eigenvalues; c: a grey style image, rank-1 covariance; d: several per cent at the clamp
    content, style, image, tf = cases['b_photo']
    e = np.linalg.eigvalsh(R.mean_cov(R.moments(content.reshape(-1, 3)), content.size // 3)[1])
    assert e[2] > 20 * e[1] and e[0] > 1e-6
    _, style, _, _ = cases['c_grey_style']
    assert np.array_equal(style[..., 0], style[..., 1]) and np.array_equal(style[..., 0], style[..., 2])
    e = np.linalg.eigvalsh(R.mean_cov(R.moments(style.reshape(-1, 3)), style.size // 3)[1])
    assert e[2] > 1e-2 and abs(e[1]) < 1e-8 and abs(e[0]) < 1e-8                 # the 1e-8 clamp decides the style side
    _, _, image, _ = cases['d_clamped']
    assert np.mean((image == 0.0) | (image == 1.0)) > 0.03
    for _, _, image, tf in cases.values():
        assert image.dtype == np.float32 and tf.dtype == np.float32
        assert np.array_equal(tf[3], np.array([0, 0, 0, 1], np.float32))


def test_restatement_equals_reference(cases):
    for name, (content, style, image, tf) in cases.items():
        r_image, r_tf = R.match(content, style)
        assert r_tf.dtype == np.float32 and r_image.dtype == np.float32
        dA, db = np.abs(r_tf[:3, :3] - tf[:3, :3]).max(), np.abs(r_tf[:3, 3] - tf[:3, 3]).max()
        di = np.abs(r_image - image).max()
        print('{:14s} restatement |dA| {:.3e} |db| {:.3e} |dimage| {:.3e}'.format(name, dA, db, di))
        assert dA <= TOL_A and db <= TOL_B and di <= TOL_IMAGE, name
        assert np.array_equal(r_tf[3], tf[3])


def test_solve_color_transform_equals_reference(cases):
    """solve_color_transform fed the restatement's moments: the golden color_tf, and with the restatement's f32 chain the golden
    image.  It is host code: it runs without a device and takes tensors or arrays."""
    from nerfstyle_amd.color_match import solve_color_transform
    for name, (content, style, image, tf) in cases.items():
        rows, srows = content.reshape(-1, 3), style.reshape(-1, 3)
        mc, ms = R.moments(rows), R.moments(srows)
        got = solve_color_transform(torch.from_numpy(mc), rows.shape[0], ms, srows.shape[0])
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, 4) and got.device.type == 'cpu'
        got = got.numpy()
        dA, db = np.abs(got[:3, :3] - tf[:3, :3]).max(), np.abs(got[:3, 3] - tf[:3, 3]).max()
        di = np.abs(R.apply(rows, got).reshape(image.shape) - image).max()
        print('{:14s} solve       |dA| {:.3e} |db| {:.3e} |dimage| {:.3e}'.format(name, dA, db, di))
        assert dA <= TOL_A and db <= TOL_B and di <= TOL_IMAGE, name
        assert np.array_equal(got[3], np.array([0, 0, 0, 1], np.float32))
        # two fp64 eigen-solvers of the same 3x3 matrices: the same transform up to rounding of A's size
        ref = R.solve(mc, rows.shape[0], ms, srows.shape[0])
        assert np.abs(got - ref).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max()), name
    with pytest.raises(ValueError):
        solve_color_transform(torch.zeros(8, dtype=torch.float64), 4, torch.zeros(9, dtype=torch.float64), 4)


def test_grey_content_shows_the_eigenvalue_clamp():
    """A grey content set has a rank-1 covariance: two eigenvalues are clamped to 1e-8 and the gain along them reaches
    sqrt(style eigenvalue / 1e-8).  The reference's own f32 SVD noise dominates there, so this case is held to the fp64
    restatement only: the clamp is what keeps everything finite."""
    from nerfstyle_amd.color_match import solve_color_transform
    rng = np.random.default_rng(5)
    content = np.repeat(rng.random((2 * 9 * 11, 1)), 3, axis=1).astype(np.float32)
    style = rng.random((7 * 6, 3)).astype(np.float32)
    mc, ms = R.moments(content), R.moments(style)
    got = solve_color_transform(mc, content.shape[0], ms, style.shape[0]).numpy()
    ref = R.solve(mc, content.shape[0], ms, style.shape[0])
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    gain = np.linalg.norm(got[:3, :3].astype(np.float64), 2)
    e_s = np.linalg.eigvalsh(R.mean_cov(ms, style.shape[0])[1])
    assert 100.0 < gain <= 1.001 * np.sqrt(e_s[2] / 1e-8)                     # without the clamp: 1 / sqrt(~0)
    # relative to the gain: the two solvers pick different bases of the degenerate eigenspace and sum in another order
    assert np.abs(got - ref).max() <= 1e-6 * gain
    out = R.apply(content, got)
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
    # the mean still lands on the style's mean, up to the f32 rounding of A: three entries a row, each off by at most
    # eps / 2 of the gain, times a mean of at most 1
    mu_s = ms[:3] / style.shape[0]
    mu_c = mc[:3] / content.shape[0]
    assert np.abs(got[:3, :3].astype(np.float64) @ mu_c + got[:3, 3] - mu_s).max() < 2 * np.finfo(np.float32).eps * gain


def test_apply_restatement_properties():
    rng = np.random.default_rng(6)
    rows = rng.random((257, 4)).astype(np.float32)
    rows[:, 3] = 1e30
    ident = np.eye(4, dtype=np.float32)
    assert np.array_equal(R.apply(rows, ident), rows)
    tf = np.eye(4, dtype=np.float32)
    tf[:3, :3] = rng.standard_normal((3, 3)).astype(np.float32)
    tf[:3, 3] = rng.standard_normal(3).astype(np.float32)
    out = R.apply(rows, tf, clamp=False)
    exact = rows[:, :3].astype(np.float64) @ tf[:3, :3].astype(np.float64).T + tf[:3, 3].astype(np.float64)
    assert (np.abs(out[:, :3] - exact) <= 3 * R.apply_bound(rows, tf)).all()       # three roundings, one bound each at most
    assert np.array_equal(out[:, 3], rows[:, 3])
    assert np.array_equal(R.apply(rows, tf), np.concatenate([np.clip(out[:, :3], 0, 1), rows[:, 3:]], 1))


def _proto(src, name):
    m = re.search(r'\b(?:int|uint64_t)\s+' + name + r'\s*\(([^)]*)\)\s*;', src)
    assert m, name + ' is not declared in include/nsr.h'
    return [a.strip() for a in m.group(1).split(',')]


def test_symbols_signatures_and_host_refusals(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nsr.h')).read(), flags=re.S)
    for name, nargs in (('nsr_color_moments_workspace_bytes', 1), ('nsr_color_moments', 6), ('nsr_color_apply', 7)):
        assert hasattr(so, name), 'libnsr_hip.so does not export ' + name
        declared = _proto(src, name)
        res, args = _lib.SIGNATURES[name]
        assert len(declared) == len(args) == nargs, name
        for a, t in zip(declared, args):
            assert (t is _lib.vp) == ('*' in a or a.startswith('nsr_stream_t')), (name, a)
            assert (t is _lib.u64) == a.startswith('uint64_t') and (t is _lib.u32) == a.startswith('uint32_t'), (name, a)
    assert _lib.ABI_VERSION == 6
    L = _lib.lib()
    # the grid is a function of n alone: ceil(n / 1024) blocks of nine doubles, at most 2048
    assert L.nsr_color_moments_workspace_bytes(1) == 72
    assert L.nsr_color_moments_workspace_bytes(1024) == 72 and L.nsr_color_moments_workspace_bytes(1025) == 2 * 72
    assert L.nsr_color_moments_workspace_bytes(70001) == 69 * 72
    assert L.nsr_color_moments_workspace_bytes(35 * 1008 * 756) == 2048 * 72
    rows, rows2, mom, ws, tf = (ctypes.c_void_p(a) for a in (4096, 65536, 8192, 12288, 16384))   # never dereferenced
    # refused before anything touches a device: n == 0, stride outside {3, 4}, NULL pointers
    assert L.nsr_color_moments(rows, 0, 3, mom, ws, None) == -1
    assert L.nsr_color_moments(rows, 8, 2, mom, ws, None) == -1 and L.nsr_color_moments(rows, 8, 5, mom, ws, None) == -1
    assert L.nsr_color_moments(None, 8, 3, mom, ws, None) == -1
    assert L.nsr_color_moments(rows, 8, 3, None, ws, None) == -1
    assert L.nsr_color_moments(rows, 8, 3, mom, None, None) == -1
    assert L.nsr_color_apply(rows, rows2, 0, 4, tf, 1, None) == -1
    assert L.nsr_color_apply(rows, rows2, 8, 1, tf, 1, None) == -1
    assert L.nsr_color_apply(None, rows2, 8, 4, tf, 1, None) == -1
    assert L.nsr_color_apply(rows, None, 8, 4, tf, 1, None) == -1
    assert L.nsr_color_apply(rows, rows2, 8, 4, None, 1, None) == -1
    # src and dst that overlap without being equal: 8 rows of 16 B from 4096 reach 4224
    for stride, off in ((4, 16), (4, 112), (3, 12), (3, 84)):
        assert L.nsr_color_apply(rows, ctypes.c_void_p(4096 + off), 8, stride, tf, 1, None) == -1, (stride, off)
        assert L.nsr_color_apply(ctypes.c_void_p(4096 + off), rows, 8, stride, tf, 1, None) == -1, (stride, off)


def test_wrappers_refuse_cpu_tensors(built):
    from nerfstyle_amd import color_match as CM
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ResidentDataset
    rows = torch.rand(10, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        CM.color_moments(rows)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        CM.apply_color_transform(rows, torch.eye(4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        CM.match_colors_for_image_set(torch.rand(2, 4, 5, 3), torch.rand(3, 3, 3))
    ds = ResidentDataset(np.random.default_rng(0).random((2, 3, 4, 5), np.float32), np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)),
                         Intrinsics(4, 5, 5.0, 5.0, 2.5, 2.0), 1.0, 'cpu')
    assert ds.color_tf is None
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ds.match_colors(torch.rand(3, 6, 6))
    with pytest.raises(ValueError, match='style_image'):
        ds.match_colors(torch.rand(6, 6, 3))
