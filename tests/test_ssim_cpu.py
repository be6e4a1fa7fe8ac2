"""SSIM, host side: the two restatements of the definition (tests/ssim_ref.py) against each other, their basic properties, the
C ABI's two new symbols and every refusal nsr_ssim makes before it touches a device, and the Python wrapper's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


@pytest.mark.parametrize('shape', [(13, 12), (11, 11)])
def test_the_two_restatements_agree(shape):
    H, W = shape
    for kind, x, y in R.image_pairs(H, W, seed=3):
        for padding in ('same', 'valid'):
            a, b = R.ssim_ref(x, y, padding), R.ssim_loops(x, y, padding)
            for k in ('value', 'channels', 'map', 'grad'):
                assert np.abs(np.asarray(a[k]) - np.asarray(b[k])).max() <= 1e-12, (kind, padding, k)
            assert float(np.abs(a['grad']).max()) > 1e-6
    # 11x11 'valid': one counted pixel per channel
    a = R.ssim_ref(x, y, 'valid')
    if shape == (11, 11):
        assert np.count_nonzero(a['map']) == 3 and abs(a['map'][5, 5].mean() - a['value']) < 1e-15


def test_window_is_the_f32_rounded_gaussian():
    from nerfstyle_amd.ssim import TILE, window
    g = window()
    assert g.dtype == torch.float32 and g.shape == (11,)
    assert np.array_equal(g.numpy().astype(np.float64), R.window64())
    assert abs(float(R.window64().sum()) - 1.0) < 1e-7 and np.array_equal(R.window64(), R.window64()[::-1])
    assert TILE == 32


def test_ssim_of_an_image_with_itself_is_one():
    x = R.pattern(23, 17, 1)
    for padding in ('same', 'valid'):
        a = R.ssim_ref(x, x, padding)
        assert abs(float(a['value']) - 1.0) < 1e-12 and np.abs(a['grad']).max() < 1e-12
        assert np.abs(a['channels'] - 1.0).max() < 1e-12


def test_same_and_valid_agree_on_the_interior_map():
    _, x, y = R.image_pairs(29, 31, seed=2)[0]
    s, v = R.ssim_ref(x, y, 'same'), R.ssim_ref(x, y, 'valid')
    assert np.abs(s['map'][5:-5, 5:-5] - v['map'][5:-5, 5:-5]).max() < 1e-13
    assert np.count_nonzero(v['map'][:5]) == 0 and np.count_nonzero(v['map'][:, -5:]) == 0
    assert abs(float(v['value']) - v['map'][5:-5, 5:-5].mean()) < 1e-14
    assert abs(float(s['value']) - s['map'].mean()) < 1e-14


def _proto(src, name):
    m = re.search(r'\b(?:int|uint64_t)\s+' + name + r'\s*\(([^)]*)\)\s*;', src)
    assert m, name + ' is not declared in include/nsr.h'
    return [a.strip() for a in m.group(1).split(',')]


def test_header_ctypes_table_and_library_agree(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nsr.h')).read(), flags=re.S)
    for name, nargs in (('nsr_ssim_workspace_bytes', 3), ('nsr_ssim', 16)):
        assert hasattr(so, name), 'libnsr_hip.so does not export ' + name
        declared = _proto(src, name)
        res, args = _lib.SIGNATURES[name]
        assert len(declared) == len(args) == nargs, name
        for a, t in zip(declared, args):
            assert (t is _lib.vp) == ('*' in a or a.startswith('nsr_stream_t')), (name, a)
            assert (t is _lib.u32) == a.startswith('uint32_t') and (t is _lib.f32) == (a.startswith('float ') and '*' not in a), (name, a)
    assert _lib.SIGNATURES['nsr_ssim_workspace_bytes'][0] is _lib.u64 and _lib.SIGNATURES['nsr_ssim'][0] is _lib.i32
    assert _lib.ABI_VERSION == 6 and _lib.lib().nsr_abi_version() == 6


def test_workspace_size(built):
    from nerfstyle_amd import _lib
    from nerfstyle_amd.ssim import TILE
    ws = _lib.lib().nsr_ssim_workspace_bytes
    prev = (0, 0)
    for H, W in ((1, 1), (3, 4), (TILE, TILE), (TILE + 1, TILE), (37, 64), (126, 168), (378, 504), (756, 1008)):
        tiles = -(-H // TILE) * -(-W // TILE)
        no, yes = ws(H, W, 0), ws(H, W, 1)
        assert no == tiles * 3 * 8                                   # one fp64 partial per tile and channel
        assert yes >= no + H * W * 9 * 4 and yes - (no + H * W * 9 * 4) < 8 and no < yes
        assert no % 8 == 0 and yes % 8 == 0
        assert no >= prev[0] and yes > prev[1]
        prev = (no, yes)
    assert ws(0, 5, 1) == 0 and ws(5, 0, 0) == 0


def test_refusals_before_any_device(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    img, tgt, out, ws, grad, smap = (vp(a) for a in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20))   # never dereferenced

    def call(img=img, si=3, pi=16, tgt=tgt, st=3, pt=16, H=12, W=16, valid=0, out=out, smap=None, grad=None, ws=ws):
        return L.nsr_ssim(img, si, pi, tgt, st, pt, H, W, valid, 1.0, None, out, smap, grad, ws, None)

    assert call(H=0) == -1 and call(W=0) == -1
    for s in (0, 1, 2, 5, 8):
        assert call(si=s) == -1 and call(st=s) == -1
    assert call(pi=15) == -1 and call(pt=15) == -1
    assert call(H=10, valid=1) == -1 and call(W=10, pi=10, pt=10, valid=1) == -1 and call(valid=2) == -1
    assert call(img=None) == -1 and call(tgt=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
    # alignment: 4 bytes, 16 for stride 4, 8 for out and the workspace
    assert call(img=vp((1 << 20) + 2)) == -1 and call(tgt=vp((2 << 20) + 1)) == -1
    assert call(img=vp((1 << 20) + 4), si=4) == -1 and call(tgt=vp((2 << 20) + 8), st=4) == -1
    assert call(out=vp((3 << 20) + 4)) == -1 and call(ws=vp((4 << 20) + 4)) == -1
    assert call(grad=vp((5 << 20) + 2)) == -1 and call(smap=vp((6 << 20) + 1)) == -1
    # grad or ssim_map overlapping an input: 12 x 16 pixels of 12 B from 1 MiB reach 1 MiB + 2304
    for off in (0, 12, 2300):
        for base in (1 << 20, 2 << 20):
            assert call(grad=vp(base + off)) == -1 and call(smap=vp(base + off)) == -1
            assert call(grad=vp(base - 2304 + 4 + off)) == -1
    # a pitched stride-4 input reaches further: ((11 * 40 + 15) * 4 + 3) * 4 = 7292 bytes
    assert call(si=4, pi=40, grad=vp((1 << 20) + 7288)) == -1
    assert call(grad=grad, smap=vp((5 << 20) + 1000)) == -1


def test_python_refusals(built):
    from nerfstyle_amd import ssim as S
    x, y = torch.rand(16, 20, 3), torch.rand(16, 20, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ssim(x, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.dssim_loss(x.view(-1, 3), y.view(-1, 3), 16, 20)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.frame_metrics(x, y)
    with pytest.raises(ValueError, match=r'permute\(1, 2, 0\)'):
        S.ssim(torch.rand(3, 16, 20), y)
    with pytest.raises(RuntimeError, match='target'):
        S.ssim(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='padding'):
        S.ssim(x, y, padding='reflect')
    with pytest.raises(ValueError, match='padding'):
        S.dssim_loss(x, y, padding='full')


def test_style_criterion_ssim_lambda_defaults_off():
    import inspect
    from nerfstyle_amd.stylize import StyleCriterion
    assert inspect.signature(StyleCriterion).parameters['ssim_lambda'].default == 0.0
    crit = StyleCriterion(None, None)
    assert crit.ssim_lambda == 0.0 and crit.last_ssim is None
