"""Host side of the per-ray geometry terms (nsr_ray_geometry_forward / _backward, raymarching.ray_geometry,
Renderer.geometry_terms): the closed-form backward the kernel implements equals autograd on the definitions in fp64, the
entry points are declared, exported, bound and check their arguments before anything touches a device, the renderer switch
is opt-in, and CPU tensors are refused."""
import ctypes

import numpy as np
import pytest
import torch

import ray_geometry_ref as G


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


@pytest.mark.parametrize('is_ndc', [False, True])
def test_closed_form_equals_autograd_in_fp64(is_ndc):
    """helpers.edge_rays(3, is_ndc, replicas=1): outputs and the three gradients to 1e-10 of the largest reference entry.
    The serial-fp32 evaluation of the same formula is printed beside it: what the number format alone costs."""
    c = G.geometry_case(is_ndc, replicas=1)
    args = (c['sig'], c['deltas'], c['rays'], c['nears'], c['fars'], c['T_thresh'], is_ndc)
    assert (c['depth'][c['valid']] > 0).sum() >= 5 and (c['depth'][c['valid']] == 0).sum() >= 5       # both sides of the clamp
    assert c['dist'][c['valid']].min() > 0
    for which in G.UPSTREAM:
        gd, gx = G.upstream(c, which)
        depth, dist, grad = G.closed_form(*args, gd, gx, np.float64)
        ref = c['grads'][which]
        scale = np.abs(ref).max()
        assert scale > 0
        err = np.abs(grad - ref).max() / scale
        _, _, g32 = G.closed_form(*args, gd, gx, np.float32)
        print(is_ndc, which, 'max|ref|', scale, 'fp64 closed form', err, 'serial fp32', np.abs(g32 - ref).max() / scale)
        assert err <= 1e-10
        assert np.abs(depth - c['depth']).max() <= 1e-10 * np.abs(c['depth']).max()
        assert np.abs(dist - c['dist']).max() <= 1e-10 * np.abs(c['dist']).max()
        assert np.array_equal(grad == 0, ref == 0)                 # live samples, the stopping one included, and nothing else
    # the ray without a range, the empty ray and the dropped one
    rays = c['rays']
    for row in (c['miss'], int(np.nonzero(rays[:, 2] == 0)[0][0]), len(rays) - 1):
        assert c['depth'][rays[row, 0]] == 0 and c['dist'][rays[row, 0]] == 0
        assert (c['grads']['both'][rays[row, 1]:rays[row, 1] + rays[row, 2]] == 0).all()


@pytest.mark.parametrize('is_ndc', [False, True])
def test_serial_fp32_meets_the_gpu_bars(is_ndc):
    """The bars of tests/test_gpu_ray_geometry.py are not measured on the kernel: the formula evaluated serially in fp32 on
    the GPU test's inputs must meet each of them with the factor 4 left for the reassociation of the wave scans."""
    c = G.geometry_case(is_ndc)
    args = (c['sig'], c['deltas'], c['rays'], c['nears'], c['fars'], c['T_thresh'], is_ndc)
    for which in G.UPSTREAM:
        gd, gx = G.upstream(c, which)
        depth, dist, grad = G.closed_form(*args, gd, gx, np.float32)
        ref = c['grads'][which]
        e_grad = np.abs(grad - ref).max() / np.abs(ref).max()
        e_depth, e_dist = np.abs(depth - c['depth']).max(), np.abs(dist - c['dist']).max()
        print(is_ndc, which, 'serial fp32: grad', e_grad, 'depth', e_depth, 'distortion', e_dist)
        assert 4 * e_grad <= 1e-4 and 4 * e_depth <= 2e-4 and 4 * e_dist <= 2e-5 * max(1.0, np.abs(c['dist']).max())


def test_entry_points_are_declared_exported_and_bound(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    assert hasattr(so, 'nsr_ray_geometry_forward') and hasattr(so, 'nsr_ray_geometry_backward')
    res, args = _lib.SIGNATURES['nsr_ray_geometry_forward']
    assert res is _lib.i32 and len(args) == 13 and args[5:9] == [_lib.u32, _lib.u32, _lib.f32, _lib.i32]
    res, args = _lib.SIGNATURES['nsr_ray_geometry_backward']
    assert res is _lib.i32 and len(args) == 14 and args[8:12] == [_lib.u32, _lib.u32, _lib.f32, _lib.i32]
    assert _lib.lib().nsr_abi_version() == _lib.ABI_VERSION


def _fwd(L, ptrs, N=8):
    return L.nsr_ray_geometry_forward(*ptrs[:5], 64, N, 1e-4, 0, *ptrs[5:], None)


def _bwd(L, ptrs, N=8):
    return L.nsr_ray_geometry_backward(*ptrs[:8], 64, N, 1e-4, 0, ptrs[8], None)


def test_argument_checks_answer_on_the_host(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    # empty work is a no-op success, whatever else is passed
    assert _fwd(L, [None] * 8, N=0) == 0 and _bwd(L, [None] * 9, N=0) == 0
    # every required pointer, one at a time
    for k in range(8):
        assert _fwd(L, [None if j == k else fake for j in range(8)]) == -1, k
    for k in range(2, 9):
        assert _bwd(L, [None if j == k else fake for j in range(9)]) == -1, k
    # deltas rows are read as 8-byte pairs
    assert _fwd(L, [fake, ctypes.c_void_p(4100)] + [fake] * 6) == -1
    assert _bwd(L, [fake, fake, fake, ctypes.c_void_p(4100)] + [fake] * 5) == -1


def test_geometry_terms_is_opt_in():
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    from nerfstyle_amd.style_nerf import StyleTCNerf
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False)
    _, intr, _ = load_room_cameras()
    r = Renderer(m, RendererConfig.llff(), intr, 2.0, raymarch_channels=8)
    assert r.geometry_terms is False


def test_no_cpu_fallback(built):
    from nerfstyle_amd import raymarching
    c = G.geometry_case(False, replicas=1)
    t = [torch.tensor(np.array(c[k])) for k in ('sig', 'deltas', 'rays', 'nears', 'fars')]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        raymarching.ray_geometry(*t, c['T_thresh'])
