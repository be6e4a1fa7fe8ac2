"""Host side of the streaming inference render (nsr_render_rays_infer / Renderer.render_test_fused): the entry point is
declared, exported and bound, its argument checks answer before anything touches a device, and the host layer is opt-in and has
no CPU fallback."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def _desc(nc=5):
    from nerfstyle_amd import _lib
    offsets = (np.arange(17, dtype=np.int32) * 4096).copy()
    d = _lib.FieldDesc()
    d.L, d.H, d.S, d.num_classes = 16, 16, 0.5, nc
    d.table_dtype, d.compute_dtype = _lib.NSR_F16, _lib.NSR_F16
    for i in range(3):
        d.bbox_min[i], d.bbox_size[i] = -2.0, 4.0
    d.density_scale = 1.0
    d.offsets = offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return d, offsets


def _call(L, desc, ptr, N, is_ndc=0, C=2, stats=None):
    return L.nsr_render_rays_infer(desc, ptr, ptr, ptr, ptr, None, N, ptr, ptr, ptr, 2.0, 0.0, 1024, is_ndc, C, 128, 1e-4,
                                   ptr, ptr, ptr, stats, None)


def test_entry_point_is_declared_exported_and_bound(built):
    from nerfstyle_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'nsr.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'\bint\s+nsr_render_rays_infer\s*\(', src)
    assert hasattr(ctypes.CDLL(built), 'nsr_render_rays_infer')
    assert 'nsr_render_rays_infer' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['nsr_render_rays_infer'][1]) == 22
    L = _lib.lib()
    assert L.nsr_abi_version() == _lib.ABI_VERSION


def test_argument_checks_answer_on_the_host(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    # all-NULL pointers -> NSR_ERR_INVALID_ARG
    assert _call(L, None, None, 8) == -1
    # empty work is a no-op success, whatever else is passed
    assert _call(L, None, None, 0) == 0
    assert _call(L, None, None, 0, is_ndc=1, C=17) == 0
    # NDC and more than 16 cascades are not built: NSR_ERR_UNSUPPORTED, before the pointers are looked at
    assert _call(L, None, None, 8, is_ndc=1) == -2
    assert _call(L, None, None, 8, C=17) == -2
    # every pointer given (never dereferenced: the calls below return before a launch)
    fake = ctypes.c_void_p(4096)
    desc, keep = _desc(nc=14)
    assert _call(L, ctypes.byref(desc), fake, 8) == -2          # class rows 3..15 of one output tile: nc <= 13
    desc, keep = _desc(nc=5)
    assert _call(L, ctypes.byref(desc), fake, 8, is_ndc=1) == -2
    assert _call(L, ctypes.byref(desc), fake, 8, C=17) == -2
    assert _call(L, ctypes.byref(desc), fake, 8, C=0) == -1
    assert _call(L, ctypes.byref(desc), ctypes.c_void_p(4100), 8) == -1    # tables: 16-byte rows


def _cpu_renderer():
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    from nerfstyle_amd.style_nerf import StyleTCNerf
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False)
    _, intr, _ = load_room_cameras()
    return Renderer(m, RendererConfig.llff(), intr, 2.0, raymarch_channels=8)


def test_fused_inference_is_opt_in(built):
    r = _cpu_renderer()
    assert r.fused_inference is False
    assert r.last_infer_stats() is None


def test_render_test_fused_has_no_cpu_fallback(built):
    from nerfstyle_amd.common import RayBatch
    r = _cpu_renderer()
    rays = RayBatch.__new__(RayBatch)
    rays.origins = torch.zeros(4, 3)
    rays.dirs = torch.tensor([[0., 0., 1.]]).repeat(4, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        r.render_test_fused(rays)
    r.fused_inference = True
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        r.render_test(rays)
