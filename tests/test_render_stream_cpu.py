"""Host side of the streaming render with a choice of composite (nsr_render_rays_stream / Renderer.render_train_fused): the entry
point is declared, exported and bound, its argument checks answer before anything touches a device, and the host layer is opt-in
and leaves every call with autograd on, or of an NDC scene, to the existing render_train."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFER, TRAIN = 0, 1


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


def _call(L, desc, ptr, N, composite=TRAIN, C=2, rgb_map=None, depth_norm=None, classes=None, counts=None, stats=None):
    return L.nsr_render_rays_stream(desc, ptr, ptr, ptr, ptr, None, N, ptr, ptr, ptr, 2.0, 0.0, 1024, C, 128, 1e-4, composite,
                                    ptr, ptr, ptr, rgb_map, depth_norm, classes, counts, stats, None)


def _header_params(src, name):
    """The parameter list of `name` as include/nsr.h declares it, comments removed."""
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
    assert m, name
    return [' '.join(p.split()) for p in m.group(1).split(',')]


def test_entry_point_is_declared_exported_and_bound(built):
    from nerfstyle_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'nsr.h')).read()
    params = _header_params(src, 'nsr_render_rays_stream')
    res, args = _lib.SIGNATURES['nsr_render_rays_stream']
    print(len(params), 'parameters')
    assert res is _lib.i32 and len(args) == len(params) == 26
    # the ctypes table matches the header, parameter by parameter
    for decl, ct in zip(params, args):
        if decl.startswith('const nsr_field_desc *'):
            want = ctypes.POINTER(_lib.FieldDesc)
        elif '*' in decl or decl.startswith('nsr_stream_t'):
            want = _lib.vp
        elif decl.startswith('uint32_t'):
            want = _lib.u32
        elif decl.startswith('float'):
            want = _lib.f32
        else:
            assert decl.startswith('int '), decl
            want = _lib.i32
        assert ct is want, (decl, ct)
    assert re.search(r'enum\s+nsr_stream_composite\s*\{\s*NSR_STREAM_INFER\s*=\s*0\s*,\s*NSR_STREAM_TRAIN\s*=\s*1\s*\}', src)
    assert (_lib.NSR_STREAM_INFER, _lib.NSR_STREAM_TRAIN) == (0, 1)
    assert hasattr(ctypes.CDLL(built), 'nsr_render_rays_stream')
    # nsr_render_rays_infer keeps its signature
    assert len(_header_params(src, 'nsr_render_rays_infer')) == len(_lib.SIGNATURES['nsr_render_rays_infer'][1]) == 22


def test_abi_versions_agree(built):
    from nerfstyle_amd import _lib
    src = open(os.path.join(ROOT, 'nerfstyle_amd', 'csrc', 'ray_util.hip')).read()
    m = re.search(r'int\s+nsr_abi_version\s*\(\s*void\s*\)\s*\{\s*return\s+(\d+)\s*;', src)
    assert m and int(m.group(1)) == _lib.ABI_VERSION
    assert _lib.lib().nsr_abi_version() == _lib.ABI_VERSION


def test_argument_checks_answer_on_the_host(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    # empty work is a no-op success, whatever else is passed
    assert _call(L, None, None, 0) == 0
    assert _call(L, None, None, 0, composite=7, C=17, classes=fake) == 0
    # all-NULL pointers -> NSR_ERR_INVALID_ARG
    assert _call(L, None, None, 8) == -1
    desc, keep = _desc(nc=5)
    d = ctypes.byref(desc)
    # a composite outside the enum -> NSR_ERR_INVALID_ARG
    for bad in (2, -1, 7):
        assert _call(L, d, fake, 8, composite=bad) == -1
    # more than 16 cascades, more than 13 classes -> NSR_ERR_UNSUPPORTED
    assert _call(L, d, fake, 8, C=17) == -2
    assert _call(L, d, fake, 8, composite=INFER, C=17) == -2
    desc14, keep14 = _desc(nc=14)
    assert _call(L, ctypes.byref(desc14), fake, 8, rgb_map=fake, depth_norm=fake, classes=fake) == -2
    assert _call(L, d, fake, 8, C=0) == -1
    assert _call(L, d, ctypes.c_void_p(4100), 8) == -1          # tables: 16-byte rows
    # the epilogue outputs: all NULL, or rgb_map + depth_norm, and classes exactly when there are class channels
    for composite in (INFER, TRAIN):
        assert _call(L, d, fake, 8, composite=composite, rgb_map=fake) == -1
        assert _call(L, d, fake, 8, composite=composite, depth_norm=fake) == -1
        assert _call(L, d, fake, 8, composite=composite, classes=fake) == -1
        assert _call(L, d, fake, 8, composite=composite, rgb_map=fake, depth_norm=fake) == -1          # nc = 5: classes missing
        assert _call(L, d, fake, 8, composite=composite, rgb_map=fake, classes=fake) == -1
    desc0, keep0 = _desc(nc=0)
    assert _call(L, ctypes.byref(desc0), fake, 8, rgb_map=fake, depth_norm=fake, classes=fake) == -1    # nc = 0: no classes


def _cpu_renderer():
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras
    from nerfstyle_amd.style_nerf import StyleTCNerf
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False)
    _, intr, _ = load_room_cameras()
    return Renderer(m, RendererConfig.llff(), intr, 2.0, raymarch_channels=8)


def _cpu_rays():
    from nerfstyle_amd.common import RayBatch
    rays = RayBatch.__new__(RayBatch)
    rays.origins = torch.zeros(4, 3)
    rays.dirs = torch.tensor([[0., 0., 1.]]).repeat(4, 1)
    return rays


class _Reached(Exception):
    pass


def _trap(r, monkeypatch):
    """render_train_fused raises _Reached; the first step of the existing path raises RuntimeError('existing path')."""
    def fused(*a, **k):
        raise _Reached()

    def march(*a, **k):
        raise RuntimeError('existing path')
    monkeypatch.setattr(r, 'render_train_fused', fused)
    monkeypatch.setattr(r, 'march_train', march)
    r.update_occ = False


def test_fused_nograd_train_is_opt_in(built, monkeypatch):
    r = _cpu_renderer()
    assert r.fused_nograd_train is False
    _trap(r, monkeypatch)
    with torch.no_grad(), pytest.raises(RuntimeError, match='existing path'):
        r.render_train(_cpu_rays())


def test_dispatch_takes_the_fused_path_only_without_grad_and_ndc(built, monkeypatch):
    r = _cpu_renderer()
    r.fused_nograd_train = True
    _trap(r, monkeypatch)
    with torch.no_grad(), pytest.raises(_Reached):
        r.render_train(_cpu_rays())
    # autograd on: the existing path
    with torch.enable_grad(), pytest.raises(RuntimeError, match='existing path'):
        r.render_train(_cpu_rays())
    # NDC: the existing path
    r.cfg.use_ndc = True
    with torch.no_grad(), pytest.raises(RuntimeError, match='existing path'):
        r.render_train(_cpu_rays())
    r.cfg.use_ndc = False
    # fewer composited channels than the model has: the existing path
    r.raymarch_channels = 3
    with torch.no_grad(), pytest.raises(RuntimeError, match='existing path'):
        r.render_train(_cpu_rays())


def test_render_train_fused_has_no_cpu_fallback(built):
    r = _cpu_renderer()
    r.update_occ = False
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        r.render_train_fused(_cpu_rays())
