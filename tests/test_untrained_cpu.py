"""Untrained cells without a GPU: the entry point is declared, exported and bound with the same argument count; the NumPy
restatement of the frustum test (untrained_ref.py) is conservative against brute force and behaves on hand-made cameras; the host
layer refuses what it must and computes the frustum it documents."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import untrained_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAME = 'nsr_occ_mark_untrained'


def test_symbol_and_signatures():
    from nerfstyle_amd import _lib, build
    assert hasattr(ctypes.CDLL(build.build()), NAME), 'libnsr_hip.so does not export ' + NAME
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nsr.h')).read(), flags=re.S)
    proto = re.search(r'\bint\s+' + NAME + r'\s*\(([^)]*)\)\s*;', src)
    assert proto, NAME + ' is not declared in include/nsr.h'
    declared = [a.strip() for a in proto.group(1).split(',')]
    res, args = _lib.SIGNATURES[NAME]
    assert res is _lib.i32 and len(args) == len(declared) == 17
    # doubles where the header says double, pointers where it has a *
    for a, t in zip(declared, args):
        assert (t is _lib.f64) == a.startswith('double') and (t is _lib.vp) == ('*' in a or a.startswith('nsr_stream_t')), a
    assert _lib.ABI_VERSION == 6
    L = _lib.lib()
    # refused before anything touches a device
    assert L.nsr_occ_mark_untrained(None, None, 1, 8, 1.0, None, 1, -1.0, 1.0, -1.0, 1.0, 0, 1.0, 1, None, None, None) == -1


# ---- cameras ---------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """[3,4] fp32 pose whose camera-frame +z (camera_flip = 0) points from eye to target"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), eye[:, None]], 1).astype(F32)


W, H_PIX, FOCAL = 48, 36, 40.0
CAM = (FOCAL, FOCAL, W / 2.0, H_PIX / 2.0)
THREE = np.stack([look_at((0.3, 0.2, -3.0), (0.0, 0.0, 0.0)), look_at((2.5, 0.5, 1.0), (0.2, -0.3, 0.0)),
                  look_at((-0.4, 0.3, 0.5), (1.0, 1.0, -1.0))])          # two outside the box, one inside it


def _points_in_frusta(poses, n, rng, depth_max=7.0):
    """n points per camera, uniform in pixel coordinates over [0,w] x [0,h] and in depth, fp64"""
    pts = []
    for P in np.asarray(poses, F32).astype(np.float64):
        u, v, depth = rng.random(n) * W, rng.random(n) * H_PIX, rng.random(n) * depth_max
        c = np.stack([(u - CAM[2]) / CAM[0], (v - CAM[3]) / CAM[1], np.ones(n)], 1)
        pts.append(P[:, 3] + (c * depth[:, None]) @ P[:, :3].T)
    return np.concatenate(pts)


def _cells_fp64(xyz, C, H, bound):
    """the march's cell formula (rm_probe.h: level >= the point's own mip level, n = clamp((x / b + 1) H / 2)) evaluated in fp64:
    the cells that CONTAIN the exact point"""
    _, e = np.frexp(np.abs(xyz).max(1))
    m1 = np.clip(e, 0, C - 1)
    out = []
    for level in range(C):
        p = xyz[m1 <= level]
        b = min(2.0 ** level, float(bound))
        n = np.clip(np.floor((p / b + 1) * (0.5 * H)), 0, H - 1).astype(np.int64)
        out.append(level * H ** 3 + U.morton(n[:, 0], n[:, 1], n[:, 2]).astype(np.int64))
    return np.concatenate(out)


def test_restatement_is_conservative_against_brute_force():
    """H = 16, C = 2, three cameras, 200 000 points inside the frusta.  margin_cells = 1 is the claim of include/nsr.h for exact
    positions: no cell that contains such a point is unseen.  The default margin is the claim for the march's own fp32 index."""
    H, C, bound = 16, 2, 2.0
    rng = np.random.default_rng(0)
    frustum = U.pinhole_frustum(W, H_PIX, *CAM)
    pts = _points_in_frusta(THREE, 200000 // 3 + 1, rng)
    inside = pts[np.abs(pts).max(1) <= bound]
    assert inside.shape[0] > 50000
    cnt = U.counts(C, H, bound, THREE, frustum, 0, 1.0)
    hit = np.unique(_cells_fp64(inside, C, H, bound))
    assert hit.size > 500 and (cnt[hit] > 0).all()
    assert 0 < (cnt == 0).sum() < cnt.size
    cnt15 = U.counts(C, H, bound, THREE, frustum, 0, 1.5)
    hit32 = np.unique(U.march_cells(inside.astype(F32), C, H, bound))
    assert (cnt15[hit32] > 0).all() and (cnt15 >= cnt).all()
    # per camera too: a point of camera k's frustum is in a cell that camera k sees
    for k in range(3):
        own = _points_in_frusta(THREE[k:k + 1], 20000, rng)
        own = own[np.abs(own).max(1) <= bound]
        assert (U.counts(C, H, bound, THREE[k:k + 1], frustum, 0, 1.0)[np.unique(_cells_fp64(own, C, H, bound))] == 1).all()


def test_narrow_camera_on_the_axis():
    H, C, bound = 16, 2, 2.0
    pose = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -4.0]]], F32)            # at (0, 0, -4), looking along +z
    frustum = U.pinhole_frustum(32, 32, 160.0, 160.0, 16.0, 16.0)                   # +-0.1
    assert frustum == (-0.1, 0.1, -0.1, 0.1)
    grid = np.zeros(C * H ** 3, F32)
    cnt, g, bits, n_un = U.mark(grid, np.full(C * H ** 3 // 8, 0xFF, np.uint8), C, H, bound, pose, frustum, 0, 1.0, 1)
    iz = np.arange(H, dtype=np.uint32)
    for cas in range(C):
        for a in (7, 8):
            for b in (7, 8):
                assert (cnt[cas * H ** 3 + U.morton(np.full(H, a), np.full(H, b), iz)] == 1).all()
        for a in (0, H - 1):
            for b in (0, H - 1):
                col = cas * H ** 3 + U.morton(np.full(H, a), np.full(H, b), iz).astype(np.int64)
                assert (cnt[col] == 0).all() and (g[col] == -1).all()
                assert not (bits[col // 8] >> (col % 8) & 1).any()
    share = n_un.astype(np.float64) / H ** 3
    assert ((share > 0) & (share < 1)).all() and n_un.sum() == (g == -1).sum()
    seen = cnt > 0
    assert (g[seen] == 0).all() and np.array_equal(np.unpackbits(bits, bitorder='little').astype(bool), seen)


def test_camera_looking_away_marks_everything():
    H, C, bound = 16, 2, 2.0
    pose = np.array([[[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, -4.0]]], F32)          # at (0, 0, -4), looking along -z
    grid = np.random.default_rng(1).random(C * H ** 3).astype(F32)
    cnt, g, bits, n_un = U.mark(grid, np.full(C * H ** 3 // 8, 0xFF, np.uint8), C, H, bound, pose, (-0.5, 0.5, -0.5, 0.5), 0, 2.5, 1)
    assert not cnt.any() and (g == -1).all() and not bits.any() and (n_un == H ** 3).all()
    # the same pose with the z flip looks at the box
    assert U.counts(C, H, bound, pose, (-0.5, 0.5, -0.5, 0.5), 1, 1.0).any()


@pytest.mark.parametrize('camera_flip', range(8))
def test_flip_with_matching_pose_columns(camera_flip):
    """negating column k of R together with flip bit k leaves every ray, and so every count, unchanged; the principal point is
    off the centre, so that the flip alone does change them"""
    H, C, bound = 16, 2, 2.0
    frustum = U.pinhole_frustum(W, H_PIX, 40.0, 38.0, 17.5, 23.25)
    flipped = THREE.copy()
    flipped[:, :, :3] *= np.asarray(U.flips(camera_flip), F32)
    base = U.counts(C, H, bound, THREE, frustum, 0, 1.0)
    assert np.array_equal(U.counts(C, H, bound, flipped, frustum, camera_flip, 1.0), base)
    if camera_flip:
        assert not np.array_equal(U.counts(C, H, bound, THREE, frustum, camera_flip, 1.0), base)


# ---- host layer ------------------------------------------------------------------------------------------------------------------
def _renderer(use_ndc=False):
    from nerfstyle_amd.common import BBox, Intrinsics
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.style_nerf import StyleTCNerf
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 2, use_dir=False)
    cfg = RendererConfig.llff()
    cfg.grid_size, cfg.use_ndc = 16, use_ndc
    return Renderer(m, cfg, Intrinsics(H_PIX, W, *CAM), 2.0, raymarch_channels=5)


def test_use_ndc_raises():
    with pytest.raises(NotImplementedError, match='mark_untrained_grid: use_ndc'):
        _renderer(use_ndc=True).mark_untrained_grid(THREE)


def test_cpu_grid_raises():
    from nerfstyle_amd import raymarching
    r = _renderer()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        r.mark_untrained_grid(THREE)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        raymarching.mark_untrained_grid(r.density_grid, r.density_bitfield, torch.tensor(THREE), (-1, 1, -1, 1), 0, 2.0, 2, 16, 1.5, 1)
    assert not r.density_grid.any() and not r.density_bitfield.any()


def test_lens_frustum():
    from nerfstyle_amd.rays import frustum_bounds
    cam = (383.8, 380.1, 250.7, 190.2)
    pin = frustum_bounds(504, 378, *cam)
    assert pin == U.pinhole_frustum(504, 378, *cam)
    assert pin == ((0 - 250.7) / 383.8, (504 - 250.7) / 383.8, (0 - 190.2) / 380.1, (378 - 190.2) / 380.1)
    assert frustum_bounds(504, 378, *cam, 0.0, 0.0) == pin                                  # k1 = k2 = 0: exactly the pinhole one
    for k1, k2 in ((0.05, 0.0), (0.08, 0.01), (-0.08, 0.02)):
        got = frustum_bounds(504, 378, *cam, k1, k2)
        assert got == U.lens_frustum(504, 378, cam + (k1, k2))
        assert got[0] < got[1] and got[2] < got[3]
        if k1 > 0:
            assert got[0] < pin[0] and got[1] > pin[1] and got[2] < pin[2] and got[3] > pin[3]     # contains the pinhole one
    # barrel distortion: the extreme of an edge is near its middle, not at a corner
    x = (504 - 250.7) / 383.8
    assert frustum_bounds(504, 378, *cam, -0.08, 0.0)[1] > x * (1 + (x * x + ((378 - 190.2) / 380.1) ** 2) * -0.08)
