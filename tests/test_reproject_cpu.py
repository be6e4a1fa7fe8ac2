"""View reprojection without a GPU: the NumPy restatement's own properties (tests/reproject_ref.py), the per-pixel body of the
kernel compiled by the host compiler (csrc/reproject_core.h through tests/reproject_host.cpp) against the restatement on the
analytic scene, and everything nerfstyle_amd/consistency.py decides on the host."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import reproject_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9


@pytest.fixture(scope='module')
def scene():
    return R.make_scene()


@pytest.fixture(scope='module')
def scene_ref(scene):
    return R.reproject_frames(scene['rgb'], scene['dist'], scene['poses'], scene['intr'], R.ALL_PAIRS, scene['camera_flip'], 0.01)


def test_scene_has_margins_and_every_outcome(scene, scene_ref):
    """what lets a mask be compared exactly: no pixel that reaches a threshold of steps 3 to 5 lies within 1e-9 relative of it
    (z against 0 relative to the distance, u / w against the frame relative to its size, |r - tbar| against depth_tol r relative
    to r), and every outcome occurs"""
    res = scene_ref[3]
    for pair, r in zip(R.ALL_PAIRS, res):
        for name, m in r['margin'].items():
            assert m > MARGIN, (pair, name, m)
    seen = np.unique(np.concatenate([r['outcome'] for r in res[:len(R.SCENE_PAIRS)]]))
    assert sorted(seen.tolist()) == sorted(R.OUTCOMES), [R.OUTCOMES[c] for c in seen]
    assert np.isnan(scene['dist']).sum() == 1 and (scene['dist'] == -1.0).sum() == 1
    # the views agree where they see the same surface: the error of the valid pixels is the bilinear interpolation's
    rmse = R.warp_error(scene_ref[2], scene['intr'][5], scene['intr'][4])[:, 0]
    assert np.nanmax(rmse) < 0.02


def test_identical_camera_pair(scene):
    """(a, a): a pixel lands on itself, so inside the frame's outer ring the mask is "has a surface" and nothing is lost"""
    full = R.make_scene(holes=False)
    W, H = full['intr'][4], full['intr'][5]
    for a in range(4):
        r = R.reproject_pair(full['rgb'], full['dist'], full['poses'], full['intr'], a, a, full['camera_flip'], 0.01)
        inner = np.zeros((H, W), bool)
        inner[1:-1, 1:-1] = True
        surf = R.has_surface(full['dist'][a]).reshape(H, W)
        assert surf[inner].all()
        assert np.array_equal(r['mask'].reshape(H, W)[inner].astype(bool), surf[inner])
        assert R.warp_error([[r['sse'], r['n_valid']]], H, W)[0, 0] < 1e-6
    # with holes: a pixel without a surface is never valid, one with a surface on all of its 3 x 3 neighbourhood always is
    r = R.reproject_pair(scene['rgb'], scene['dist'], scene['poses'], scene['intr'], 0, 0, scene['camera_flip'], 0.01)
    surf = R.has_surface(scene['dist'][0]).reshape(H, W)
    mask = r['mask'].reshape(H, W).astype(bool)
    assert not mask[~surf].any()
    solid = np.zeros_like(surf)
    solid[1:-1, 1:-1] = np.logical_and.reduce([surf[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    assert solid.sum() > 400 and mask[solid].all()
    assert R.warp_error([[r['sse'], r['n_valid']]], H, W)[0, 0] < 1e-6


def test_one_pixel_translation_shifts_by_a_column():
    """identity rotations, no flip, a fronto-parallel plane at depth Z: moving the src camera by Z / fx along x moves every
    point by exactly one column"""
    W, H, fx, fy, Z = 16, 9, 20.0, 24.0, 5.0
    intr = (fx, fy, 8.0, 4.5, W, H)
    poses = np.zeros((2, 3, 4), np.float32)
    poses[:, :, :3] = np.eye(3)
    poses[1, 0, 3] = Z / fx
    d, _ = R.pixel_dirs(poses[0], intr, 0)
    dist = np.tile((Z / d[2]).astype(np.float32), (2, 1))
    rgb = np.random.default_rng(3).random((2, H * W, 3)).astype(np.float32)
    r = R.reproject_pair(rgb, dist, poses, intr, 0, 1, 0, 0.01)
    mask, warped = r['mask'].reshape(H, W), r['warped'].reshape(H, W, 3)
    assert mask[:, 2:].all() and not mask[:, 0].any()
    assert np.allclose(warped[:, 2:], rgb[1].reshape(H, W, 3)[:, 1:-1], rtol=0, atol=1e-7)
    # and the other way round the image moves to the left
    r = R.reproject_pair(rgb, dist, poses, intr, 1, 0, 0, 0.01)
    assert np.allclose(r['warped'].reshape(H, W, 3)[:, :-2], rgb[0].reshape(H, W, 3)[:, 1:-1], rtol=0, atol=1e-7)


def test_core_header_on_the_host_matches_the_restatement(scene, scene_ref, tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'reproject_host')
    subprocess.run([cxx, '-O2', '-std=c++17', '-ffp-contract=off', os.path.join(ROOT, 'tests', 'reproject_host.cpp'), '-o', exe], check=True)
    fx, fy, cx, cy, W, H = scene['intr']
    pairs = np.asarray(R.ALL_PAIRS + [(7, 0)], np.int32)           # the last names a frame that does not exist: skipped
    F, P, HW = scene['poses'].shape[0], pairs.shape[0], H * W
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(src, 'wb') as f:
        f.write(np.asarray([F, H, W, P], np.uint32).tobytes() + np.asarray([scene['camera_flip']], np.int32).tobytes() +
                np.asarray([fx, fy, cx, cy], np.float32).tobytes() + np.asarray([0.01], np.float64).tobytes() +
                scene['poses'].tobytes() + scene['dist'].tobytes() + scene['rgb'].tobytes() + pairs.tobytes())
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    raw = open(dst, 'rb').read()
    mask = np.frombuffer(raw, np.uint8, P * HW).reshape(P, HW)
    warped = np.frombuffer(raw, np.float32, P * HW * 3, offset=P * HW).reshape(P, HW, 3)
    stats = np.frombuffer(raw, np.float64, P * 2, offset=P * HW * 13).reshape(P, 2)
    want_w, want_m, want_s, res = scene_ref
    assert np.array_equal(mask[:-1], want_m)
    assert np.abs(warped[:-1].astype(np.float64) - want_w.astype(np.float64)).max() <= 2.0 ** -23
    assert np.array_equal(stats[:-1, 1], want_s[:, 1])
    for i, rr in enumerate(res):
        assert abs(stats[i, 0] - rr['sse']) <= R.sse_tolerance(rr, scene['intr']), (i, stats[i, 0], rr['sse'])
    assert not mask[-1].any() and not warped[-1].any() and not stats[-1].any()


# ---- what consistency.py decides on the host -------------------------------------------------------------------------------
def _frames(F=3, H=4, W=5):
    from nerfstyle_amd.common import Intrinsics
    return (torch.zeros(F, H * W, 3), torch.ones(F, H * W), torch.zeros(F, 3, 4), Intrinsics(H, W, 10.0, 10.0, W / 2, H / 2))


def test_sequence_pairs():
    from nerfstyle_amd.consistency import sequence_pairs
    assert sequence_pairs(4, 1) == [(0, 1), (1, 2), (2, 3)]
    assert sequence_pairs(9, 7) == [(0, 7), (1, 8)]
    assert sequence_pairs(3, 3) == [] and sequence_pairs(3, 5) == []
    for F, gap in ((0, 1), (4, 0), (4, -1)):
        with pytest.raises(ValueError):
            sequence_pairs(F, gap)


def test_reproject_frames_refuses_bad_arguments_on_the_host():
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.consistency import reproject_frames
    rgb, dist, poses, intr = _frames()
    for pairs in ([(0, 3)], [(-1, 0)], [(0, 1, 2)], torch.tensor([[0, 5]]), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int64),
                  torch.zeros(1, 2), [(0.5, 1)]):
        with pytest.raises(ValueError, match='pairs'):
            reproject_frames(rgb, dist, poses, intr, pairs)
    with pytest.raises(ValueError, match='rgb'):
        reproject_frames(rgb[:, :-1], dist, poses, intr, [(0, 1)])
    with pytest.raises(ValueError, match='dist'):
        reproject_frames(rgb, dist[:2], poses, intr, [(0, 1)])
    with pytest.raises(ValueError, match='poses'):
        reproject_frames(rgb, dist, poses[:, :, :3], intr, [(0, 1)])
    with pytest.raises(ValueError, match='float32'):
        reproject_frames(rgb.double(), dist, poses, intr, [(0, 1)])
    with pytest.raises(ValueError, match='float32'):
        reproject_frames(rgb, dist.half(), poses, intr, [(0, 1)])
    with pytest.raises(ValueError, match='contiguous'):
        reproject_frames(torch.zeros(3, 3, 20).permute(0, 2, 1), dist, poses, intr, [(0, 1)])
    with pytest.raises(ValueError, match='W >= 2'):
        reproject_frames(torch.zeros(3, 4, 3), torch.ones(3, 4), poses, Intrinsics(4, 1, 10.0, 10.0, 0.5, 2.0), [(0, 1)])
    with pytest.raises(ValueError, match='H >= 2'):
        reproject_frames(torch.zeros(3, 4, 3), torch.ones(3, 4), poses, Intrinsics(1, 4, 10.0, 10.0, 2.0, 0.5), [(0, 1)])
    with pytest.raises(ValueError, match='depth_tol'):
        reproject_frames(rgb, dist, poses, intr, [(0, 1)], depth_tol=-0.1)
    # the [F, H, W, 3] / [F, H, W] forms pass the shape checks; with everything in order a CPU tensor meets "no CPU fallback"
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        reproject_frames(rgb.view(3, 4, 5, 3), dist.view(3, 4, 5), poses, intr, [(0, 1), (2, 2)])


def test_c_abi_refuses_before_any_launch():
    from nerfstyle_amd import build, _lib
    build.build()
    lib = _lib.lib()
    assert lib.nsr_reproject_frames_workspace_bytes(5, 23, 37) == 5 * 4 * 16          # ceil(851 / 256) = 4 slots of two doubles
    assert lib.nsr_reproject_frames_workspace_bytes(2, 756, 1008) == 2 * 2977 * 16
    assert lib.nsr_reproject_frames_workspace_bytes(1, 1, 37) == 0 and lib.nsr_reproject_frames_workspace_bytes(1, 23, 1) == 0
    assert lib.nsr_reproject_frames_workspace_bytes(1, 1 << 16, 1 << 15) == 0
    call = lib.nsr_reproject_frames
    assert call(None, None, None, 2, 23, 37, 30.0, 30.0, 18.0, 11.0, 0, None, 1, 0.01, None, None, None, None, None) == -1
    assert call(None, None, None, 2, 23, 1, 30.0, 30.0, 18.0, 11.0, 0, None, 1, 0.01, None, None, None, None, None) == -1
    assert call(None, None, None, 2, 23, 37, 30.0, 30.0, 18.0, 11.0, 0, None, 0, 0.01, None, None, None, None, None) == 0   # P = 0


def test_warp_error_on_hand_made_stats():
    from nerfstyle_amd.consistency import warp_error
    stats = torch.tensor([[3.0, 4.0], [0.0, 10.0], [0.0, 0.0], [0.75, 1.0]], dtype=torch.float64)
    out = warp_error(stats, 4, 5)
    assert out.dtype == torch.float64 and tuple(out.shape) == (4, 2)
    assert out[0, 0].item() == 0.5 and out[0, 1].item() == 0.2
    assert out[1, 0].item() == 0.0 and out[1, 1].item() == 0.5
    assert torch.isnan(out[2, 0]) and out[2, 1].item() == 0.0
    assert out[3, 0].item() == 0.5 and out[3, 1].item() == 0.05
    assert np.allclose(out.numpy(), R.warp_error(stats.numpy(), 4, 5), equal_nan=True, rtol=0, atol=0)
    with pytest.raises(ValueError):
        warp_error(torch.zeros(3), 4, 5)
