"""View reprojection on the GPU (nsr_reproject_frames, nerfstyle_amd/consistency.py) against the NumPy restatement
(tests/reproject_ref.py) on the analytic scene, and Renderer.render_rgbd / view_consistency on a small renderer.

Bounds.  mask and n_valid: equal exactly (the scene keeps every pixel 1e-9 away from the thresholds, asserted below).  warped:
2^-23 absolute, one f32 rounding of a value in [0, 1].  sse: reproject_ref.sse_tolerance, which derives its two terms."""
import ctypes

import numpy as np
import pytest
import torch

import reproject_ref as R

pytestmark = pytest.mark.gpu
MARGIN = 1e-9


def _intr(scene):
    from nerfstyle_amd.common import Intrinsics
    fx, fy, cx, cy, W, H = scene['intr']
    return Intrinsics(H, W, fx, fy, cx, cy)


def _dev(scene, dev, frames=None):
    sl = slice(None) if frames is None else slice(0, frames)
    return tuple(torch.tensor(np.ascontiguousarray(scene[k][sl]), device=dev) for k in ('rgb', 'dist', 'poses'))


def _assert_margins(res):
    for r in res:
        for name, m in r['margin'].items():
            assert m > MARGIN, (name, m)


def _compare(scene, pairs, got, want):
    warped, mask, stats = got
    want_w, want_m, want_s, res = want
    _assert_margins(res)
    assert np.array_equal(mask.cpu().numpy(), want_m)
    if warped is not None:
        assert np.abs(warped.cpu().numpy().astype(np.float64) - want_w.astype(np.float64)).max() <= 2.0 ** -23
    stats = stats.cpu().numpy()
    assert np.array_equal(stats[:, 1], want_s[:, 1])
    for i, r in enumerate(res):
        err, tol = abs(stats[i, 0] - r['sse']), R.sse_tolerance(r, scene['intr'])
        print('pair', pairs[i], 'sse', stats[i, 0], 'ref', r['sse'], 'err', err, 'tol', tol)
        assert err <= tol, (pairs[i], stats[i, 0], r['sse'], err, tol)


@pytest.fixture(scope='module')
def scene():
    return R.make_scene()


@pytest.fixture(scope='module')
def scene_ref(scene):
    return R.reproject_frames(scene['rgb'], scene['dist'], scene['poses'], scene['intr'], R.SCENE_PAIRS, scene['camera_flip'], 0.01)


@pytest.fixture(scope='module')
def scene_got(scene, dev):
    from nerfstyle_amd.consistency import reproject_frames
    rgb, dist, poses = _dev(scene, dev)
    return reproject_frames(rgb, dist, poses, _intr(scene), R.SCENE_PAIRS, camera_flip=scene['camera_flip'], depth_tol=0.01)


def test_scene_against_the_restatement(scene, scene_ref, scene_got):
    """37 x 23 (851 pixels: four blocks a pair, the last one partly empty), five pairs: an (a, a) pair, a repeated pair, the
    camera that faces away as dst and as src"""
    seen = np.unique(np.concatenate([r['outcome'] for r in scene_ref[3]]))
    assert sorted(seen.tolist()) == sorted(R.OUTCOMES)
    _compare(scene, R.SCENE_PAIRS, scene_got, scene_ref)
    warped, mask, stats = scene_got
    assert warped.dtype == torch.float32 and mask.dtype == torch.uint8 and stats.dtype == torch.float64
    assert torch.equal(warped[0], warped[2]) and torch.equal(mask[0], mask[2]) and torch.equal(stats[0], stats[2])   # the repeated pair
    assert not warped[mask == 0].any()


def test_accepts_image_shaped_frames(scene, scene_got, dev):
    from nerfstyle_amd.consistency import reproject_frames
    rgb, dist, poses = _dev(scene, dev)
    _, _, W, H = scene['intr'][2:]
    got = reproject_frames(rgb.view(-1, H, W, 3), dist.view(-1, H, W), poses, _intr(scene), torch.tensor(R.SCENE_PAIRS),
                           camera_flip=scene['camera_flip'])
    for g, w in zip(got, scene_got):
        assert torch.equal(g, w)


def test_two_by_two(dev):
    """W = H = 2, P = 1: a fronto-parallel plane, the src camera 0.3 of a pixel to the right and a quarter of a pixel down: one
    dst pixel lands inside the 2 x 2 frame"""
    from nerfstyle_amd.consistency import reproject_frames
    fx, Z = 20.0, 5.0
    intr = (fx, fx, 1.0, 1.0, 2, 2)
    poses = np.zeros((2, 3, 4), np.float32)
    poses[:, :, :3] = np.eye(3)
    poses[1, 0, 3], poses[1, 1, 3] = 0.3 * Z / fx, 0.25 * Z / fx
    d, _ = R.pixel_dirs(poses[0], intr, 0)
    scene = {'rgb': np.random.default_rng(5).random((2, 4, 3)).astype(np.float32), 'dist': np.tile((Z / d[2]).astype(np.float32), (2, 1)),
             'poses': poses, 'intr': intr}
    want = R.reproject_frames(scene['rgb'], scene['dist'], poses, intr, [(0, 1)], 0, 0.01)
    assert want[1].tolist() == [[0, 0, 0, 1]]
    got = reproject_frames(*_dev(scene, dev), _intr(scene), [(0, 1)], camera_flip=0, depth_tol=0.01)
    _compare(scene, [(0, 1)], got, want)


def test_metric_only_gives_the_same_stats(scene, scene_got, dev):
    from nerfstyle_amd.consistency import reproject_frames
    rgb, dist, poses = _dev(scene, dev)
    for ww, wm in ((False, False), (True, False), (False, True)):
        warped, mask, stats = reproject_frames(rgb, dist, poses, _intr(scene), R.SCENE_PAIRS, camera_flip=scene['camera_flip'],
                                               want_warped=ww, want_mask=wm)
        assert (warped is not None) == ww and (mask is not None) == wm
        assert torch.equal(stats, scene_got[2])


def test_two_calls_are_bit_identical(scene, scene_got, dev):
    from nerfstyle_amd.consistency import reproject_frames
    rgb, dist, poses = _dev(scene, dev)
    again = reproject_frames(rgb, dist, poses, _intr(scene), R.SCENE_PAIRS, camera_flip=scene['camera_flip'], depth_tol=0.01)
    for g, w in zip(again, scene_got):
        assert torch.equal(g, w)


def _abi(scene, tensors, pairs_dev, warped, mask, stats, ws):
    """the C entry point itself, every buffer the caller's"""
    from nerfstyle_amd import _lib as L
    fx, fy, cx, cy, W, H = scene['intr']
    rgb, dist, poses = tensors
    return L.lib().nsr_reproject_frames(L.p(rgb), L.p(dist), L.p(poses), rgb.shape[0], H, W, fx, fy, cx, cy, scene['camera_flip'],
                                        L.p(pairs_dev), pairs_dev.shape[0], 0.01, L.p(warped), L.p(mask), L.p(stats), L.p(ws), L.stream())


def _abi_buffers(scene, P, dev):
    from nerfstyle_amd import _lib as L
    W, H = scene['intr'][4], scene['intr'][5]
    nbytes = int(L.lib().nsr_reproject_frames_workspace_bytes(P, H, W))
    assert nbytes == P * -(-H * W // 256) * 16
    return (torch.full((P, H * W, 3), 7.0, device=dev), torch.full((P, H * W), 255, dtype=torch.uint8, device=dev),
            torch.full((P, 2), -1.0, dtype=torch.float64, device=dev), torch.empty(nbytes // 8, dtype=torch.float64, device=dev))


def test_inside_a_captured_graph(scene, scene_got, dev):
    tensors = _dev(scene, dev)
    pairs_dev = torch.tensor(R.SCENE_PAIRS, dtype=torch.int32, device=dev)
    warped, mask, stats, ws = _abi_buffers(scene, len(R.SCENE_PAIRS), dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _abi(scene, tensors, pairs_dev, warped, mask, stats, ws) == 0        # warm-up: the code object is loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _abi(scene, tensors, pairs_dev, warped, mask, stats, ws) == 0
    for _ in range(2):
        warped.fill_(7.0); mask.fill_(255); stats.fill_(-1.0); ws.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip((warped, mask, stats), scene_got):
            assert torch.equal(g, w)


def test_pair_out_of_range_at_the_c_abi(scene, scene_got, dev):
    """the host check of reproject_frames bypassed: the entry point skips a pair that names a frame outside [0, F)"""
    tensors = _dev(scene, dev)
    pairs = [(0, 1), (5, 0), (0, -1), (2, 2), (1 << 30, 1)]
    pairs_dev = torch.tensor(pairs, dtype=torch.int32, device=dev)
    warped, mask, stats, ws = _abi_buffers(scene, len(pairs), dev)
    assert _abi(scene, tensors, pairs_dev, warped, mask, stats, ws) == 0
    torch.cuda.synchronize()
    for i in (1, 2, 4):
        assert stats[i].tolist() == [0.0, 0.0] and not mask[i].any() and not warped[i].any()
    for i, j in ((0, 0), (3, 1)):
        assert torch.equal(stats[i], scene_got[2][j]) and torch.equal(mask[i], scene_got[1][j]) and torch.equal(warped[i], scene_got[0][j])


def test_full_size_frames(dev):
    """1008 x 756, two frames, both directions: 2977 slots a pair through the final kernel, rows of warped past 2^21 pixels"""
    from nerfstyle_amd.consistency import reproject_frames
    scene = R.make_scene(1008, 756)
    scene = dict(scene, rgb=scene['rgb'][:2], dist=scene['dist'][:2], poses=scene['poses'][:2])
    pairs = [(0, 1), (1, 0)]
    want = R.reproject_frames(scene['rgb'], scene['dist'], scene['poses'], scene['intr'], pairs, scene['camera_flip'], 0.01)
    assert min(r['n_valid'] for r in want[3]) > 600000
    got = reproject_frames(*_dev(scene, dev), _intr(scene), pairs, camera_flip=scene['camera_flip'], depth_tol=0.01)
    _compare(scene, pairs, got, want)


# ---- the renderer's side ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_renderer(dev):
    """the small renderer of the GPU render tests: the seeded field with its last layers spread, an analytic occupancy grid, a
    64 x 48 frame of the room cameras"""
    from nerfstyle_amd import raymarching
    from nerfstyle_amd.common import BBox, Intrinsics
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras, synthetic_density_grid
    from nerfstyle_amd.style_nerf import StyleTCNerf
    from oracle import torch_port as TP
    nc = 5
    ref = TP.Field(num_classes=nc, table_scale=0.5)
    with torch.no_grad():
        ref.p_density[2048:] *= 16.0
        ref.p_color2[-1024:] *= 16.0
        ref.p_class[2048:] *= 16.0
    model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), nc, enc_dtype=torch.float32, use_dir=False)
    sd = model.state_dict()
    sd.update({'x_density_embedder.embeddings': ref.emb_density.detach(), 'x_color_embedder.embeddings': ref.emb_color.detach(),
               'density_net.params': ref.p_density.detach(), 'color1_net.params': ref.p_color1.detach(),
               'color2_net.params': ref.p_color2.detach(), 'class_net.params': ref.p_class.detach()})
    model.load_state_dict(sd)
    poses, intr, _ = load_room_cameras()
    cfg = RendererConfig.llff()
    cfg.density_scale = 40.0
    assert not cfg.use_ndc
    small = Intrinsics(48, 64, intr.fx * 64 / intr.w, intr.fy * 64 / intr.w, 32., 24.)
    r = Renderer(model, cfg, small, 2.0, raymarch_channels=3 + nc).to(dev)
    r.density_grid = torch.tensor(synthetic_density_grid(2.0, 128, 48, 0), device=dev)
    r.density_bitfield = raymarching.packbits(r.density_grid, 0.5)
    r.update_occ = False
    return r, torch.tensor(np.asarray(poses[:3], np.float32), device=dev)


def test_render_rgbd(small_renderer):
    r, poses = small_renderer
    want = r.render(poses[1])
    got = r.render_rgbd(poses[1], min_opacity=0.5)
    for k in ('rgb_map', 'trans_map', 'classes'):
        assert torch.equal(got[k], want[k]), k
    ws, dist = got['weights_sum'], got['distance']
    N = r.intr.h * r.intr.w
    assert tuple(ws.shape) == (N,) and tuple(dist.shape) == (N,) and dist.dtype == torch.float32
    hit = ws >= 0.5
    assert 0.2 * N < int(hit.sum()) < N, int(hit.sum())
    assert (dist[~hit] == 0).all()
    print('distance - near >=', float((dist - got['nears'])[hit].min()), ' far - distance >=', float((got['fars'] - dist)[hit].min()))
    assert (dist[hit] >= got['nears'][hit]).all() and (dist[hit] <= got['fars'][hit]).all()
    # another threshold moves only the cut
    loose = r.render_rgbd(poses[1], min_opacity=0.05)
    assert torch.equal(loose['distance'][hit], dist[hit]) and int((loose['distance'] > 0).sum()) >= int(hit.sum())
    r.fused_inference = True
    try:
        with pytest.raises(NotImplementedError, match='fused_inference'):
            r.render_rgbd(poses[1])
    finally:
        r.fused_inference = False
    r.cfg.use_ndc = True
    try:
        with pytest.raises(NotImplementedError, match='use_ndc'):
            r.render_rgbd(poses[1])
    finally:
        r.cfg.use_ndc = False


def test_view_consistency(small_renderer):
    from nerfstyle_amd.consistency import reproject_frames, warp_error
    r, poses = small_renderer
    H, W = r.intr.h, r.intr.w
    out = r.view_consistency(poses, gaps=(1, 2))
    assert sorted(out) == [1, 2]
    for gap, t in out.items():
        assert tuple(t.shape) == (3 - gap, 2) and t.dtype == torch.float64 and t.is_cuda
        cov = t[:, 1]
        assert ((cov >= 0) & (cov <= 1)).all()
    print('view consistency', {g: t.tolist() for g, t in out.items()})
    frames = [r.render_rgbd(poses[i]) for i in range(3)]
    rgb, dist = torch.stack([f['rgb_map'] for f in frames]), torch.stack([f['distance'] for f in frames])
    again = r.view_consistency(poses, gaps=(1, 2), frames=(rgb, dist))
    for gap in (1, 2):
        assert torch.equal(again[gap], out[gap])
    _, mask, stats = reproject_frames(rgb, dist, poses[:, :3].contiguous(), r.intr, [(1, 1)], camera_flip=r.cfg.flip_camera)
    err = warp_error(stats, H, W)
    assert float(err[0, 0]) < 1e-6 and 0.0 < float(err[0, 1]) <= 1.0
    assert not mask[0][dist[1] == 0].any()
