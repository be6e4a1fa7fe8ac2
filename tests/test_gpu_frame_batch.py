"""GPU: mixed-frame ray batches -- nsr_generate_rays_frames against nsr_generate_rays per segment (bit for bit), its backward
against the fp64 restatement of tests/frame_batch_ref.py, nsr_draw_frame_batch against the restated Philox draw, and
Renderer.render_frames against per-frame Renderer.render calls on the same pixels (outputs, pose gradient, arena gradient).

Bars.  Backward: the bound of any fp32 summation order with the product's rounding, count_f * 2^-23 * sum |term| per entry
(tests/test_gpu_pose_grad.py holds nsr_generate_rays_backward to the same).  Renderer outputs: bit-identical.  Pose gradient
of the render: rel-L2 5e-3 (f16), the bar of test_pose_gradient_end_to_end; arena.grad: rel-L2 2e-5."""
import numpy as np
import pytest
import torch

import frame_batch_ref as FR
from helpers import rel_l2, render_setup, room_cameras

pytestmark = pytest.mark.gpu
U23 = 2.0 ** -23
W, H = 24, 16
CAM = (20.0, 21.0, 11.5, 8.25)                       # fx, fy, cx, cy
SEG = [2, 0, 2, 1, 2]
GUARD = 64
KS = [1, 63, 64, 65, 257]
# the backward's mapping: a thread per segment below K = 64, then ceil(K / 256) blocks per segment, at most 64: 1000 is four
# blocks with a partial last one, 16500 is 65 blocks' worth on 64 (the stride over the segment is taken)
KS_BWD = KS + [1000, 16500]


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _poses(F=3):
    return np.ascontiguousarray(np.asarray(room_cameras()['poses'], np.float32)[:F, :3, :])


def _guarded(n, dev, dtype=torch.float32, fill=7.0, inner=None):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    if inner is not None:
        buf[GUARD:GUARD + n] = inner
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill=7.0):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------
def _forward(dev, poses_d, seg_d, pix_d, S, K, flip, F):
    from nerfstyle_amd import _lib as L
    N = S * K
    bo, ro = _guarded(N * 3, dev)
    bd, rd = _guarded(N * 3, dev)
    L.check(L.lib().nsr_generate_rays_frames(L.p(poses_d), F, W, H, *CAM, flip, L.p(seg_d), L.p(pix_d), S, K, L.p(ro), L.p(rd),
                                             L.stream()), 'generate_rays_frames')
    assert _guards_intact(bo, N * 3) and _guards_intact(bd, N * 3)
    return ro.view(N, 3).clone(), rd.view(N, 3).clone()


@pytest.mark.parametrize('camera_flip', [0, 5])
@pytest.mark.parametrize('K', KS)
def test_forward_is_generate_rays_per_segment(dev, K, camera_flip):
    from nerfstyle_amd import _lib as L
    poses, S, F = _poses(), len(SEG), 3
    rng = np.random.default_rng(100 * K + camera_flip)
    pix = rng.integers(0, W * H, S * K).astype(np.int32)
    poses_d, pix_d = T(poses, dev), T(pix, dev)
    want_o, want_d = torch.empty(S * K, 3, device=dev), torch.empty(S * K, 3, device=dev)
    for s, f in enumerate(SEG):
        sl = slice(s * K, (s + 1) * K)
        L.check(L.lib().nsr_generate_rays(L.p(poses_d[f]), W, H, *CAM, camera_flip, L.p(pix_d[sl]), K, L.p(want_o[sl]), L.p(want_d[sl]),
                                          L.stream()), 'generate_rays')
    got_o, got_d = _forward(dev, poses_d, T(np.asarray(SEG, np.int32), dev), pix_d, S, K, camera_flip, F)
    assert torch.equal(got_o, want_o) and torch.equal(got_d, want_d)
    assert bool(torch.isfinite(got_d).all()) and float((got_d.norm(dim=1) - 1).abs().max()) < 1e-6
    # a segment that names no frame: NaN rows for it, the others untouched
    for bad_s, bad in ((3, F), (0, -1)):
        seg = np.asarray(SEG, np.int32)
        seg[bad_s] = bad
        o, d = _forward(dev, poses_d, T(seg, dev), pix_d, S, K, camera_flip, F)
        sel = torch.zeros(S * K, dtype=torch.bool, device=dev)
        sel[bad_s * K:(bad_s + 1) * K] = True
        assert bool(torch.isnan(o[sel]).all()) and bool(torch.isnan(d[sel]).all())
        assert torch.equal(o[~sel], want_o[~sel]) and torch.equal(d[~sel], want_d[~sel])


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------
def _backward(dev, poses_d, seg_d, pix_d, go_d, gd_d, S, K, flip, F, ws=None):
    """-> grad_poses [F,3,4]; the workspace arrives as NaN between guard bands unless one is handed in"""
    from nerfstyle_amd import _lib as L
    n_ws = int(L.lib().nsr_generate_rays_frames_backward_workspace_bytes(F, S, K)) // 8
    wbuf = None
    if ws is None:
        wbuf, ws = _guarded(n_ws, dev, dtype=torch.float64, inner=float('nan'))
    obuf, out = _guarded(F * 12, dev)
    L.check(L.lib().nsr_generate_rays_frames_backward(L.p(poses_d), F, W, H, *CAM, flip, L.p(seg_d), L.p(pix_d), S, K, L.p(go_d), L.p(gd_d),
                                                      L.p(ws), L.p(out), L.stream()), 'generate_rays_frames_backward')
    assert _guards_intact(obuf, F * 12) and (wbuf is None or _guards_intact(wbuf, n_ws))
    return out.view(F, 3, 4).clone()


@pytest.mark.parametrize('camera_flip', [0, 5])
@pytest.mark.parametrize('K', KS_BWD)
def test_backward_per_frame(dev, K, camera_flip):
    F, S = 4, len(SEG)                                  # frame 3 is in no segment
    poses = _poses(F)
    rng = np.random.default_rng(7 * K + camera_flip)
    pix = rng.integers(0, W * H, S * K).astype(np.int32)
    g_o, g_d = rng.standard_normal((S * K, 3)).astype(np.float32), rng.standard_normal((S * K, 3)).astype(np.float32)
    poses_d = T(poses, dev)

    def run(seg, pix, g_o, g_d):
        a = (T(np.asarray(seg, np.int32), dev), T(pix, dev), T(g_o, dev), T(g_d, dev))
        got = _backward(dev, poses_d, *a, S, K, camera_flip, F)
        assert torch.equal(got, _backward(dev, poses_d, *a, S, K, camera_flip, F))            # two calls: the same bits
        return got.cpu().numpy()

    def check(got, seg, pix, g_o, g_d, what):
        want, mag, count = FR.pose_gradient(poses, W, *CAM, camera_flip, seg, pix, K, g_o, g_d)
        err, bound = np.abs(got - want), count[:, None, None] * U23 * mag
        for f in range(F):
            if count[f]:
                print('K=%d flip=%d %s frame %d (%d rays): max err / bound %.3f' % (K, camera_flip, what, f, count[f],
                                                                                     float((err[f] / bound[f]).max())))
                assert np.any(got[f] != 0)
            else:
                assert np.all(got[f] == 0)                # exact zeros
        assert np.all(np.isfinite(got)) and np.all(err <= bound)

    got = run(SEG, pix, g_o, g_d)
    assert list(FR.pose_gradient(poses, W, *CAM, camera_flip, SEG, pix, K, g_o, g_d)[2]) == [K, K, 3 * K, 0]
    check(got, SEG, pix, g_o, g_d, 'as drawn')
    # segments 0 and 1 (frames 2 and 0) trade places with their rays: the same sums in another order
    order = np.concatenate([np.arange(s * K, (s + 1) * K) for s in (1, 0, 2, 3, 4)])
    seg2 = [SEG[1], SEG[0]] + SEG[2:]
    got2 = run(seg2, pix[order], g_o[order], g_d[order])
    check(got2, seg2, pix[order], g_o[order], g_d[order], 'swapped')
    check(got2, SEG, pix, g_o, g_d, 'swapped, against the unswapped reference')
    # a segment naming no frame adds nothing, anywhere
    seg3 = list(SEG)
    seg3[2] = -1
    check(run(seg3, pix, g_o, g_d), seg3, pix, g_o, g_d, 'one segment out of range')


@pytest.mark.parametrize('K', [5, 257])
def test_backward_graph_replays_equal_eager(dev, K):
    F, S = 4, len(SEG)
    poses_d = T(_poses(F), dev)
    rng = np.random.default_rng(K)

    def contents(seg):
        return (np.asarray(seg, np.int32), rng.integers(0, W * H, S * K).astype(np.int32),
                rng.standard_normal((S * K, 3)).astype(np.float32), rng.standard_normal((S * K, 3)).astype(np.float32))
    static = [T(a, dev) for a in contents(SEG)]
    from nerfstyle_amd import _lib as L
    ws = torch.empty(int(L.lib().nsr_generate_rays_frames_backward_workspace_bytes(F, S, K)) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(F * 12, device=dev)

    def call():
        L.check(L.lib().nsr_generate_rays_frames_backward(L.p(poses_d), F, W, H, *CAM, 3, L.p(static[0]), L.p(static[1]), S, K,
                                                          L.p(static[2]), L.p(static[3]), L.p(ws), L.p(out), L.stream()),
                'generate_rays_frames_backward')
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for seg in ([1, 1, 3, 0, 2], [0, 2, 2, 2, 1]):
        for dst, src in zip(static, contents(seg)):
            dst.copy_(T(src, dev))
        eager = _backward(dev, poses_d, *static, S, K, 3, F)
        out.fill_(7.0)
        ws.fill_(float('nan'))
        graph.replay()
        assert torch.equal(out.view(F, 3, 4), eager) and float(eager.abs().sum()) > 0


# ---- 3. draw ---------------------------------------------------------------------------------------------------------------------
SEED = 0x9e3779b97f4a7c15
F_DRAW, P_DRAW = 7, W * H


def _draw(dev, S, K, sequence, seqdev=None, stream_id=0, fixed=None, advance=0, out=None):
    from nerfstyle_amd import _lib as L
    if out is None:
        out = (torch.full((S,), -9, dtype=torch.int32, device=dev), torch.full((S * K,), -9, dtype=torch.int32, device=dev),
               torch.full((S * K,), -9, dtype=torch.int64, device=dev))
    L.check(L.lib().nsr_draw_frame_batch(F_DRAW, P_DRAW, S, K, SEED, sequence, L.p(seqdev), stream_id, L.p(fixed), advance,
                                         L.p(out[0]), L.p(out[1]), L.p(out[2]), L.stream()), 'draw_frame_batch')
    return out


def _same(got, want):
    return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


@pytest.mark.parametrize('S,K', [(5, 64), (1, 1), (3, 257)])
def test_draw_is_the_restated_draw(dev, S, K):
    got = _draw(dev, S, K, 11)
    want = FR.draw(F_DRAW, P_DRAW, S, K, SEED, 11)
    assert _same(got, want)
    seg, pix, rows = (g.cpu().numpy() for g in got)
    assert seg.min() >= 0 and seg.max() < F_DRAW and pix.min() >= 0 and pix.max() < P_DRAW
    assert rows.dtype == np.int64 and rows.min() >= 0 and rows.max() < F_DRAW * P_DRAW
    assert np.array_equal(rows, np.repeat(seg.astype(np.int64), K) * P_DRAW + pix)
    # the rank draws another batch from the same seed
    other = _draw(dev, S, K, 11, stream_id=1)
    assert _same(other, FR.draw(F_DRAW, P_DRAW, S, K, SEED, 11, stream_id=1))
    assert not _same(other, want)
    # fixed frames: honoured, and the pixels are the free draw's
    fixed = np.asarray([6, 0, 3, 3, 1][:S], np.int32)
    got_f = _draw(dev, S, K, 11, fixed=T(fixed, dev))
    assert _same(got_f, FR.draw(F_DRAW, P_DRAW, S, K, SEED, 11, fixed_frames=fixed))
    assert np.array_equal(got_f[0].cpu().numpy(), fixed) and np.array_equal(got_f[1].cpu().numpy(), pix)
    # the device word: added to the host sequence (modulo 2^32), incremented by exactly one per advancing call
    seqdev = torch.tensor([5, 77], dtype=torch.int32, device=dev)
    assert _same(_draw(dev, S, K, 11, seqdev=seqdev), FR.draw(F_DRAW, P_DRAW, S, K, SEED, 16)) and seqdev.tolist() == [5, 77]
    assert _same(_draw(dev, S, K, 11, seqdev=seqdev, advance=1), FR.draw(F_DRAW, P_DRAW, S, K, SEED, 16)) and seqdev.tolist() == [6, 77]
    assert _same(_draw(dev, S, K, 11, seqdev=seqdev, advance=1), FR.draw(F_DRAW, P_DRAW, S, K, SEED, 17)) and seqdev.tolist() == [7, 77]
    assert _same(_draw(dev, S, K, 0xfffffffe, seqdev=seqdev), FR.draw(F_DRAW, P_DRAW, S, K, SEED, 0xfffffffe + 7))


def test_draw_graph_replays_advance(dev):
    S, K = 5, 64
    seqdev = torch.zeros(1, dtype=torch.int32, device=dev)
    out = _draw(dev, S, K, 3)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _draw(dev, S, K, 3, seqdev=seqdev, advance=1, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _draw(dev, S, K, 3, seqdev=seqdev, advance=1, out=out)
    seqdev.fill_(40)
    seen = []
    for k in range(2):
        for t in out:
            t.fill_(-9)
        graph.replay()
        assert int(seqdev[0]) == 41 + k
        assert _same(out, FR.draw(F_DRAW, P_DRAW, S, K, SEED, 3 + 40 + k))
        seen.append(out[1].clone())
    assert not torch.equal(seen[0], seen[1])


def test_dataset_draw_and_rows(dev):
    from nerfstyle_amd.common import Intrinsics
    from nerfstyle_amd.dataset import ResidentDataset
    rng = np.random.default_rng(9)
    F = 3
    ds = ResidentDataset(rng.random((F, 3, H, W)).astype(np.float32), np.asarray(room_cameras()['poses'], np.float32)[:F],
                         Intrinsics(H, W, *CAM), 2.0, dev, seg_maps=rng.integers(0, 5, (F, H, W)), num_classes=5)
    b = ds.draw(5, 65, seed=SEED, sequence=2, stream_id=1)
    assert (b.S, b.K) == (5, 65) and _same((b.seg_frame, b.pix, b.rows), FR.draw(F, W * H, 5, 65, SEED, 2, stream_id=1))
    ray_frame = b.seg_frame.long().repeat_interleave(65)
    assert torch.equal(ds.target_rgb_rows[b.rows], ds.targets[ray_frame, b.pix.long(), :3])
    assert torch.equal(ds.target_cls_rows[b.rows], ds.targets[ray_frame, b.pix.long(), 3].long())
    ptrs = [t.data_ptr() for t in (b.seg_frame, b.pix, b.rows)]
    seqdev = torch.tensor([4], dtype=torch.int32, device=dev)
    b2 = ds.draw(5, 65, seed=SEED, sequence=2, sequence_dev=seqdev, advance=True, frames=T(np.asarray([2, 2, 0, 1, 0], np.int32), dev), out=b)
    assert b2 is b and ptrs == [t.data_ptr() for t in (b.seg_frame, b.pix, b.rows)] and int(seqdev[0]) == 5
    assert _same((b.seg_frame, b.pix, b.rows), FR.draw(F, W * H, 5, 65, SEED, 6, fixed_frames=[2, 2, 0, 1, 0]))


# ---- 4. / 5. the renderer --------------------------------------------------------------------------------------------------------
DENSITY_SCALE = 40.0
S_R, K_R = 4, 96
FRAMES_R = [0, 1, 1, 0]


def _renderer_and_batch(dev):
    from nerfstyle_amd.dataset import FrameBatch
    r, _, poses, intr, _ = render_setup(dev, nc=5, compute_dtype=torch.float16, contrast=16.0)
    r.cfg.density_scale = DENSITY_SCALE
    Wf, Hf = intr.size()
    # the draw of ResidentDataset.draw without a resident dataset: two frames' worth of rows, frames fixed so that both occur
    from nerfstyle_amd import _lib as L
    seg = torch.empty(S_R, dtype=torch.int32, device=dev)
    pix = torch.empty(S_R * K_R, dtype=torch.int32, device=dev)
    rows = torch.empty(S_R * K_R, dtype=torch.int64, device=dev)
    L.check(L.lib().nsr_draw_frame_batch(2, Wf * Hf, S_R, K_R, 1234, 0, None, 0, L.p(T(np.asarray(FRAMES_R, np.int32), dev)), 0, L.p(seg),
                                         L.p(pix), L.p(rows), L.stream()), 'draw_frame_batch')
    batch = FrameBatch(seg, pix, rows, S_R, K_R)
    assert seg.tolist() == FRAMES_R and torch.equal(rows, seg.long().repeat_interleave(K_R) * (Wf * Hf) + pix.long())
    ray_frame = torch.tensor(FRAMES_R, device=dev).repeat_interleave(K_R)
    return r, np.asarray(poses, np.float32)[:, :3, :], batch, ray_frame


def test_render_frames_rows_are_render_rows(dev):
    r, poses, batch, ray_frame = _renderer_and_batch(dev)
    P = T(poses[:3], dev)
    with torch.no_grad(), r.occupancy_frozen():
        out = r.render_frames(P, batch)
        assert out['target'] is None and out['rgb_map'].shape == (S_R * K_R, 3)
        assert float(out['trans_map'].min()) < 0.5                                  # the rays do hit the seeded scene
        for f in (0, 1):
            sel = ray_frame == f
            one = r.render(P[f], pix_subset=batch.pix[sel], training=True)
            for k in ('rgb_map', 'trans_map', 'classes'):
                d = float((out[k][sel] - one[k]).abs().max())
                print('frame %d %s: max |render_frames - render| %.3e' % (f, k, d))
                assert torch.equal(out[k][sel], one[k])
    with pytest.raises(NotImplementedError, match='training render'):
        r.render_frames(P, batch, training=False)


def test_render_frames_pose_gradient(dev):
    r, poses, batch, ray_frame = _renderer_and_batch(dev)
    N = S_R * K_R
    target = torch.tensor(np.random.default_rng(4).random((N, 3)).astype(np.float32), device=dev)
    r.pose_gradients = True
    P = T(poses[:3], dev).clone().requires_grad_()                                  # frame 2 is in no segment
    out = r.render_frames(P, batch)
    (((out['rgb_map'] - target) ** 2).sum() * (1.0 / N)).backward()
    assert P.grad is not None and P.grad.shape == (3, 3, 4)
    got, got_arena = P.grad.cpu().numpy(), r.model.arena.grad.clone()
    assert np.all(got[2] == 0) and np.all(np.isfinite(got))
    on = {k: out[k].detach().clone() for k in ('rgb_map', 'trans_map', 'classes')}

    r.model.arena.grad.zero_()
    want = np.zeros((2, 3, 4), np.float32)
    for f in (0, 1):
        sel = ray_frame == f
        pose = T(poses[f], dev).clone().requires_grad_()
        one = r.render(pose, pix_subset=batch.pix[sel], training=True)
        (((one['rgb_map'] - target[sel]) ** 2).sum() * (1.0 / N)).backward()
        want[f] = pose.grad.cpu().numpy()
    want_arena = r.model.arena.grad.clone()
    assert np.linalg.norm(want[0]) > 0 and np.linalg.norm(want[1]) > 0
    for f in (0, 1):
        print('frame %d pose gradient: rel-L2 %.3e (|want| %.3e)' % (f, rel_l2(got[f], want[f]), np.linalg.norm(want[f])))
    err = rel_l2(got[:2], want)
    print('render_frames pose gradient: rel-L2 %.3e' % err)
    assert err <= 5e-3
    assert all(rel_l2(got[f], want[f]) <= 5e-3 for f in (0, 1))
    e_arena = rel_l2(got_arena.cpu().numpy(), want_arena.cpu().numpy())
    print('arena.grad: rel-L2 %.3e (|want| %.3e)' % (e_arena, float(want_arena.norm())))
    assert float(want_arena.norm()) > 0 and e_arena <= 2e-5

    # the switch off, or poses that do not require grad: the switch-on forward's outputs, nothing recorded towards the poses
    for switch, req in ((False, True), (True, False)):
        r.pose_gradients = switch
        P2 = T(poses[:3], dev).clone().requires_grad_(req)
        off = r.render_frames(P2, batch)
        (((off['rgb_map'] - target) ** 2).sum() * (1.0 / N)).backward()
        assert P2.grad is None
        for k in on:
            assert torch.equal(off[k].detach(), on[k]), k
