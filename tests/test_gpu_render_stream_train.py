"""GPU: the streaming render with the TRAINING composite (Renderer.render_train_fused -> nsr_render_rays_stream, NSR_STREAM_TRAIN:
march, fused field, training composite and render_train's epilogue in one kernel, no sample buffer) against the buffered no-grad
render_train, the CPU oracle and a host replay of the stop rule; edge rays, work-list order, capture, memory, the stylisation
stage's pass 1, and the inference mode of the shared entry point against nsr_render_rays_infer.

Every test prints the figures it asserts on (run with -s to see them)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import render_setup as _setup

pytestmark = pytest.mark.gpu

PATCHES = ((180, 130, 96, 64), (180, 130, 100, 60))     # x, y, w, h on room pose 5; the second is no multiple of the 8 x 8 tile
OPAQUE = 400.0                                          # density_scale at which the synthetic boxes are opaque surfaces
INFER, TRAIN = 0, 1


def _box(p):
    from nerfstyle_amd.common import Box2D
    return Box2D(*p)


def _rays(r, pose, **kw):
    from nerfstyle_amd.rays import generate_rays
    rays, _ = generate_rays(pose, r.intr, None, camera_flip=r.cfg.flip_camera, device=r.device, **kw)
    return rays


def _random_pix(intr, n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(intr.w * intr.h, generator=g)[:n].to(dev)


def _both(r, pose, **kw):
    """render(training=True) without autograd: the buffered path (which must not have dropped a ray), then the streaming one."""
    with torch.no_grad():
        r.fused_nograd_train = False
        a = r.render(pose, None, training=True, **kw)
        assert not bool(r.last_call_overflowed())
        r.fused_nograd_train = True
        b = r.render(pose, None, training=True, **kw)
        r.fused_nograd_train = False
    return a, b


def _maxdiff(a, b):
    return float((a - b).abs().max()) if a.numel() else 0.0


def _assert_equals_buffered(a, b, tag):
    """The project's compositing bar (tests/test_gpu_raymarching.py, _assert_equals_single_pass): 2e-5 on colours and classes,
    2e-3 on the depth's finite entries."""
    d_rgb, d_cls = _maxdiff(a['rgb_map'], b['rgb_map']), _maxdiff(a['classes'], b['classes'])
    ok = torch.isfinite(a['trans_map'])
    d_dep = _maxdiff(a['trans_map'][ok], b['trans_map'][ok])
    print('{}: max|rgb| {:.3e}  max|classes| {:.3e}  max|depth| {:.3e}  finite depths {} of {}'.format(
        tag, d_rgb, d_cls, d_dep, int(ok.sum()), ok.numel()))
    assert d_rgb < 2e-5 and d_cls < 2e-5, (tag, d_rgb, d_cls)
    assert d_dep < 2e-3, (tag, d_dep)
    assert torch.equal(ok, torch.isfinite(b['trans_map']))
    assert not torch.isnan(b['rgb_map']).any() and not torch.isnan(b['classes']).any()


def _as_dict(t):
    return {'rgb_map': t[0], 'trans_map': t[1], 'classes': t[2]}


def _raw(r, rays_o, rays_d, composite, order=None, epilogue=True, counts=True):
    """nsr_render_rays_stream itself -> dict of everything it wrote."""
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import raymarching
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, r.aabb, r.cfg.min_near)
    N, C, dev = rays_o.shape[0], r.raymarch_channels, rays_o.device
    o = {'ws': torch.empty(N, device=dev), 'depth': torch.empty(N, device=dev), 'image': torch.empty(N, C, device=dev),
         'stats': torch.zeros(2, dtype=torch.int32, device=dev)}
    if epilogue:
        o.update({'rgb_map': torch.empty(N, 3, device=dev), 'trans_map': torch.empty(N, device=dev),
                  'classes': torch.empty(N, C - 3, device=dev)})
    if counts:
        o['n'] = torch.full((N,), -1, dtype=torch.int32, device=dev)
    desc = r.model._desc(r.cfg.density_scale)
    L.check(L.lib().nsr_render_rays_stream(
        ctypes.byref(desc), L.p(r.model._gather_tables()), L.p(r.model._mlp_flat()), L.p(rays_o), L.p(rays_d), L.p(order), N,
        L.p(nears), L.p(fars), L.p(r.march_bitfield), float(r.bound), 0., r.cfg.max_steps, r.cascade, r.cfg.grid_size,
        float(r.cfg.t_thresh), composite, L.p(o['ws']), L.p(o['depth']), L.p(o['image']), L.p(o.get('rgb_map')),
        L.p(o.get('trans_map')), L.p(o.get('classes')), L.p(o.get('n')), L.p(o['stats']), L.stream()), 'render_rays_stream')
    return o


def _same_bits(a, b, keys):
    return all(torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k])) for k in keys)


ALL_KEYS = ('ws', 'depth', 'image', 'rgb_map', 'trans_map', 'classes', 'n')


# ---- 1. equals the buffered no-grad training render ------------------------------------------------------------------------------
@pytest.mark.parametrize('table_dtype,compute_dtype,density_scale', [
    (torch.float16, torch.float16, OPAQUE), (torch.float16, torch.float16, None),
    (torch.float32, torch.float16, OPAQUE), (torch.float32, torch.float16, None),
    (torch.float16, torch.bfloat16, OPAQUE)])
def test_fused_equals_buffered_nograd_render_train(dev, table_dtype, compute_dtype, density_scale):
    """A 96 x 64 patch, a 100 x 60 patch and 2 048 random pixels of room pose 5, default capacity, flag off against flag on."""
    r, _, poses, intr, _ = _setup(dev, table_dtype=table_dtype, compute_dtype=compute_dtype)
    if density_scale is not None:
        r.cfg.density_scale = density_scale
    pose = torch.tensor(poses[5], device=dev)
    for tag, kw, N in (('96x64', {'patch': _box(PATCHES[0])}, 96 * 64), ('100x60', {'patch': _box(PATCHES[1])}, 100 * 60),
                       ('2048 px', {'pix_subset': _random_pix(intr, 2048, 1, dev)}, 2048)):
        a, b = _both(r, pose, **kw)
        _assert_equals_buffered(a, b, '{} {} {} ds={}'.format(tag, table_dtype, compute_dtype, r.cfg.density_scale))
        print('  min rgb {:.3f}  stats {}'.format(float(b['rgb_map'].min()), r.last_infer_stats().tolist()))
        assert float(b['rgb_map'].min()) < 0.9          # something was rendered
        assert int(r.last_infer_stats()[1]) == N


# ---- 2. against the CPU oracle -----------------------------------------------------------------------------------------------------
def test_fused_matches_oracle_training_chain(O, dev):
    """2 048 seeded random pixels, contrast-16 checkpoint, density_scale 40, against the oracle's march_rays_train -> field_forward
    -> composite_rays_train_forward -> render_epilogue: PSNR > 45 dB, swapping the oracle's colour channels costs more than 20 dB,
    classes within 5e-2 * max(1, |cls|max)."""
    r, ref, poses, intr, bits = _setup(dev, contrast=16.0)
    r.cfg.density_scale = 40.0
    np.random.seed(69420)
    N = 2048
    pix = np.random.choice(intr.w * intr.h, N, replace=False)
    ro, rd = O.generate_rays(poses[0], intr.w, intr.h, intr.fx, intr.fy, intr.cx, intr.cy, 3, pix_indices=pix)
    aabb = np.array([-2, -2, -2, 2, 2, 2], np.float32)
    near, far = O.near_far_from_aabb(ro, rd, aabb, 0.2)
    fp = O.FieldParams(ref.emb_density.detach().numpy(), ref.emb_color.detach().numpy(), ref.p_density.detach().numpy(),
                       ref.p_color1.detach().numpy(), ref.p_color2.detach().numpy(), ref.p_class.detach().numpy(), ref.offsets,
                       ref.pls, num_classes=ref.nc)
    xyzs, _, deltas, rays, cnt = O.march_rays_train(ro, rd, 2.0, bits, 2, 128, near, far, 1024, align=128)
    out_o, sig, _ = O.field_forward(fp, xyzs)
    ws, depth, image = O.composite_rays_train_forward((sig * np.float32(40.0)).astype(np.float32), out_o, deltas, rays, 1e-4)
    rgb_o, _, cls_o = O.render_epilogue(ws, depth, image, near, far)

    r.fused_nograd_train = True
    with torch.no_grad():
        out = r.render(torch.tensor(poses[0], device=dev), None, training=True, pix_subset=torch.tensor(pix, device=dev))
    rgb = out['rgb_map'].cpu().numpy()
    psnr = O.compute_psnr(float(np.mean((rgb - rgb_o) ** 2)))
    swapped = O.compute_psnr(float(np.mean((rgb - rgb_o[:, ::-1]) ** 2)))
    d_cls = float(np.abs(out['classes'].cpu().numpy() - cls_o).max())
    print('PSNR vs oracle chain {:.1f} dB, with swapped channels {:.1f} dB, max|classes| {:.3e} (|cls|max {:.3f}), oracle samples {}'.format(
        psnr, swapped, d_cls, float(np.abs(cls_o).max()), int(cnt[0])))
    assert int(r.last_infer_stats()[1]) == N and int(r.last_infer_stats()[0]) > 0
    assert psnr > 45.0, psnr
    assert swapped < psnr - 20.0
    assert d_cls < 5e-2 * max(1.0, np.abs(cls_o).max())


# ---- 3. the stop rule is the training one, per ray ---------------------------------------------------------------------------------
def _replay_train_stop(sigmas, deltas, rays_info, thresh):
    """Host replay, float32, of the stop rule of kernel_composite_rays_train_forward (raymarching.cu:846-872) over marched samples:
    per ray (row of rays_info) the number of samples accumulated -- the running product is tested AFTER the sample, and the sample
    that takes it below `thresh` is the last one."""
    info = rays_info.cpu().numpy()
    off, ns = info[:, 1].astype(np.int64), info[:, 2].astype(np.int64)
    total = int((off + ns).max())
    sig = sigmas[:total].cpu().numpy().astype(np.float32)
    dt = deltas[:total, 0].cpu().numpy().astype(np.float32)
    T = np.ones(len(off), np.float32)
    count = np.zeros(len(off), np.int64)
    alive = ns > 0
    k = 0
    while alive.any():
        i = np.nonzero(alive)[0]
        idx = off[i] + k
        alpha = (np.float32(1.0) - np.exp(-sig[idx] * dt[idx])).astype(np.float32)
        T[i] = T[i] * (np.float32(1.0) - alpha)
        count[i] += 1
        stop = (T[i] < np.float32(thresh)) | (k + 1 >= ns[i])
        alive[i[stop]] = False
        k += 1
    return count


@pytest.mark.parametrize('density_scale', [OPAQUE, None])
def test_stop_rule_is_the_training_one_per_ray(dev, density_scale):
    """n_composited of every ray lies between the host replays of the training stop rule at 2 T_thresh and at T_thresh / 2 over
    the sigmas and deltas that march_train + model.field give for the same rays (a factor-2 bracket is far outside the float
    error of a product near 1e-4, and the count is monotone in the threshold).  Opaque: the upper counts sum to less than the
    emitted samples, and the inference composite accumulates at least as many samples on every ray and more on some.  Fog: no
    ray reaches the threshold, and the counts are the emitted counts exactly."""
    r, _, poses, _, _ = _setup(dev)
    if density_scale is not None:
        r.cfg.density_scale = density_scale
    rays = _rays(r, torch.tensor(poses[5], device=dev), patch=_box(PATCHES[0]))
    N = rays.origins.shape[0]
    with torch.no_grad():
        mt = r.march_train(rays)
        sigmas, _ = r.model.field(mt['xyzs'], sigma_only=False, m_dev=mt['counter'], density_scale=r.cfg.density_scale)
    emitted = int(mt['counter'][0])
    info = mt['rays_info'].cpu().numpy()
    assert emitted == int(info[:, 2].sum()) and emitted < mt['M']
    assert np.array_equal(np.sort(info[:, 0]), np.arange(N))
    lo = np.zeros(N, np.int64); hi = np.zeros(N, np.int64); per_ray = np.zeros(N, np.int64)
    lo[info[:, 0]] = _replay_train_stop(sigmas, mt['deltas'], mt['rays_info'], 2 * r.cfg.t_thresh)
    hi[info[:, 0]] = _replay_train_stop(sigmas, mt['deltas'], mt['rays_info'], r.cfg.t_thresh / 2)
    per_ray[info[:, 0]] = info[:, 2]
    o = _raw(r, rays.origins, rays.dirs, TRAIN)
    n_t = o['n'].cpu().numpy().astype(np.int64)
    stats = o['stats'].cpu().numpy()
    print('ds={}: emitted {}  replay lo {}  hi {}  composited {}  ({:.3f} of emitted)  rays below lo {}  above hi {}'.format(
        r.cfg.density_scale, emitted, int(lo.sum()), int(hi.sum()), int(n_t.sum()), n_t.sum() / emitted, int((n_t < lo).sum()),
        int((n_t > hi).sum())))
    assert (lo <= hi).all()
    if density_scale is not None:
        assert int(hi.sum()) < emitted                  # precondition on the input: rays do stop early on this scene
    else:
        assert np.array_equal(lo, per_ray) and np.array_equal(hi, per_ray)      # precondition: no ray reaches the threshold
        assert np.array_equal(n_t, per_ray)
    assert (lo <= n_t).all() and (n_t <= hi).all()
    assert int(stats[0]) == int(n_t.sum()) and int(stats[1]) == N
    if density_scale is not None:
        n_i = _raw(r, rays.origins, rays.dirs, INFER)['n'].cpu().numpy().astype(np.int64)
        print('  inference composite: {} samples, {} rays with more samples than the training composite'.format(
            int(n_i.sum()), int((n_i > n_t).sum())))
        assert (n_t <= n_i).all() and (n_t < n_i).any()


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------------
def test_rays_that_miss_the_box_equal_the_buffered_path(dev):
    r, _, poses, intr, _ = _setup(dev)
    r.cfg.density_scale = OPAQUE
    g = torch.Generator().manual_seed(3)
    rays = _rays(r, torch.tensor(poses[5], device=dev), pix_subset=_random_pix(intr, 1024, 3, dev))
    ro, rd = rays.origins.clone(), rays.dirs.clone()
    ro[:512] = torch.tensor([5.0, 5.0, 5.0], device=dev) + 0.01 * torch.rand(512, 3, generator=g).to(dev)
    rd[:512] = torch.nn.functional.normalize(torch.tensor([1.0, 1.0, 1.0], device=dev) + 0.1 * torch.rand(512, 3, generator=g).to(dev), dim=-1)
    rays.origins, rays.dirs = ro, rd
    with torch.no_grad():
        want = _as_dict(r.render_train(rays))
        assert not bool(r.last_call_overflowed())
    got = _as_dict(r.render_train_fused(rays))
    raw = _raw(r, ro, rd, TRAIN)
    for tag, b in (('render_train_fused', got), ('raw call', raw)):
        for k in ('rgb_map', 'classes', 'trans_map'):
            d = _maxdiff(torch.nan_to_num(want[k]), torch.nan_to_num(b[k]))
            print('{} {}: max|diff| {:.3e}'.format(tag, k, d))
            assert d < (2e-3 if k == 'trans_map' else 2e-5), (tag, k, d)
        assert torch.equal(torch.nan_to_num(want['rgb_map'][:512]), torch.nan_to_num(b['rgb_map'][:512]))
        assert torch.equal(torch.nan_to_num(want['trans_map'][:512]), torch.nan_to_num(b['trans_map'][:512]))
        assert torch.equal(torch.isnan(want['trans_map']), torch.isnan(b['trans_map']))
    assert torch.equal(got['rgb_map'][:512], torch.ones(512, 3, device=dev)) and float(got['classes'][:512].abs().max()) == 0.0
    assert float(raw['ws'][:512].abs().max()) == 0.0 and int(raw['n'][:512].abs().max()) == 0
    assert float(got['rgb_map'][512:].min()) < 0.9      # the other half does see the scene
    assert int(raw['stats'][1]) == 1024
    # the half that hits is what it is without the missing half in the batch
    alone = _raw(r, ro[512:].contiguous(), rd[512:].contiguous(), TRAIN)
    assert _same_bits({k: raw[k][512:] for k in ALL_KEYS}, alone, ALL_KEYS)


def test_empty_occupancy_renders_white(dev):
    r, _, poses, _, _ = _setup(dev)
    r.density_bitfield = torch.zeros_like(r.density_bitfield)
    r.fused_nograd_train = True
    with torch.no_grad():
        out = r.render(torch.tensor(poses[5], device=dev), None, patch=_box(PATCHES[0]), training=True)
    assert torch.equal(out['rgb_map'], torch.ones_like(out['rgb_map']))
    assert float(out['classes'].abs().max()) == 0.0
    stats = r.last_infer_stats().cpu().numpy()
    assert int(stats[0]) == 0 and int(stats[1]) == 96 * 64
    rays = _rays(r, torch.tensor(poses[5], device=dev), patch=_box(PATCHES[0]))
    raw = _raw(r, rays.origins, rays.dirs, TRAIN)
    assert torch.equal(raw['rgb_map'], torch.ones_like(raw['rgb_map'])) and float(raw['classes'].abs().max()) == 0.0
    assert int(raw['stats'][0]) == 0 and int(raw['n'].abs().max()) == 0


def test_full_occupancy_constant_density_equals_the_buffered_path(dev):
    """All-ones bitfield and a density net whose last layer is zero (sigma = density_scale everywhere): every ray marches the whole
    box, up to max_steps samples."""
    r, _, poses, intr, _ = _setup(dev)
    r.density_bitfield = torch.full_like(r.density_bitfield, 255)
    with torch.no_grad():
        r.model.arena[r.model.table_elems + 2048: r.model.table_elems + 3072] = 0
    pose = torch.tensor(poses[5], device=dev)
    pix = _random_pix(intr, 2048, 5, dev)
    a, b = _both(r, pose, pix_subset=pix)
    _assert_equals_buffered(a, b, 'full occupancy')
    stats = r.last_infer_stats().cpu().numpy()
    rays = _rays(r, pose, pix_subset=pix)
    raw = _raw(r, rays.origins, rays.dirs, TRAIN)
    _assert_equals_buffered(a, raw, 'full occupancy, raw call')
    print('samples per ray {:.1f}, longest ray {}'.format(stats[0] / 2048, int(raw['n'].max())))
    assert stats[0] > 2048 * 100 and int(stats[1]) == 2048
    assert int(raw['n'].max()) == r.cfg.max_steps
    assert float(b['rgb_map'].min()) < 0.9


@pytest.mark.parametrize('n_rays', [1, 17, 4097])
def test_ray_counts_that_exercise_refill_and_tails(dev, n_rays):
    r, _, poses, intr, _ = _setup(dev)
    r.cfg.density_scale = OPAQUE
    pose = torch.tensor(poses[5], device=dev)
    pix = _random_pix(intr, n_rays, 7, dev)
    a, b = _both(r, pose, pix_subset=pix)
    _assert_equals_buffered(a, b, 'N={}'.format(n_rays))
    assert int(r.last_infer_stats()[1]) == n_rays
    rays = _rays(r, pose, pix_subset=pix)
    raw = _raw(r, rays.origins, rays.dirs, TRAIN)
    _assert_equals_buffered(a, raw, 'N={}, raw call'.format(n_rays))
    assert int(raw['stats'][1]) == n_rays and int(raw['n'].min()) >= 0


# ---- 5. order-free and capturable --------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_work_list_order(dev):
    r, _, poses, _, _ = _setup(dev)
    r.cfg.density_scale = OPAQUE
    rays = _rays(r, torch.tensor(poses[5], device=dev), patch=_box(PATCHES[0]))
    N = rays.origins.shape[0]
    g = torch.Generator().manual_seed(11)
    perm = torch.randperm(N, generator=g).to(torch.int32).to(dev)
    base = _raw(r, rays.origins, rays.dirs, TRAIN)
    shuffled = _raw(r, rays.origins, rays.dirs, TRAIN, order=perm)
    assert _same_bits(base, shuffled, ALL_KEYS + ('stats',))
    assert float(base['ws'].max()) > 0.5


def test_capture_and_replay_equals_eager(dev):
    """One render_train_fused captured on static ray buffers (single stream), replayed for two poses written into them."""
    r, _, poses, _, _ = _setup(dev)
    r.cfg.density_scale = OPAQUE
    box, shape = _box(PATCHES[0]), PATCHES[0][2:]
    ray_sets = [_rays(r, torch.tensor(poses[i], device=dev), patch=box) for i in (5, 9)]
    eager = [tuple(t.clone() for t in r.render_train_fused(rs, dense_shape=shape)) for rs in ray_sets]
    static = _rays(r, torch.tensor(poses[0], device=dev), patch=box)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r.render_train_fused(static, dense_shape=shape)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = r.render_train_fused(static, dense_shape=shape)
    for rs, want in zip(ray_sets, eager):
        static.origins.copy_(rs.origins)
        static.dirs.copy_(rs.dirs)
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip(outs, want):
            assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(w))
    assert float(eager[0][0].min()) < 0.9 and not torch.equal(eager[0][0], eager[1][0])


# ---- 6. inference mode unchanged ---------------------------------------------------------------------------------------------------
def test_stream_entry_in_inference_mode_is_render_rays_infer(dev):
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import raymarching
    r, _, poses, _, _ = _setup(dev)
    r.cfg.density_scale = OPAQUE
    rays = _rays(r, torch.tensor(poses[5], device=dev), patch=_box(PATCHES[0]))
    ro, rd = rays.origins, rays.dirs
    nears, fars = raymarching.near_far_from_aabb(ro, rd, r.aabb, r.cfg.min_near)
    N, C = ro.shape[0], r.raymarch_channels
    ws, depth, image = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, C, device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    desc = r.model._desc(r.cfg.density_scale)
    L.check(L.lib().nsr_render_rays_infer(
        ctypes.byref(desc), L.p(r.model._gather_tables()), L.p(r.model._mlp_flat()), L.p(ro), L.p(rd), None, N, L.p(nears),
        L.p(fars), L.p(r.march_bitfield), float(r.bound), 0., r.cfg.max_steps, 0, r.cascade, r.cfg.grid_size,
        float(r.cfg.t_thresh), L.p(ws), L.p(depth), L.p(image), L.p(stats), L.stream()), 'render_rays_infer')
    o = _raw(r, ro, rd, INFER, epilogue=False, counts=False)
    assert torch.equal(o['ws'], ws) and torch.equal(o['depth'], depth) and torch.equal(o['image'], image)
    assert torch.equal(o['stats'], stats)
    assert float(ws.max()) > 0.5
    # and the optional outputs change nothing of the raw ones
    e = _raw(r, ro, rd, INFER)
    assert torch.equal(e['ws'], ws) and torch.equal(e['depth'], depth) and torch.equal(e['image'], image)
    assert torch.equal(e['rgb_map'], image[:, :3] + (1 - ws).unsqueeze(-1)) and int(e['n'].sum()) == int(stats[0])


# ---- 7. memory ----------------------------------------------------------------------------------------------------------------------
def test_full_frame_memory_is_bounded_by_rays(dev):
    """Full 504 x 378 frame, flag on: the peak over the call stays within 256 B x N + 1 MB (bound and method of
    test_full_frame_memory_is_bounded_by_rays in tests/test_gpu_render_infer.py).  The buffered path's peak, at 256 samples per ray
    instead of its default 1 024, is printed beside it, not asserted."""
    r, _, poses, intr, _ = _setup(dev, cap=256)
    r.cfg.density_scale = OPAQUE
    pose = torch.tensor(poses[0], device=dev)
    N = intr.w * intr.h
    peaks = {}
    with torch.no_grad():
        for fused in (True, False):
            r.fused_nograd_train = fused
            out = r.render(pose, None, training=True)           # first call: the f16 table copy and the cached work list exist afterwards
            del out
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = r.render(pose, None, training=True)
            torch.cuda.synchronize()
            peaks[fused] = torch.cuda.max_memory_allocated() - before
            assert out['rgb_map'].shape == (N, 3)
            del out
    print('peak over the call, {} rays: fused {:.1f} MB ({:.0f} B/ray), buffered render_train at 256 samples per ray {:.1f} MB'.format(
        N, peaks[True] / 1e6, peaks[True] / N, peaks[False] / 1e6))
    assert peaks[True] <= 256 * N + (1 << 20), peaks


# ---- 8. the stylisation stage's pass 1 ----------------------------------------------------------------------------------------------
def test_stylisation_pass_1_and_the_deferred_gradient(dev):
    """stylize.render_full_frame at 504 x 378 with the flag on against off, and deferred_backprop_step (mean of squares,
    patch_graphs=None): the arena gradient equals the flag-off run's at rel-L2 < 2e-5."""
    from nerfstyle_amd.stylize import deferred_backprop_step, render_full_frame
    r, _, poses, intr, _ = _setup(dev, cap=256)
    r.cfg.density_scale = OPAQUE
    pose = torch.tensor(poses[0], device=dev)
    frames, grads = {}, {}
    SCALE = 65536.0                     # f16 MFMA operands: see test_deferred_backprop_equals_direct_and_trains_only_colour_table
    for fused in (False, True):
        r.fused_nograd_train = fused
        frames[fused] = render_full_frame(r, pose)
        if not fused:
            assert not bool(r.last_call_overflowed())
        if r.model.arena.grad is not None:
            r.model.arena.grad.zero_()
        deferred_backprop_step(r, pose, lambda rgb: (rgb ** 2).mean(), patch_size=200, loss_scale=SCALE)
        grads[fused] = r.model.arena.grad.detach().clone()
    d = _maxdiff(frames[False], frames[True])
    num = float((grads[True] - grads[False]).double().norm())
    den = float(grads[False].double().norm())
    print('full frame max|rgb| {:.3e}  min rgb {:.3f}  gradient rel-L2 {:.3e} (norm {:.3e})'.format(
        d, float(frames[True].min()), num / den, den))
    assert frames[True].shape == (intr.h, intr.w, 3) and float(frames[True].min()) < 0.9
    assert d < 2e-5
    assert den > 0 and num / den < 2e-5


# ---- the occupancy bookkeeping of render_train -------------------------------------------------------------------------------------
def test_step_bookkeeping_is_render_trains(dev):
    """With update_occ set and no update due: local_step advances by one and the ring slot receives (samples shaded, N)."""
    r, _, poses, intr, _ = _setup(dev)
    r.cfg.density_scale = OPAQUE
    r.update_occ = True
    r.local_step = 1
    assert not r.occupancy_update_due()
    r.fused_nograd_train = True
    with torch.no_grad():
        r.render(torch.tensor(poses[5], device=dev), None, training=True, pix_subset=_random_pix(intr, 2048, 1, dev))
    slot = r.step_counter[1].tolist()
    print('ring slot', slot, 'stats', r.last_infer_stats().tolist())
    assert r.local_step == 2 and slot[1] == 2048 and slot[0] > 0 and slot == r.last_infer_stats().tolist()
    assert not bool(r.last_call_overflowed())
    assert int(r.step_counter[2:].abs().sum()) == 0 and int(r.step_counter[0].abs().sum()) == 0
