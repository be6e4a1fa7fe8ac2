"""GPU: per-frame exposure -- nsr_recon_loss_exposure against the NumPy fp64 restatement of tests/exposure_ref.py through the C
ABI, and through recon_loss, ExposureRefiner and the renderer.

Bars (derived in exposure_ref.py's docstring, none tuned):
  grad_rgb_map   elementwise 2^-20 * (2 w s_ / 3N) * gain * (|p| + |t|)
  grad_exposure  2^-20 * ln2 * sum over the frame's rays of (2 w s_ / 3N) * |p| * (|p| + |t|)
  ray_err        2^-22 relative plus 2^-22 * (|p| + |t|)^2 absolute
  grad_classes, mse, ce and the total: 2e-6, what tests/test_gpu_error_map.py holds nsr_recon_loss_weighted to.  That test runs
                 at scale * factor = 1; the total and grad_classes are linear in s_ = scale * factor (512 here), so their bar is
                 2e-6 * s_; mse and ce (loss_out[1], [2]) are unscaled and keep 2e-6.
  524 289 rays   the value to 1e-5 relative: under 40 fp32 additions on any path through thread loop, wave tree, block tree and
                 final pass.
Everything said to be bit-identical is compared as integers."""
import numpy as np
import pytest
import torch

import exposure_ref as XR
from helpers import rel_l2, render_setup

pytestmark = pytest.mark.gpu
SCALE, FACTOR = 1024.0, 0.5
S_ = SCALE * FACTOR
SMALL = [(1, 1, 1), (3, 1, 2), (5, 63, 3), (2, 64, 2), (2, 65, 2), (3, 257, 2), (65, 2, 3), (130, 1, 3)]
LARGE = (3, 174763, 2)                               # N = 524 289 = 2048 * 256 + 1


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def make(S, K, F, nc=5, use_pix=True, use_w=True, seed=0, seg=None, exposure=None):
    """seeded inputs as NumPy arrays in the kernel's dtypes: rgb_map in [0.05, 0.95], targets in [0, 1], exposure in [-2, 2],
    weights in [0.25, 4]; every frame of [0, F) named where S allows it"""
    rng = np.random.default_rng([seed, S, K, F])
    N = S * K
    P = N + 7 if use_pix else N
    a = dict(S=S, K=K, F=F, N=N, nc=nc)
    a['rgb_map'] = rng.uniform(0.05, 0.95, (N, 3)).astype(np.float32)
    a['target_rgb'] = rng.uniform(0.0, 1.0, (P, 3)).astype(np.float32)
    a['exposure'] = rng.uniform(-2.0, 2.0, (F, 3)).astype(np.float32) if exposure is None else np.asarray(exposure, np.float32)
    a['seg_frame'] = ((np.arange(S) * 7 + rng.integers(0, F)) % F).astype(np.int32) if seg is None else np.asarray(seg, np.int32)
    a['pix'] = rng.permutation(P)[:N].astype(np.int64) if use_pix else None
    a['ray_weight'] = rng.uniform(0.25, 4.0, N).astype(np.float32) if use_w else None
    a['classes'] = (rng.standard_normal((N, nc)) * 2).astype(np.float32) if nc else None
    a['target_cls'] = rng.integers(0, nc, P).astype(np.int64) if nc else None
    return a


def reference(a):
    return XR.loss(a['rgb_map'], a['target_rgb'], a['exposure'], a['seg_frame'], a['K'], pix=a['pix'], ray_weight=a['ray_weight'],
                   classes=a['classes'], target_cls=a['target_cls'], ce_lambda=1e-3, s_=S_)


class Call:
    """the device tensors of one set of inputs and the outputs of nsr_recon_loss_exposure (or _weighted) on them, pre-filled with 7"""

    def __init__(self, dev, a, want_err=True, exposure_t=None, scaled=True):
        from nerfstyle_amd import _lib as L
        self.a, self.dev = a, dev
        d = {k: (None if a[k] is None else T(a[k], dev)) for k in ('rgb_map', 'target_rgb', 'exposure', 'seg_frame', 'pix', 'ray_weight',
                                                                    'classes', 'target_cls')}
        if exposure_t is not None:
            d['exposure'] = exposure_t
        self.d = d
        self.scale, self.factor = (torch.tensor(SCALE, device=dev), FACTOR) if scaled else (None, 1.0)
        N, nc = a['N'], a['nc']
        self.g_rgb = torch.full((N, 3), 7.0, device=dev)
        self.g_cls = torch.full((N, nc), 7.0, device=dev) if nc else None
        self.g_exp = torch.full((a['F'], 3), 7.0, device=dev)
        self.ray_err = torch.full((N,), 7.0, device=dev) if want_err else None
        self.out = torch.full((3,), 7.0, device=dev)
        self.ws = torch.empty(int(L.lib().nsr_recon_loss_exposure_workspace_bytes(N, a['F'], a['S'], a['K'])) // 8, dtype=torch.float64,
                              device=dev)

    def run(self):
        from nerfstyle_amd import _lib as L
        a, d = self.a, self.d
        L.check(L.lib().nsr_recon_loss_exposure(L.p(d['rgb_map']), L.p(d['classes']), a['N'], a['nc'], L.p(d['target_rgb']),
                                                L.p(d['target_cls']), L.p(d['pix']), L.p(d['ray_weight']), L.p(d['exposure']), a['F'],
                                                L.p(d['seg_frame']), a['S'], a['K'], 1e-3, self.factor, L.p(self.scale), L.p(self.g_rgb),
                                                L.p(self.g_cls), L.p(self.g_exp), L.p(self.ray_err), L.p(self.out), L.p(self.ws),
                                                L.stream()), 'recon_loss_exposure')
        return self

    def run_weighted(self):
        from nerfstyle_amd import _lib as L
        a, d = self.a, self.d
        L.check(L.lib().nsr_recon_loss_weighted(L.p(d['rgb_map']), L.p(d['classes']), a['N'], a['nc'], L.p(d['target_rgb']),
                                                L.p(d['target_cls']), L.p(d['pix']), L.p(d['ray_weight']), 1e-3, self.factor, L.p(self.scale),
                                                L.p(self.g_rgb), L.p(self.g_cls), L.p(self.ray_err), L.p(self.out), L.p(self.ws),
                                                L.stream()), 'recon_loss_weighted')
        return self

    def outputs(self):
        return [t for t in (self.out, self.g_rgb, self.g_cls, self.g_exp, self.ray_err) if t is not None]


def same_bits(x, y):
    return all(torch.equal(bits(p), bits(q)) for p, q in zip(x.outputs(), y.outputs())) and len(x.outputs()) == len(y.outputs())


def ratios(c, r, value_rel=None):
    """the worst ratio of |kernel - restatement| to its bar, per output; asserts nothing"""
    def worst(got, want, bound):
        got = got.double().cpu().numpy()
        bound = np.broadcast_to(np.asarray(bound, np.float64), got.shape)
        err = np.abs(got - want)
        assert np.all(np.isfinite(got))
        return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))
    res = {'grad_rgb_map': worst(c.g_rgb, r['grad_rgb_map'], r['bound_rgb']),
           'grad_exposure': worst(c.g_exp, r['grad_exposure'], r['bound_exposure'])}
    if c.ray_err is not None:
        res['ray_err'] = worst(c.ray_err, r['ray_err'], r['bound_err'])
    if c.g_cls is not None:
        res['grad_classes'] = worst(c.g_cls, r['grad_classes'], 2e-6 * S_)
    out = c.out.double().cpu().numpy()
    if value_rel is None:
        res['total'] = abs(out[0] - r['total']) / (2e-6 * S_)
        res['mse'] = abs(out[1] - r['mse']) / 2e-6
        res['ce'] = abs(out[2] - r['ce']) / 2e-6
    else:
        res['total'] = abs(out[0] - r['total']) / (value_rel * abs(r['total']))
        res['mse'] = abs(out[1] - r['mse']) / (value_rel * abs(r['mse']))
        res['ce'] = abs(out[2] - r['ce']) / (value_rel * abs(r['ce'])) if r['ce'] else float(out[2] != 0.0)
    return res


def fold(worst, res):
    for k, v in res.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'S%d-K%d-F%d' % s)
def test_parity(dev, shape):
    S, K, F = shape
    worst = {}
    for k, (nc, use_pix, use_w, want_err) in enumerate((nc, p, w, e) for nc in (0, 5) for p in (False, True) for w in (False, True)
                                                       for e in (False, True)):
        a = make(S, K, F, nc=nc, use_pix=use_pix, use_w=use_w, seed=k)
        c = Call(dev, a, want_err=want_err).run()
        assert all(bool((t != 7.0).all()) for t in c.outputs()[1:])             # every element written
        fold(worst, ratios(c, reference(a)))
    print('S=%d K=%d F=%d: worst error / bar  %s' % (S, K, F, '  '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_parity_two_rays_per_thread(dev):
    """N = 2048 * 256 + 1: the first thread of the capped grid takes a second ray; everything on"""
    S, K, F = LARGE
    a = make(S, K, F, nc=5, use_pix=True, use_w=True)
    c = Call(dev, a).run()
    res = ratios(c, reference(a), value_rel=1e-5)
    print('S=%d K=%d F=%d: worst error / bar  %s' % (S, K, F, '  '.join('%s %.3f' % kv for kv in sorted(res.items()))))
    assert all(v <= 1.0 for v in res.values()), res


# ---- 2. zero exposure is the weighted loss ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 63, 3), (3, 257, 2)], ids=lambda s: 'S%d-K%d-F%d' % s)
def test_zero_exposure_is_the_weighted_loss(dev, shape):
    S, K, F = shape
    for use_w in (True, False):
        a = make(S, K, F, use_w=use_w, exposure=np.zeros((F, 3)))
        c = Call(dev, a).run()
        w = Call(dev, a).run_weighted()
        for name, x, y in (('loss_out', c.out, w.out), ('grad_rgb_map', c.g_rgb, w.g_rgb), ('grad_classes', c.g_cls, w.g_cls),
                           ('ray_err', c.ray_err, w.ray_err)):
            assert torch.equal(bits(x), bits(y)), name
        r = reference(a)
        res = ratios(c, r)
        assert res['grad_exposure'] <= 1.0 and np.all(r['grad_exposure'] != 0.0) and bool((c.g_exp != 0).all())


# ---- 3. frames nobody names, frames out of range ---------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [5, 65])
def test_unnamed_frames_get_positive_zero(dev, K):
    a = make(6, K, 4, seg=[0, 2, 2, 0, 0, 2])
    c = Call(dev, a).run()
    g = bits(c.g_exp).cpu().numpy()
    assert np.all(g[[1, 3]] == 0) and np.all(g[[0, 2]] != 0)                 # +0.0: no bit set, the sign bit included
    assert all(v <= 1.0 for v in ratios(c, reference(a)).values())


@pytest.mark.parametrize('K', [5, 65])
def test_out_of_range_frames(dev, K):
    F = 3
    a = make(5, K, F, seg=[0, -1, 2, F, 1])
    # the exposure rows inside a larger allocation whose neighbouring rows are NaN
    big = torch.full((F + 2, 3), float('nan'), device=dev)
    big[1:F + 1] = T(a['exposure'], dev)
    c = Call(dev, a, exposure_t=big[1:F + 1]).run()
    r = reference(a)                                                         # gain 1 for those rays, their terms in no row
    outside = r['frame'] == -1
    assert outside.sum() == 2 * K
    assert all(not bool(torch.isnan(t).any()) for t in c.outputs())
    res = ratios(c, r)
    assert all(v <= 1.0 for v in res.values()), res
    # the gain-1 gradient of those rays is the weighted loss's, bit for bit
    w = Call(dev, a).run_weighted()
    rows = T(np.nonzero(outside)[0], dev)
    assert torch.equal(bits(c.g_rgb[rows]), bits(w.g_rgb[rows]))


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 63, 3), (3, 257, 2)], ids=lambda s: 'S%d-K%d-F%d' % s)
def test_garbage_in_the_workspace_changes_nothing(dev, shape):
    a = make(*shape)
    x, y = Call(dev, a), Call(dev, a)
    x.ws.fill_(float('nan'))
    y.ws.view(torch.uint8).fill_(0x5a)
    assert same_bits(x.run(), y.run())
    y.ws.fill_(float('inf'))
    assert same_bits(x, y.run()) and bool((x.g_exp != 0).all())


@pytest.mark.parametrize('K', [5, 257])
def test_graph_replays_equal_eager(dev, K):
    S, F = 5, 3
    a = make(S, K, F)
    static = Call(dev, a)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # this call alone: one chain of four kernels
        static.run()
    for k, seg in enumerate(([1, 1, 2, 0, 2], [0, 2, 2, 2, 1], [2, 0, 1, 1, 0])):
        b = make(S, K, F, seed=k + 1, seg=seg)
        for name in ('seg_frame', 'rgb_map'):
            static.d[name].copy_(T(b[name], dev))
            a[name] = b[name]
        eager = Call(dev, a).run()
        for t in static.outputs():
            t.fill_(7.0)
        static.ws.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(static, eager) and float(eager.g_exp.abs().sum()) > 0
        assert all(v <= 1.0 for v in ratios(static, reference(a)).values())


# ---- 5. autograd and recovery ------------------------------------------------------------------------------------------------------
def test_autograd_reaches_the_parameter(dev):
    from nerfstyle_amd.exposure import ExposureRefiner
    from nerfstyle_amd.recon_loss import last_terms, recon_loss
    S, K, F = 4, 96, 3
    a = make(S, K, F)
    abi = Call(dev, a).run()
    d = abi.d
    ref = ExposureRefiner(F, zero_mean=False).to(dev)
    with torch.no_grad():
        ref.log2_gain.copy_(d['exposure'])
    err = torch.empty(S * K, device=dev)

    def loss_of(rgb, cls, **kw):
        return recon_loss(rgb, cls, d['target_rgb'], d['target_cls'], pix=d['pix'], factor=FACTOR, scale=abi.scale, ray_weight=d['ray_weight'],
                          ray_err_out=err, exposure=ref(), seg_frame=d['seg_frame'], rays_per_segment=K, **kw)
    for backward in (False, True):
        ref.log2_gain.grad = None
        rgb, cls = d['rgb_map'].clone().requires_grad_(), d['classes'].clone().requires_grad_()
        loss = loss_of(rgb, cls, backward=backward)
        if backward:
            assert not loss.requires_grad
        else:
            loss.backward()
        assert torch.equal(bits(ref.log2_gain.grad), bits(abi.g_exp)) and torch.equal(bits(rgb.grad), bits(abi.g_rgb))
        assert torch.equal(bits(cls.grad), bits(abi.g_cls)) and torch.equal(bits(err), bits(abi.ray_err))
        assert torch.equal(bits(loss), bits(abi.out[0])) and torch.equal(bits(last_terms(loss)), bits(abi.out[1:]))
    # only the exposure requires grad: still reaches it
    ref.log2_gain.grad = None
    loss_of(d['rgb_map'], None, backward=True)
    assert ref.log2_gain.grad is not None and bool((ref.log2_gain.grad != 0).all())
    # zero_mean: the projected gradient
    zm = ExposureRefiner(F).to(dev)
    with torch.no_grad():
        zm.log2_gain.copy_(d['exposure'])
    e = zm()
    e.retain_grad()
    recon_loss(d['rgb_map'], None, d['target_rgb'], pix=d['pix'], exposure=e, seg_frame=d['seg_frame'], rays_per_segment=K).backward()
    assert torch.allclose(zm.log2_gain.grad, e.grad - e.grad.mean(0, keepdim=True), rtol=1e-5, atol=1e-7 * float(e.grad.abs().max()))


def test_adam_recovers_the_gains(dev):
    """targets = rgb_map * 2**e_true, e_true in [-1, 1], 4 096 rays over 8 frames; torch Adam, lr 0.1 decayed by 0.985 per step,
    400 steps (exposure_ref.recover).  On the fp64 restatement on the CPU that loop ends with max |e - e_true| = 2.148e-5; the
    bar here is ten times that, 2.148e-4."""
    from nerfstyle_amd.exposure import ExposureRefiner
    from nerfstyle_amd.recon_loss import recon_loss
    rgb, target, seg, e_true = XR.recovery_inputs()
    rgb, target, seg = T(rgb, dev), T(target, dev), T(seg, dev)
    ref = ExposureRefiner(XR.REC_F, zero_mean=False).to(dev)

    def grad_of():
        recon_loss(rgb, None, target, exposure=ref(), seg_frame=seg, rays_per_segment=XR.REC_K, backward=True)
    err = float(np.abs(XR.recover(ref.log2_gain, grad_of) - e_true).max())
    print('recovery: max |e - e_true| %.3e, bar %.3e' % (err, XR.REC_BAR))
    assert err <= XR.REC_BAR


# ---- 6. through the renderer -------------------------------------------------------------------------------------------------------
S_R, K_R, FRAMES_R = 4, 96, [0, 1, 1, 0]


def test_through_the_renderer(dev):
    """the (4, 96) mixed-frame batch over the seeded checkpoint of tests/test_gpu_frame_batch.py"""
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd.dataset import FrameBatch
    from nerfstyle_amd.exposure import ExposureRefiner
    from nerfstyle_amd.recon_loss import recon_loss
    r, _, poses, intr, _ = render_setup(dev, nc=5, compute_dtype=torch.float16, contrast=16.0)
    r.cfg.density_scale = 40.0
    Wf, Hf = intr.size()
    N, F = S_R * K_R, 3
    seg = torch.empty(S_R, dtype=torch.int32, device=dev)
    pix = torch.empty(N, dtype=torch.int32, device=dev)
    rows = torch.empty(N, dtype=torch.int64, device=dev)
    L.check(L.lib().nsr_draw_frame_batch(2, Wf * Hf, S_R, K_R, 1234, 0, None, 0, L.p(T(np.asarray(FRAMES_R, np.int32), dev)), 0, L.p(seg),
                                         L.p(pix), L.p(rows), L.stream()), 'draw_frame_batch')
    batch = FrameBatch(seg, pix, rows, S_R, K_R)
    P = T(np.asarray(poses, np.float32)[:F, :3, :], dev)
    target = T(np.random.default_rng(4).random((N, 3)).astype(np.float32), dev)
    ref = ExposureRefiner(F, zero_mean=False).to(dev)

    def step(gains):
        """-> (arena.grad, log2_gain.grad, rgb_map) of one render and loss; gains None: recon_loss without exposure"""
        r.model.arena.grad = None
        ref.log2_gain.grad = None
        if gains is not None:
            with torch.no_grad():
                ref.log2_gain.copy_(gains)
        out = r.render_frames(P, batch)
        kw = {} if gains is None else dict(exposure=ref(), seg_frame=batch.seg_frame, rays_per_segment=batch.K)
        recon_loss(out['rgb_map'], None, target, backward=True, **kw)
        return r.model.arena.grad.clone(), ref.log2_gain.grad, out['rgb_map'].detach().float().contiguous()

    gains = T(np.asarray([[0.5, -0.25, 0.75], [-0.5, 0.25, -0.75], [1.0, 1.0, 1.0]], np.float32), dev)
    arena_on, g_exp, rgb_map = step(gains)
    # the stand-alone call on the returned rgb_map
    a = dict(S=S_R, K=K_R, F=F, N=N, nc=0, rgb_map=rgb_map.cpu().numpy(), target_rgb=target.cpu().numpy(), exposure=gains.cpu().numpy(),
             seg_frame=np.asarray(FRAMES_R, np.int32), pix=None, ray_weight=None, classes=None, target_cls=None)
    alone = Call(dev, a, want_err=False, scaled=False).run()
    assert g_exp is not None and torch.equal(bits(g_exp), bits(alone.g_exp))
    assert bool((g_exp[:2] != 0).all()) and bool((bits(g_exp[2]) == 0).all())   # frame 2 is in no segment
    assert float(arena_on.float().norm()) > 0
    arena_off, none, _ = step(None)
    assert none is None
    arena_zero, g_zero, _ = step(torch.zeros(F, 3, device=dev))
    d_on = rel_l2(arena_on.float().cpu().numpy(), arena_off.float().cpu().numpy())
    d_zero = rel_l2(arena_zero.float().cpu().numpy(), arena_off.float().cpu().numpy())
    print('arena.grad against the run without exposure: rel-L2 %.3e with gains, %.3e with gains of exactly 1' % (d_on, d_zero))
    assert d_on > 1e-2 and d_zero <= 2e-5
    assert bool((g_zero[:2] != 0).all())
