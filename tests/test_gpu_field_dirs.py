"""GPU parity of the view-dependent colour path (SH direction encoding in the fused field), through the C ABI.

References: tests/sh_ref.py (fp64 SH table; the view-dependent wiring composed from oracle.mlp_forward's rounding emulation
and torch_port's fp32 autograd modules).  Bars are the project's existing ones: SH encode <= 4e-6 abs (fp32 encode
arithmetic); forward rel-L2 <= 2e-3 (f16) / 1e-2 (bf16) against the rounding-emulating reference and <= 5e-3 / 3e-2 against
pure fp32; backward rel-L2 <= 5e-3 (f16) / 3e-2 (bf16) per parameter block against autograd through the rounding-emulating
restatement.
"""
import ctypes

import numpy as np
import pytest
import torch

import sh_ref as SH
from helpers import rel_l2

pytestmark = pytest.mark.gpu

FWD_BAR = {'f16': (2e-3, 5e-3), 'bf16': (1e-2, 3e-2)}
BWD_BAR = {'f16': 5e-3, 'bf16': 3e-2}


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


_REFS = {}


def _ref(nc):
    if nc not in _REFS:
        _REFS[nc] = SH.FieldDirs(num_classes=nc)
    return _REFS[nc]


def _pair(dev, dt, table_dtype, nc=5):
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.style_nerf import StyleTCNerf
    ref = _ref(nc)
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), nc, enc_dtype=table_dtype, view_dependent=True,
                    compute_dtype=torch.float16 if dt == 'f16' else torch.bfloat16)
    sd = m.state_dict()
    sd['x_density_embedder.embeddings'] = ref.emb_density.detach()
    sd['x_color_embedder.embeddings'] = ref.emb_color.detach()
    sd['density_net.params'] = ref.p_density.detach()
    sd['color1_net.params'] = ref.p_color1.detach()
    sd['color2_net.params'] = ref.color2_params().detach()
    sd['class_net.params'] = ref.p_class.detach()
    m.load_state_dict(sd)
    return m.to(dev), ref


def _inputs(M, seed, bad=True):
    rng = np.random.default_rng(seed)
    pts = (rng.random((M, 3)) * 4 - 2).astype(np.float32)
    if bad and M >= 16:
        out = rng.random(M) < 0.03
        pts[out] *= 1.5                     # ~3 % outside the box (some land inside again: fine)
        pts[1] = [np.nan, 0.1, 0.2]
        pts[M // 2] = [0.3, np.nan, np.nan]
    d = rng.standard_normal((M, 3))
    dirs = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return pts, dirs


def _fwd(m, pts, dirs, perm=None, mlp=None, with_dirs=True, feats=None):
    from nerfstyle_amd import _lib as L
    M = pts.shape[0]
    sig = torch.full((M,), -1.0, device=pts.device)
    rgb = torch.full((M, m.out_channels), -1.0, device=pts.device)
    desc = m._desc(1.0)
    mlp = m._mlp_flat() if mlp is None else mlp
    if with_dirs:
        st = L.lib().nsr_field_forward_dirs(ctypes.byref(desc), L.p(m._gather_tables()), L.p(mlp), L.p(pts), M, None, L.p(sig),
                                            L.p(rgb), L.p(feats), L.p(perm), L.p(dirs), L.stream())
    else:
        st = L.lib().nsr_field_forward(ctypes.byref(desc), L.p(m._gather_tables()), L.p(mlp), L.p(pts), M, None, L.p(sig),
                                       L.p(rgb), L.p(feats), L.p(perm), L.stream())
    assert st == 0
    return sig, rgb


def test_sh_encode(dev):
    from nerfstyle_amd.style_nerf import SHEncoder
    _, dirs = _inputs(1000, 1)
    dirs = np.concatenate([dirs, np.eye(3, dtype=np.float32), -np.eye(3, dtype=np.float32)])
    ref = SH.sh_ref(dirs)
    out = SHEncoder.encode_dirs(T(dirs, dev)).cpu().numpy()
    assert out.shape == (1006, 16)
    err = np.abs(out - ref).max()
    print('sh encode max abs error', err)
    assert err <= 4e-6
    # the module takes what the reference feeds the encoder: (d + 1) / 2
    out2 = SHEncoder(4)(T((dirs + 1) / 2, dev)).cpu().numpy()
    assert np.abs(out2 - ref).max() <= 4e-6


@pytest.mark.parametrize('dt,table_dtype,nc', [('f16', torch.float32, 5), ('f16', None, 1), ('bf16', torch.float32, 13),
                                               ('bf16', None, 5)])
def test_field_forward_dirs(O, dev, dt, table_dtype, nc):
    m, ref = _pair(dev, dt, table_dtype, nc)
    half = table_dtype is None
    from nerfstyle_amd import _lib as L
    desc = m._desc(1.0)
    # with 16-bit tables and a permutation the LATTICE kernel runs, with directions too (it fits four workgroups per CU)
    assert L.lib().nsr_field_forward_uses_lattice(ctypes.byref(desc), 1, 1) == int(half)
    for M in (1, 16, 17, 1000):
        pts, dirs = _inputs(M, 20 + M)
        p, d = T(pts, dev), T(dirs, dev)
        sig, rgb = _fwd(m, p, d)
        # a NaN position encodes to zeros in the kernels, like one outside the box; the reference is given the latter
        pts_ref = np.where(np.isnan(pts).any(axis=1, keepdims=True), np.float32(9.0), pts)
        out_e, sig_e = SH.field_forward_dirs(O, ref, pts_ref, dirs, half=dt, table_half=half)
        out_f, _ = SH.field_forward_dirs(O, ref, pts_ref, dirs, half=None, table_half=half)
        rn = rgb.cpu().numpy()
        e, f = rel_l2(rn, out_e), rel_l2(rn, out_f)
        print(dt, table_dtype, nc, M, 'rel-L2 emulated', e, 'fp32', f)
        assert e <= FWD_BAR[dt][0] and f <= FWD_BAR[dt][1]
        assert np.all(np.isfinite(rn))
        # sigma and the class channels: bit-identical to the direction-less entry point on the same inputs
        sig0, rgb0 = _fwd(m, p, d, with_dirs=False)
        assert torch.equal(sig, sig0) and torch.equal(rgb[:, 3:], rgb0[:, 3:])
        # spatial walk (the lattice kernel with 16-bit tables) against the plain walk: bit-identical per sample
        perm = m.sample_order(p)
        sig1, rgb1 = _fwd(m, p, d, perm=perm)
        assert torch.equal(sig, sig1) and torch.equal(rgb, rgb1)
        rperm = T(np.random.default_rng(M).permutation(M).astype(np.int32), dev)
        sig2, rgb2 = _fwd(m, p, d, perm=rperm)
        assert torch.equal(sig, sig2) and torch.equal(rgb, rgb2)


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_first_layer_column_probe(O, dev, dt):
    """First layer zeroed except ONE column: the output must be the reference's for that column -- every SH column (the
    permuted K = 32 weight image), and one color1 column."""
    m, ref = _pair(dev, dt, torch.float32)
    pts, dirs = _inputs(16, 3, bad=False)
    p, d = T(pts, dev), T(dirs, dev)
    vec = (4 * np.random.default_rng(4).standard_normal(64)).astype(np.float32)
    base = SH.mlp_block(ref)
    p2, psh = ref.p_color2.detach().clone(), ref.p_sh.detach().clone()
    try:
        for kind, k in [('sh', k) for k in range(16)] + [('c1', 5)]:
            mlp = base.copy()
            mlp[6144:7168] = 0
            mlp[15360:] = 0
            (mlp[15360:] if kind == 'sh' else mlp[6144:7168]).reshape(64, 16)[:, k] = vec
            with torch.no_grad():
                ref.p_color2.copy_(torch.tensor(mlp[6144:12288]))
                ref.p_sh.copy_(torch.tensor(mlp[15360:]))
            _, rgb = _fwd(m, p, d, mlp=T(mlp, dev))
            out_e, _ = SH.field_forward_dirs(O, ref, pts, dirs, half=dt)
            assert rel_l2(rgb.cpu().numpy()[:, :3], out_e[:, :3]) <= FWD_BAR[dt][0], (kind, k)
            # and the probe can tell: with the column ignored the colour would be sigmoid(0), several bars away
            assert rel_l2(np.full_like(out_e[:, :3], 0.5), out_e[:, :3]) > 3 * FWD_BAR[dt][0], (kind, k)
    finally:
        with torch.no_grad():
            ref.p_color2.copy_(p2)
            ref.p_sh.copy_(psh)


def test_view_dependence(dev):
    m, _ = _pair(dev, 'f16', None)
    pts, d1 = _inputs(1000, 5, bad=False)
    _, d2 = _inputs(1000, 6, bad=False)
    p = T(pts, dev)
    s1, r1 = _fwd(m, p, T(d1, dev))
    s2, r2 = _fwd(m, p, T(d2, dev))
    assert torch.equal(s1, s2) and torch.equal(r1[:, 3:], r2[:, 3:])
    assert rel_l2(r1[:, :3].cpu().numpy(), r2[:, :3].cpu().numpy()) > FWD_BAR['f16'][1]


def _bwd(m, pts, dirs, gs, gr, perm=None, feats=None, want_mlp=True, td=1, tc=1):
    from nerfstyle_amd import _lib as L
    M = pts.shape[0]
    dev = pts.device
    gt = torch.zeros(m.table_elems, device=dev)
    gm = torch.zeros(16384, device=dev)
    ws = None
    if perm is not None:
        ws = torch.empty(int(L.lib().nsr_field_backward_workspace_bytes(M, 1)) // 4, device=dev)
    desc = m._desc(1.0)
    st = L.lib().nsr_field_backward_dirs(ctypes.byref(desc), L.p(m._gather_tables()), L.p(m._mlp_flat()), L.p(pts), M, None,
                                         L.p(gs), L.p(gr), L.p(gt), L.p(gm) if want_mlp else None, td, tc, L.p(feats), L.p(perm),
                                         L.p(ws), L.p(dirs), L.stream())
    assert st == 0
    return gt.cpu().numpy().reshape(-1, 2, 2), gm.cpu().numpy()


def _autograd(ref, pts, dirs, gs, gr, dt, table_half):
    for p in ref.parameters():
        p.grad = None
    out, sig = ref(torch.tensor(pts), torch.tensor(dirs), half=dt, table_half=table_half)
    ((sig[:, 0] * torch.tensor(gs)).sum() + (out * torch.tensor(gr)).sum()).backward()
    g = {k: getattr(ref, k).grad.numpy().copy() for k in ('emb_density', 'emb_color', 'p_density', 'p_color1', 'p_color2',
                                                           'p_class', 'p_sh')}
    return g


def _check_blocks(tag, gt, gm, g, dt, nc):
    bar = BWD_BAR[dt]
    blocks = {
        'sh columns [64,16]': (gm[15360:], g['p_sh']),
        'color2 first layer [64,16]': (gm[6144:7168], g['p_color2'][:1024]),
        'color2 rest': (gm[7168:12288], g['p_color2'][1024:]),
        'density net': (gm[0:3072], g['p_density']),
        'color1 net': (gm[3072:6144], g['p_color1']),
        'class net': (gm[12288:15360], g['p_class']),
        'density table': (gt[:, 0, :], g['emb_density']),
        'colour table': (gt[:, 1, :], g['emb_color']),
    }
    errs = {k: rel_l2(a, b) for k, (a, b) in blocks.items()}
    print(tag, dt, {k: '%.2e' % v for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= bar, (tag, k, v)


def _grads(M, nc, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(M) * 1e-2).astype(np.float32), rng.standard_normal((M, 3 + nc)).astype(np.float32)


@pytest.mark.parametrize('dt,table_dtype', [('f16', torch.float32), ('bf16', None)])
@pytest.mark.parametrize('M', [17, 1000])
def test_field_backward_dirs_tracker(dev, dt, table_dtype, M):
    m, ref = _pair(dev, dt, table_dtype)
    pts, dirs = _inputs(M, 30 + M, bad=False)
    pts[0] = [2.5, 0, 0]                                           # one sample outside the box
    gs, gr = _grads(M, 5, 31)
    p, d = T(pts, dev), T(dirs, dev)
    gt, gm = _bwd(m, p, d, T(gs, dev), T(gr, dev))
    g = _autograd(ref, pts, dirs, gs, gr, dt, table_dtype is None)
    _check_blocks('tracker M=%d' % M, gt, gm, g, dt, 5)
    # with saved features
    feats = torch.empty(((M + 15) // 16) * 512, dtype=torch.int32, device=dev)
    _fwd(m, p, d, feats=feats)
    gt2, gm2 = _bwd(m, p, d, T(gs, dev), T(gr, dev), feats=feats)
    _check_blocks('tracker+feats M=%d' % M, gt2, gm2, g, dt, 5)
    # grad_mlp == NULL: the same table gradient (up to the atomics' summation order), no weight gradient
    gt3, gm3 = _bwd(m, p, d, T(gs, dev), T(gr, dev), want_mlp=False)
    assert rel_l2(gt3, gt) <= 1e-5 and not gm3.any()


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_field_backward_dirs_gout_and_colour_only(dev, dt):
    M = 4096
    m, ref = _pair(dev, dt, None)
    pts, dirs = _inputs(M, 40, bad=False)
    gs, gr = _grads(M, 5, 41)
    p, d = T(pts, dev), T(dirs, dev)
    perm = m.sample_order(p)
    feats = torch.empty(((M + 15) // 16) * 512, dtype=torch.int32, device=dev)
    _fwd(m, p, d, perm=perm, feats=feats)
    gt, gm = _bwd(m, p, d, T(gs, dev), T(gr, dev), perm=perm, feats=feats)
    g = _autograd(ref, pts, dirs, gs, gr, dt, True)
    _check_blocks('gradients-out M=%d' % M, gt, gm, g, dt, 5)
    # the tracker path on the same inputs: reported, not gated (nobody has measured it)
    gt_t, gm_t = _bwd(m, p, d, T(gs, dev), T(gr, dev))
    print('tracker against gradients-out, sh block rel-L2:', rel_l2(gm_t[15360:], gm[15360:]))
    # colour-table-only kernel: grad_mlp NULL, density table off -- the colour table gradient of the full call
    gt_c, gm_c = _bwd(m, p, d, T(gs, dev), T(gr, dev), perm=perm, feats=feats, want_mlp=False, td=0, tc=1)
    assert not gm_c.any() and not gt_c[:, 0, :].any()
    assert rel_l2(gt_c[:, 1, :], gt[:, 1, :]) <= 1e-5
    assert rel_l2(gt_c[:, 1, :], g['emb_color']) <= BWD_BAR[dt]


def test_model_forward_backward_and_adam_step(dev):
    """StyleTCNerf(view_dependent=True): forward(pts, dirs) uses dirs, the backward fills the new block, FusedAdam moves it."""
    from nerfstyle_amd.optim import FusedAdam
    m, ref = _pair(dev, 'f16', None)
    M = 1000
    pts, dirs = _inputs(M, 50, bad=False)
    gs, gr = _grads(M, 5, 51)
    p, d = T(pts, dev), T(dirs, dev)
    rgbs, sig = m(p, d)
    _, rgb_abi = _fwd(m, p, d)
    assert torch.equal(rgbs.detach(), rgb_abi)
    assert torch.equal(m(p), sig.detach())                                   # sigma only: no directions needed
    with pytest.raises(ValueError, match='dirs'):
        m.field(p)
    opt = FusedAdam(m, lr=1e-2)
    opt.zero_grad()
    before = m.state_dict()['color2_net.params'].clone()
    ((sig[:, 0] * T(gs, dev)).sum() + (rgbs * T(gr, dev)).sum()).backward()
    g = _autograd(ref, pts, dirs, gs, gr, 'f16', True)
    ga = m.grad_arena.cpu().numpy()
    assert rel_l2(ga[m.table_elems + 15360:], g['p_sh']) <= BWD_BAR['f16']
    opt.step()
    after = m.state_dict()['color2_net.params']
    first_b, first_a = before[:2048].view(64, 32), after[:2048].view(64, 32)
    assert (first_a[:, 16:] != first_b[:, 16:]).float().mean() > 0.9         # the SH columns moved
    assert (first_a[:, :16] != first_b[:, :16]).float().mean() > 0.9
