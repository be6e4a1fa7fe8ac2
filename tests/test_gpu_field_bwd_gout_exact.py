"""The gradients-out ("GOUT") field backward at the edges of its branch-free tile loop.

k_field_bwd_gout runs every 16-sample tile with all 64 lanes active: a lane past the sample count computes on the sample
its clamped index names and every value it could contribute is selected to zero; the wave's last tile requests itself
again as "the next tile"; only the store of the per-sample encoder gradients is masked.  The cases below put the sample
count on every side of those edges and compare, as test_gpu_field_bwd_gout.py does and with its bars, the GOUT path's
gradient arena region by region against the fused run-tracker path (same MFMA operands, another order of the fp32 sums):
tables rel-L2 <= 2e-5, the four MLP blocks 1.73e-6 / 1.59e-6 / 1.51e-6 / 1.52e-6.  Two GOUT calls on the same inputs
must leave the same `gout` words.

Launch geometry (nsr_field_backward): one workgroup per four tiles up to 256 workgroups, a workgroup's tiles split into
four contiguous wave ranges.  So
  * M = 1, 15, 16, 17, 63, 64, 65: one tile per wave, the last one with 1, 15, 16, 1, 15, 16, 1 samples;
  * M = 16 * 1283 + 1: 1 284 tiles = 214 workgroups of six, wave ranges of two tiles: the last wave of the last workgroup
    runs exactly one full tile and then a one-sample tail;
  * M = 16 401 and 49 157: ranges of 2, 2, 1, 0 and of 4, 4, 4, 1 tiles (several full tiles, then the tail);
  * a device-side count strictly inside a tile with a larger capacity M, and a count of 0 (nothing runs, all gradients 0).
From M = 63 on, one sample in eight lies outside the box and one in eight has a NaN coordinate.  Without saved features
the kernel walks the buffers in order, so there the bad samples are put exactly at the head, the middle and the end of full
tiles; with them it walks the permutation, and the test checks from the permutation that bad samples did land on slots
0, 7 and 15 of tiles.  Every third row of the upstream gradients is exactly zero.

Saturated activations: tables scaled so that pre-activations are large -- the colour sigmoids reach exactly 0 or 1 and
the density logit passes trunc_exp's +-15 clamp (both asserted on the forward's outputs) -- bf16 compute, whose range
holds the activations; the gradients must still agree with the tracker's within the same bars."""
import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu

TABLE_BAR = 2e-5
MLP_BAR = {'density_net': 1.73e-6, 'color1_net': 1.59e-6, 'color2_net': 1.51e-6, 'class_net': 1.52e-6}

ONE_FULL_PLUS_ONE = 16 * 1283 + 1
SMALL = (1, 15, 16, 17, 63, 64, 65)
LOOP = (ONE_FULL_PLUS_ONE, 16 * 1024 + 17, 16 * 1024 * 3 + 5)
# (M, compute dtype, classes, table dtype, saved features)
CASES = [(M, 'f16', 5, 'f16', ft) for M in SMALL for ft in (True, False)] + \
        [(ONE_FULL_PLUS_ONE, cd, nc, td, True) for cd in ('f16', 'bf16') for nc in (1, 5, 13) for td in ('f16', 'f32')] + \
        [(ONE_FULL_PLUS_ONE, cd, 5, 'f16', False) for cd in ('f16', 'bf16')] + \
        [(M, cd, 5, 'f16', ft) for M in LOOP[1:] for cd, ft in (('f16', True), ('bf16', True), ('f16', False))]
# (capacity M, device-side count): strictly inside a tile, in a wave's first tile and behind full tiles; and nothing
COUNTS = [(100, 37), (4099, 1000), (ONE_FULL_PLUS_ONE, 16 * 1283 - 9), (16 * 1024 * 3 + 5, 16 * 1024 * 2 + 3), (4099, 0)]

_models = {}


def _model(dev, cd, nc, td):
    """one model per configuration: seeded MLPs as built, tables spread to +-0.5 (mixed ReLU masks, activations in the
    normal range of both 16-bit types)"""
    key = (cd, nc, td)
    if key not in _models:
        from nerfstyle_amd.common import BBox
        from nerfstyle_amd.config import NetworkConfig
        from nerfstyle_amd.style_nerf import StyleTCNerf
        m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), nc, enc_dtype=torch.float32 if td == 'f32' else None,
                        use_dir=False, compute_dtype=torch.float16 if cd == 'f16' else torch.bfloat16)
        g = torch.Generator().manual_seed(4321)
        with torch.no_grad():
            m.arena[:m.table_elems] = torch.rand(m.table_elems, generator=g) - 0.5
        _models[key] = m.to(dev)
    return _models[key]


def _bad_mask(M):
    """(outside the box, NaN): slots 0, 7 and 15 of alternating tiles, and one sample in eight of the rest"""
    i = np.arange(M)
    dead = (i % 8 == 3) & (M >= 63)
    nan = (i % 8 == 6) & (M >= 63)
    if M >= 63:
        for k, slot in enumerate((0, 7, 15)):                # tiles 0, 2, 4 (outside) and 1, 3, 5 (NaN), where they exist
            if 32 * k + slot < M:
                dead[32 * k + slot] = True
                nan[32 * k + slot] = False
            if 32 * k + 16 + slot < M:
                nan[32 * k + 16 + slot] = True
                dead[32 * k + 16 + slot] = False
    return dead, nan


def _inputs(M, nc, dev):
    rng = np.random.default_rng(7000 + M)
    pts = (rng.random((M, 3)) * 3.6 - 1.8).astype(np.float32)
    dead, nan = _bad_mask(M)
    pts[dead, rng.integers(0, 3)] = 2.5                          # outside the +-2 box
    pts[nan, rng.integers(0, 3)] = np.nan
    gs = (rng.standard_normal(M) * 1e-2).astype(np.float32)
    gr = rng.standard_normal((M, 3 + nc)).astype(np.float32)
    zero = np.arange(M) % 3 == 1
    gs[zero] = 0.0
    gr[zero] = 0.0
    return (torch.as_tensor(pts, device=dev), torch.as_tensor(gs, device=dev), torch.as_tensor(gr, device=dev),
            dead | nan)


def _backward(m, xyzs, perm, gs, gr, m_dev=None):
    m.arena.grad = None
    m.grad_arena = None
    sig, rgb = m.field(xyzs, False, m_dev, perm=perm)
    torch.autograd.backward([sig, rgb], [gs, gr])
    return m.arena.grad.detach().cpu().numpy().copy(), sig.detach(), rgb.detach()


def _gout_bits(m, M):
    return m._bwd_ws[:M * 64].view(torch.int32).cpu().numpy().copy()


def _compare(m, tag, g_tracker, g_gout, g_again):
    from nerfstyle_amd.style_nerf import MLP_LAYOUT
    assert np.isfinite(g_tracker).all() and np.isfinite(g_gout).all(), tag
    te = m.table_elems
    figures, failed = [], []
    for e, name in enumerate(('density table', 'colour table')):
        w, g = g_tracker[:te].reshape(m.rows, 2, 2)[:, e], g_gout[:te].reshape(m.rows, 2, 2)[:, e]
        assert float(np.abs(w).sum()) > 0, name
        figures.append((name, rel_l2(g, w), TABLE_BAR))
    for name, off, n in MLP_LAYOUT:
        w, g = g_tracker[te + off: te + off + n], g_gout[te + off: te + off + n]
        assert float(np.abs(w).sum()) > 0, name
        figures.append((name, rel_l2(g, w), MLP_BAR[name]))
    for name, r, bar in figures:
        print('%s | %-13s rel-L2 %.3g (bar %s)' % (tag, name, r, bar))
        if not r <= bar:
            failed.append((name, r, bar))
    assert not failed, failed
    for name, off, n in MLP_LAYOUT:
        assert rel_l2(g_again[te + off: te + off + n], g_gout[te + off: te + off + n]) <= MLP_BAR[name], name


def _run(m, M, xyzs, gs, gr, feats, tag, m_dev=None, count=None):
    """tracker path, GOUT path twice; returns the GOUT path's forward outputs"""
    count = M if count is None else count
    m.save_features = feats
    try:
        perm = m.sample_order(xyzs, m_dev)
        g_tracker, _, _ = _backward(m, xyzs, None, gs, gr, m_dev)
        g_gout, sig, rgb = _backward(m, xyzs, perm, gs, gr, m_dev)
        assert not getattr(m, '_spatial_scatter_unsupported', False)       # the second run did take the GOUT path
        bits1 = _gout_bits(m, M)
        g_again, _, _ = _backward(m, xyzs, perm, gs, gr, m_dev)
        bits2 = _gout_bits(m, M)
    finally:
        m.save_features = True
    if count == 0:
        assert not g_tracker.any() and not g_gout.any(), tag
        return perm, sig, rgb
    _compare(m, tag, g_tracker, g_gout, g_again)
    # rows of samples at or past the count are never written: compare the written ones (all of them without a count)
    rows = perm[:count].cpu().numpy().astype(np.int64) if m_dev is not None else np.arange(M)
    assert np.array_equal(bits1.reshape(M, 64)[rows], bits2.reshape(M, 64)[rows]), 'gout differs between two runs on the same inputs'
    return perm, sig, rgb


@pytest.mark.parametrize('M,cd,nc,td,feats', CASES,
                         ids=['M%d-%s-nc%d-tab%s-%s' % (c[:4] + ('feats' if c[4] else 'gather',)) for c in CASES])
def test_gout_tile_edges(dev, M, cd, nc, td, feats):
    m = _model(dev, cd, nc, td)
    xyzs, gs, gr, bad = _inputs(M, nc, dev)
    perm, _, _ = _run(m, M, xyzs, gs, gr, feats, 'M=%d %s nc=%d tables %s feats=%d' % (M, cd, nc, td, feats))
    if feats and M >= 16 * 1024:
        # where the permutation put the samples outside the box / with a NaN: head, middle and end of tiles among them
        slot = np.nonzero(bad[perm.cpu().numpy().astype(np.int64)])[0]
        slot = slot[slot < (M // 16) * 16] % 16
        assert {0, 7, 15} <= set(slot.tolist())


@pytest.mark.parametrize('M,count', COUNTS, ids=['M%d-count%d' % c for c in COUNTS])
def test_gout_device_count(dev, M, count):
    m = _model(dev, 'f16', 5, 'f16')
    xyzs, gs, gr, _ = _inputs(M, 5, dev)
    m_dev = torch.tensor([count], dtype=torch.int32, device=dev)
    _run(m, M, xyzs, gs, gr, True, 'M=%d count=%d' % (M, count), m_dev=m_dev, count=count)


@pytest.mark.parametrize('M', (65, ONE_FULL_PLUS_ONE))
def test_gout_saturated_activations(dev, M):
    m = _model(dev, 'bf16', 5, 'f16')
    xyzs, gs, gr, _ = _inputs(M, 5, dev)
    te = m.table_elems
    with torch.no_grad():
        saved = m.arena[:te].clone()
        m.arena[:te] = saved * 1e4
    try:
        _, sig, rgb = _run(m, M, xyzs, gs, gr, True, 'saturated M=%d' % M)
    finally:
        with torch.no_grad():
            m.arena[:te] = saved
    col = rgb[:, :3]
    n01 = int(((col == 0) | (col == 1)).sum())
    nclamp = int(((sig > 3.3e6) | (sig < 3.0e-7)).sum())          # |logit| > 15: exp(+-15) = 3.27e6, 3.06e-7
    print('saturated M=%d: %d of %d colours exactly 0 or 1, %d of %d logits past the clamp' % (M, n01, col.numel(), nclamp, M))
    assert n01 > 0 and nclamp > 0
