"""The gradients-out ("GOUT") field backward against the fused run-tracker backward, region by region.

Every case runs StyleTCNerf forward (saved features) + backward twice on the same parameters and inputs: with a
`nsr_sample_order` permutation (k_field_bwd_gout, whose weight-gradient MFMAs are inline-assembly blocks
on AGPR accumulators, + k_table_scatter) and without (k_field_bwd_tracker: builtin MFMAs only).  Both feed
every MFMA the same operands; what differs is the order of the fp32 sums (the walk order of the samples, and with it
which wave accumulates which tile).  The gradient arena is compared PER REGION, not as one norm:

  * density table, colour table: rel-L2 <= 2e-5, the bar test_gpu_table_scatter_carry.py and test_gpu_field.py use
    for this pair of paths;
  * each of the four MLP blocks (density, color1, color2, class) separately: the bar of a net is 4 x the largest
    rel-L2 the PARENT of the commit that added this file gave for that net over all cases below, capped at 1e-4
    (MLP_BAR; the parent's figures are in DESIGN.md "(r5)").  A re-opened MFMA operand hazard showed as 5e-4 .. 1e-3
    on the weight gradients (DESIGN.md "(r3)"), well above the cap.  Seen to bite: one net's GOUT weight gradient
    scaled by 1 + 1e-3 in a scratch build fails its cases (DESIGN.md "(r5)").

Shapes: M in {1, 17, 16 * 3 + 5, 4099} samples: one tile, a full and a 1-sample tile, a 5-sample tail, many
workgroups.  nsr_field_backward launches one workgroup per four tiles up to 256 workgroups, so up to 16 384 samples a
wave runs at most ONE tile (the prologue alone); the loop edges need more: M = 16 * 1024 + 17 gives waves of 2, 2, 1
and 0 tiles (one loop edge, and the wave without work), M = 16 * 1024 * 3 + 5 waves of 4, 4, 4 and 1 tiles (the
steady state of the input prefetch, which looks two tiles ahead).  From M = 17 on the positions hold one sample
outside the box and one NaN (M = 1 is one live sample); every third row of the upstream gradients is exactly zero.
M = 4099 runs the full product compute dtype x num_classes x table dtype, the other sizes f16 / 5 classes / f16
tables, the largest also bf16.

The per-sample encoder gradients the GOUT kernel writes (its `gout` buffer, the model's backward workspace) must be
bit-identical in two runs on the same inputs: every sample's chain is computed by one lane group in a fixed order.
(The table gradients behind them go through k_table_scatter's float atomics, whose order the public entry does not
fix, so they are not compared bit for bit.)"""
import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu

TABLE_BAR = 2e-5
# 4 x the parent's largest per-net rel-L2 over CASES (4.33e-7, 3.97e-7, 3.78e-7, 3.80e-7; all below the 1e-4 cap)
MLP_BAR = {'density_net': 1.73e-6, 'color1_net': 1.59e-6, 'color2_net': 1.51e-6, 'class_net': 1.52e-6}

SIZES = (1, 17, 16 * 3 + 5, 4099)
LOOP_SIZES = (16 * 1024 + 17, 16 * 1024 * 3 + 5)
CASES = [(M, 'f16', 5, 'f16') for M in SIZES[:-1]] + \
        [(SIZES[-1], cd, nc, td) for cd in ('f16', 'bf16') for nc in (1, 5, 13) for td in ('f16', 'f32')] + \
        [(M, 'f16', 5, 'f16') for M in LOOP_SIZES] + [(LOOP_SIZES[-1], 'bf16', 5, 'f16')]

_models = {}


def _model(dev, cd, nc, td):
    """one model per configuration: seeded MLPs as built, tables spread to +-0.5 so that the ReLU masks are mixed and
    the activations sit in the normal range of both 16-bit types"""
    key = (cd, nc, td)
    if key not in _models:
        from nerfstyle_amd.common import BBox
        from nerfstyle_amd.config import NetworkConfig
        from nerfstyle_amd.style_nerf import StyleTCNerf
        m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), nc, enc_dtype=torch.float32 if td == 'f32' else None,
                        use_dir=False, compute_dtype=torch.float16 if cd == 'f16' else torch.bfloat16)
        g = torch.Generator().manual_seed(1234)
        with torch.no_grad():
            m.arena[:m.table_elems] = torch.rand(m.table_elems, generator=g) - 0.5
        _models[key] = m.to(dev)
    return _models[key]


def _inputs(M, nc, dev):
    rng = np.random.default_rng(1000 + M)
    pts = (rng.random((M, 3)) * 3.6 - 1.8).astype(np.float32)
    if M >= 17:
        pts[3] = [2.5, 0.1, -0.3]                                # outside the +-2 box
        pts[7] = [np.nan, 0.2, 0.4]
    if M > 4096:
        pts[M - 2] = [0.3, -7.0, 0.3]                            # one more of each in the last, partial tile
        pts[M - 1] = [0.1, 0.2, np.nan]
    gs = (rng.standard_normal(M) * 1e-2).astype(np.float32)
    gr = rng.standard_normal((M, 3 + nc)).astype(np.float32)
    zero = np.arange(M) % 3 == 1
    gs[zero] = 0.0
    gr[zero] = 0.0
    return torch.as_tensor(pts, device=dev), torch.as_tensor(gs, device=dev), torch.as_tensor(gr, device=dev)


def _backward(m, xyzs, perm, gs, gr):
    m.arena.grad = None
    m.grad_arena = None
    assert m.save_features
    sig, rgb = m.field(xyzs, False, None, perm=perm)
    torch.autograd.backward([sig, rgb], [gs, gr])
    return m.arena.grad.detach().cpu().numpy().copy()


def _gout_bits(m, M):
    return m._bwd_ws[:M * 64].view(torch.int32).cpu().numpy().copy()


@pytest.mark.parametrize('M,cd,nc,td', CASES, ids=['M%d-%s-nc%d-tab%s' % c for c in CASES])
def test_gout_vs_tracker_per_region(dev, M, cd, nc, td):
    from nerfstyle_amd.style_nerf import MLP_LAYOUT
    m = _model(dev, cd, nc, td)
    xyzs, gs, gr = _inputs(M, nc, dev)
    perm = m.sample_order(xyzs)
    g_tracker = _backward(m, xyzs, None, gs, gr)
    g_gout = _backward(m, xyzs, perm, gs, gr)
    assert not getattr(m, '_spatial_scatter_unsupported', False)       # the second run did take the GOUT path
    bits1 = _gout_bits(m, M)
    g_again = _backward(m, xyzs, perm, gs, gr)
    bits2 = _gout_bits(m, M)
    assert np.isfinite(g_tracker).all() and np.isfinite(g_gout).all()

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
        print('M=%d %s nc=%d tables %s | %-13s rel-L2 %.3g (bar %s)' % (M, cd, nc, td, name, r, bar))
        if not r <= bar:
            failed.append((name, r, bar))
    assert not failed, failed
    # the same weight gradients from the same launch geometry: the second GOUT run may differ from the first only by the
    # order in which the workgroups' atomics land
    for name, off, n in MLP_LAYOUT:
        assert rel_l2(g_again[te + off: te + off + n], g_gout[te + off: te + off + n]) <= MLP_BAR[name], name
    assert np.array_equal(bits1, bits2), 'gout differs between two runs on the same inputs'
