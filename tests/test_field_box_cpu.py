"""CPU: what tests/field_box_ref.py claims about its inputs and references, proved without a GPU -- the conditions the GPU
tests of the per-axis box (test_gpu_field_box.py) and of the derivative kernels' edges (test_gpu_field_derivative_edges.py)
rest on, and the mutations those tests must notice, tried on the float64 restatement of the two kernels."""
import numpy as np
import pytest
import torch

import field_box_ref as FB
from helpers import rel_l2

DG_BAR = {'f16': 5e-3, 'bf16': 3e-2}
XG_BAR_MODEL = 1e-2          # above the position gradient's bar (4x the fp32 restatement's own error: 7e-4 on the odd box)
M_ODD = 4099                 # the sample count the bars of test_field_backward are stated at


@pytest.mark.parametrize('M', [117, 4609])
def test_exact_box_points_are_exact_in_fp32(M):
    xc, xb, dead = FB.exact_points(M)
    ok = FB.exactness_report(M)
    assert ok.shape == (M, 3) and ok.all(), np.argwhere(~ok)[:5]                  # every point, no exception
    uc, ub = FB.unit_f32(xc, FB.CUBE_MIN, FB.CUBE_SIZE), FB.unit_f32(xb, FB.EXACT_MIN, FB.EXACT_SIZE)
    assert np.array_equal(uc.view(np.uint32), ub.view(np.uint32))                 # the encoder input: the same bits
    with np.errstate(invalid='ignore'):
        live = np.all((uc >= 0) & (uc <= 1), axis=1)
    assert np.array_equal(live, ~dead)
    # the promised edge points are all there
    assert np.isnan(xb).any() and np.isposinf(xb).any() and np.isneginf(xb).any()
    fin = np.where(np.isfinite(uc), uc, 0.5)
    for k in range(3):
        assert (fin[:, k] > 1).any() and (fin[:, k] < 0).any() and (uc[live, k] == 0).any() and (uc[live, k] == 1).any()
        assert M < 1000 or ((uc[live, k] > 0) & (uc[live, k] < 0.5)).any()        # the encoded shell below the box
    assert ((uc[live] > 0) & (uc[live] < 0.5)).any()
    mn, mx = np.asarray(FB.EXACT_MIN, np.float32), (np.asarray(FB.EXACT_MIN) + np.asarray(FB.EXACT_SIZE)).astype(np.float32)
    assert (xb == mn[None]).all(axis=1).any() and (xb == mx[None]).all(axis=1).any()
    s = np.flatnonzero(dead) % 16
    assert {0, 7, 15} <= set(s.tolist())


@pytest.mark.parametrize('M', [117, 4609])
def test_exact_reference_gradients_scale_without_rounding(M):
    """grads_box[:, k] * (size_k / 4) == grads_cube[:, k] can hold bit for bit only if neither side leaves the normal range"""
    xc, _, dead = FB.exact_points(M)
    ref = FB.field_ref(5, 0.5)
    for ds in (1.0, 1.5):
        _, g = FB.density_gradient_f64(ref, xc, FB.CUBE_MIN, FB.CUBE_SIZE, ds)
        a = np.abs(g[~dead])
        assert (a > 0).mean() > 0.99
        nz = a[a > 0]
        assert nz.min() > 2.0 ** -126 * 2.0 ** 4 and nz.max() < np.finfo(np.float32).max / 2.0 ** 4
        assert not g[dead].any()


def test_float64_restatement_is_equivariant_and_matches_autograd():
    """the restatement used for the mutations: box at x == cube at x' times 4 / size, and on the cube it is autograd's answer"""
    xc, xb, dead = FB.exact_points(117)
    ref = FB.field_ref(5, 0.5).double()
    s_c, g_c = FB.density_gradient_f64(ref, xc, FB.CUBE_MIN, FB.CUBE_SIZE)
    s_b, g_b = FB.density_gradient_f64(ref, xb, FB.EXACT_MIN, FB.EXACT_SIZE)
    assert np.array_equal(s_c, s_b) and np.array_equal(g_b * (np.asarray(FB.EXACT_SIZE) / 4.0)[None], g_c)
    pt = torch.tensor(xc[~dead].astype(np.float64), requires_grad=True)
    ref(pt, sigma_only=True).sum().backward()
    assert rel_l2(g_c[~dead], pt.grad.numpy()) <= 1e-9
    eg = np.random.default_rng(1).standard_normal((117, 16, 4))
    x_c = FB.position_gradient_f64(ref, xc, eg, FB.CUBE_MIN, FB.CUBE_SIZE)
    x_b = FB.position_gradient_f64(ref, xb, eg, FB.EXACT_MIN, FB.EXACT_SIZE)
    assert np.array_equal(x_b * (np.asarray(FB.EXACT_SIZE) / 4.0)[None], x_c)
    want = FB.position_gradient_ref(ref, xc, eg, ~dead, FB.CUBE_MIN, FB.CUBE_SIZE, False, torch.float64)
    assert rel_l2(x_c[~dead], want) <= 1e-9


@pytest.mark.parametrize('min_res', [16, 2])
def test_odd_box_points_keep_their_cells(min_res):
    """Redraw share: a uniform point has 48 (level, axis) products u * res_l, each within 2^-10 of an integer with probability
    2^-9, so 48 / 512 = 9.4 % of the points are expected to be drawn again (measured 9.4 % and 9.0 %).  A share of 1 % would
    need a window of 2^-13.2, narrower than the 2^-10.4 by which the two sides' u * res can differ at the finest level; the
    window is the property that matters, so it stands, and the share is held to 10.5 %: a builder that rejects more than the
    geometry explains is broken."""
    x, dead, redrawn = FB.odd_points(M_ODD, 0, min_res)
    print('min_res=%d: %d of %d points drawn again (%.1f %%)' % (min_res, redrawn, M_ODD, 100.0 * redrawn / M_ODD))
    assert 0.08 * M_ODD <= redrawn <= 0.105 * M_ODD
    res = FB.resolutions(min_res)
    u32 = FB.unit_f32(x, FB.ODD_MIN, FB.ODD_SIZE)
    with np.errstate(invalid='ignore'):
        live = np.all((u32 >= 0) & (u32 <= 1), axis=1)
    assert np.array_equal(live, ~dead) and dead.sum() >= 9
    u64 = FB.unit_f64(x, FB.ODD_MIN, FB.ODD_SIZE)
    xp = FB.to_cube_f64(x, FB.ODD_MIN, FB.ODD_SIZE)
    u_ref32 = FB.unit_f32(xp.astype(np.float32), FB.CUBE_MIN, FB.CUBE_SIZE)       # what the fp32 reference forms from x'
    c_kernel, c_ref32, c_64 = (FB.cells(u[live], res, d) for u, d in ((u32, np.float32), (u_ref32, np.float32), (u64, np.float64)))
    assert np.array_equal(c_kernel, c_64) and np.array_equal(c_ref32, c_64)
    for k in range(3):
        assert (u32[live, k] == 0).any() and (u32[live, k] == 1).any()


def test_swapped_axis_factors_are_far_outside_the_bars():
    x, dead, _ = FB.odd_points(M_ODD)
    ref = FB.field_ref(5, 1.0)
    f = 4.0 / np.asarray(FB.ODD_SIZE)
    swap = (f[[0, 2, 1]] / f)[None]                                              # y and z factors exchanged
    for dt in ('f16', 'bf16'):
        g = FB.density_gradient_ref(ref, x, ~dead, FB.ODD_MIN, FB.ODD_SIZE, dt, True)
        r = rel_l2(g * swap, g)
        print('density gradient %s: rel-L2 of the swapped reference %.3f (bar %g)' % (dt, r, DG_BAR[dt]))
        assert r > 10 * DG_BAR[dt]
    eg = np.random.default_rng(5).standard_normal((M_ODD, 16, 4)).astype(np.float32)
    w64, w32 = (FB.position_gradient_ref(ref, x, eg, ~dead, FB.ODD_MIN, FB.ODD_SIZE, True, d) for d in (torch.float64, torch.float32))
    bar = 4 * rel_l2(w32, w64)
    assert 0 < bar < XG_BAR_MODEL and rel_l2(w64 * swap, w64) > 10 * bar


@pytest.mark.parametrize('min_res', [16, 2])
def test_every_isolated_level_has_a_gradient_on_each_axis(min_res):
    x, good = FB.edge_points(65)
    ref = FB.field_ref(5, 1.0, min_res)
    emb0 = (ref.emb_density.detach().clone(), ref.emb_color.detach().clone())
    eg = np.random.default_rng(65).standard_normal((65, 16, 4))
    for l in range(16):
        FB.keep_level(ref, emb0, l)
        _, g = FB.density_gradient_f64(ref, x, FB.CUBE_MIN, FB.CUBE_SIZE)
        xg = FB.position_gradient_f64(ref, x, eg, FB.CUBE_MIN, FB.CUBE_SIZE)
        assert np.all(np.abs(g[good]).max(axis=0) > 0) and np.all(np.abs(xg[good]).max(axis=0) > 0), l
        assert not g[~good].any() and not xg[~good].any()


def test_fast_levels_of_the_two_grids():
    """min_res = 2: levels whose size is no power of two next to fast ones, so both instantiations of the row helpers run"""
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig, PosEncConfig
    from nerfstyle_amd.style_nerf import StyleTCNerf
    for min_res in (2, 16):
        m = StyleTCNerf(NetworkConfig(pos_enc=PosEncConfig(min_res=min_res)), BBox.from_radius(2.0), 1)
        fast = FB.fast_levels(m._offsets_np, min_res)
        print('min_res=%d fast_levels=%#06x' % (min_res, fast))
        assert fast != 0 and fast != 0xFFFF
        calls = [all(fast >> l & 1 for l in lv) for lv in ((0, 2, 4, 6), (1, 3, 5, 7), (8, 10, 12, 14), (9, 11, 13, 15))]
        assert any(calls) and not all(calls)                                     # FAST = true and FAST = false calls both


def test_models_of_box_and_cube_share_one_grid():
    """StyleTCNerf derives the level scale from the box's largest side; model_cfg compensates, so that a box model takes the
    cube model's state_dict"""
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.style_nerf import StyleTCNerf
    cube = StyleTCNerf(FB.model_cfg(FB.CUBE_SIZE), BBox.from_radius(2.0), 1)
    for mn, sz in ((FB.EXACT_MIN, FB.EXACT_SIZE), (FB.ODD_MIN, FB.ODD_SIZE)):
        box = StyleTCNerf(FB.model_cfg(sz), BBox(np.asarray(mn), np.asarray(mn) + np.asarray(sz)), 1)
        assert box.S == cube.S and np.array_equal(box._offsets_np, cube._offsets_np)
        d = box._desc()
        assert tuple(d.bbox_min) == tuple(np.float32(mn)) and tuple(d.bbox_size) == tuple(np.float32(sz))


def test_mutations_are_noticed():
    """Each mutation of the restatement is seen by an exact case (the box / cube relation breaks) or leaves a bar."""
    ref = FB.field_ref(5, 1.0).double()
    emb0 = (ref.emb_density.detach().clone(), ref.emb_color.detach().clone())
    xc, xb, dead = FB.exact_points(117)
    xo, dead_o, _ = FB.odd_points(M_ODD)
    xe, good_e = FB.edge_points(65)
    rng = np.random.default_rng(9)
    eg117, ego, ege = (rng.standard_normal((n, 16, 4)) for n in (117, M_ODD, 65))
    ratio = (np.asarray(FB.EXACT_SIZE) / 4.0)[None]
    # the count case: 65 slots, 41 counted, a permutation whose counted part names three slots past the count
    count = 41
    perm = np.arange(65)
    perm[:count] = rng.permutation(count)
    perm[[2, 17, 40]] = [50, 64, 41]
    eg_nan = ege.copy()
    eg_nan[count:] = np.nan
    clean_o_dg = FB.density_gradient_f64(ref, xo, FB.ODD_MIN, FB.ODD_SIZE)[1]
    clean_o_xg = FB.position_gradient_f64(ref, xo, ego, FB.ODD_MIN, FB.ODD_SIZE)
    noticed = {}
    for mut in FB.MUTATIONS:
        exact, bars, who = 0, 0, []
        with torch.no_grad():
            ref.emb_density.copy_(emb0[0])
            ref.emb_color.copy_(emb0[1])
        # exact cases: the kernel is mutated on both sides of the relation
        b = FB.density_gradient_f64(ref, xb, FB.EXACT_MIN, FB.EXACT_SIZE, mut=mut)[1] * ratio
        c = FB.density_gradient_f64(ref, xc, FB.CUBE_MIN, FB.CUBE_SIZE, mut=mut)[1]
        exact += int(not np.array_equal(b, c))
        b = FB.position_gradient_f64(ref, xb, eg117, FB.EXACT_MIN, FB.EXACT_SIZE, mut=mut) * ratio
        c = FB.position_gradient_f64(ref, xc, eg117, FB.CUBE_MIN, FB.CUBE_SIZE, mut=mut)
        exact += int(not np.array_equal(b, c))
        got = FB.position_gradient_f64(ref, xe, eg_nan, FB.CUBE_MIN, FB.CUBE_SIZE, count=count, perm=perm, mut=mut)
        exact += int(bool(np.isnan(got).any() or got[count:].any()))
        # bar cases: the odd box against the unmutated answer
        who.append(('odd box density gradient', rel_l2(FB.density_gradient_f64(ref, xo, FB.ODD_MIN, FB.ODD_SIZE, mut=mut)[1], clean_o_dg),
                    DG_BAR['bf16']))
        who.append(('odd box position gradient', rel_l2(FB.position_gradient_f64(ref, xo, ego, FB.ODD_MIN, FB.ODD_SIZE, mut=mut), clean_o_xg),
                    XG_BAR_MODEL))
        if mut == 'cell_scale_level_x2':
            for l in range(16):
                FB.keep_level(ref, emb0, l)
                w = FB.density_gradient_f64(ref, xe, FB.CUBE_MIN, FB.CUBE_SIZE)[1]
                who.append(('level %d alone, density gradient' % l,
                            rel_l2(FB.density_gradient_f64(ref, xe, FB.CUBE_MIN, FB.CUBE_SIZE, mut=mut)[1], w), DG_BAR['bf16']))
        bars = sum(r > bar for _, r, bar in who)
        noticed[mut] = (exact, bars)
        print('   ' + '; '.join('%s %.3g' % (n, r) for n, r, bar in who if r > bar))
        print('%-22s noticed by %d of 3 exact cases and %d bar cases' % (mut, exact, bars))
        assert exact + bars >= 1, mut
    assert noticed['size0_everywhere'][0] >= 2 and noticed['out_scale_swapped'][0] >= 2 and noticed['min_wrong_axis'][0] >= 2
    assert noticed['perm_bound_dropped'] == (1, 0)
    assert noticed['cell_scale_level_x2'][1] >= 2            # the odd box's density gradient and the isolated level
