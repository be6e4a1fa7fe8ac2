"""CPU: the float64 encoder restatement (tests/grid_encode_ref.py) against the C oracle and the PyTorch port, and the
exactness conditions of every exact case that tests/test_gpu_grid_encode_edges.py launches."""
import numpy as np
import pytest
import torch

import grid_encode_ref as G

EXACT = G.exact_cases()


@pytest.mark.parametrize('c', EXACT, ids=lambda c: c.id)
def test_exact_case_conditions(c):
    """all terms dyadic within 24 bits, sum |terms| < 2^24 / 4096 (forward, table backward called twice and into the pre-fill);
    the input gradient with its own unit (1 with align_corners, whose weights are 0 or 1; 2^-8 without)"""
    ref = c.reference(check=True)
    c.conditions(ref)
    x = ref['x']
    assert len(ref['bad']) == (0 if c.B == 1 else min(c.B, 3 if c.B == 257 else 2 if c.B < 257 else 4))
    assert not G.inside(x[ref['bad']]).any() and G.inside(np.delete(x, ref['bad'], axis=0)).all()
    assert np.abs(ref['out']).max() > 0 and np.abs(ref['ge']).max() > 0
    assert np.abs(ref['gi']).max() > 0 or c.B == 1
    if c.emb_half:
        assert np.array_equal(ref['emb'], ref['emb'].astype(np.float16).astype(np.float32))
        r16 = G.round_f16(ref['out'])
        assert np.abs(r16 - ref['out']).max() <= 2.0 ** -9                 # rounds, but nowhere near overflow
    if c.dup:
        assert len(np.unique(x[G.inside(x)], axis=0)) == 8 and c.B == 4096


def test_exact_cases_cover_both_row_branches_with_style():
    """style != 0 reaches the hash xor term and the dense style_mul term with its modulo (a tiled level that holds
    (res + 1)^3 rows, size not a power of two), and the main cross has every C x gridtype x align x style"""
    seen = set()
    for c in EXACT:
        if c.style:
            for lv in G.fill_levels(c.offsets(), c.S, G.H_EXACT, c.gt):
                seen.add('hash' if lv['use_hash'] else ('dense_style' if lv['style_mul'] else 'dense_wrapped'))
                if not lv['use_hash'] and lv['style_mul']:
                    assert lv['size'] & (lv['size'] - 1) and c.style * lv['style_mul'] > lv['size']
    assert seen == {'hash', 'dense_style', 'dense_wrapped'}
    main = {(c.C, c.gridtype, c.align, c.style) for c in EXACT if c.tag == 'main'}
    assert len(main) == 32
    assert {c.L for c in EXACT} >= {1, 2, 16} and {c.B for c in EXACT} >= {1, 255, 256, 257, 4096}


def test_resolutions_match_the_oracle(O):
    for pls, L in ((2.0, 16), (np.sqrt(2.0), 32), (1.45, 16), (O.per_level_scale_from_cfg(), 16)):
        S = G.grid_S(pls)
        assert np.array_equal(np.array(G.resolutions(L, S, 16), np.uint32), O.grid_resolutions(L, float(S), 16))
    assert G.grid_S(2.0) == 1.0 and G.grid_S(np.sqrt(2.0)) == 0.5


_GENERAL = [(C, gridtype, align, style, pls, L) for (C, gridtype, align, style, pls, L) in (
    (2, 'hash', True, 0, 1.45, 16), (2, 'hash', False, 3, 1.45, 16), (1, 'tiled', False, 3, 1.45, 16), (4, 'tiled', True, 5, 2.0, 3),
    (8, 'hash', False, 7, 2.0, 3), (2, 'tiled', False, 1, np.sqrt(2.0), 32), (2, 'hash', True, 3, np.sqrt(2.0), 32))]


@pytest.mark.parametrize('C,gridtype,align,style,pls,L', _GENERAL)
def test_restatement_against_the_c_oracle(O, C, gridtype, align, style, pls, L):
    """rows bit for bit against O.grid_corner_rows; forward and table backward on an fp32 table against
    O.grid_encode_forward / O.grid_encode_backward (fp32 sums: 4e-6 * max|table|, and rel L2 1e-5, the GPU tests' bars), style
    included; rows outside [0, 1] give zeros and no gradient in both."""
    gt = 0 if gridtype == 'hash' else 1
    off = G.offsets_for(L, pls, 16, 14, align)
    S = G.grid_S(pls)
    rng = np.random.default_rng(C + L)
    B = 300
    x = rng.random((B, 3)).astype(np.float32)
    x[:4] = [[1.2, 0.5, 0.5], [0.5, -0.1, 0.5], [0, 0, 0], [1, 1, 1]]
    x[4] = [3 / 16, 0.5, 1.0]
    emb = (rng.random((int(off[-1]), C)) * 2 - 1).astype(np.float32)
    rows_o = O.grid_corner_rows(x, off, pls, 16, gt, align, style).astype(np.int64)               # [L, B, 8]
    ok = G.inside(x)
    for l, lv in enumerate(G.fill_levels(off, S, 16, gt)):
        _, rows, _, _, _ = G.corners(x, lv, align, style)
        assert np.array_equal(rows[ok], rows_o[l][ok]), l
    out = G.forward(x, emb, off, S, 16, gt, align, style)
    out_o = O.grid_encode_forward(x, emb, off, pls, 16, gt, align, style)
    assert np.abs(out - out_o).max() <= 4e-6 and not out[:2].any() and not out_o[:2].any()
    g = rng.standard_normal((B, L * C)).astype(np.float32)
    ge, touched = G.backward(g, x, off, emb.shape[0], C, S, 16, gt, align, style)
    ge_o = O.grid_encode_backward(g, x, off, emb.shape[0], C, pls, 16, gt, align, style)
    assert np.linalg.norm(ge - ge_o) <= 1e-5 * np.linalg.norm(ge_o)
    assert not ge[~touched].any() and not ge_o[~touched].any()
    # the [L, B, C] layout is the same numbers
    out_l = G.forward(x, emb, off, S, 16, gt, align, style, out_blc=0)
    assert np.array_equal(out_l.transpose(1, 0, 2).reshape(B, L * C), out)
    g_l = np.ascontiguousarray(g.reshape(B, L, C).transpose(1, 0, 2))
    assert np.array_equal(G.backward(g_l, x, off, emb.shape[0], C, S, 16, gt, align, style, grad_blc=0)[0], ge)


@pytest.mark.parametrize('C,gridtype,align', [(2, 'hash', True), (4, 'tiled', False), (1, 'hash', False)])
def test_input_gradient_against_float64_autograd(C, gridtype, align):
    """style 0 (the PyTorch port takes none): forward, table gradient and input gradient against float64 autograd"""
    from oracle import torch_port as TP
    gt = 0 if gridtype == 'hash' else 1
    off = G.offsets_for(16, 1.45, 16, 14, align)
    rng = np.random.default_rng(3 + C)
    x = rng.random((200, 3)).astype(np.float32)
    x[0] = [1.0, 0.25, 0.0]
    emb = (rng.random((int(off[-1]), C)) * 2 - 1).astype(np.float32)
    g = rng.standard_normal((200, 16 * C)).astype(np.float32)

    def port(dtype):
        xt = torch.tensor(x, dtype=dtype, requires_grad=True)
        et = torch.tensor(emb, dtype=dtype, requires_grad=True)
        o = TP.grid_encode(xt, et, off, 1.45, 16, align, gt)
        o.backward(torch.tensor(g, dtype=dtype))
        return [t.detach().numpy().astype(np.float64) for t in (o, xt.grad, et.grad)]
    S = G.grid_S(1.45)
    mine = [G.forward(x, emb, off, S, 16, gt, align), G.input_backward(g, x, emb, off, S, 16, gt, align),
            G.backward(g, x, off, emb.shape[0], C, S, 16, gt, align)[0]]
    # The float64 port forms position, cell and fraction in float64; the restatement, as the kernel, in fp32 and only the rest
    # in float64.  The rule of test_gpu_grid_input_grad.py: its error against the float64 port is at most 4 x the error of the
    # same port run in float32 (same fp32 cells and fractions, fp32 sums on top).
    for name, m, r64, r32 in zip(('forward', 'input gradient', 'table gradient'), mine, port(torch.float64), port(torch.float32)):
        e_mine, e_f32 = np.linalg.norm(m - r64) / np.linalg.norm(r64), np.linalg.norm(r32 - r64) / np.linalg.norm(r64)
        assert 0 < e_f32 and e_mine <= 4 * e_f32, (name, e_mine, e_f32)


def test_exact_lattice_reference_equals_the_c_oracle_bit_for_bit(O):
    """on the exact operands the C oracle's fp32 sums round nothing either: equal bytes, style included"""
    for c in EXACT[5:32:9] + [c for c in EXACT if c.tag in ('L16', 'dup')][:3]:
        ref = c.reference()
        x = np.where(np.isnan(ref['x']), np.float32(2.0), ref['x'])                              # the oracle's stand-in for NaN
        out = G.forward(ref['x'], ref['emb'], ref['off'], c.S, 16, c.gt, c.align, c.style)
        out_o = O.grid_encode_forward(x, ref['emb'], ref['off'], G.PLS_EXACT, 16, c.gt, c.align, c.style)
        assert np.array_equal(out.astype(np.float32), out_o), c.id
        g = ref['grad'] if c.blc else np.ascontiguousarray(ref['grad'].transpose(1, 0, 2).reshape(c.B, -1))
        ge_o = O.grid_encode_backward(g, x, ref['off'], ref['emb'].shape[0], c.C, G.PLS_EXACT, 16, c.gt, c.align, c.style)
        assert np.array_equal(ref['ge'].astype(np.float32), ge_o), c.id
