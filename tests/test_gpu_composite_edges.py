"""GPU parity of the training composite (composite.hip: one wave per ray, one lane per sample, wave scans, carries
between 64-sample trips, ballot early stop) on rays built so that the stop lands on chosen lanes -- helpers.edge_rays:
lane 0, 13, 14, 62, 63, the first lane of the second and third trip, the ray's last sample, never; a ray without
samples, one that ends exactly at M (dropped), slots that no ray owns.  tests/test_oracle_cpu.py proves on the CPU that
the oracle stops where the builder intends and that no transmittance is within 10 % of T_thresh, so the zero patterns
compared here cannot differ by a threshold flip.

Tolerances are those of test_gpu_raymarching.py's composite tests (__expf vs expf, reassociated scans)."""
import numpy as np
import pytest
import torch

from helpers import EDGE_T_THRESH, edge_rays, owned_slots

pytestmark = pytest.mark.gpu

_oracle_cache = {}


def _case(O, C, is_ndc):
    """inputs, seeded output gradients and the oracle's results for them, computed once per (C, is_ndc) and never written"""
    key = (C, is_ndc)
    if key not in _oracle_cache:
        sig, rgb, deltas, rays, M, stop = edge_rays(C, is_ndc)
        N = len(rays)
        rng = np.random.default_rng(100 + C)
        gws, gim = rng.standard_normal(N).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)
        fwd = O.composite_rays_train_forward(sig, rgb, deltas, rays, EDGE_T_THRESH, is_ndc=is_ndc)
        bwd = O.composite_rays_train_backward(gws, gim, sig, rgb, deltas, rays, fwd[0], fwd[2], EDGE_T_THRESH, is_ndc=is_ndc)
        case = dict(sig=sig, rgb=rgb, deltas=deltas, rays=rays, M=M, N=N, gws=gws, gim=gim, fwd=fwd, bwd=bwd,
                    owned=owned_slots(rays, M))
        for v in list(case.values()) + list(fwd) + list(bwd):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle_cache[key] = case
    return _oracle_cache[key]


def T(a, dev):
    return torch.as_tensor(np.array(a), device=dev)          # (a copy: the cached arrays are read-only)


def _check_backward(gs, gr, gs_o, gr_o, owned):
    assert np.isfinite(gs[owned]).all() and np.isfinite(gr[owned]).all()
    assert np.abs(gr[owned] - gr_o[owned]).max() < 5e-5
    assert np.abs(gs[owned] - gs_o[owned]).max() < 1e-4 * max(1.0, np.abs(gs_o).max())
    # the sharp one: exactly the oracle's samples are without a gradient (zero-density prefixes have grad_rgbs == 0 and
    # grad_sigmas != 0, the stopping sample and everything behind it have neither, and so has the dropped ray)
    assert np.array_equal(gs[owned] == 0, gs_o[owned] == 0)
    assert np.array_equal((gr[owned] == 0).all(1), (gr_o[owned] == 0).all(1))
    assert (gs_o[owned] == 0).sum() > 1000 and (gs_o[owned] != 0).sum() > 1000


@pytest.mark.parametrize('is_ndc', [False, True])
@pytest.mark.parametrize('C', [8, 4, 3])
def test_composite_train_edge_rays(O, dev, C, is_ndc):
    """Forward and backward through the Python wrapper.  For C = 8 and 4 a second run hands the colours over one float
    into a larger allocation: not 16-byte aligned, so the launch takes the runtime-C kernel (scalar loads) in place of
    the float4 one, and the two must agree to the bit."""
    from nerfstyle_amd import raymarching as R
    k = _case(O, C, is_ndc)
    ws_o, d_o, im_o = k['fwd']
    gs_o, gr_o = k['bwd']

    def run(misaligned):
        s_t = T(k['sig'], dev).requires_grad_()
        if misaligned:
            buf = torch.zeros(k['M'] * C + 1, device=dev)
            buf[1:] = T(k['rgb'], dev).view(-1)
            r_t = buf[1:].view(k['M'], C).detach()
            assert r_t.is_contiguous() and r_t.data_ptr() % 16 == 4
        else:
            r_t = T(k['rgb'], dev)
            assert r_t.data_ptr() % 16 == 0
        r_t.requires_grad_()
        ws, depth, image = R.composite_rays_train(s_t, r_t, T(k['deltas'], dev), T(k['rays'], dev), EDGE_T_THRESH, is_ndc)
        (ws * T(k['gws'], dev)).sum().add((image * T(k['gim'], dev)).sum()).backward()
        return [x.detach().cpu().numpy() for x in (ws, depth, image, s_t.grad, r_t.grad)]

    res = run(False)
    ws, depth, image, gs, gr = res
    assert np.abs(ws - ws_o).max() < 2e-5
    assert np.abs(image - im_o).max() < 2e-5
    assert np.abs(depth - d_o).max() < 2e-4
    _check_backward(gs, gr, gs_o, gr_o, k['owned'])
    # the dropped ray and the one without samples: exact zeros
    for idx in (k['rays'][-1, 0], k['rays'][k['rays'][:, 2] == 0][0, 0]):
        assert ws[idx] == 0 and depth[idx] == 0 and (image[idx] == 0).all()
    assert ws[k['rays'][-2, 0]] > 0
    if C in (8, 4):
        for a, b in zip(res, run(True)):
            assert np.array_equal(a, b)


def _nan_buffers(M, C, dev, guard=4096):
    gs = torch.full((M + guard,), float('nan'), device=dev)
    gr = torch.full(((M + guard) * C,), float('nan'), device=dev)
    return gs, gr


def _check_nan_prefilled(gs_t, gr_t, gs_o, gr_o, k, C):
    M, owned = k['M'], k['owned']
    gs, gr = gs_t.cpu().numpy(), gr_t.cpu().numpy().reshape(-1, C)
    assert np.isnan(gs[M:]).all() and np.isnan(gr[M:]).all()                          # nothing behind the M samples
    assert np.isnan(gs[:M][~owned]).all() and np.isnan(gr[:M][~owned]).all()          # nothing in a slot no ray owns
    _check_backward(gs[:M], gr[:M], gs_o, gr_o, owned)
    o = k['rays'][-1, 1]                                                               # the dropped ray's slot inside the buffer
    assert gs[o] == 0 and (gr[o] == 0).all()


@pytest.mark.parametrize('C,is_ndc', [(8, False), (8, True), (3, False), (4, True)])
def test_composite_train_backward_into_nan_filled_gradients(O, dev, C, is_ndc):
    """include/nsr.h: grad_sigmas / grad_rgbs need not arrive zeroed.  The Python wrapper zero-fills them anyway, so this
    calls the C ABI the way raymarching.py does, with both pre-filled with NaN: every slot a ray owns comes back finite
    and equal to the oracle (the tails behind an early stop and the dropped ray's slot as zeros), every other slot and
    the guard behind index M are still NaN."""
    from nerfstyle_amd import _lib as L
    k = _case(O, C, is_ndc)
    ws_o, _, im_o = k['fwd']
    gs_t, gr_t = _nan_buffers(k['M'], C, dev)
    ins = [T(k[n], dev) for n in ('gws', 'gim', 'sig', 'rgb', 'deltas', 'rays')] + [T(ws_o, dev), T(im_o, dev)]
    L.check(L.lib().nsr_composite_rays_train_backward(
        L.p(ins[0]), L.p(ins[1]), L.p(ins[2]), L.p(ins[3]), L.p(ins[4]), L.p(ins[5]), int(is_ndc), L.p(ins[6]), L.p(ins[7]),
        k['M'], k['N'], C, EDGE_T_THRESH, L.p(gs_t), L.p(gr_t), L.stream()), 'composite_rays_train_backward')
    torch.cuda.synchronize()
    _check_nan_prefilled(gs_t, gr_t, k['bwd'][0], k['bwd'][1], k, C)


@pytest.mark.parametrize('C', [8, 5])
def test_render_train_backward_into_nan_filled_gradients(O, dev, C):
    """The same for nsr_render_train_backward, whose inputs are the gradients of the epilogue's outputs: rgb_map =
    image[:, :3] + (1 - weights_sum) and classes = image[:, 3:] (renderer.py:229-233), so the oracle's backward takes
    grad_image = [grad_rgb_map, grad_classes] and grad_weights_sum minus the three colour gradients."""
    from nerfstyle_amd import _lib as L
    k = _case(O, C, False)
    ws_o, _, im_o = k['fwd']
    gim, gws = k['gim'], k['gws']
    g_rgb, g_cls = np.ascontiguousarray(gim[:, :3]), np.ascontiguousarray(gim[:, 3:])
    gws_eff = gws - ((gim[:, 0] + gim[:, 1]) + gim[:, 2])
    gs_o, gr_o = O.composite_rays_train_backward(gws_eff, gim, k['sig'], k['rgb'], k['deltas'], k['rays'], ws_o, im_o, EDGE_T_THRESH)
    gs_t, gr_t = _nan_buffers(k['M'], C, dev)
    ins = [T(a, dev) for a in (g_rgb, g_cls, gws, k['sig'], k['rgb'], k['deltas'], k['rays'], ws_o, im_o)]
    L.check(L.lib().nsr_render_train_backward(
        *[L.p(t) for t in ins], k['M'], k['N'], C, EDGE_T_THRESH, L.p(gs_t), L.p(gr_t), L.stream()), 'render_train_backward')
    torch.cuda.synchronize()
    _check_nan_prefilled(gs_t, gr_t, gs_o, gr_o, k, C)
