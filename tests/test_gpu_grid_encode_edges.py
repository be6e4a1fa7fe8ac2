"""GPU: the stand-alone hash-grid encoder entry points (nsr_grid_encode_forward / _backward / _input_backward,
csrc/gridenc.hip) and `GridEncoder` at their edges.

Exact part: lattice probes (tests/grid_encode_ref.py: per_level_scale 2, H 16, inputs on multiples of 1/16, integer tables and
gradients) for which every weight, product and sum is an fp32 number, so forward, table gradient and input gradient must have
the BYTES of the float64 restatement, whatever order the atomics land in.  The conditions are asserted on the CPU in
tests/test_grid_encode_ref_cpu.py for every case used here.  No tolerance appears in this part.

General-valued part: random inputs and tables on a reduced cross of the same axes, plus L = 32; every bar is one the suite
already uses and is cited where it is applied.
"""
import ctypes

import numpy as np
import pytest
import torch

import grid_encode_ref as G
from helpers import rel_l2

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -2


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _offp(off):
    return off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


class Enc:
    """the three entry points for one configuration, on device tensors"""

    def __init__(self, dev, off, C, S, H, gt, align, style, blc):
        self.dev, self.off, self.C, self.L, self.S, self.H, self.gt, self.align, self.style, self.blc = \
            dev, np.ascontiguousarray(off, np.int32), C, len(off) - 1, float(S), H, gt, int(align), style, blc

    def forward(self, x, emb):
        from nerfstyle_amd import _lib as L
        B = x.shape[0]
        out = torch.full((B, self.L * self.C) if self.blc else (self.L, B, self.C), -7.0, dtype=emb.dtype, device=self.dev)
        L.check(L.lib().nsr_grid_encode_forward(L.p(x), L.p(emb), L.dt(emb.dtype), _offp(self.off), L.p(out), B, 3, self.C, self.L,
                                                self.S, self.H, 0, self.gt, self.align, self.style, self.blc, L.stream()), 'forward')
        return out

    def backward(self, grad, x, ge):
        from nerfstyle_amd import _lib as L
        L.check(L.lib().nsr_grid_encode_backward(L.p(grad), L.dt(grad.dtype), L.p(x), _offp(self.off), L.p(ge), x.shape[0], 3, self.C,
                                                 self.L, self.S, self.H, self.gt, self.align, self.style, self.blc, L.stream()),
                'backward')
        return ge

    def input_backward(self, grad, x, emb):
        from nerfstyle_amd import _lib as L
        gi = torch.full((x.shape[0], 3), -7.0, device=self.dev)
        L.check(L.lib().nsr_grid_encode_input_backward(L.p(grad), L.dt(grad.dtype), L.p(x), L.p(emb), L.dt(emb.dtype),
                                                       _offp(self.off), L.p(gi), x.shape[0], 3, self.C, self.L, self.S, self.H,
                                                       self.gt, self.align, self.style, self.blc, L.stream()), 'input_backward')
        return gi


def _f32_bytes(a):
    a32 = np.ascontiguousarray(a, np.float32)
    assert np.array_equal(a32.astype(np.float64), a)                       # the reference is an fp32 number already
    return a32.view(np.uint32)


def _bytes(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ---------------------------------------------------------------------------------------------
# exact lattice probes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.exact_cases(), ids=lambda c: c.id)
def test_exact_lattice_bytes(dev, c):
    ref = c.reference()
    e = Enc(dev, ref['off'], c.C, c.S, G.H_EXACT, c.gt, c.align, c.style, c.blc)
    x = T(ref['x'], dev)
    emb = T(ref['emb'], dev).to(torch.float16 if c.emb_half else torch.float32)
    grad = T(ref['grad'], dev).to(torch.float16 if c.grad_half else torch.float32)
    bad = ref['bad']
    # forward
    out = e.forward(x, emb)
    if c.emb_half:
        assert np.array_equal(_bytes(out), G.round_f16(ref['out']).astype(np.float16).view(np.uint16))
    else:
        assert np.array_equal(_bytes(out), _f32_bytes(ref['out']))
    o = out.float().cpu().numpy()
    o = o.reshape(c.B, c.L, c.C) if c.blc else o.transpose(1, 0, 2)
    assert not o[bad].any() and np.abs(o).max() > 0                        # outside [0, 1] and NaN: zero rows
    # table gradient: into zeros, a second time into the same buffer, and into a pre-filled buffer
    ge = e.backward(grad, x, torch.zeros(emb.shape, device=dev))
    ge_b = _bytes(ge).copy()
    assert np.array_equal(ge_b, _f32_bytes(ref['ge']))
    assert not ge_b[~ref['touched']].any()                                 # rows nobody touched: exactly +0
    assert np.array_equal(_bytes(e.backward(grad, x, ge)), _f32_bytes(2 * ref['ge']))
    pre = e.backward(grad, x, T(ref['pre'], dev))
    assert np.array_equal(_bytes(pre), _f32_bytes(ref['pre'].astype(np.float64) + ref['ge']))
    assert np.array_equal(pre.cpu().numpy()[~ref['touched']], ref['pre'][~ref['touched']])
    # input gradient
    gi = e.input_backward(grad, x, emb)
    assert np.array_equal(_bytes(gi), _f32_bytes(ref['gi']))
    assert not _bytes(gi)[bad].any()
    if bad:
        # no table gradient from the rows outside: the same call without them adds the same bytes
        keep = np.setdiff1d(np.arange(c.B), bad)
        g_blc = ref['grad'].reshape(c.B, c.L, c.C) if c.blc else ref['grad'].transpose(1, 0, 2)
        gk = g_blc[keep]
        gk = np.ascontiguousarray(gk.reshape(len(keep), -1) if c.blc else gk.transpose(1, 0, 2))
        ge2 = e.backward(T(gk, dev).to(grad.dtype), T(ref['x'][keep], dev), torch.zeros(emb.shape, device=dev))
        assert np.array_equal(_bytes(ge2), ge_b)


# ---------------------------------------------------------------------------------------------
# general-valued edges
# ---------------------------------------------------------------------------------------------
SQRT2 = float(np.sqrt(2.0))
# C, gridtype, align, style, f16 table, f16 grad, [B, L*C] layout, per_level_scale, L, log2_hashmap_size
_GENERAL = [
    (2, 'hash', True, 0, False, False, 1, 1.45, 16, 14),
    (1, 'tiled', False, 3, False, False, 0, 1.45, 16, 14),
    (4, 'hash', False, 3, True, False, 1, 1.45, 16, 14),
    (8, 'tiled', True, 3, False, True, 1, 1.45, 16, 13),
    (8, 'hash', True, 0, True, True, 0, 1.45, 16, 13),
    (2, 'hash', False, 3, False, False, 1, SQRT2, 32, 14),
    (2, 'tiled', True, 0, True, False, 1, SQRT2, 32, 14),
    (4, 'tiled', False, 0, False, False, 1, 2.0, 1, 13),
]


def _per_level(ge, ge_ref, off):
    """table backward: rel L2 < 1e-5 and equal zero pattern (test_gpu_field.py::test_grid_encode_half_tables_and_backward),
    per level so that a small coarse level cannot hide behind the mass of the fine ones"""
    worst = 0.0
    for l in range(len(off) - 1):
        a, b = ge[off[l]:off[l + 1]], ge_ref[off[l]:off[l + 1]]
        assert np.linalg.norm(b) > 0, l
        err = rel_l2(a, b)
        worst = max(worst, err)
        assert err < 1e-5, (l, err)
        assert np.array_equal(a == 0, b == 0), l
    return worst


@pytest.mark.parametrize('C,gridtype,align,style,emb_half,grad_half,blc,pls,L,log2', _GENERAL)
def test_general_values_against_the_float64_restatement(dev, C, gridtype, align, style, emb_half, grad_half, blc, pls, L, log2):
    gt = 0 if gridtype == 'hash' else 1
    S = G.grid_S(pls)
    assert L != 32 or S == 0.5
    off = G.offsets_for(L, pls, 16, log2, align)
    rng = np.random.default_rng(40 + C + L)
    B = 1000
    x = rng.random((B, 3)).astype(np.float32)
    x[:8] = [[1.25, 0.5, 0.5], [0.5, -1e-3, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, np.float32(1) + np.float32(2.0 ** -23)],
             [1, 1, 1], [0, 0, 0], [1.0, 0.3, 0.0], [3 / 16, 0.4, 15 / 16]]
    x[B - 1] = [0.5, np.nan, 0.5]
    bad = [0, 1, 2, 3, B - 1]
    emb = (rng.random((int(off[-1]), C)) * 2 - 1).astype(np.float32)
    if emb_half:
        emb = emb.astype(np.float16).astype(np.float32)
    g = rng.standard_normal((B, L, C)).astype(np.float32)
    if grad_half:
        g = g.astype(np.float16).astype(np.float32)
    g = np.ascontiguousarray(g.reshape(B, L * C) if blc else g.transpose(1, 0, 2))
    e = Enc(dev, off, C, S, 16, gt, align, style, blc)
    xd = T(x, dev)
    embd = T(emb, dev).to(torch.float16 if emb_half else torch.float32)
    gd = T(g, dev).to(torch.float16 if grad_half else torch.float32)
    a = (off, S, 16, gt, align, style)
    # forward
    out = e.forward(xd, embd).float().cpu().numpy()
    ref = G.forward(x, emb, *a, out_blc=blc)
    if emb_half:
        # one f16 ulp of the rounded float64 value (test_grid_encode_half_tables_and_backward)
        r16 = G.round_f16(ref)
        d = np.abs(out - r16)
        ulp = np.spacing(np.maximum(np.abs(r16), 2.0 ** -14).astype(np.float16)).astype(np.float32)
        print('forward f16: max error %.3e, %.2e of the values off by one ulp' % (d.max(), (d > 0).mean()))
        assert np.all(d <= ulp)
    else:
        # 4e-6 * max|table| (test_grid_encode_forward_fp32_and_rows; the tables there and here fill [-1, 1])
        print('forward fp32: max abs error %.3e against 4e-6 * %.3f' % (np.abs(out - ref).max(), np.abs(emb).max()))
        assert np.abs(out - ref).max() <= 4e-6 * np.abs(emb).max()
    ob = out.reshape(B, L, C) if blc else out.transpose(1, 0, 2)
    assert not ob[bad].any()
    # table backward
    ge = e.backward(gd, xd, torch.zeros(emb.shape, device=dev)).cpu().numpy()
    ge_ref, touched = G.backward(g, x, off, emb.shape[0], C, *a[1:], grad_blc=blc)
    print('table backward: worst level rel L2 %.3e' % _per_level(ge, ge_ref, off))
    assert not ge[~touched].any()
    # input backward: at most 4 x the error of the float32 restatement (test_gpu_grid_input_grad.py)
    gi = e.input_backward(gd, xd, embd).cpu().numpy()
    ok = np.setdiff1d(np.arange(B), bad)
    gi64 = G.input_backward(g, x, emb, *a, grad_blc=blc)
    gi32 = G.input_backward(g, x, emb, *a, grad_blc=blc, dtype=np.float32)
    e_kernel, e_f32 = rel_l2(gi[ok], gi64[ok]), rel_l2(gi32[ok], gi64[ok])
    print('input backward: kernel %.3e  float32 restatement %.3e' % (e_kernel, e_f32))
    assert not gi[bad].any() and np.linalg.norm(gi64) > 0 and e_f32 > 0
    assert e_kernel <= 4 * e_f32


def test_grid_encoder_under_autocast_backward_takes_f16_gradient(dev):
    """GridEncoder under autocast with a backward: the table is cast to f16, the output is f16 and so the gradient arrives as
    f16 -- the f16-gradient instantiations of the table and input backward.  The table gradient equals, per level to rel L2
    1e-5 with an equal zero pattern (the table-backward bar above), the float64 restatement fed the f16-rounded gradient, and
    the fp32-gradient entry point fed the same rounded values; the input gradient keeps the 4 x float32-restatement rule."""
    from nerfstyle_amd.gridencoder import GridEncoder
    C, L, pls = 2, 16, 1.45
    enc = GridEncoder(3, L, C, pls, 16, 14, gridtype='hash', align_corners=False)
    off = enc.offsets.numpy().astype(np.int32).copy()
    assert np.array_equal(off, G.offsets_for(L, pls, 16, 14, False))
    rng = np.random.default_rng(9)
    emb = (rng.random((int(off[-1]), C)) * 2 - 1).astype(np.float16).astype(np.float32)
    B = 1000
    xh = (rng.random((B, 3)) * 2 - 1).astype(np.float32)
    g = rng.standard_normal((B, L * C)).astype(np.float32)
    g16 = g.astype(np.float16).astype(np.float32)
    enc = enc.to(dev)
    with torch.no_grad():
        enc.embeddings.copy_(T(emb, dev))
    xt = T(xh, dev).requires_grad_()
    with torch.autocast('cuda', dtype=torch.float16):
        out = enc(xt)
    assert out.dtype == torch.float16
    out.backward(T(g, dev).to(torch.float16))
    assert enc.embeddings.grad.dtype == torch.float32
    ge = enc.embeddings.grad.cpu().numpy()
    xin = ((xh + np.float32(1)) / np.float32(2)).astype(np.float32)            # GridEncoder.forward, bound = 1
    a = (off, G.grid_S(pls), 16, 0, False, 0)
    ge_ref, touched = G.backward(g16, xin, off, emb.shape[0], C, *a[1:])
    print('autocast table backward: worst level rel L2 %.3e' % _per_level(ge, ge_ref, off))
    assert not ge[~touched].any()
    e = Enc(dev, off, C, a[1], 16, 0, False, 0, 1)
    ge32 = e.backward(T(g16, dev), T(xin, dev), torch.zeros(emb.shape, device=dev)).cpu().numpy()
    _per_level(ge, ge32, off)
    gi64 = G.input_backward(g16, xin, emb, *a) * 0.5                           # d xin / d x = 1 / (2 bound)
    gi32 = G.input_backward(g16, xin, emb, *a, dtype=np.float32) * 0.5
    e_kernel, e_f32 = rel_l2(xt.grad.cpu().numpy(), gi64), rel_l2(gi32, gi64)
    print('autocast input backward: kernel %.3e  float32 restatement %.3e' % (e_kernel, e_f32))
    assert e_f32 > 0 and e_kernel <= 4 * e_f32


def test_error_returns_write_nothing(dev):
    from nerfstyle_amd import _lib as L
    lib = L.lib()
    B, C, Lv = 40, 2, 3
    off = np.ascontiguousarray(np.concatenate([G.offsets_for(Lv, 2.0, 16, 13, False), np.zeros(40, np.int32)]))
    rows = int(off[Lv])
    x = torch.full((B, 3), 0.5, device=dev)
    emb = torch.ones(rows, 4, device=dev)
    grad = torch.ones(B, 33 * 4, device=dev)
    out = torch.full((B, 33 * 4), -7.0, device=dev)
    ge = torch.full((rows, 4), -7.0, device=dev)
    gi = torch.full((B, 3), -7.0, device=dev)
    st = L.stream()

    def fwd(b=B, D=3, c=C, lv=Lv, gt=0, dt=L.NSR_F32):
        return lib.nsr_grid_encode_forward(L.p(x), L.p(emb), dt, _offp(off), L.p(out), b, D, c, lv, 1.0, 16, 0, gt, 0, 0, 1, st)

    def bwd(b=B, D=3, c=C, lv=Lv, gt=0, dt=L.NSR_F32):
        return lib.nsr_grid_encode_backward(L.p(grad), dt, L.p(x), _offp(off), L.p(ge), b, D, c, lv, 1.0, 16, gt, 0, 0, 1, st)

    def ibwd(b=B, D=3, c=C, lv=Lv, gt=0, dt=L.NSR_F32, edt=L.NSR_F32):
        return lib.nsr_grid_encode_input_backward(L.p(grad), dt, L.p(x), L.p(emb), edt, _offp(off), L.p(gi), b, D, c, lv, 1.0, 16, gt,
                                                  0, 0, 1, st)
    for f in (fwd, bwd, ibwd):
        assert f(c=3) == UNSUPPORTED and f(D=2) == UNSUPPORTED and f(dt=L.NSR_BF16) == UNSUPPORTED, f.__name__
        assert f(lv=0) == INVALID and f(lv=33) == INVALID and f(gt=2) == INVALID, f.__name__
        assert f(b=0) == OK
    assert ibwd(edt=L.NSR_BF16) == UNSUPPORTED
    assert lib.nsr_grid_encode_forward(L.p(x), L.p(emb), L.NSR_F32, _offp(off), L.p(out), B, 3, C, Lv, 1.0, 16, 1, 0, 0, 0, 1,
                                       st) == UNSUPPORTED                    # calc_grad_inputs: no dy_dx buffer here
    assert lib.nsr_grid_encode_forward(None, L.p(emb), L.NSR_F32, _offp(off), L.p(out), B, 3, C, Lv, 1.0, 16, 0, 0, 0, 0, 1,
                                       st) == INVALID
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ge == -7.0).all()) and bool((gi == -7.0).all())
    assert fwd() == OK and bwd() == OK and ibwd() == OK                      # the same calls with valid arguments do write
    torch.cuda.synchronize()
    assert bool((out.reshape(-1)[:B * Lv * C] != -7.0).all()) and bool((gi != -7.0).all()) and bool((ge != -7.0).any())
