"""GPU: input gradients of the stand-alone hash-grid encoder (nsr_grid_encode_input_backward, GridEncoder on inputs that
require grad).

Reference: autograd of oracle.torch_port.grid_encode in float64 on the same table values.  Bound: the kernel's rel-L2 error
against it is at most 4x the error of the SAME restatement run in float32 (both form the cell and the fraction in fp32 the same
way, so both see the same cells; the factor covers the kernel's different summation order).  Measured on MI355X: see DESIGN.md
"Position gradients".  Rows whose input is outside [0,1] or NaN are exactly zero, and two calls give the same bits (no atomics).
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu

B = 257                    # one 256-thread block and one sample
PLS = 1.45
LOG2_T = 14                # levels 0 and 1 are dense, the others hashed (or wrapped, gridtype 'tiled')
N_BAD = 6                  # leading rows: outside [0,1] or NaN


def _inputs(align):
    rng = np.random.default_rng(17)
    x = rng.random((B, 3)).astype(np.float32)
    x[0] = [1.25, 0.5, 0.5]
    x[1] = [0.5, -1e-3, 0.5]
    x[2] = [0.5, 0.5, np.float32(1.0) + np.float32(2.0 ** -23)]
    x[3] = [np.nan, 0.5, 0.5]
    x[4] = [0.5, 0.5, np.nan]
    x[5] = [-0.0, 2.0, 0.5]
    x[6] = [1.0, 1.0, 1.0]                       # exactly 1: the last cell, fraction 1
    x[7] = [1.0, 0.3, 0.0]
    x[8] = [0.0, 0.0, 0.0]
    if align:                                    # on cell faces of level 0 (k / 16 is exact)
        x[9] = [3 / 16, 0.4, 0.6]
        x[10] = [0.4, 7 / 16, 15 / 16]
        x[11] = [5 / 16, 9 / 16, 12 / 16]
    return x


def _reference(x, emb, grad, offsets, align, gt, dtype):
    from oracle import torch_port as TP
    xt = torch.tensor(x[N_BAD:], dtype=dtype, requires_grad=True)
    out = TP.grid_encode(xt, torch.tensor(emb, dtype=dtype), offsets, PLS, base_resolution=16, align_corners=align, gridtype=gt)
    out.backward(torch.tensor(grad[N_BAD:], dtype=dtype))
    return xt.grad.numpy().astype(np.float64)


@pytest.mark.parametrize('align', [True, False])
@pytest.mark.parametrize('gridtype', ['hash', 'tiled'])
@pytest.mark.parametrize('half', [False, True])
@pytest.mark.parametrize('C', [1, 2, 4, 8])
def test_input_gradient_against_float64_autograd(dev, C, half, gridtype, align):
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd.gridencoder import GridEncoder
    enc = GridEncoder(3, 16, C, PLS, 16, LOG2_T, gridtype=gridtype, align_corners=align)
    off = enc.offsets.numpy().astype(np.int32).copy()
    gt = 0 if gridtype == 'hash' else 1
    rng = np.random.default_rng(100 + C)
    emb = (rng.random((int(off[-1]), C)) * 2 - 1).astype(np.float32)
    if half:
        emb = emb.astype(np.float16).astype(np.float32)
    grad = rng.standard_normal((B, 16 * C)).astype(np.float32)
    x = _inputs(align)

    emb_d = torch.tensor(emb, device=dev).to(torch.float16 if half else torch.float32).contiguous()
    x_d, g_d = torch.tensor(x, device=dev), torch.tensor(grad, device=dev)
    S = float(np.float32(np.log2(PLS)))

    def run():
        gi = torch.full((B, 3), 7.0, device=dev)                  # the kernel writes every row
        L.check(L.lib().nsr_grid_encode_input_backward(
            L.p(g_d), L.NSR_F32, L.p(x_d), L.p(emb_d), L.dt(emb_d.dtype), off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            L.p(gi), B, 3, C, 16, S, 16, gt, int(align), 0, 1, L.stream()), 'grid_encode_input_backward')
        return gi
    got, again = run(), run()
    assert torch.equal(got, again)                                # bit-identical: fixed summation order, no atomics
    got = got.cpu().numpy()
    assert np.all(got[:N_BAD] == 0)                               # outside [0,1] and NaN: exactly zero
    ref64 = _reference(x, emb, grad, off, align, gt, torch.float64)
    ref32 = _reference(x, emb, grad, off, align, gt, torch.float32)
    e_kernel, e_f32 = rel_l2(got[N_BAD:], ref64), rel_l2(ref32, ref64)
    print('C=%d half=%d %s align=%d: kernel %.3e  float32 restatement %.3e' % (C, half, gridtype, align, e_kernel, e_f32))
    assert np.linalg.norm(ref64) > 0 and e_f32 > 0
    assert e_kernel <= 4 * e_f32


def test_grid_encoder_module_fills_input_grad(dev):
    """GridEncoder on inputs that require grad: x.grad is the chain rule through forward's (x + bound) / (2 bound), the
    table gradient is what it was, and inputs that do not require grad still take the path without the input gradient."""
    from nerfstyle_amd.gridencoder import GridEncoder
    from oracle import torch_port as TP
    enc = GridEncoder(3, 16, 2, PLS, 16, LOG2_T, gridtype='hash', align_corners=True).to(dev)
    rng = np.random.default_rng(5)
    emb = (rng.random(tuple(enc.embeddings.shape)) * 2 - 1).astype(np.float32)
    with torch.no_grad():
        enc.embeddings.copy_(torch.tensor(emb, device=dev))
    xh = (rng.random((B, 3)) * 2 - 1).astype(np.float32)         # the module's inputs live in [-bound, bound]
    x = torch.tensor(xh, device=dev).requires_grad_()
    enc(x).sum().backward()
    assert x.grad is not None and x.grad.shape == (B, 3) and float(x.grad.abs().sum()) > 0
    ge = enc.embeddings.grad.clone()
    # float32 restatement: the same (x + 1) / 2 and the same fp32 cells as the module, so the two differ by fp32 rounding
    # of sums of 16 x 2 x 4 terms only (a few 1e-7 relative; 1e-4 leaves room for cancellation in the sums)
    xt = torch.tensor(xh, dtype=torch.float32, requires_grad=True)
    TP.grid_encode((xt + 1) / 2, torch.tensor(emb), enc.offsets.cpu().numpy(), PLS, 16, True, 0).sum().backward()
    assert rel_l2(x.grad.cpu().numpy(), xt.grad.numpy()) < 1e-4
    enc.embeddings.grad = None
    x2 = torch.tensor(xh, device=dev)
    enc(x2).sum().backward()
    assert x2.grad is None and torch.equal(enc.embeddings.grad != 0, ge != 0)
    assert rel_l2(enc.embeddings.grad.cpu().numpy(), ge.cpu().numpy()) < 1e-5
