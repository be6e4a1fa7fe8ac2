"""Host side of the position gradients (nsr_field_density_gradient, nsr_grid_encode_input_backward) and the formula behind
them: both entry points are exported and bound under the unchanged ABI version, their argument checks answer before anything
touches a device, and a NumPy restatement of the forward-mode chain the fused kernel runs -- features and their three tangents
in cell units, the level resolution folded into the first layer's columns, the ReLU mask taken from the value chain, the
clamped exponential of trunc_exp -- equals autograd through the PyTorch restatement of the field in float64."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def _desc(Lv=16):
    from nerfstyle_amd import _lib
    offsets = (np.arange(17, dtype=np.int32) * 4096).copy()
    d = _lib.FieldDesc()
    d.L, d.H, d.S, d.num_classes = Lv, 16, 0.5, 5
    d.table_dtype, d.compute_dtype = _lib.NSR_F16, _lib.NSR_F16
    for i in range(3):
        d.bbox_min[i], d.bbox_size[i] = -2.0, 4.0
    d.density_scale = 1.0
    d.offsets = offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return d, offsets


def test_symbols_resolve_and_abi_is_unchanged(built):
    from nerfstyle_amd import _lib
    so = ctypes.CDLL(built)
    assert hasattr(so, 'nsr_field_density_gradient') and hasattr(so, 'nsr_grid_encode_input_backward')
    assert len(_lib.SIGNATURES['nsr_field_density_gradient'][1]) == 10
    assert len(_lib.SIGNATURES['nsr_grid_encode_input_backward'][1]) == 18
    L = _lib.lib()
    assert L.nsr_abi_version() == 6 and _lib.ABI_VERSION == 6


def test_forward_entry_point_still_rejects_calc_grad_inputs(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    off = (np.arange(17, dtype=np.int32) * 4096).copy()
    offp = off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.nsr_grid_encode_forward(fake, fake, _lib.NSR_F32, offp, fake, 8, 3, 2, 16, 0.5, 16, 1, 0, 1, 0, 1, None) == -2


def test_argument_checks_answer_on_the_host(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    off = (np.arange(17, dtype=np.int32) * 4096).copy()
    offp = off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def grid(B=8, D=3, Lv=16, gi=fake, grad=fake):
        return L.nsr_grid_encode_input_backward(grad, _lib.NSR_F32, fake, fake, _lib.NSR_F32, offp, gi, B, D, 2, Lv, 0.5, 16, 0, 1,
                                                0, 1, None)
    assert grid(B=0) == 0 and grid(B=0, gi=None, D=7) == 0      # empty work is a no-op success, whatever else is passed
    assert grid(gi=None) == -1 and grid(grad=None) == -1         # NSR_ERR_INVALID_ARG
    assert grid(D=2) == -2                                       # NSR_ERR_UNSUPPORTED
    assert grid(Lv=0) == -1 and grid(Lv=33) == -1

    def field(desc, M=8, grads=fake, tables=fake):
        return L.nsr_field_density_gradient(desc, tables, fake, fake, M, None, None, grads, 0, None)
    desc, keep = _desc()
    assert field(None, M=0) == 0 and field(ctypes.byref(desc), M=0, grads=None) == 0
    assert field(None) == -1
    assert field(ctypes.byref(desc), grads=None) == -1
    assert field(ctypes.byref(desc), tables=ctypes.c_void_p(4100)) == -1     # tables: 16-byte rows
    desc8, keep8 = _desc(Lv=8)
    assert field(ctypes.byref(desc8)) == -2                                   # two K=32 halves: 16 levels or nothing


def _forward_mode_numpy(ref, pts):
    """The chain k_field_density_grad runs, float64: (sigma [M], grad [M,3], logit [M])."""
    from oracle import torch_port as TP
    emb = ref.emb_density.detach().numpy().astype(np.float64)
    p = ref.p_density.detach().numpy().astype(np.float64)
    W1, W2 = p[:2048].reshape(64, 32), p[2048:3072].reshape(16, 64)[0]
    S = np.float32(np.log2(ref.pls))
    res = np.array([TP.level_resolution(l, S, ref.min_res) for l in range(16)], np.float64)
    u = ((pts + ref.bound) / (2 * ref.bound) + 1) / 2
    dudx = 1.0 / (2 * (2 * ref.bound))                         # field_unit: 1 / (2 * bbox_size)
    M = pts.shape[0]
    live = np.all((u >= 0) & (u <= 1), axis=1)
    x = np.zeros((M, 32))
    t = np.zeros((3, M, 32))                                   # tangents in cell units (without res_l)
    for l in range(16):
        size = int(ref.offsets[l + 1] - ref.offsets[l])
        pos = u * res[l]
        c = np.minimum(np.floor(pos), res[l] - 1)
        f = pos - c
        ci = torch.from_numpy(c.astype(np.int64))[:, None, :] + TP._CORNERS[None]
        rows = (TP._row_index(ci, int(res[l]), size) + int(ref.offsets[l])).numpy()            # [M, 8]
        v = emb[rows]                                                                          # [M, 8, 2]
        w1 = np.stack([1 - f, f], axis=-1)                                                      # [M, axis, bit]
        for idx in range(8):
            w = w1[:, 0, idx & 1] * w1[:, 1, (idx >> 1) & 1] * w1[:, 2, idx >> 2]
            x[:, 2 * l:2 * l + 2] += w[:, None] * v[:, idx]
        for gd in range(3):
            d0, d1 = [d for d in range(3) if d != gd]
            for j in range(4):
                b0, b1 = j & 1, j >> 1
                w = w1[:, d0, b0] * w1[:, d1, b1]
                left = (b0 << d0) | (b1 << d1)
                t[gd, :, 2 * l:2 * l + 2] += w[:, None] * (v[:, left | (1 << gd)] - v[:, left])
    x[~live] = 0
    t[:, ~live] = 0
    cell = np.repeat(res / res[15], 2)                         # the second image of W1: res_l / res_15 in the columns
    h = x @ W1.T
    logit = np.maximum(h, 0) @ W2
    mask = h > 0                                               # from the VALUE chain
    grad = np.zeros((M, 3))
    for k in range(3):
        dh = (t[k] @ (W1 * cell[None, :]).T) * mask
        grad[:, k] = np.exp(np.clip(logit, -15, 15)) * (dh @ W2) * res[15] * dudx
    return np.exp(logit), grad, logit


@pytest.mark.parametrize('table_scale', [0.5, 200.0])
def test_forward_mode_chain_equals_autograd_in_float64(table_scale):
    from oracle import torch_port as TP
    ref = TP.Field(num_classes=5, table_scale=table_scale).double()
    rng = np.random.default_rng(3)
    pts = rng.random((32, 3)) * 4 - 2
    pts[0] = [2.5, 0.1, 0.2]                                   # outside the box: zero features, zero gradient
    pts[1] = [2.0, 2.0, 2.0]                                   # the box corner: the last cell, frac = 1
    pt = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    sig = ref(pt, sigma_only=True)
    sig.sum().backward()
    s_np, g_np, logit = _forward_mode_numpy(ref, pts)
    assert np.allclose(s_np, sig.detach().numpy()[:, 0], rtol=1e-9, atol=0)
    want = pt.grad.numpy()
    assert np.abs(want).max() > 0 and np.all(want[0] == 0) and np.all(g_np[0] == 0)
    assert np.linalg.norm(g_np - want) <= 1e-9 * np.linalg.norm(want)
    assert np.abs(g_np - want).max() <= 1e-9 * np.abs(want).max()
    if table_scale > 1:                                        # the clamp of trunc_exp's backward is in play, both ways
        assert (logit > 15).any() and (logit < -15).any()
    else:
        assert np.abs(logit).max() < 15
