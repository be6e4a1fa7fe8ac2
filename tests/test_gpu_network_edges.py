"""GPU: the stand-alone MLP entry points (nsr_mlp_forward / nsr_mlp_backward, csrc/mlp.hip) and `Network` at their edges.

Exact part: operands for which every product and every sum is an exactly representable integer (tests/mlp_exact_ref.py; the
conditions are asserted on the CPU in tests/test_mlp_exact_cpu.py for every case used here), so y, dx and dparams must have the
BYTES of the float64 reference -- no tolerance, whatever order the MFMA, the LDS atomics and the global atomics sum in.  One
misplaced row, column, lane, padding mask or dropped sample changes an integer.

General-valued part: prefix equality in bytes (a tile's columns are independent), and the dispatch cases and the Sigmoid
depths test_gpu_field.py never launches, through test_network_forward_backward's own comparison and bars.  The only bar that
is not an existing one is the sigmoid's, measured as mlp_exact_ref.sigmoid_bar describes.
"""
import numpy as np
import pytest
import torch

import mlp_exact_ref as R
from helpers import rel_l2

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -2
_TDT = {'f16': torch.float16, 'bf16': torch.bfloat16}
_REF = {}


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _cd(dt):
    from nerfstyle_amd import _lib as L
    return L.NSR_F16 if dt == 'f16' else L.NSR_BF16


def _forward(dev, c, params, x, act=0):
    from nerfstyle_amd import _lib as L
    y = torch.full((x.shape[0], c.n_out), -7.0, device=dev)
    L.check(L.lib().nsr_mlp_forward(L.p(x), L.p(params), x.shape[0], c.n_in, c.n_out, 64, c.nh, act, _cd(c.dt), L.p(y), L.stream()),
            'mlp_forward')
    return y


def _backward(dev, c, params, x, dy, dx=True, dparams=None, act=0):
    """dparams: None -> NULL, else the tensor accumulated into"""
    from nerfstyle_amd import _lib as L
    gx = torch.full_like(x, -7.0) if dx else None
    L.check(L.lib().nsr_mlp_backward(L.p(x), L.p(params), None, L.p(dy), x.shape[0], c.n_in, c.n_out, 64, c.nh, act, _cd(c.dt),
                                     L.p(gx), L.p(dparams), L.stream()), 'mlp_backward')
    return gx


def _bytes(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _reference(c):
    """computed once per case, shared, read-only"""
    key = (c.id, c.seed)
    if key not in _REF:
        x, dy = c.inputs()
        p = c.weights()
        _REF[key] = (p, x, dy, R.reference(p, x, dy, c.n_in, c.nh, c.n_out))
    return _REF[key]


# ---------------------------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.exact_cases(), ids=lambda c: c.id)
def test_exact_bytes_all_dispatch_cases_and_tile_edges(dev, c):
    """y, dx, dparams == float64 reference, in bytes; padded rows; optional outputs; accumulation."""
    p, x, dy, ref = _reference(c)
    pt, xt, dyt = T(p, dev), T(x, dev), T(dy, dev)
    y = _forward(dev, c, pt, xt)
    dp = torch.zeros_like(pt)
    dx = _backward(dev, c, pt, xt, dyt, dparams=dp)
    y_b, dx_b, dp_b = _bytes(y), _bytes(dx), _bytes(dp)
    assert np.array_equal(y_b, R.f32_bytes(ref['o']))
    assert np.array_equal(dx_b, R.f32_bytes(ref['dx']))
    assert np.array_equal(dp_b, R.f32_bytes(ref['dparams']))
    if c.n_out < 16:
        assert not dp_b[-(16 - c.n_out) * 64:].any()                       # padded rows: exactly +0
    # padded rows of the last layer hold 1000 (exact in both compute types): nothing of them reaches any output
    if c.n_out < 16:
        pp = T(c.weights(pad_value=1000.0), dev)
        assert np.array_equal(_bytes(_forward(dev, c, pp, xt)), y_b)
        dp2 = torch.zeros_like(pt)
        assert np.array_equal(_bytes(_backward(dev, c, pp, xt, dyt, dparams=dp2)), dx_b)
        assert np.array_equal(_bytes(dp2), dp_b)                           # the padded part included: it stays zero
    # optional outputs
    dp3 = torch.zeros_like(pt)
    assert _backward(dev, c, pt, xt, dyt, dx=False, dparams=dp3) is None
    assert np.array_equal(_bytes(dp3), dp_b)
    assert np.array_equal(_bytes(_backward(dev, c, pt, xt, dyt, dparams=None)), dx_b)
    # accumulation: a second backward doubles the integers; a pre-filled buffer keeps its contents
    _backward(dev, c, pt, xt, dyt, dparams=dp)
    assert np.array_equal(_bytes(dp), R.f32_bytes(2 * ref['dparams']))
    pre = np.random.default_rng(c.seed).integers(-3, 4, p.shape).astype(np.float32)
    dp4 = T(pre, dev)
    _backward(dev, c, pt, xt, dyt, dparams=dp4)
    assert np.array_equal(_bytes(dp4), R.f32_bytes(pre.astype(np.float64) + ref['dparams']))


@pytest.mark.parametrize('c', R.large_cases(), ids=lambda c: c.id)
def test_exact_bytes_at_the_workgroup_cap(dev, c):
    """M = 16 * 65536 + 17: 2048 workgroups of 33 tiles each, the trailing ones with an empty tile range, a 1-sample tail."""
    p, x, dy, ref = _reference(c)
    pt, xt, dyt = T(p, dev), T(x, dev), T(dy, dev)
    assert np.array_equal(_bytes(_forward(dev, c, pt, xt)), R.f32_bytes(ref['o']))
    dp = torch.zeros_like(pt)
    dx = _backward(dev, c, pt, xt, dyt, dparams=dp)
    assert np.array_equal(_bytes(dx), R.f32_bytes(ref['dx']))
    assert np.array_equal(_bytes(dp), R.f32_bytes(ref['dparams']))
    _REF.pop((c.id, c.seed))                                                          # a few hundred MB: not kept for the session


@pytest.mark.parametrize('c', R.sigmoid_cases(), ids=lambda c: c.id)
def test_sigmoid_of_an_exact_preactivation(dev, c):
    """o is exact, so y - sigmoid64(o) is the error of the device's 1 / (1 + expf(-o)) alone.  Bar: the larger of 4 x the max
    abs error of the same fp32 expression on the CPU (torch) and 2^-23.  Measured on MI355X: see DESIGN.md, "Stand-alone
    encoder and MLP edges"."""
    from nerfstyle_amd import _lib as L
    p, x, dy, ref = _reference(c)
    y = _forward(dev, c, T(p, dev), T(x, dev), act=L.NSR_ACT_SIGMOID).cpu().numpy().astype(np.float64)
    bar, e32, y64 = R.sigmoid_bar(ref['o'])
    err = float(np.abs(y - y64).max())
    print('sigmoid %s: kernel max abs error %.3e, fp32 expression on the CPU %.3e, bar %.3e' % (c.id, err, e32, bar))
    assert err <= bar


# ---------------------------------------------------------------------------------------------
# general-valued edges
# ---------------------------------------------------------------------------------------------
def _network(dev, n_in, n_out, nh, act, dt):
    from nerfstyle_amd.network import Network
    return Network(n_in, n_out, {'otype': 'FullyFusedMLP', 'activation': 'ReLU', 'output_activation': act, 'n_neurons': 64,
                                 'n_hidden_layers': nh}, seed=7, dtype=_TDT[dt]).to(dev)


_PREFIX = [(dt, n_in, nh, 'None') for (dt, n_in, nh) in R.DISPATCH] + [('f16', 32, 1, 'Sigmoid'), ('bf16', 16, 2, 'Sigmoid')]


@pytest.mark.parametrize('dt,n_in,nh,act', _PREFIX)
def test_short_calls_give_the_bytes_of_a_long_one(dev, dt, n_in, nh, act):
    """Random normal inputs, the seeded Xavier parameters of Network: a call with M in {1, 15, 16, 17, 65} returns, for y and
    for dx, the bytes of the 1000-sample call on its first M samples (the columns of a tile are independent)."""
    from nerfstyle_amd import _lib as L
    n_out = 5
    net = _network(dev, n_in, n_out, nh, act, dt)
    c = R.Case(dt, n_in, nh, n_out, 1000, 0)
    a = L.NSR_ACT_SIGMOID if act == 'Sigmoid' else L.NSR_ACT_NONE
    rng = np.random.default_rng(21)
    x = T(rng.standard_normal((1000, n_in)).astype(np.float32), dev)
    dy = T(rng.standard_normal((1000, n_out)).astype(np.float32), dev)
    pt = net.params.detach().contiguous()
    y_long = _forward(dev, c, pt, x, act=a)
    dx_long = _backward(dev, c, pt, x, dy, dparams=None, act=a)
    assert torch.isfinite(y_long).all() and torch.isfinite(dx_long).all() and float(dx_long.abs().sum()) > 0
    for M in (1, 15, 16, 17, 65):
        xs, dys = x[:M].clone(), dy[:M].clone()                             # own allocations: nothing behind row M to read
        assert torch.equal(_forward(dev, c, pt, xs, act=a), y_long[:M]), M
        assert torch.equal(_backward(dev, c, pt, xs, dys, dparams=None, act=a), dx_long[:M]), M


def _mlp_emulated(x, params, n_in, n_out, nh, oa, half):
    """oracle.torch_port.mlp with operand rounding (the restatement test_network_forward_backward uses), statement for
    statement, with one correction: the gradient mask of a hidden unit is taken on the ROUNDED activation, which is the kernels'
    documented rule (mm_relu_mask in csrc/mfma_tiles.h: "forward activation (post-ReLU, rounded) was not > 0"), and the caller
    runs it in float64.  torch_port.mlp lets the gradient through wherever its pre-activation is > 0, also where that rounds
    to zero (below 2^-25 in f16), and in fp32 its own summation error decides what such a unit rounds to.  Sums of 32 products
    of f16 numbers land there now and then: at M = 4099, seed 8, n_in = 32, one hidden layer, unit 56 of sample 4012 is
    1.1e-8 exactly (1.5e-8 or more in an fp32 sum), the kernel rounds it to zero and masks it, and that one sample alone moves
    the rel L2 of dx from 3.0e-4 to 4.485e-3 against torch_port.mlp -- in a float64 CPU emulation of the kernel's roundings
    just as on the MI355X, so it is the restatement that differs there, not the kernel."""
    from oracle import torch_port as TP
    d, p = n_in, 0
    a = TP.quant(x, half)
    for li, (o, i) in enumerate([(64, d)] + [(64, 64)] * (nh - 1) + [(16, 64)]):
        w = TP.quant(params[p:p + o * i].view(o, i), half)
        p += o * i
        a = a @ w.t()
        if li < nh:
            a = TP.quant(torch.relu(a), half)
            a = a * (a.detach() > 0)
    a = a[:, :n_out]
    return torch.sigmoid(a) if oa == 'sigmoid' else a


_UNLAUNCHED = [(32, 5, 2, 'None'), (16, 3, 1, 'None'), (32, 3, 1, 'Sigmoid'), (32, 3, 2, 'Sigmoid')]


@pytest.mark.parametrize('cfg', _UNLAUNCHED)
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
def test_unlaunched_dispatch_cases_and_sigmoid_depths(O, dev, cfg, dt):
    """The comparison and the bars of test_gpu_field.py::test_network_forward_backward (the rounding-emulating restatement and
    the fp32 one; forward 2e-3 / 1e-2 and 5e-3 / 3e-2, backward 4e-3 / 2.5e-2 and 5e-2 / 1.5e-1 for f16 / bf16), at M = 4099,
    for the dispatch cases that test does not launch -- (32, 2 hidden) and (16, 1 hidden) -- and Sigmoid with 1 and 2 hidden
    layers.  This also carries the sigmoid backward, whose dy * sigma' is rounded to the compute type and so is not exact.
    The rounding-emulating restatement takes its gradient mask on the rounded activation: see _mlp_emulated."""
    from oracle import torch_port as TP
    n_in, n_out, nh, act = cfg
    net = _network(dev, n_in, n_out, nh, act, dt)
    rng = np.random.default_rng(8)
    M = 4099
    x = rng.standard_normal((M, n_in)).astype(np.float32)
    p = net.params.detach().cpu().numpy()
    xt = T(x, dev).requires_grad_()
    y = net(xt)
    assert y.shape == (M, n_out)
    oa = 'sigmoid' if act == 'Sigmoid' else 'none'
    yn = y.detach().cpu().numpy()
    e_emul = rel_l2(yn, O.mlp_forward(x, p, n_in, n_out, 64, nh, oa, half=dt))
    e_f32 = rel_l2(yn, O.mlp_forward(x, p, n_in, n_out, 64, nh, oa, half=None))
    print('%s %s forward: emulated %.3e  fp32 %.3e' % (dt, cfg, e_emul, e_f32))
    assert e_emul < (2e-3 if dt == 'f16' else 1e-2)
    assert e_f32 < (5e-3 if dt == 'f16' else 3e-2)
    g = rng.standard_normal(yn.shape).astype(np.float32)
    y.backward(T(g, dev))
    gp = net.params.grad.cpu().numpy()
    for half, tol in ((dt, 4e-3 if dt == 'f16' else 2.5e-2), (None, 5e-2 if dt == 'f16' else 1.5e-1)):
        rdt = torch.float32 if half is None else torch.float64
        xc = torch.tensor(x, dtype=rdt, requires_grad=True)
        pc = torch.tensor(p, dtype=rdt, requires_grad=True)
        if half is None:
            TP.mlp(xc, pc, n_in, n_out, nh, 64, oa, half=None).backward(torch.tensor(g))
        else:
            yc = _mlp_emulated(xc, pc, n_in, n_out, nh, oa, half)
            assert torch.equal(yc.detach(), TP.mlp(xc.detach(), pc.detach(), n_in, n_out, nh, 64, oa, half=half))
            yc.backward(torch.tensor(g, dtype=rdt))
        e_dx, e_dp = rel_l2(xt.grad.cpu().numpy(), xc.grad.numpy()), rel_l2(gp, pc.grad.numpy())
        print('%s %s backward vs %s: dx %.3e  dparams %.3e' % (dt, cfg, half, e_dx, e_dp))
        assert e_dx < tol, (half, 'dx')
        assert e_dp < tol, (half, 'dparams')
    assert np.all(gp.reshape(-1)[-(16 - n_out) * 64:] == 0)


@pytest.mark.parametrize('c', R.module_cases(), ids=lambda c: c.id)
def test_network_autograd_with_one_side_frozen(dev, c):
    """Network through autograd with x.requires_grad = False (dx = NULL) and with params.requires_grad = False
    (dparams = NULL), on the exact operands: the gradient that is asked for has the bytes of the float64 reference."""
    p, x, dy, ref = _reference(c)
    net = _network(dev, c.n_in, c.n_out, c.nh, 'None', c.dt)
    with torch.no_grad():
        net.params.copy_(T(p, dev))
    xt = T(x, dev)
    y = net(xt)
    y.backward(T(dy, dev))
    assert xt.grad is None and np.array_equal(_bytes(y), R.f32_bytes(ref['o']))
    assert np.array_equal(_bytes(net.params.grad), R.f32_bytes(ref['dparams']))
    net.params.grad = None
    net.params.requires_grad_(False)
    xt = T(x, dev).requires_grad_()
    net(xt).backward(T(dy, dev))
    assert net.params.grad is None and np.array_equal(_bytes(xt.grad), R.f32_bytes(ref['dx']))


def test_error_returns_write_nothing(dev):
    from nerfstyle_amd import _lib as L
    lib = L.lib()
    M = 40
    x = torch.ones(M + 1, 64, device=dev)                                   # room for n_in = 64 and an off-alignment view
    p = torch.zeros(64 * 64 * 3 + 32 * 64, device=dev)
    dy = torch.ones(M, 32, device=dev)
    y = torch.full((M, 32), -7.0, device=dev)
    dx = torch.full((M + 1, 64), -7.0, device=dev)
    dp = torch.full_like(p, -7.0)
    st = L.stream()

    def fwd(n_in=32, n_out=5, nn=64, nh=1, act=0, xp=None, m=M):
        return lib.nsr_mlp_forward(xp or L.p(x), L.p(p), m, n_in, n_out, nn, nh, act, L.NSR_F16, L.p(y), st)

    def bwd(n_in=32, n_out=5, nn=64, nh=1, act=0, xp=None, dxp=None, m=M):
        return lib.nsr_mlp_backward(xp or L.p(x), L.p(p), None, L.p(dy), m, n_in, n_out, nn, nh, act, L.NSR_F16, dxp or L.p(dx),
                                    L.p(dp), st)
    for f in (fwd, bwd):
        for kw in ({'n_in': 8}, {'n_in': 64}, {'nn': 128}, {'nh': 0}, {'nh': 3}, {'n_out': 0}, {'n_out': 17}):
            assert f(**kw) == UNSUPPORTED, (f.__name__, kw)
        assert f(act=2) == INVALID and f(act=-1) == INVALID
        assert f(xp=L.p(x) + 4) == INVALID
        assert f(m=0) == OK
    assert bwd(dxp=L.p(dx) + 4) == INVALID
    assert lib.nsr_mlp_forward(None, L.p(p), M, 32, 5, 64, 1, 0, L.NSR_F16, L.p(y), st) == INVALID
    assert lib.nsr_mlp_forward(L.p(x), L.p(p), M, 32, 5, 64, 1, 0, L.NSR_F32, L.p(y), st) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((dx == -7.0).all()) and bool((dp == -7.0).all())
    assert fwd() == OK and bwd() == OK                                      # the same call with valid arguments does write
    torch.cuda.synchronize()
    assert bool((y.reshape(-1)[:M * 5] != -7.0).all()) and bool((dx.reshape(-1)[:M * 32] != -7.0).all())
