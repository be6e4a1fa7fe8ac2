"""CPU: the operand-exact MLP restatement (tests/mlp_exact_ref.py) and its conditions, for every case that
tests/test_gpu_network_edges.py launches: the exactness conditions hold (asserted inside `reference(check=True)`), and the
restatement equals oracle.torch_port.mlp with float64 autograd -- exactly, the values being small integers.  The two
workgroup-cap cases (M = 16 * 65536 + 17) run the conditions only: the same code, checked against the oracle at the other
sizes, restated over 2^20 samples."""
import numpy as np
import pytest
import torch

import mlp_exact_ref as R

SMALL = R.exact_cases() + R.sigmoid_cases() + R.module_cases()


def _torch_reference(c, params, x, dy):
    from oracle import torch_port as TP
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    pt = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    y = TP.mlp(xt, pt, c.n_in, c.n_out, c.nh, 64, 'none', half=None)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return y.detach().numpy(), xt.grad.numpy(), pt.grad.numpy()


@pytest.mark.parametrize('c', SMALL, ids=lambda c: c.id)
def test_conditions_and_oracle_agreement(c):
    params = c.weights()
    x, dy = c.inputs()
    assert x.shape == (c.M, c.n_in) and np.abs(x).max() <= 2 and np.abs(dy).max() <= 2
    assert set(np.unique(params)) <= {-1.0, 0.0, 1.0}
    ref = R.reference(params, x, dy, c.n_in, c.nh, c.n_out, dt=c.dt, check=True)
    y, dx, dp = _torch_reference(c, params, x, dy)
    assert np.array_equal(ref['o'], y) and np.array_equal(ref['dx'], dx) and np.array_equal(ref['dparams'], dp)
    assert not ref['dparams'][-(16 - c.n_out) * 64:].any() if c.n_out < 16 else True
    for k in ('o', 'dx', 'dparams'):
        R.f32_bytes(ref[k])                                   # asserts that the cast to fp32 is exact
    if c.M >= 16:
        assert np.abs(ref['dparams']).max() > 0 and np.abs(ref['dx']).max() > 0


@pytest.mark.parametrize('c', SMALL[::9], ids=lambda c: c.id)
def test_padded_rows_do_not_reach_the_reference(c):
    """rows n_out..15 of the last layer set to 1000 (exact in f16 and bf16): same y, dx and unpadded dparams"""
    x, dy = c.inputs()
    a = R.reference(c.weights(), x, dy, c.n_in, c.nh, c.n_out)
    b = R.reference(c.weights(pad_value=1000.0), x, dy, c.n_in, c.nh, c.n_out)
    for k in ('o', 'dx', 'dparams'):
        assert np.array_equal(a[k], b[k])
    assert np.float32(1000.0) == np.float32(np.float16(1000.0)) and torch.tensor(1000.0).bfloat16().float().item() == 1000.0


def test_weight_patterns_are_asymmetric_and_bounded():
    for (dt, n_in, nh) in R.DISPATCH:
        ws = R.split(R.make_weights(5, n_in, nh, 16), n_in, nh)
        for w in ws:
            o, i = w.shape
            n = max(o, i)
            assert (w != 0).sum(1).max() <= (2 if o == 16 else 3) * n // o and (w != 0).sum(0).max() <= 3 * n // i
            assert not np.array_equal(w, np.roll(w, 1, 0)) and not np.array_equal(w, np.roll(w, 1, 1))
            assert not np.array_equal(w[[1, 0] + list(range(2, o))], w)           # two swapped rows are visible
            if o == i:
                assert not np.array_equal(w, w.T)


def test_every_dispatch_case_meets_every_edge():
    cases = R.exact_cases()
    for d in R.DISPATCH:
        mine = [c for c in cases if (c.dt, c.n_in, c.nh) == d]
        assert sorted(c.M for c in mine) == sorted(R.M_EDGES) and {c.n_out for c in mine} == set(R.N_OUTS)
    assert R.M_EDGES[-1] == 16 * 128 + 1 and max(R.M_EDGES) < 5000
    # launch geometry (mlp_launch): 513 samples -> 33 tiles in two workgroups; the cap: 2048 workgroups of 33 tiles, of which
    # the trailing ones start past the last tile
    ntiles = (R.M_LARGE + 15) // 16
    nb = min((ntiles + 31) // 32, 2048)
    per = (ntiles + nb - 1) // nb
    assert ((513 + 15) // 16, ((513 + 15) // 16 + 31) // 32) == (33, 2)
    assert (nb, per) == (2048, 33) and (nb - 1) * per >= ntiles


@pytest.mark.parametrize('c', R.large_cases(), ids=lambda c: c.id)
def test_workgroup_cap_cases_meet_the_conditions(c):
    x, dy = c.inputs()
    assert np.abs(x).max() == 1
    rows = np.abs(dy).sum(1) > 0
    assert 0.5 / 64 < rows.mean() < 1.5 / 64 and rows[(c.M - 1) // 16 * 16:].any()
    ref = R.reference(c.weights(), x, dy, c.n_in, c.nh, c.n_out, dt=c.dt, check=True)
    assert 0 < ref['dparams_abs_max'] < R.ACC_MAX


def test_sigmoid_bar_is_measured_not_chosen():
    c = R.sigmoid_cases()[0]
    x, dy = c.inputs()
    o = R.reference(c.weights(), x, dy, c.n_in, c.nh, c.n_out)['o']
    bar, e32, y64 = R.sigmoid_bar(o)
    assert bar == max(4 * e32, 2.0 ** -23) and 0 <= e32 < 2.0 ** -22
    assert len(np.unique(o)) > 8 and ((y64 > 1e-3) & (y64 < 1 - 1e-3)).sum() > 8      # not all saturated
