"""GPU: the total-variation regulariser (nsr_grid_tv, nerfstyle_amd/tv.py) against the fp64 restatement (tv_ref.py).

The gradient bound is derived, not tuned (tv_ref.Grad.bound): every entry lies within (k + 4) 2^-23 |c scale| A of the
reference, k the number of draws added to the row and A the sum of |difference| over them; where the gradient held values
before the call, their magnitude joins A, because every running sum the atomics round includes them.

The tiny grid (L = 3, H = 4, per_level_scale 2, log2_hashmap_size 9: resolutions 4, 8, 16) is hashed on all three levels with
the 'hash' grid type -- the row function's style axis never fits -- with up to 3, 4 and 13 vertices on a row; level 0 is dense
(a row per vertex) with the 'tiled' type.  Atomic sums of three or more terms depend on their order, so the bit-for-bit
comparison of two calls runs on the dense level 0, and on the hashed one for the rows that at most two draws add to."""
import numpy as np
import pytest
import torch

import tv_ref as T
from test_tv_cpu import TINY

pytestmark = pytest.mark.gpu

OFF = T.grid_offsets(**TINY)
S, H, ROWS = T.grid_S(TINY['per_level_scale']), TINY['base_resolution'], int(OFF[-1])
SEED = 0x1234567855aa
LAM4 = (0.3, 0.7, 0.45, 1.1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lam_of(rf):
    return LAM4[:rf]


@pytest.fixture(scope='module')
def tables():
    """rows of 4 and 2 lanes, random in +-1: {rf: host [ROWS, rf] f32}"""
    rng = np.random.default_rng(11)
    return {rf: rng.uniform(-1, 1, (ROWS, rf)).astype(np.float32) for rf in (4, 2)}


def run(table, dev, lam, n_samples, base=None, **kw):
    """one nsr_grid_tv call into a gradient buffer that holds `base` (zeros by default) -> (host gradient, value or None)"""
    from nerfstyle_amd.tv import grid_tv
    t = torch.from_numpy(table).to(dev)
    g = torch.zeros_like(t) if base is None else torch.from_numpy(base).to(dev)
    v = grid_tv(t, g, lam, OFF, S, H, n_samples=n_samples, seed=kw.pop('seed', SEED), **kw)
    return g.cpu().numpy(), v


def check(got, ref, base=None, what=''):
    """got [ROWS, lanes] against base + ref within the bound on the rows ref touches; every other row keeps base's bits"""
    base = np.zeros_like(got) if base is None else base
    err = np.abs(got[ref.rows].astype(np.float64) - (base[ref.rows].astype(np.float64) + ref.grad))
    bound = ref.bound(base[ref.rows])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print('{}: {} rows, max k {}, worst error / bound {:.3f}, max |grad| {:.3e}'.format(what, len(ref.rows), int(ref.k.max()), worst,
                                                                                        float(np.abs(ref.grad).max())))
    assert (err <= bound).all(), (what, worst)
    other = np.ones(len(got), bool)
    other[ref.rows] = False
    assert np.array_equal(bits(got[other]), bits(base[other])), what
    assert np.abs(ref.grad).max() > 0


# ---- 1. sweep --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rf', [4, 2])
def test_sweep(tables, dev, rf):
    table, lam = tables[rf], lam_of(rf)
    ref = T.gradient(table, OFF, S, H, lam, 8192)
    assert ref.k.sum() == 125 + 729 + 4913 and len(ref.rows) == 102 + 406 + 512
    got, _ = run(table, dev, lam, 8192)
    check(got, ref, what='sweep rf {}'.format(rf))
    # accumulates: onto a random gradient, which stays underneath
    base = np.random.default_rng(12).uniform(-1, 1, table.shape).astype(np.float32)
    got, _ = run(table, dev, lam, 8192, base=base)
    check(got, ref, base, what='sweep onto a filled gradient rf {}'.format(rf))
    assert np.abs(got - base).max() > 1e-4


@pytest.mark.parametrize('rf', [4, 2])
def test_sweep_level0_twice_bit_for_bit(tables, dev, rf):
    table, lam = tables[rf], lam_of(rf)
    # dense level 0 (tiled): one add per address
    ref = T.gradient(table, OFF, S, H, lam, 8192, gridtype=1, level_mask=0b001)
    assert len(ref.rows) == 125 and (ref.k == 1).all()
    a, _ = run(table, dev, lam, 8192, gridtype=1, level_mask=0b001)
    b, _ = run(table, dev, lam, 8192, gridtype=1, level_mask=0b001)
    check(a, ref, what='dense level 0')
    assert np.array_equal(bits(a), bits(b))
    # hashed level 0: two terms added to zero commute exactly; the rows with three may differ in the last bit
    ref = T.gradient(table, OFF, S, H, lam, 8192, level_mask=0b001)
    a, _ = run(table, dev, lam, 8192, level_mask=0b001)
    b, _ = run(table, dev, lam, 8192, level_mask=0b001)
    check(a, ref, what='hashed level 0')
    few = np.ones(ROWS, bool)
    few[ref.rows[ref.k > 2]] = False
    assert np.array_equal(bits(a[few]), bits(b[few])) and (ref.k <= 2).sum() >= 100


# ---- 2. sampled ------------------------------------------------------------------------------------------------------------------
# n_samples = 1000: levels 0 and 1 (125 and 729 vertices) still sweep and level 2 draws; 500: level 0 sweeps, levels 1 and 2 draw
@pytest.mark.parametrize('rf,n', [(4, 1000), (2, 1000), (4, 500), (2, 500)])
def test_sampled(tables, dev, rf, n):
    from nerfstyle_amd.tv import grid_tv
    table, lam = tables[rf], lam_of(rf)
    lvs = T.levels(OFF, S, H)
    assert [T.draws(lv, l, n)[1] for l, lv in enumerate(lvs)] == [True, n >= 729, False]
    ref0 = T.gradient(table, OFF, S, H, lam, n, seed=SEED, seq=7)
    got, _ = run(table, dev, lam, n, sequence=7)
    check(got, ref0, what='sampled rf {} n {}'.format(rf, n))
    # another stream draws differently, and as the restatement says
    ref1 = T.gradient(table, OFF, S, H, lam, n, seed=SEED, seq=7, stream_id=1)
    assert not np.array_equal(ref1.rows, ref0.rows)
    got1, _ = run(table, dev, lam, n, sequence=7, stream_id=1)
    check(got1, ref1, what='sampled, stream 1')
    assert not np.array_equal(bits(got1), bits(got))
    # two calls with advance: the host sequence plus the device word, which moves on after each call
    t = torch.from_numpy(table).to(dev)
    g = torch.zeros_like(t)
    seq_dev = torch.tensor([40], dtype=torch.int32, device=dev)
    for _ in range(2):
        grid_tv(t, g, lam, OFF, S, H, n_samples=n, seed=SEED, sequence=3, sequence_dev=seq_dev, advance=True)
    both = T.add(T.gradient(table, OFF, S, H, lam, n, seed=SEED, seq=43), T.gradient(table, OFF, S, H, lam, n, seed=SEED, seq=44))
    check(g.cpu().numpy(), both, what='two advancing calls')
    assert int(seq_dev.item()) == 42


# ---- 3. lanes and levels ---------------------------------------------------------------------------------------------------------
def test_zero_lambda_lanes_keep_their_bits(tables, dev):
    table, lam = tables[4], (0.3, 0.3, 0.0, 0.0)
    base = np.random.default_rng(13).uniform(-1, 1, table.shape).astype(np.float32)
    base[5, 2], base[6, 3] = np.float32('nan'), np.float32(-0.0)
    got, _ = run(table, dev, lam, 1000, base=base)
    assert np.array_equal(bits(got[:, 2:]), bits(base[:, 2:]))
    ref = T.gradient(table, OFF, S, H, lam, 1000, seed=SEED)
    assert not ref.grad[:, 2:].any()
    base[:, 2:] = got[:, 2:] = 0                                      # (NaN would fail the comparison of the other lanes' rows)
    check(got, ref, base, what='density lanes only')


def test_level_mask(tables, dev):
    table, lam = tables[4], LAM4
    base = np.random.default_rng(14).uniform(-1, 1, table.shape).astype(np.float32)
    got, _ = run(table, dev, lam, 1000, base=base, level_mask=0b010)
    ref = T.gradient(table, OFF, S, H, lam, 1000, level_mask=0b010, seed=SEED)
    assert ref.rows.min() >= OFF[1] and ref.rows.max() < OFF[2]
    check(got, ref, base, what='level 1 only')
    for lo, hi in ((OFF[0], OFF[1]), (OFF[2], OFF[3])):
        assert np.array_equal(bits(got[lo:hi]), bits(base[lo:hi]))


# ---- 4. scale --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rf', [4, 2])
def test_scale(tables, dev, rf):
    table, lam = tables[rf], lam_of(rf)
    got, _ = run(table, dev, lam, 1000, scale=0.5, scale_dev=torch.tensor(1024.0, device=dev))
    ref = T.gradient(table, OFF, S, H, lam, 1000, seed=SEED, scale=512.0)
    check(got, ref, what='scale 0.5 x 1024')
    plain = T.gradient(table, OFF, S, H, lam, 1000, seed=SEED)
    assert np.allclose(ref.grad, 512.0 * plain.grad, rtol=1e-12, atol=0)


# ---- 5. value --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rf,n_samples', [(4, 8192), (4, 1000), (2, 8192), (2, 1000)])
def test_value(tables, dev, rf, n_samples):
    from nerfstyle_amd.tv import grid_tv
    table, lam = tables[rf], (LAM4[0], 0.0, LAM4[2], LAM4[3])[:rf]
    t = torch.from_numpy(table).to(dev)
    g = torch.zeros_like(t)
    v1 = grid_tv(t, g, lam, OFF, S, H, n_samples=n_samples, seed=SEED, level_mask=0b101, want_value=True)
    v2 = grid_tv(t, g, lam, OFF, S, H, n_samples=n_samples, seed=SEED, level_mask=0b101, want_value=True)
    assert v1.dtype == torch.float64 and tuple(v1.shape) == (3, rf) and torch.equal(v1, v2)
    ref, n = T.value(table, OFF, S, H, lam, n_samples, level_mask=0b101, seed=SEED)
    got = v1.cpu().numpy()
    print('value rf {} n {}: worst error / bound {:.3e}'.format(
        rf, n_samples, float((np.abs(got - ref) / np.maximum(n[:, None] * 6 * 2.0 ** -52 * ref, 1e-300)).max())))
    assert (np.abs(got - ref) <= n[:, None] * 6 * 2.0 ** -52 * ref).all()
    assert not got[1].any() and not got[:, 1].any() and (got[0, 0] > 0.1) and (got[2, 0] > 0.1)      # masked level, zero lane
    # with the gradient too, the gradient is what the call without the value gives
    ref_g = T.add(*[T.gradient(table, OFF, S, H, lam, n_samples, level_mask=0b101, seed=SEED)] * 2)
    check(g.cpu().numpy(), ref_g, what='gradient beside the value')
    # value only: a sentinel gradient buffer is never passed, and stays
    sentinel = torch.full_like(t, 7.25)
    v3 = grid_tv(t, None, lam, OFF, S, H, n_samples=n_samples, seed=SEED, level_mask=0b101, want_value=True)
    assert torch.equal(v3, v1) and bool((sentinel == 7.25).all())


# ---- 6. descent ------------------------------------------------------------------------------------------------------------------
def test_descent(tables, dev):
    """twenty steps of t -= lr grad on the exact (swept) gradient: the curvature is at most 2 * 12 * 3 / 125 = 0.58 (twelve
    edge ends per vertex, up to three vertices on a row of level 0), so lr = 1 is far inside 2 / curvature"""
    from nerfstyle_amd.tv import grid_tv
    t = torch.from_numpy(tables[4]).to(dev).clone()
    lam = (1.0, 1.0, 1.0, 1.0)
    last = None
    for step in range(21):
        g = torch.zeros_like(t)
        total = float(grid_tv(t, g, lam, OFF, S, H, n_samples=8192, seed=SEED, want_value=True).sum())
        assert last is None or total < last, (step, total, last)
        last = total
        t -= 1.0 * g
    assert total < 0.5 * float(grid_tv(torch.from_numpy(tables[4]).to(dev), None, lam, OFF, S, H, n_samples=8192, seed=SEED,
                                       want_value=True).sum())


# ---- 7. the model and the encoder ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model(dev):
    from helpers import render_setup
    return render_setup(dev)[0].model


def _model_ref(m, lam4, seq):
    table = m.arena.detach()[:m.table_elems].view(m.rows, 4).cpu().numpy()
    return T.gradient(table, m._offsets_np, m.S, int(m.cfg.pos_enc.min_res), lam4, 4096, seed=0, seq=seq)


def _check_model(m, tv, lam4, lanes):
    rng = np.random.default_rng(15)
    g = m._ensure_grad()
    base = rng.uniform(-1, 1, g.numel()).astype(np.float32)
    base[:m.table_elems].reshape(m.rows, 4)[:, lanes] = 0              # the lanes under test from zero, everything else filled
    g.copy_(torch.from_numpy(base))
    seq = int(tv.sequence_dev.item())
    tv.add_grad()
    assert int(tv.sequence_dev.item()) == seq + 1 and m.arena.grad.data_ptr() == g.data_ptr()
    got = g.cpu().numpy()
    ref = _model_ref(m, lam4, seq)
    assert len(ref.rows) > 16 * 3000 and ref.rows.max() >= m._offsets_np[15]          # all 16 levels of the real grid
    gt, bt = got[:m.table_elems].reshape(m.rows, 4), base[:m.table_elems].reshape(m.rows, 4)
    other = [k for k in range(4) if k not in lanes]
    assert np.array_equal(bits(gt[:, other]), bits(bt[:, other]))                     # the other table
    assert np.array_equal(bits(got[m.table_elems:]), bits(base[m.table_elems:]))      # the MLP region
    err = np.abs(gt[ref.rows].astype(np.float64) - ref.grad)
    bound = ref.bound()
    print('model lanes {}: {} rows, worst error / bound {:.3f}'.format(lanes, len(ref.rows), float((err / np.maximum(bound, 1e-300))[:, lanes].max())))
    assert (err <= bound)[:, lanes].all() and np.abs(ref.grad[:, lanes]).max() > 0
    untouched = np.ones(m.rows, bool)
    untouched[ref.rows] = False
    assert not gt[untouched][:, lanes].any()
    g.zero_()


def test_model_density(model, dev):
    from nerfstyle_amd.tv import TVRegulariser
    _check_model(model, TVRegulariser(model, lambda_density=1e-3, n_samples=4096), (1e-3, 1e-3, 0.0, 0.0), [0, 1])


def test_model_color(model, dev):
    from nerfstyle_amd.tv import TVRegulariser
    _check_model(model, TVRegulariser(model, lambda_color=1e-3, n_samples=4096), (0.0, 0.0, 1e-3, 1e-3), [2, 3])


def test_model_untrained_table_raises(model):
    from nerfstyle_amd.tv import TVRegulariser
    try:
        model.train_density_table = False
        with pytest.raises(ValueError, match='train_density_table'):
            TVRegulariser(model, lambda_density=1e-3, n_samples=4096)
        TVRegulariser(model, lambda_color=1e-3, n_samples=4096)                        # the trained table is fine
        model.train_density_table, model.train_color_table = True, False
        with pytest.raises(ValueError, match='train_color_table'):
            TVRegulariser(model, lambda_color=1e-3, n_samples=4096)
    finally:
        model.train_density_table = model.train_color_table = True


def _encoder(dev, seed):
    from nerfstyle_amd.gridencoder import GridEncoder
    enc = GridEncoder(level_dim=2, **TINY).to(dev)
    assert list(enc.offsets.cpu().numpy()) == list(OFF)
    table = np.random.default_rng(seed).uniform(-1, 1, (ROWS, 2)).astype(np.float32)
    with torch.no_grad():
        enc.embeddings.copy_(torch.from_numpy(table))
    return enc, table


def test_encoder_grad_total_variation(dev):
    enc, table = _encoder(dev, 16)
    assert enc.embeddings.grad is None
    enc.grad_total_variation(0.25, n_samples=1000, seed=5)
    assert enc.embeddings.grad.dtype == torch.float32
    ref = T.gradient(table, OFF, S, H, (0.25, 0.25), 1000, seed=5, seq=0)
    check(enc.embeddings.grad.cpu().numpy(), ref, what='encoder, first call')
    enc.grad_total_variation(0.25, n_samples=1000, seed=5)                             # draws afresh, accumulates
    check(enc.embeddings.grad.cpu().numpy(), T.add(ref, T.gradient(table, OFF, S, H, (0.25, 0.25), 1000, seed=5, seq=1)),
          what='encoder, second call')


# ---- 8. capture ------------------------------------------------------------------------------------------------------------------
def test_capture(dev):
    from nerfstyle_amd.tv import TVRegulariser
    enc, table = _encoder(dev, 17)
    tv = TVRegulariser(enc, weight=0.25, n_samples=1000, seed=9)
    scale = torch.tensor(8.0, device=dev)
    tv.add_grad(scale)                                                                 # warm: the code object is loaded, .grad exists
    torch.cuda.synchronize()
    enc.embeddings.grad.zero_()
    before = int(tv.sequence_dev.item())
    assert before == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tv.add_grad(scale)
    torch.cuda.synchronize()
    assert int(tv.sequence_dev.item()) == before and not bool(enc.embeddings.grad.any())     # captured, not run
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert int(tv.sequence_dev.item()) == before + 2
    ref = T.add(*[T.gradient(table, OFF, S, H, (0.25, 0.25), 1000, seed=9, seq=before + i, scale=8.0) for i in range(2)])
    check(enc.embeddings.grad.cpu().numpy(), ref, what='two replays')
