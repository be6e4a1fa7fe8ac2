"""GPU: what test_gpu_tv.py leaves unexecuted in csrc/grid_tv.hip, against the same fp64 restatement (tv_ref.py) and under the
same derived bars -- the gradient within tv_ref.Grad.bound with every untouched row keeping its bits (test_gpu_tv.check), the
value within n 6 2^-52 of the reference per (level, lane) and bit-equal between two calls.

  1. rows of 1 and 8 floats: the scalar-load instantiation, and the only one that reads a row as two float4 and uses every
     entry of TvArgs::c.  Every lane has a column and a weight of its own, so a lane computed from another's is far off.
  2. one dense 'tiled' level of resolution 80 (test_tv_cpu.BIG): 531 441 vertices, more than the 2048 x 256 threads the launch
     is capped at, so the sweep and 524 289 draws take the grid-stride loop's second trip, the sweep's 2048 partial sums give
     every thread of the final pass eight, and 65 537 draws (257 blocks) are the first count at which that pass strides.
     These start from a zero gradient: a vertex lost or added twice is worth |c g|, which only a bound without the magnitude
     of earlier contents sees at c = 2 lambda / 531 441 (test_tv_cpu.test_big_level_checks_see_a_lost_wrap).
  3. the sweep/draw switch at n_samples = V and V - 1, several levels of the 'tiled' type in one launch (level 0 a row per
     vertex, the others folded onto fewer rows than vertices), and levels with fewer draws than the launch is sized for.
  4. what the entry point refuses, with real device buffers: the gradient keeps a sentinel."""
import ctypes

import numpy as np
import pytest
import torch

import tv_ref as T
from test_gpu_tv import SEED, bits, check
from test_tv_cpu import BIG, BIG_DRAWS, BIG_LAM, BIG_SEED, BIG_TRIP, BIG_V, TINY, big, big_refs, big_table

pytestmark = pytest.mark.gpu

OFF = T.grid_offsets(**TINY)
S, H, ROWS = T.grid_S(TINY['per_level_scale']), TINY['base_resolution'], int(OFF[-1])
TINY_GRID = (OFF, S, H)
LAM8 = (0.3, 0.7, 0.45, 1.1, 0.9, 0.2, 0.6, 1.3)


def lam_of(rf):
    return LAM8[:rf]


@pytest.fixture(scope='module')
def tables():
    """rows of 1, 8 and 4 lanes, random in +-1: {rf: host [ROWS, rf] f32}"""
    rng = np.random.default_rng(21)
    return {rf: rng.uniform(-1, 1, (ROWS, rf)).astype(np.float32) for rf in (1, 8, 4)}


def filled(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def run(table, dev, lam, n_samples, base=None, grid=TINY_GRID, **kw):
    """one nsr_grid_tv call into a gradient buffer that holds `base` (zeros by default) -> (host gradient, value or None)"""
    from nerfstyle_amd.tv import grid_tv
    t = torch.from_numpy(table).to(dev)
    g = torch.zeros_like(t) if base is None else torch.from_numpy(base).to(dev)
    v = grid_tv(t, g, lam, *grid, n_samples=n_samples, seed=kw.pop('seed', SEED), **kw)
    return g.cpu().numpy(), v


def check_value(got, ref, n, what):
    """got [L, lanes] (device) within n 6 2^-52 ref of the reference; a masked level or a lane without weight is exactly 0"""
    got = got.cpu().numpy()
    bar = n[:, None] * 6 * 2.0 ** -52 * ref
    print('{}: worst error / bound {:.3e}'.format(what, float((np.abs(got - ref) / np.maximum(bar, 1e-300)).max())))
    assert got.dtype == np.float64 and got.shape == ref.shape and (np.abs(got - ref) <= bar).all(), what
    return got


# ---- 1. rows of 1 and 8 floats ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rf', [1, 8])
def test_sweep(tables, dev, rf):
    table, lam = tables[rf], lam_of(rf)
    ref = T.gradient(table, OFF, S, H, lam, 8192)
    assert ref.k.sum() == 125 + 729 + 4913 and len(ref.rows) == 102 + 406 + 512 and ref.grad.shape[1] == rf
    got, _ = run(table, dev, lam, 8192)
    check(got, ref, what='sweep rf {}'.format(rf))
    base = filled(table.shape, 22)
    got, _ = run(table, dev, lam, 8192, base=base)
    check(got, ref, base, what='sweep onto a filled gradient rf {}'.format(rf))
    assert (np.abs(got - base).max(0) > 1e-4).all()                                   # every lane


@pytest.mark.parametrize('rf', [1, 8])
def test_sweep_dense_level0_twice_bit_for_bit(tables, dev, rf):
    table, lam = tables[rf], lam_of(rf)
    ref = T.gradient(table, OFF, S, H, lam, 8192, gridtype=1, level_mask=0b001)
    assert len(ref.rows) == 125 and (ref.k == 1).all()
    a, _ = run(table, dev, lam, 8192, gridtype=1, level_mask=0b001)
    b, _ = run(table, dev, lam, 8192, gridtype=1, level_mask=0b001)
    check(a, ref, what='dense level 0 rf {}'.format(rf))
    assert np.array_equal(bits(a), bits(b))


# n_samples = 1000: levels 0 and 1 sweep and level 2 draws; 500: level 0 sweeps, levels 1 and 2 draw
@pytest.mark.parametrize('rf,n', [(1, 1000), (8, 1000), (1, 500), (8, 500)])
def test_sampled(tables, dev, rf, n):
    from nerfstyle_amd.tv import grid_tv
    table, lam = tables[rf], lam_of(rf)
    assert [T.draws(lv, l, n)[1] for l, lv in enumerate(T.levels(OFF, S, H))] == [True, n >= 729, False]
    ref0 = T.gradient(table, OFF, S, H, lam, n, seed=SEED, seq=7)
    got, _ = run(table, dev, lam, n, sequence=7)
    check(got, ref0, what='sampled rf {} n {}'.format(rf, n))
    ref1 = T.gradient(table, OFF, S, H, lam, n, seed=SEED, seq=7, stream_id=1)
    assert not np.array_equal(ref1.rows, ref0.rows)
    got1, _ = run(table, dev, lam, n, sequence=7, stream_id=1)
    check(got1, ref1, what='sampled rf {} n {}, stream 1'.format(rf, n))
    assert not np.array_equal(bits(got1), bits(got))
    # two calls with advance: the host sequence plus the device word, which moves on after each call
    t = torch.from_numpy(table).to(dev)
    g = torch.zeros_like(t)
    seq_dev = torch.tensor([40], dtype=torch.int32, device=dev)
    for _ in range(2):
        grid_tv(t, g, lam, OFF, S, H, n_samples=n, seed=SEED, sequence=3, sequence_dev=seq_dev, advance=True)
    both = T.add(T.gradient(table, OFF, S, H, lam, n, seed=SEED, seq=43), T.gradient(table, OFF, S, H, lam, n, seed=SEED, seq=44))
    check(g.cpu().numpy(), both, what='two advancing calls rf {} n {}'.format(rf, n))
    assert int(seq_dev.item()) == 42


@pytest.mark.parametrize('rf,n_samples', [(1, 8192), (1, 1000), (8, 8192), (8, 1000)])
def test_value(tables, dev, rf, n_samples):
    """level 1 masked; rf 8 with lane 5 (the second float4) without weight, rf 1 with its only lane on and then off"""
    from nerfstyle_amd.tv import grid_tv
    table = tables[rf]
    lam = LAM8[:5] + (0.0,) + LAM8[6:] if rf == 8 else lam_of(rf)
    t = torch.from_numpy(table).to(dev)
    g = torch.zeros_like(t)
    kw = dict(n_samples=n_samples, seed=SEED, level_mask=0b101, want_value=True)
    v1 = grid_tv(t, g, lam, OFF, S, H, **kw)
    v2 = grid_tv(t, g, lam, OFF, S, H, **kw)
    assert v1.dtype == torch.float64 and tuple(v1.shape) == (3, rf) and torch.equal(v1, v2)
    ref, n = T.value(table, OFF, S, H, lam, n_samples, level_mask=0b101, seed=SEED)
    got = check_value(v1, ref, n, 'value rf {} n {}'.format(rf, n_samples))
    on = [k for k in range(rf) if lam[k]]
    assert not got[1].any() and (got[0, on] > 0.1).all() and (got[2, on] > 0.1).all()
    if rf == 8:
        assert not got[:, 5].any() and len(set(got[0])) == 8                          # no lane reports another's
    # with the gradient too, the gradient is what the call without the value gives
    ref_g = T.add(*[T.gradient(table, OFF, S, H, lam, n_samples, level_mask=0b101, seed=SEED)] * 2)
    check(g.cpu().numpy(), ref_g, what='gradient beside the value rf {} n {}'.format(rf, n_samples))
    # value only
    v3 = grid_tv(t, None, lam, OFF, S, H, **kw)
    assert torch.equal(v3, v1)
    if rf == 1:
        # the only lane without weight: nothing is summed and nothing written, the gradient keeps a NaN and a -0.0
        base = filled(table.shape, 23)
        base[5, 0], base[6, 0] = np.float32('nan'), np.float32(-0.0)
        got_g, v0 = run(table, dev, (0.0,), n_samples, base=base, level_mask=0b101, want_value=True)
        assert not v0.cpu().numpy().any() and np.array_equal(bits(got_g), bits(base))


@pytest.mark.parametrize('rf', [1, 8])
def test_scale(tables, dev, rf):
    table, lam = tables[rf], lam_of(rf)
    got, _ = run(table, dev, lam, 1000, scale=0.5, scale_dev=torch.tensor(1024.0, device=dev))
    ref = T.gradient(table, OFF, S, H, lam, 1000, seed=SEED, scale=512.0)
    check(got, ref, what='scale 0.5 x 1024 rf {}'.format(rf))
    plain = T.gradient(table, OFF, S, H, lam, 1000, seed=SEED)
    assert np.allclose(ref.grad, 512.0 * plain.grad, rtol=1e-12, atol=0)


def test_rf8_zero_lambda_lanes_in_both_halves_keep_their_bits(tables, dev):
    """lanes 3 and 4 off: the last float of the first float4 and the first of the second"""
    table = tables[8]
    lam = LAM8[:3] + (0.0, 0.0) + LAM8[5:]
    ref = T.gradient(table, OFF, S, H, lam, 1000, seed=SEED)
    assert not ref.grad[:, 3:5].any() and (np.abs(ref.grad).max(0)[[0, 1, 2, 5, 6, 7]] > 0).all()
    base = filled(table.shape, 24)
    r0, r1 = int(ref.rows[3]), int(ref.rows[len(ref.rows) // 2])                     # rows the call adds to
    base[r0, 3], base[r0, 4], base[r1, 3], base[r1, 4] = np.float32('nan'), np.float32(-0.0), np.float32(-0.0), np.float32('nan')
    got, _ = run(table, dev, lam, 1000, base=base)
    assert np.array_equal(bits(got[:, 3:5]), bits(base[:, 3:5]))
    base[:, 3:5] = got[:, 3:5] = 0                                    # (NaN would fail the comparison of the other lanes' rows)
    check(got, ref, base, what='rf 8, lanes 3 and 4 off')
    assert not np.isnan(got).any()


@pytest.mark.parametrize('rf', [1, 8])
def test_encoder_grad_total_variation(dev, rf):
    from nerfstyle_amd.gridencoder import GridEncoder
    enc = GridEncoder(level_dim=rf, **TINY).to(dev)
    assert list(enc.offsets.cpu().numpy()) == list(OFF) and tuple(enc.embeddings.shape) == (ROWS, rf)
    table = filled((ROWS, rf), 25)
    with torch.no_grad():
        enc.embeddings.copy_(torch.from_numpy(table))
    assert enc.embeddings.grad is None
    lam = (0.25,) * rf
    enc.grad_total_variation(0.25, n_samples=1000, seed=5)
    assert enc.embeddings.grad.dtype == torch.float32
    ref = T.gradient(table, OFF, S, H, lam, 1000, seed=5, seq=0)
    check(enc.embeddings.grad.cpu().numpy(), ref, what='encoder level_dim {}, first call'.format(rf))
    enc.grad_total_variation(0.25, n_samples=1000, seed=5)                             # draws afresh, accumulates
    check(enc.embeddings.grad.cpu().numpy(), T.add(ref, T.gradient(table, OFF, S, H, lam, 1000, seed=5, seq=1)),
          what='encoder level_dim {}, second call'.format(rf))


# ---- 2. more than one trip of both strided loops ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big_level():
    off, S_, H_, lv = big()
    assert not lv['use_hash'] and T.vertex_count(lv) == BIG_V > BIG_TRIP == 2048 * 256 and lv['size'] >= BIG_V
    table = big_table()
    assert table.shape[1] == 2 and table.nbytes < 5 << 20
    return table, (off, S_, H_), big_refs(table)


def _big_base(table):
    """zeros, but for the level's seven padding rows past the last vertex, which no call may touch"""
    base = np.zeros_like(table)
    base[BIG_V:] = 7.25
    assert 0 < len(base) - BIG_V < 8
    return base


def test_big_sweep_wraps_the_grid(big_level, dev):
    table, grid, refs = big_level
    ref, ref_v, n = refs[BIG_V]
    assert len(ref.rows) == BIG_V and (ref.k == 1).all() and n[0] == BIG_V             # exactly one add for every vertex
    base = _big_base(table)
    kw = dict(base=base, grid=grid, gridtype=1, seed=BIG_SEED, want_value=True)
    a, v1 = run(table, dev, BIG_LAM, BIG_V, **kw)
    b, v2 = run(table, dev, BIG_LAM, BIG_V, **kw)
    check(a, ref, base, what='resolution 80 swept')
    assert np.array_equal(bits(a), bits(b))
    # 2048 partial sums per lane: eight for every thread of the final pass
    check_value(v1, ref_v, n, 'resolution 80 swept, value')
    assert torch.equal(v1, v2) and (ref_v > 0.1).all()


def test_big_sampled_257_blocks(big_level, dev):
    table, grid, refs = big_level
    n_samples = BIG_DRAWS[0]
    ref, ref_v, n = refs[n_samples]
    assert n_samples == 65537 < BIG_V and n[0] == n_samples and ref.k.sum() == n_samples
    base = _big_base(table)
    kw = dict(base=base, grid=grid, gridtype=1, seed=BIG_SEED, want_value=True)
    a, v1 = run(table, dev, BIG_LAM, n_samples, **kw)
    _, v2 = run(table, dev, BIG_LAM, n_samples, **kw)
    check(a, ref, base, what='resolution 80, 65 537 draws')
    check_value(v1, ref_v, n, 'resolution 80, 65 537 draws, value')
    assert torch.equal(v1, v2)


def test_big_sampled_one_draw_past_a_trip(big_level, dev):
    table, grid, refs = big_level
    n_samples = BIG_DRAWS[1]
    ref = refs[n_samples][0]
    assert BIG_TRIP < n_samples == 524289 < BIG_V and ref.k.sum() == n_samples        # draws, not a sweep; one takes a second trip
    base = _big_base(table)
    a, _ = run(table, dev, BIG_LAM, n_samples, base=base, grid=grid, gridtype=1, seed=BIG_SEED)
    check(a, ref, base, what='resolution 80, 524 289 draws')


# ---- 3. the sweep/draw switch, several tiled levels, uneven draw counts ----------------------------------------------------------
@pytest.mark.parametrize('level,n', [(1, 729), (1, 728), (2, 4913), (2, 4912)])
def test_sweep_threshold(tables, dev, level, n):
    table, lam = tables[4], lam_of(4)
    lvs = T.levels(OFF, S, H)
    V = T.vertex_count(lvs[level])
    assert n in (V, V - 1) and T.draws(lvs[level], level, n, SEED)[1] == (n == V)
    assert [T.draws(lv, l, n, SEED)[1] for l, lv in enumerate(lvs)] == [True, n >= 729, n >= 4913]
    ref = T.gradient(table, OFF, S, H, lam, n, seed=SEED)
    got, v = run(table, dev, lam, n, want_value=True)
    check(got, ref, what='level {} at n_samples {}'.format(level, n))
    ref_v, cnt = T.value(table, OFF, S, H, lam, n, seed=SEED)
    assert cnt[level] == n
    check_value(v, ref_v, cnt, 'level {} at n_samples {}, value'.format(level, n))
    # the level alone, so that its rows are compared at the level's own c = 2 lambda / n
    one = T.gradient(table, OFF, S, H, lam, n, seed=SEED, level_mask=1 << level)
    assert one.k.sum() == n
    got, _ = run(table, dev, lam, n, level_mask=1 << level)
    check(got, one, what='level {} alone at n_samples {}'.format(level, n))


# the smallest table that leaves level 0 of the tiled type a row per vertex: 2^7 = 128 >= 125 (2^6 would fold it).  The tiled
# type never hashes; levels 1 and 2 (729 and 4913 vertices) are folded onto the same 128 rows by index % size, level 2 without a
# z stride at all
MIXED = dict(TINY, log2_hashmap_size=7)


def _mixed():
    off = T.grid_offsets(**MIXED)
    lvs = T.levels(off, S, H, 1)
    rows = [T.grid_row(lv, *T.all_vertices(lv).T) for lv in lvs]
    assert list(off) == [0, 128, 256, 384] and not any(lv['use_hash'] for lv in lvs)
    assert len(np.unique(rows[0])) == 125                                              # level 0: dense
    assert T.levels(T.grid_offsets(**dict(TINY, log2_hashmap_size=6)), S, H, 1)[0]['size'] < 125
    for l in (1, 2):                                                                   # levels 1, 2: many vertices on a row
        assert lvs[l]['size'] == 128 < T.vertex_count(lvs[l]) and np.unique(rows[l], return_counts=True)[1].min() > 1
    return off


@pytest.mark.parametrize('rf', [4, 8])
@pytest.mark.parametrize('n', [8192, 500])
def test_mixed_tiled_levels(dev, rf, n):
    off = _mixed()
    table, lam = filled((int(off[-1]), rf), 26), lam_of(rf)
    base = filled(table.shape, 27)
    ref = T.gradient(table, off, S, H, lam, n, gridtype=1, seed=SEED)
    assert ref.k.sum() == (125 + 729 + 4913 if n == 8192 else 125 + 500 + 500)
    got, _ = run(table, dev, lam, n, base=base, grid=(off, S, H), gridtype=1)
    check(got, ref, base, what='tiled levels 0-2 rf {} n {}'.format(rf, n))
    # level 0 has 125 draws whatever n is: the blocks past them add nothing, its three spare rows keep their bits
    mine = ref.rows[ref.rows < off[1]]
    assert len(mine) == 125 and np.array_equal(bits(got[125:128]), bits(base[125:128]))
    # onto zeros, where the bound is the call's own
    got, _ = run(table, dev, lam, n, grid=(off, S, H), gridtype=1)
    check(got, ref, what='tiled levels 0-2 onto zeros rf {} n {}'.format(rf, n))


@pytest.mark.parametrize('rf', [1, 4, 8])
def test_uneven_draw_counts(tables, dev, rf):
    """n_samples = 500: the launch has two blocks per level, level 0 has 125 draws -- its second block, and the first block's
    threads past 125, add nothing"""
    table, lam = tables[rf], lam_of(rf)
    base = filled(table.shape, 28)
    ref = T.gradient(table, OFF, S, H, lam, 500, seed=SEED)
    l0 = T.gradient(table, OFF, S, H, lam, 500, seed=SEED, level_mask=0b001)
    assert l0.k.sum() == 125 and np.array_equal(l0.rows, ref.rows[ref.rows < OFF[1]]) and len(l0.rows) == 102
    got, _ = run(table, dev, lam, 500, base=base)
    check(got, ref, base, what='uneven draw counts rf {}'.format(rf))
    outside = np.ones(int(OFF[1]), bool)
    outside[l0.rows] = False
    assert outside.sum() == 26 and np.array_equal(bits(got[:OFF[1]][outside]), bits(base[:OFF[1]][outside]))
    # level 0 alone in the same launch shape, from zeros
    got, _ = run(table, dev, lam, 500, level_mask=0b001)
    check(got, l0, what='uneven draw counts, level 0 alone rf {}'.format(rf))


# ---- 4. refused before any launch ------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_gradient_alone(dev):
    from nerfstyle_amd import _lib as L
    lib = L.lib()
    t = torch.from_numpy(filled((ROWS + 1, 8), 29)).to(dev)           # a spare row: an offset pointer still has ROWS rows behind it
    g = torch.full_like(t, 7.25)
    seq_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    value = torch.zeros(3, 8, dtype=torch.float64, device=dev)
    ws = torch.zeros(int(lib.nsr_grid_tv_workspace_bytes(3, 1000, 8)) // 8, dtype=torch.float64, device=dev)
    lam = (ctypes.c_float * 8)(*LAM8)
    off_p = OFF.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert t.data_ptr() % 16 == 0

    def call(rf=4, shift=0, n_samples=1000, gridtype=0, seq=None, advance=0, val=None, work=None):
        return lib.nsr_grid_tv(t.data_ptr() + shift, g.data_ptr(), rf, lam, off_p, 3, S, H, gridtype, 0xffffffff, n_samples, SEED, 0,
                               seq, 0, advance, 1.0, None, val, work, L.stream())

    bad = -1                                                           # NSR_ERR_INVALID_ARG
    for rf in (0, 3, 16):
        assert call(rf=rf) == bad, rf
    assert call(n_samples=0) == bad
    assert call(gridtype=2) == bad
    assert call(advance=1, seq=None) == bad
    assert call(val=value.data_ptr(), work=None) == bad
    assert call(rf=2, shift=4) == bad                                  # a row of two floats is one 8-byte read
    assert call(rf=4, shift=8) == bad and call(rf=8, shift=8) == bad   # rows of four and eight floats are read 16 bytes at a time
    torch.cuda.synchronize()
    assert bool((g == 7.25).all()) and int(seq_dev.item()) == 0 and not bool(value.any())
    # the same call with nothing wrong goes through, at every width and with everything the refusals named
    for rf in (1, 2, 4, 8):
        assert call(rf=rf, seq=seq_dev.data_ptr(), advance=1, val=value.data_ptr(), work=ws.data_ptr()) == 0
    assert call(rf=1, shift=4) == 0 and call(rf=2, shift=8) == 0 and call(rf=4, shift=16) == 0
    torch.cuda.synchronize()
    assert int(seq_dev.item()) == 4 and bool((g[:ROWS] != 7.25).any()) and bool((value > 0).all())
