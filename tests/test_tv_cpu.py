"""Total-variation regulariser without a GPU: the restatement (tv_ref.py) against torch autograd of its own loss, its row
function against the oracle's, the estimator's mean, the neighbour counts at the lattice's border, what the C entry point and
the host layer refuse before anything touches a device, and the facts about the resolution-80 level that the GPU edge tests
(test_gpu_tv_edges.py) rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tv_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the tiny grid of the GPU tests: resolutions 4, 8, 16; V = 125, 729, 4913 vertices in 128, 512, 512 rows.  With the 'hash' grid
# type every level is hashed (the row function's style axis of 512 never fits), up to 3, 4 and 13 vertices on a row; with the
# 'tiled' type level 0 is dense, a row per vertex
TINY = dict(num_levels=3, per_level_scale=2.0, base_resolution=4, log2_hashmap_size=9)


def tiny(gridtype=0):
    off = T.grid_offsets(**TINY)
    return off, T.grid_S(TINY['per_level_scale']), TINY['base_resolution'], T.levels(off, T.grid_S(2.0), 4, gridtype)


# one 'tiled' level of resolution 80 for the GPU edge tests: side 81, V = 531 441 vertices in 531 448 rows, a row per vertex.  The
# launch is capped at 2048 blocks of 256 threads = 524 288 draws a trip, so the sweep and 524 289 draws wrap the grid-stride loop;
# 65 537 draws are 257 blocks, the first count at which the value's final pass strides over its partials
BIG = dict(num_levels=1, per_level_scale=2.0, base_resolution=80, log2_hashmap_size=20)
BIG_V, BIG_TRIP, BIG_DRAWS, BIG_LAM, BIG_SEED = 81 ** 3, 2048 * 256, (65537, 524289), (0.3, 0.7), 0x1234567855aa


def big():
    off = T.grid_offsets(**BIG)
    S = T.grid_S(BIG['per_level_scale'])
    return off, S, BIG['base_resolution'], T.levels(off, S, BIG['base_resolution'], 1)[0]


def big_table():
    """rows of two lanes, random in +-1; the same in the CPU and the GPU module"""
    return np.random.default_rng(31).uniform(-1, 1, (int(T.grid_offsets(**BIG)[-1]), 2)).astype(np.float32)


def big_refs(table):
    """the references of the resolution-80 level, each built once: {n_samples: (Grad, value [1, 2], n [1])}"""
    off, S, H, _ = big()
    return {n: (T.gradient(table, off, S, H, BIG_LAM, n, gridtype=1, seed=BIG_SEED),) + T.value(table, off, S, H, BIG_LAM, n, gridtype=1,
                                                                                                seed=BIG_SEED)
            for n in (BIG_V,) + BIG_DRAWS}


def test_tiny_grid_is_what_the_tests_assume():
    off, S, H, lv = tiny()
    assert [v['res'] for v in lv] == [4, 8, 16] and [T.vertex_count(v) for v in lv] == [125, 729, 4913]
    assert list(off) == [0, 128, 640, 1152]
    assert all(v['use_hash'] for v in lv)
    # the tiled grid type is dense wherever the level has a row per vertex
    assert not T.levels(off, S, H, 1)[0]['use_hash']
    xyz = T.all_vertices(T.levels(off, S, H, 1)[0])
    assert len(np.unique(T.grid_row(T.levels(off, S, H, 1)[0], *xyz.T))) == 125
    # hashed levels collide: several vertices share a row
    for v, most in zip(lv, (3, 4, 13)):
        xyz = T.all_vertices(v)
        assert np.unique(T.grid_row(v, *xyz.T), return_counts=True)[1].max() == most


@pytest.mark.parametrize('gridtype', [0, 1])
def test_row_function_matches_the_oracle(gridtype):
    """every vertex of every tiny level, as the corners the oracle's own index function gives the cells' centres"""
    from oracle import oracle as O
    O.build()
    off, S, H, lvs = tiny(gridtype)
    for l, lv in enumerate(lvs):
        res = lv['res']
        c = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).reshape(-1, 3)
        x = ((c + 0.5) / res).astype(np.float32)
        rows = O.grid_corner_rows(x, off, TINY['per_level_scale'], H, gridtype=gridtype, align_corners=True)[l]      # [B, 8]
        for idx in range(8):
            v = c + np.array([(idx >> d) & 1 for d in range(3)])
            assert np.array_equal(rows[:, idx].astype(np.int64), T.grid_row(lv, v[:, 0], v[:, 1], v[:, 2])), (l, idx)


@pytest.mark.parametrize('gridtype', [0, 1])
def test_sweep_gradient_is_autograd_of_the_loss(gridtype):
    """dense (tiled level 0) and hashed levels with collisions: the sum over all vertices of what each adds is d loss / d table"""
    off, S, H, lvs = tiny(gridtype)
    rng = np.random.default_rng(3)
    table = rng.uniform(-1, 1, (int(off[-1]), 4)).astype(np.float32)
    lam = (0.3, 0.7, 0.0, 1.1)
    t = torch.tensor(table.astype(np.float64), requires_grad=True)
    T.tv_loss_torch(t, off, S, H, [np.float32(v) for v in lam], gridtype).backward()
    auto = t.grad.numpy()
    ref = T.gradient(table, off, S, H, lam, 8192, gridtype)
    got = ref.dense(int(off[-1]))
    # c is rounded to float once: 2^-24 relative on every term
    assert np.abs(got - auto).max() <= 2.0 ** -23 * ref.A.max() + 1e-15
    assert np.abs(auto).max() > 1e-4 and not got[:, 2].any()
    assert ref.k.sum() == 125 + 729 + 4913


@pytest.mark.parametrize('rf', [1, 8])
@pytest.mark.parametrize('gridtype', [0, 1])
def test_sweep_gradient_is_autograd_of_the_loss_at_rows_of_1_and_8(gridtype, rf):
    """the restatement at the widths the GPU edge tests add: every lane has a weight of its own and uses its own column"""
    off, S, H, lvs = tiny(gridtype)
    table = np.random.default_rng(5).uniform(-1, 1, (int(off[-1]), rf)).astype(np.float32)
    lam = (0.3, 0.7, 0.45, 1.1, 0.9, 0.0, 0.6, 1.3)[:rf]
    t = torch.tensor(table.astype(np.float64), requires_grad=True)
    T.tv_loss_torch(t, off, S, H, [np.float32(v) for v in lam], gridtype).backward()
    auto = t.grad.numpy()
    ref = T.gradient(table, off, S, H, lam, 8192, gridtype)
    got = ref.dense(int(off[-1]))
    assert got.shape == auto.shape == (int(off[-1]), rf)
    assert np.abs(got - auto).max() <= 2.0 ** -23 * ref.A.max() + 1e-15                # c is rounded to float once
    assert (np.abs(auto).max(0)[[k for k in range(rf) if lam[k]]] > 1e-4).all() and ref.k.sum() == 125 + 729 + 4913
    if rf == 8:
        assert not got[:, 5].any()
        # no two lanes agree: a lane computed from another lane's column or weight is off by far more than any bound
        assert all(np.abs(got[:, j] - got[:, k]).max() > 1e-3 for j in range(8) for k in range(j))
    # the value is the loss: sum_k lambda_k value[:, k] over the levels
    val, n = T.value(table, off, S, H, lam, 8192, gridtype)
    loss = float(T.tv_loss_torch(t.detach(), off, S, H, [np.float32(v) for v in lam], gridtype))
    assert list(n) == [125, 729, 4913] and abs(float((val * [float(np.float32(v)) for v in lam]).sum()) - loss) <= 1e-12 * loss


@pytest.fixture(scope='module')
def big_level():
    import time
    table = big_table()
    t0 = time.perf_counter()
    refs = big_refs(table)
    return table, refs, time.perf_counter() - t0


def test_big_level_is_what_the_gpu_tests_assume(big_level):
    table, refs, seconds = big_level
    print('resolution-80 level: the sweep and the {} / {}-draw references took {:.2f} s'.format(BIG_DRAWS[0], BIG_DRAWS[1], seconds))
    off, S, H, lv = big()
    # dense: a row per vertex, and more vertices than one trip of the capped grid covers
    assert not lv['use_hash'] and lv['res'] == 80 and lv['mul'] == [1, 81, 6561]
    assert T.vertex_count(lv) == BIG_V == 531441 > BIG_TRIP == 524288 and lv['size'] >= BIG_V
    assert table.nbytes < 5 << 20
    xyz, swept = T.draws(lv, 0, BIG_V)
    assert swept and np.array_equal(T.grid_row(lv, *xyz.T), np.arange(BIG_V))
    ref, val, n = refs[BIG_V]
    assert len(ref.rows) == BIG_V and (ref.k == 1).all() and n[0] == BIG_V
    assert -(-BIG_V // 256) > 2048                                   # 2048 partial blocks: eight for every thread of the final pass
    # the two sampled counts draw (below V): 257 blocks, and one draw more than a trip
    for n_samples, blocks in zip(BIG_DRAWS, (257, 2049)):
        xyz, swept = T.draws(lv, 0, n_samples, seed=BIG_SEED)
        assert not swept and len(xyz) == n_samples < BIG_V and -(-n_samples // 256) == blocks
        assert refs[n_samples][0].k.sum() == n_samples and refs[n_samples][2][0] == n_samples


def test_big_level_checks_see_a_lost_wrap(big_level):
    """what the GPU tests' bars can see: the one draw of the second trip (524 288), every vertex past the first trip of the
    sweep, and the partial sums past the first 256 blocks are each worth far more than the bar they are measured against"""
    table, refs, _ = big_level
    off, S, H, lv = big()
    # the last of 524 289 draws, which only the second trip reaches
    n = BIG_DRAWS[1]
    ref = refs[n][0]
    xyz = T.draws(lv, 0, n, seed=BIG_SEED)[0][BIG_TRIP:]
    assert len(xyz) == 1
    g, _, _, _, row = T.level_terms(table, lv, xyz)
    at = np.searchsorted(ref.rows, row[0])
    lost = np.abs(g[0] * [T.c_factor(v, n) for v in BIG_LAM])
    assert ref.rows[at] == row[0] and (lost > 100 * ref.bound()[at]).any()
    # the sweep's vertices past the first trip: lost (or added twice), nearly all of them miss the bound
    ref = refs[BIG_V][0]
    tail = ref.rows >= BIG_TRIP
    assert tail.sum() == BIG_V - BIG_TRIP and (np.abs(ref.grad[tail]) > 100 * ref.bound()[tail]).any(1).mean() > 0.99
    # the value of 65 537 draws without block 256 (its last draw), and of the sweep from the first 256 of 2048 blocks only
    n = BIG_DRAWS[0]
    _, val, cnt = refs[n]
    fwd = T.level_terms(table, lv, T.draws(lv, 0, n, seed=BIG_SEED)[0][65536:])[3]
    assert len(fwd) == 1 and (fwd[0] / n > 100 * n * 6 * 2.0 ** -52 * val[0]).any()
    _, val, cnt = refs[BIG_V]
    head = T.level_terms(table, lv, T.all_vertices(lv)[:65536])[3].sum(0) / BIG_V
    assert (val[0] - head > 0.8 * val[0]).all()


def test_sampled_estimator_is_unbiased():
    """the mean of a draw's contribution over all vertices, times n_l draws, is the sweep gradient"""
    off, S, H, lvs = tiny()
    rng = np.random.default_rng(4)
    table = rng.uniform(-1, 1, (int(off[-1]), 2)).astype(np.float32)
    lam, n = (0.5, 0.25), 100
    sweep = T.gradient(table, off, S, H, lam, 8192, level_mask=0b100).dense(int(off[-1]))
    lv = lvs[2]
    xyz = T.all_vertices(lv)
    g, _, _, _, row = T.level_terms(table, lv, xyz)
    expect = np.zeros_like(sweep)
    # a draw hits each vertex with probability 1 / V and carries c = 2 lambda / n; n draws
    np.add.at(expect, row + lv['offset'], g * np.array([2.0 * v / n for v in lam]) * n / len(xyz))
    assert np.abs(expect - sweep).max() <= 1e-6 * np.abs(sweep).max()
    # and the draws are uniform on the lattice: over 200 000 draws every coordinate's mean is res / 2 within 5 sigma
    one, swept = T.draws(lv, 2, 4000, seed=7)                   # n_samples < V: sampled
    assert not swept and one.min() >= 0 and one.max() <= lv['res']
    many = np.concatenate([T.draws(lv, 2, 4000, seed=7, seq=s)[0] for s in range(50)])
    sigma = np.sqrt(((lv['res'] + 1) ** 2 - 1) / 12.0 / len(many))
    assert np.abs(many.mean(0) - lv['res'] / 2).max() < 5 * sigma
    assert not np.array_equal(T.draws(lv, 2, 4000, seed=7, seq=0)[0], T.draws(lv, 2, 4000, seed=7, stream_id=1)[0])


def test_border_vertices_have_fewer_neighbours():
    off, S, H, lvs = tiny()
    lv = lvs[0]
    xyz = T.all_vertices(lv)
    nb = T.level_terms(np.ones((int(off[-1]), 1), np.float32), lv, xyz)[2]
    on_border = ((xyz == 0) | (xyz == lv['res'])).sum(1)
    assert set(nb[on_border == 0]) == {6} and set(nb[on_border == 1]) == {5}           # interior, face
    assert set(nb[on_border == 2]) == {4} and set(nb[on_border == 3]) == {3}           # edge, corner
    assert (on_border == 3).sum() == 8 and (on_border == 2).sum() == 12 * 3 and (on_border == 1).sum() == 6 * 9


# ---- the entry point -----------------------------------------------------------------------------------------------------------
def test_symbols_and_signatures():
    from nerfstyle_amd import _lib, build
    so = ctypes.CDLL(build.build())
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nsr.h')).read(), flags=re.S)
    for name, nargs in (('nsr_grid_tv', 21), ('nsr_grid_tv_workspace_bytes', 3)):
        assert hasattr(so, name), 'libnsr_hip.so does not export ' + name
        proto = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', src)
        assert proto, name + ' is not declared in include/nsr.h'
        assert len(proto.group(1).split(',')) == len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.ABI_VERSION == 6 and _lib.lib().nsr_abi_version() == 6
    assert 'grid_tv.hip' in build.SOURCES


def test_invalid_arguments_are_refused_without_a_device():
    from nerfstyle_amd import _lib
    L = _lib.lib()
    off = T.grid_offsets(**TINY)
    off_p = off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    lam = (ctypes.c_float * 8)(*([0.5] * 8))
    fake, fake_grad, fake_seq = 0x10000, 0x20000, 0x30000          # never dereferenced: every call below is refused first

    def call(tables=fake, grad=fake_grad, rf=4, lam_p=lam, offs=off_p, nl=3, n_samples=100, seq_dev=None, advance=0, value=None, ws=None,
             gridtype=0):
        return L.nsr_grid_tv(tables, grad, rf, lam_p, offs, nl, 1.0, 4, gridtype, 0xffffffff, n_samples, 0, 0, seq_dev, 0, advance, 1.0,
                             None, value, ws, None)

    assert call(tables=None) == -1
    for rf in (0, 3, 5, 6, 7, 16):
        assert call(rf=rf) == -1
    assert call(nl=33) == -1 and call(nl=0) == -1
    assert call(n_samples=0) == -1
    assert call(advance=1, seq_dev=None) == -1
    assert call(lam_p=None) == -1 and call(offs=None) == -1
    assert call(grad=None, value=None) == -1                       # nothing to compute
    assert call(value=0x40000, ws=None) == -1                      # a value needs its workspace
    assert call(gridtype=2) == -1
    assert call(tables=fake + 4) == -1                             # rows of four floats are read 16 bytes at a time
    assert L.nsr_grid_tv_workspace_bytes(3, 8192, 4) == 32 * 3 * 4 * 8
    assert L.nsr_grid_tv_workspace_bytes(16, 1 << 18, 4) == 1024 * 16 * 4 * 8
    assert L.nsr_grid_tv_workspace_bytes(16, 1 << 30, 4) == 2048 * 16 * 4 * 8      # the grid's cap


def test_host_layer_refusals():
    from nerfstyle_amd import tv
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.gridencoder import GridEncoder
    from nerfstyle_amd.style_nerf import StyleTCNerf
    off = T.grid_offsets(**TINY)
    t = torch.zeros(int(off[-1]), 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tv.grid_tv(t, torch.zeros_like(t), (1.0,) * 4, off, 1.0, 4, n_samples=100, seed=0)
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 2, use_dir=False)
    m.train_density_table = False
    with pytest.raises(ValueError, match='train_density_table'):
        tv.TVRegulariser(m, lambda_density=1e-3)
    m.train_density_table, m.train_color_table = True, False
    with pytest.raises(ValueError, match='train_color_table'):
        tv.TVRegulariser(m, lambda_color=1e-3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        tv.TVRegulariser(m, lambda_density=1e-3)                   # a trained table, but the model is on the host
    enc = GridEncoder(**TINY)
    with pytest.raises(ValueError, match='single weight'):
        tv.TVRegulariser(enc, lambda_density=1e-3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        enc.grad_total_variation(1e-3, n_samples=100)
    assert enc.embeddings.grad is None
