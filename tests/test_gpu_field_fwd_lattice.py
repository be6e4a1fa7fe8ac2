"""The forward's lattice gather (k_field_fwd_lat, field.hip) against the plain gather, word for word.

nsr_field_forward with a `perm` (16-bit tables, a level table the scatter's lattices fit) reads the rows of its coarse levels
from per-wave LDS lattices; without a `perm` it runs k_field_fwd's global gather.  Both form the same fp32 sums of the same
16-bit rows in the same order, so every case asks for EQUALITY of the bit patterns:
  * `sigmas` and `rgbs` of the perm call against the perm == NULL call (outputs are indexed by sample, not by position);
  * `feats` (tile-major in the order: lane (s, g) of tile t holds sample perm[16 t + s]) against the perm == NULL call's after
    undoing that order;
  * slots at and behind the device count keep the pattern the buffers were filled with.
Everything goes through the C ABI.  Reference LLFF grid (16 levels, 16 .. 4096), +-2 box: the encoder input of position x is
u = (x + 6) / 8, a block of the sample order is 1/1024 of u per axis.  A 256-thread workgroup takes 32 tiles, its four waves
tile w, w + 4, ...: from 5 tiles on a wave meets a second tile."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import room_cameras, small_scene

pytestmark = pytest.mark.gpu

FILL = 0x7FC12345          # a NaN pattern no kernel writes


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _model(dev, dt='f16', table_dtype=None, nc=5):
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.style_nerf import StyleTCNerf
    from oracle import torch_port as TP
    ref = TP.Field(num_classes=nc, table_scale=0.5)
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), nc, enc_dtype=table_dtype, use_dir=False,
                    compute_dtype=torch.float16 if dt == 'f16' else torch.bfloat16)
    sd = m.state_dict()
    sd.update({'x_density_embedder.embeddings': ref.emb_density.detach(), 'x_color_embedder.embeddings': ref.emb_color.detach(),
               'density_net.params': ref.p_density.detach(), 'color1_net.params': ref.p_color1.detach(),
               'color2_net.params': ref.p_color2.detach(), 'class_net.params': ref.p_class.detach()})
    m.load_state_dict(sd)
    return m.to(dev)


@pytest.fixture(scope='module')
def model(dev):
    return _model(dev)


# ---------------------------------------------------------------------------------------------
# the call and the comparison
# ---------------------------------------------------------------------------------------------
class Call:
    """static buffers of one nsr_field_forward call (so that it can be captured)"""

    def __init__(self, m, xyzs, counter, with_perm):
        from nerfstyle_amd import _lib as L
        self.L, self.m, self.xyzs, self.counter = L, m, xyzs, counter
        M = xyzs.shape[0]
        dev = xyzs.device
        self.sigmas = torch.full((M,), FILL, dtype=torch.int32, device=dev).view(torch.float32)
        self.rgbs = torch.full((M, m.out_channels), FILL, dtype=torch.int32, device=dev).view(torch.float32)
        self.feats = torch.full((((M + 15) // 16) * 512,), FILL, dtype=torch.int32, device=dev)
        self.perm = torch.zeros(M, dtype=torch.int32, device=dev) if with_perm else None
        self.desc = m._desc(1.0)
        self.tables = m._gather_tables()
        self.mlp = m._mlp_flat()

    def run(self):
        L = self.L
        L.check(L.lib().nsr_field_forward(ctypes.byref(self.desc), L.p(self.tables), L.p(self.mlp), L.p(self.xyzs),
                                          self.xyzs.shape[0], L.p(self.counter), L.p(self.sigmas), L.p(self.rgbs),
                                          L.p(self.feats), L.p(self.perm), L.stream()), 'field_forward')

    def words(self):
        torch.cuda.synchronize()
        return (self.sigmas.view(torch.int32).cpu().numpy().copy(), self.rgbs.view(torch.int32).cpu().numpy().copy(),
                self.feats.cpu().numpy().copy())


def _compare(got, want, perm, cnt, what):
    """got: the perm call's words, want: the perm == NULL call's, perm: int64 [M], cnt: samples walked"""
    sg, rg, fg = got
    sw, rw, fw = want
    M = sg.shape[0]
    assert np.array_equal(np.sort(perm[:cnt]), np.arange(cnt)), what
    assert (sw[:cnt] != FILL).all() and (rw[:cnt] != FILL).all(), what
    assert np.array_equal(sg, sw), (what, 'sigmas', int((sg != sw).sum()))
    assert np.array_equal(rg, rw), (what, 'rgbs', int((rg != rw).any(axis=1).sum()))
    assert (sg[cnt:] == FILL).all() and (rg[cnt:] == FILL).all(), what
    # feats: [tile][g][s][8 words]
    nt = (M + 15) // 16
    fg = fg.reshape(nt, 4, 16, 8)
    fw = fw.reshape(nt, 4, 16, 8)
    pos = np.arange(cnt)
    m = perm[:cnt]
    a = fg[pos // 16, :, pos % 16]
    b = fw[m // 16, :, m % 16]
    assert np.array_equal(a, b), (what, 'feats', int((a != b).any(axis=(1, 2)).sum()))
    return int(cnt)


def _check(m, pts_or_xyzs, dev, what, counter=None, perm=None, cnt=None):
    xyzs = pts_or_xyzs if torch.is_tensor(pts_or_xyzs) else T(pts_or_xyzs, dev)
    M = xyzs.shape[0]
    if perm is None:
        perm = m.sample_order(xyzs, m_dev=counter)
    ref = Call(m, xyzs, counter, False)
    ref.run()
    lat = Call(m, xyzs, counter, True)
    lat.perm.copy_(perm)
    lat.run()
    cnt = M if cnt is None else cnt
    return _compare(lat.words(), ref.words(), perm.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, cnt, what)


# ---------------------------------------------------------------------------------------------
# positions from block coordinates
# ---------------------------------------------------------------------------------------------
def _pos(u):
    return (np.asarray(u, np.float64) * 8.0 - 6.0).astype(np.float32)


def _in_block(rng, b, n):
    return (np.asarray(b, np.float64)[None, :] + 0.02 + 0.96 * rng.random((n, 3))) / 1024.0


def _block_points(rng, blocks, lo=1, hi=6):
    """lo .. hi - 1 points inside each block (bx, by, bz), block after block"""
    return _pos(np.concatenate([_in_block(rng, b, int(rng.integers(lo, hi))) for b in blocks]))


def _sites(rng, n):
    s = set()
    while len(s) < n:
        s.add((int(rng.integers(520, 1016)), int(rng.integers(520, 1016))))
    return sorted(s)


def case_one_block(rng, n):
    return _pos(_in_block(rng, (733, 801, 640), n))


def case_x_runs(rng):
    """runs of four x-neighbouring blocks (interior, from u = 0, up to u = 1): the fine levels' anchors move, the coarse stay"""
    chunks = []
    for k in (700, 701, 0, 1, 1020, 1021):
        for (y, z) in _sites(rng, 30):
            chunks.append(_block_points(rng, [(k + i, y, z) for i in range(4) if k + i < 1024]))
    return np.concatenate(chunks)


def case_morton_quad(rng):
    chunks = []
    for k in (600, 602, 0, 1022):
        for (j, z) in _sites(rng, 30):
            j &= ~1
            chunks.append(_block_points(rng, [(k, j, z), (k + 1, j, z), (k, j + 1, z), (k + 1, j + 1, z)]))
    return np.concatenate(chunks)


def case_far_apart(rng):
    """16 samples per block, the blocks 67 .. 75 apart on every axis: each tile is one block in another cell of EVERY level"""
    blocks = [(bx, by, bz) for bx in range(3, 1024, 73) for by in range(515, 1024, 71) for bz in range(520, 1024, 67)]
    assert len(blocks) > 600
    return _pos(np.concatenate([_in_block(rng, b, 16) for b in blocks[:700]]))


def case_straddle(rng):
    """5 .. 7 samples per block: tiles of two and of three blocks, neighbours in the order (x-runs) and strangers"""
    chunks = []
    for (y, z) in _sites(rng, 60):
        k = int(rng.integers(0, 1016))
        chunks.append(_block_points(rng, [(k + i, y, z) for i in range(6)], 5, 8))
    for _ in range(300):
        chunks.append(_block_points(rng, [tuple(int(v) for v in rng.integers(0, 1024, 3))], 5, 8))
    return np.concatenate(chunks)


def case_faces(rng):
    """samples exactly on block faces (u = k / 1024 is exact in fp32, and so is the way there), at u = 0 and u = 1.0 on each
    axis, and in the last cell of every level (u just below and at 1)"""
    u = []
    for _ in range(600):
        p = (rng.integers(0, 1024, 3) + rng.random(3)) / 1024.0
        ax = int(rng.integers(0, 3))
        p[ax] = float(rng.integers(0, 1025)) / 1024.0
        u.append(p)
    for ax in range(3):
        for edge in (0.0, 1.0):
            for _ in range(40):
                p = (rng.integers(512, 1024, 3) + rng.random(3)) / 1024.0
                p[ax] = edge
                u.append(p)
    for _ in range(200):                                           # the last cell: res - 1 on one, two or three axes
        p = (rng.integers(512, 1024, 3) + rng.random(3)) / 1024.0
        for ax in range(3):
            if rng.random() < 0.6:
                p[ax] = 1.0 - float(rng.random()) * 2.0 ** -float(rng.integers(4, 20))
        u.append(p)
    u += [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 1.0]]
    pts = _pos(np.array(u))
    un = (pts.astype(np.float32) + np.float32(2.0)) / np.float32(4.0)
    un = (un + np.float32(1.0)) / np.float32(2.0)
    assert (un == 1.0).sum() > 100 and (un == 0.0).sum() > 100 and ((un >= 0) & (un <= 1)).all()
    return pts


def case_dead_between(rng):
    """out-of-box and NaN positions between live ones (they encode to zeros); tiles that BEGIN with dead samples"""
    chunks = []
    for (y, z) in _sites(rng, 120):
        k = int(rng.integers(0, 1020))
        live = _block_points(rng, [(k, y, z), (k + 1, y, z)], 3, 9)
        nd = int(rng.integers(1, 20))
        dead = np.repeat(live[:1], nd, 0).copy()
        dead[:, int(rng.integers(0, 3))] = 2.0 + 8.0 * rng.random(nd).astype(np.float32) + 0.01
        dead[rng.random(nd) < 0.3] = np.nan
        chunks += [dead, live] if rng.random() < 0.5 else [live[:2], dead, live[2:]]
    return np.concatenate(chunks)


def case_many_blocks(rng, M):
    pts = _block_points(rng, [tuple(int(v) for v in rng.integers(0, 1024, 3)) for _ in range(M)], 1, 4)
    return pts[:M]


SYNTHETIC = {
    'one_block_1': lambda: case_one_block(np.random.default_rng(201), 1),
    'one_block_16': lambda: case_one_block(np.random.default_rng(202), 16),
    'one_block_17': lambda: case_one_block(np.random.default_rng(203), 17),
    'one_block_53': lambda: case_one_block(np.random.default_rng(204), 53),
    'one_block_150': lambda: case_one_block(np.random.default_rng(205), 150),     # waves with a second and third tile
    'x_runs': lambda: case_x_runs(np.random.default_rng(206)),
    'morton_quad': lambda: case_morton_quad(np.random.default_rng(207)),
    'far_apart': lambda: case_far_apart(np.random.default_rng(208)),
    'straddle': lambda: case_straddle(np.random.default_rng(209)),
    'faces': lambda: case_faces(np.random.default_rng(210)),
    'dead_between': lambda: case_dead_between(np.random.default_rng(211)),
}


@pytest.mark.parametrize('name', sorted(SYNTHETIC))
def test_synthetic_blocks(dev, model, name):
    pts = SYNTHETIC[name]()
    assert pts.shape[0] < 12000
    if name.startswith('one_block'):
        assert pts.shape[0] == int(name.split('_')[-1])
    _check(model, pts, dev, name)


def test_non_spatial_perm(dev, model):
    """a seeded shuffle instead of the order: almost every lane's cell lies outside the lattice of the tile's first sample"""
    pts = case_many_blocks(np.random.default_rng(212), 4099)
    perm = T(np.random.default_rng(213).permutation(4099).astype(np.int32), dev)
    _check(model, pts, dev, 'shuffle', perm=perm)


def test_device_count_below_capacity(dev, model):
    pts = case_x_runs(np.random.default_rng(206))
    M = pts.shape[0]
    cnt = (M - 333) // 16 * 16 - 5
    assert cnt % 16 != 0
    counter = torch.tensor([cnt, 0], dtype=torch.int32, device=dev)
    _check(model, pts, dev, 'count', counter=counter, cnt=cnt)


@pytest.fixture(scope='module')
def marched_patch(O, dev):
    """64 x 64 pixels of room pose 0 through the real march: workgroups that loop over many tiles of the real order"""
    from nerfstyle_amd import raymarching as R
    c = room_cameras()
    _, bits = small_scene()
    ys, xs = np.meshgrid(np.arange(157, 221), np.arange(220, 284), indexing='ij')
    pix = (ys * c['w'] + xs).reshape(-1)
    ro, rd = O.generate_rays(np.asarray(c['poses'][0], np.float32), c['w'], c['h'], c['fl_x'], c['fl_y'], c['cx'], c['cy'], 3,
                             pix_indices=pix)[:2]
    aabb = T(np.array([-2, -2, -2, 2, 2, 2], np.float32), dev)
    near, far = R.near_far_from_aabb(T(ro, dev), T(rd, dev), aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    xyzs = R.march_rays_train_nosync(T(ro, dev), T(rd, dev), 2.0, T(bits, dev), 2, 128, near, far, 4096 * 160, counter, 0., 1024)[0]
    cnt = int(counter[0])
    assert 4096 * 8 < cnt < xyzs.shape[0], cnt
    xyzs[cnt:] = float('nan')
    return xyzs, counter, cnt


def test_marched_patch(dev, model, marched_patch):
    xyzs, counter, cnt = marched_patch
    _check(model, xyzs, dev, 'marched', counter=counter, cnt=cnt)


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nc', [1, 5, 13])
def test_dtype_and_classes(dev, dt, nc):
    m = _model(dev, dt, None, nc)
    _check(m, case_many_blocks(np.random.default_rng(214), 4099), dev, '%s nc=%d' % (dt, nc))


def test_fp32_tables_keep_the_gather(dev):
    m = _model(dev, 'f16', torch.float32, 5)
    _check(m, case_many_blocks(np.random.default_rng(214), 4099), dev, 'fp32 tables')


def test_captured_replays_equal_eager(dev, model):
    """one capture, two replays with different permutations in the same buffer"""
    pts = case_straddle(np.random.default_rng(215))
    xyzs = T(pts, dev)
    M = pts.shape[0]
    perms = [model.sample_order(xyzs), T(np.random.default_rng(216).permutation(M).astype(np.int32), dev)]
    ref = Call(model, xyzs, None, False)
    ref.run()
    want = ref.words()
    lat = Call(model, xyzs, None, True)
    lat.perm.copy_(perms[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lat.run()                                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lat.run()
    for p in perms:
        lat.perm.copy_(p)
        lat.sigmas.view(torch.int32).fill_(FILL)
        lat.rgbs.view(torch.int32).fill_(FILL)
        lat.feats.fill_(FILL)
        graph.replay()
        _compare(lat.words(), want, p.cpu().numpy().astype(np.int64), M, 'replay')
