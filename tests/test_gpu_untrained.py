"""nsr_occ_mark_untrained (csrc/occ_untrained.hip) called through the C ABI and compared EXACTLY with its NumPy restatement
(untrained_ref.py): counts, the grid as bit patterns, the bitfield and the per-cascade totals.  There is no tolerance in this
file: every operation of the frustum test is a correctly rounded fp64 + - x in a fixed order.

Every case runs on buffers between guard bands, with counts and n_untrained pre-filled with garbage, the grid with
-1 / 0 / 0.5 / the smallest denormal / -0.0 / NaNs, the bitfield with 0xFF and then with a random pattern; each run is made twice
on fresh buffers (bit for bit the same) and a further call on the result must change nothing.  Then the interplay with
nsr_occ_update / nsr_occ_sample_points, and through the Renderer: no sample of any training ray is lost to the marks."""
import numpy as np
import pytest
import torch

import untrained_ref as U

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 4096
NSR_OK, NSR_INVALID = 0, -1
# -1, +0, 0.5, the smallest denormal, -0.0, a quiet NaN, a negative NaN with a payload
PATTERN = np.array([0xBF800000, 0x00000000, 0x3F000000, 0x00000001, 0x80000000, 0x7FC00000, 0xFFC01234], np.uint32)


class Banded:
    """`nbytes` device bytes at a 256-byte aligned address between two guard bands of random bytes"""

    def __init__(self, dev, nbytes, seed):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        self.buf = torch.randint(0, 256, (nbytes + 2 * GUARD + 256,), dtype=torch.uint8, device=dev, generator=g)
        self.off = ((self.buf.data_ptr() + GUARD + 255) & ~255) - self.buf.data_ptr()
        self.nbytes = nbytes
        self.lo, self.hi = self.buf[:self.off].clone(), self.buf[self.off + nbytes:].clone()

    def bytes(self):
        return self.buf[self.off:self.off + self.nbytes]

    def put(self, array):
        self.bytes().copy_(torch.as_tensor(np.ascontiguousarray(array).reshape(-1).view(np.uint8)))
        return self

    def get(self, dtype):
        return self.bytes().cpu().numpy().view(dtype)

    def ptr(self):
        return self.buf.data_ptr() + self.off

    def check(self, what):
        assert torch.equal(self.buf[:self.off], self.lo), 'write below ' + what
        assert torch.equal(self.buf[self.off + self.nbytes:], self.hi), 'write past the end of ' + what


# ---- cameras -----------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), eye[:, None]], 1).astype(F32)


def cameras(F, camera_flip, scale=1.0):
    """F poses [F,3,4] f32 for `camera_flip`: outside the box looking at it; INSIDE it, the centre exactly at a cell centre of
    (H = 16, cascade 0); outside looking away; two with overlapping frusta; then seeded random ones.  The columns of R carry the
    flip's signs, so the cameras look where they are meant to under every flip."""
    rng = np.random.default_rng(17)
    pool = [look_at((0.4, 0.3, -2.8), (0.1, 0.0, 0.0)),
            look_at((0.1875, -0.0625, 0.3125), (1.0, 0.6, -0.8)),
            look_at((0.0, 0.5, -3.0), (0.0, 0.5, -6.0)),
            look_at((2.6, 0.2, 0.9), (0.0, 0.0, 0.2)),
            look_at((2.4, -0.3, 1.3), (0.1, 0.2, 0.0))]
    while len(pool) < F:
        eye = rng.normal(size=3)
        eye *= rng.uniform(2.2, 3.5) / np.linalg.norm(eye)
        pool.append(look_at(eye, rng.uniform(-4.0, 4.0, 3)))                # most of them miss the box
    P = np.stack(pool[:F])
    P[:, :, 3] *= F32(scale)
    P[:, :, :3] *= np.asarray(U.flips(camera_flip), F32)
    return P


FRUSTUM = U.pinhole_frustum(48, 36, 150.0, 140.0, 22.5, 19.25)              # not symmetric: a flip that is decoded wrongly shows

# (H, C, F, bound, camera_flip, margin_cells, min_views)
CASES = [
    (8, 1, 1, 1.0, 0, 1.5, 1),            # 64 bytes: one partial block
    (8, 1, 1, 1.0, 7, 0.0, 1),
    (16, 3, 3, 1.5, 0, 1.5, 1),           # min(2^cas, bound) binds in cascades 1 and 2
    (16, 3, 3, 1.5, 3, 2.5, 2),
    (16, 3, 3, 1.5, 7, 0.0, 1),
    (32, 2, 129, 2.0, 3, 1.5, 2),         # one pose past an LDS chunk
    (32, 2, 129, 2.0, 0, 0.0, 2),
    (64, 2, 5, 4.0, 7, 2.5, 1),
    (64, 2, 5, 4.0, 3, 1.5, 2),
    (128, 1, 2, 1.0, 3, 1.5, 1),          # 1024 blocks: a byte per thread keeps this one below the 2048-block cap ...
    (128, 3, 2, 4.0, 0, 1.5, 2),          # ... 3072 blocks: the smallest grid past it, blocks 0..1023 make two trips
]
_REF = {}


def _inputs(case):
    H, C, F, bound, flip, margin, min_views = case
    cells = C * H ** 3
    rng = np.random.default_rng(H * 100 + C * 10 + F)
    grid = PATTERN[rng.integers(0, PATTERN.size, cells)].view(F32)
    random_bits = rng.integers(0, 256, cells // 8).astype(np.uint8)
    return grid, random_bits, cameras(F, flip, scale=bound / 2.0 if bound > 2 else 1.0)


def reference(case):
    """computed once per case and shared: (counts, grid after, n_untrained); the bitfield follows from counts"""
    if case not in _REF:
        H, C, F, bound, flip, margin, min_views = case
        grid, _, poses = _inputs(case)
        cnt, g, _, n_un = U.mark(grid, None, C, H, bound, poses, FRUSTUM, flip, margin, min_views)
        for a in (cnt, g, n_un):
            a.setflags(write=False)
        _REF[case] = (cnt, g, n_un)
    return _REF[case]


def call(dev, case, grid, bitfield, poses, want_counts=True, want_total=True, frustum=FRUSTUM, again=False):
    """one call on fresh banded buffers -> (status, grid bits u32, bitfield u8 | None, counts i32 | None, n_untrained u32 | None);
    again: a second call on the results, which must change nothing"""
    from nerfstyle_amd import _lib as L
    H, C, F, bound, flip, margin, min_views = case
    cells = C * H ** 3
    g = Banded(dev, cells * 4, 1).put(grid)
    b = None if bitfield is None else Banded(dev, cells // 8, 2).put(bitfield)
    cnt = Banded(dev, cells * 4, 3) if want_counts else None
    tot = Banded(dev, C * 4, 4) if want_total else None
    P = torch.as_tensor(np.ascontiguousarray(poses, F32), device=dev)
    before = [x.bytes().clone() for x in (g, b, cnt, tot) if x is not None]

    def once():
        st = L.lib().nsr_occ_mark_untrained(g.ptr(), None if b is None else b.ptr(), C, H, bound, L.p(P), F, *frustum,
                                            flip, margin, min_views, None if cnt is None else cnt.ptr(),
                                            None if tot is None else tot.ptr(), L.stream())
        torch.cuda.synchronize()
        for x, what in ((g, 'density_grid'), (b, 'the bitfield'), (cnt, 'counts'), (tot, 'n_untrained')):
            if x is not None:
                x.check(what)
        return st, g.get(np.uint32), None if b is None else b.get(np.uint8), None if cnt is None else cnt.get(np.int32), \
            None if tot is None else tot.get(np.uint32)

    out = once()
    if out[0] != NSR_OK:
        after = [x.bytes() for x in (g, b, cnt, tot) if x is not None]
        assert all(torch.equal(x, y) for x, y in zip(before, after)), 'a refused call wrote to its buffers'
    elif again:
        for x, y in zip(out, once()):
            assert (x is None and y is None) or np.array_equal(x, y), 'a second call with the same arguments changed something'
    return out


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'H{}-C{}-F{}-b{}-flip{}-m{}-v{}'.format(*c))
def test_exact_against_the_restatement(dev, case):
    H, C, F, bound, flip, margin, min_views = case
    grid, random_bits, poses = _inputs(case)
    want_cnt, want_grid, want_tot = reference(case)
    unseen = want_cnt < min_views
    clear = np.packbits(unseen.reshape(-1, 8)[:, ::-1], axis=1).reshape(-1)
    assert 0 < unseen.sum() < unseen.size, 'the case marks nothing or everything: it would not tell much'
    print('marked per cascade', want_tot, 'of', H ** 3)
    for bits_in in (np.full(C * H ** 3 // 8, 0xFF, np.uint8), random_bits):
        first = call(dev, case, grid, bits_in, poses)
        second = call(dev, case, grid, bits_in, poses, again=True)
        st, g, b, cnt, tot = first
        assert st == NSR_OK
        for x, y in zip(first[1:], second[1:]):
            assert np.array_equal(x, y), 'two runs differ'
        bad = np.flatnonzero(cnt != want_cnt)
        assert bad.size == 0, 'count of cell {}: {} != {} ({} differ)'.format(bad[0], cnt[bad[0]], want_cnt[bad[0]], bad.size)
        bad = np.flatnonzero(g != want_grid.view(np.uint32))
        assert bad.size == 0, 'cell {}: {:#x} != {:#x} ({} differ)'.format(bad[0], g[bad[0]], want_grid.view(np.uint32)[bad[0]], bad.size)
        assert np.array_equal(b, bits_in & ~clear) and np.array_equal(tot, want_tot)
        # the semantics, stated without the restatement's mark(): from the counts and the grid before alone
        before = grid.view(np.uint32)
        with np.errstate(invalid='ignore'):
            negative = grid < 0
        assert (g[unseen] == 0xBF800000).all()
        assert (g[~unseen & negative] == 0).all() and (~unseen & negative).any()
        keep = ~unseen & ~negative
        assert np.array_equal(g[keep], before[keep])
        for pat in PATTERN[2:]:                                            # 0.5, the denormal, -0.0 and both NaNs are among the kept
            assert (before[keep] == pat).any()
        assert np.array_equal(tot, unseen.reshape(C, -1).sum(1))


def _assert_camera_set():
    """the test's own cameras are what cameras() says, on the restatement (H = 16, cascade 0, flip 0)"""
    P = cameras(5, 0)
    each = [U.counts(1, 16, 1.0, P[k:k + 1], FRUSTUM, 0, 1.0) for k in range(5)]
    assert each[0].any() and each[1].any() and not each[2].any()                          # 2 looks away
    assert (np.abs(P[0, :, 3]) > 1).any() and (np.abs(P[1, :, 3]) < 1).all()            # 0 outside, 1 inside
    X, _ = U.cell_centres(1, 16, 1.0)
    assert (X[0] == P[1, :, 3].astype(np.float64)).all(1).any()                           # ... exactly at a cell centre
    assert ((each[3] > 0) & (each[4] > 0)).any() and ((each[3] > 0) != (each[4] > 0)).any()   # 3 and 4 overlap, and differ


def test_refused_arguments_and_optional_outputs(dev):
    base = (16, 3, 3, 1.5, 0, 1.5, 1)
    grid, random_bits, poses = _inputs(base)
    ok = call(dev, base, grid, random_bits, poses)
    assert ok[0] == NSR_OK
    for case in ((24, 3, 3, 1.5, 0, 1.5, 1), (16, 3, 0, 1.5, 0, 1.5, 1), (16, 3, 3, 1.5, 0, 1.5, 0), (16, 3, 3, 1.5, 0, -0.5, 1),
                 (16, 3, 3, 1.5, 0, float('nan'), 1), (16, 9, 3, 1.5, 0, 1.5, 1)):
        H, C = case[0], case[1]
        g = np.resize(grid, C * H ** 3)
        assert call(dev, case, g, np.resize(random_bits, C * H ** 3 // 8), poses)[0] == NSR_INVALID, case
    x_lo, x_hi, y_lo, y_hi = FRUSTUM
    for fr in ((x_hi, x_lo, y_lo, y_hi), (x_lo, x_lo, y_lo, y_hi), (x_lo, x_hi, y_hi, y_lo), (x_lo, x_hi, y_lo, y_lo),
               (float('nan'), x_hi, y_lo, y_hi)):
        assert call(dev, base, grid, random_bits, poses, frustum=fr)[0] == NSR_INVALID, fr
    # NULL bitfield, counts or n_untrained: accepted, the other outputs are the same
    st, g, b, cnt, tot = call(dev, base, grid, None, poses)
    assert st == NSR_OK and b is None and np.array_equal(g, ok[1]) and np.array_equal(cnt, ok[3]) and np.array_equal(tot, ok[4])
    st, g, b, cnt, tot = call(dev, base, grid, random_bits, poses, want_counts=False)
    assert st == NSR_OK and cnt is None and np.array_equal(g, ok[1]) and np.array_equal(b, ok[2]) and np.array_equal(tot, ok[4])
    st, g, b, cnt, tot = call(dev, base, grid, random_bits, poses, want_total=False)
    assert st == NSR_OK and tot is None and np.array_equal(g, ok[1]) and np.array_equal(b, ok[2]) and np.array_equal(cnt, ok[3])


def test_moved_cameras_reopen_cells(dev):
    """a call after the cameras moved: cells that became visible go from -1 to 0, learnt densities stay, cells no longer seen
    are marked"""
    _assert_camera_set()
    case = (16, 3, 3, 1.5, 0, 1.5, 1)
    H, C = 16, 3
    poses = cameras(3, 0)
    learnt = np.random.default_rng(3).random(C * H ** 3).astype(F32) + F32(0.25)
    ones = np.full(C * H ** 3 // 8, 0xFF, np.uint8)
    st, g1, b1, cnt1, _ = call(dev, case, learnt, ones, poses)
    moved = poses.copy()
    moved[0] = look_at((-2.5, 0.4, 0.3), (0.0, 0.1, 0.0))
    st2, g2, b2, cnt2, tot2 = call(dev, case, g1.view(F32), b1, moved)
    assert st == NSR_OK and st2 == NSR_OK
    opened, closed, stay = (cnt1 == 0) & (cnt2 > 0), (cnt1 > 0) & (cnt2 == 0), (cnt1 > 0) & (cnt2 > 0)
    assert opened.any() and closed.any() and stay.any()
    assert (g2[opened] == 0).all() and (g2[closed] == 0xBF800000).all() and np.array_equal(g2[stay], learnt.view(np.uint32)[stay])
    bit = np.unpackbits(b2, bitorder='little').astype(bool)
    assert bit[stay].all() and not bit[closed].any() and not bit[opened].any()      # a re-opened cell's bit waits for the next update
    assert tot2.sum() == (cnt2 == 0).sum()


def test_update_and_partial_draw_respect_the_marks(dev):
    """after marking, a full nsr_occ_update with positive sigmas on every cell leaves every marked cell at -1 with a zero bit, and
    the occupied half of a partial nsr_occ_sample_points draws no marked cell"""
    from nerfstyle_amd import _lib as L
    case = (16, 3, 3, 1.5, 0, 1.5, 1)
    H, C, bound = 16, 3, 1.5
    cells, H3 = C * H ** 3, H ** 3
    st, g, _, cnt, _ = call(dev, case, np.zeros(cells, F32), None, cameras(3, 0))
    marked = cnt == 0
    assert st == NSR_OK and 0 < marked.sum() < cells
    lib = L.lib()
    ws = Banded(dev, int(lib.nsr_occ_workspace_bytes(C, H)), 5)
    grid, bits, mean = Banded(dev, cells * 4, 6).put(g), Banded(dev, cells // 8, 7), Banded(dev, 4, 8)
    sig = torch.as_tensor((np.random.default_rng(0).random(cells) * 3 + 0.5).astype(F32), device=dev)
    assert lib.nsr_occ_update(grid.ptr(), L.p(sig), None, cells, C, H, 1, 0.95, 0.01, bits.ptr(), mean.ptr(), None, ws.ptr(),
                              L.stream()) == NSR_OK
    torch.cuda.synchronize()
    for x, what in ((ws, 'the workspace'), (grid, 'density_grid'), (bits, 'the bitfield'), (mean, 'mean_density')):
        x.check(what)
    after, bit = grid.get(F32), np.unpackbits(bits.get(np.uint8), bitorder='little').astype(bool)
    assert (after[marked] == -1).all() and not bit[marked].any()
    assert np.array_equal(after[~marked], sig.cpu().numpy()[~marked]) and bit[~marked].all()
    P = int(lib.nsr_occ_num_points(C, H, 0))
    xyzs, idx = Banded(dev, P * 12, 9), Banded(dev, P * 4, 10)
    assert lib.nsr_occ_sample_points(grid.ptr(), C, H, bound, 0, 1234, 0, None, None, xyzs.ptr(), idx.ptr(), ws.ptr(), L.stream()) == NSR_OK
    torch.cuda.synchronize()
    for x, what in ((ws, 'the workspace'), (xyzs, 'xyzs'), (idx, 'indices')):
        x.check(what)
    drawn = idx.get(np.int32).reshape(C, 2, H3 // 4)
    assert (drawn >= 0).all() and not marked[drawn[:, 1]].any()
    assert marked[drawn[:, 0]].any()                                       # the uniform half does land on marked cells; they stay -1


# ---- through the Renderer: no training sample is lost ---------------------------------------------------------------------------
def _small_renderer(dev):
    from nerfstyle_amd.common import BBox, Intrinsics
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.style_nerf import StyleTCNerf
    m = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 2, use_dir=False)
    cfg = RendererConfig.llff()
    cfg.grid_size = 32
    intr = Intrinsics(24, 32, 30.0, 29.0, 15.5, 12.25)
    r = Renderer(m, cfg, intr, 2.0, raymarch_channels=5).to(dev)
    assert r.cascade == 2
    return r, intr


def _march_all(r, intr, poses, lens):
    """the training rays of every frame (all pixels), marched through r.density_bitfield into zeroed buffers"""
    from nerfstyle_amd import raymarching
    from nerfstyle_amd.rays import generate_rays
    o, d = [], []
    for P in poses:
        rays, _ = generate_rays(P, intr, None, camera_flip=r.cfg.flip_camera, device=r.device, lens=lens)
        o.append(rays.origins), d.append(rays.dirs)
    o, d = torch.cat(o), torch.cat(d)
    N = o.shape[0]
    M = r.sample_capacity(N)
    nears, fars = raymarching.near_far_from_aabb(o, d, r.aabb, r.cfg.min_near)
    dev = r.device
    out = (torch.zeros(M, 3, device=dev), torch.zeros(M, 4, device=dev), torch.zeros(N, 3, dtype=torch.int32, device=dev))
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    raymarching.march_rays_train_nosync(o, d, r.bound, r.density_bitfield, r.cascade, r.cfg.grid_size, nears, fars, M, counter, 0.,
                                        r.cfg.max_steps, out=out)
    torch.cuda.synchronize()
    return out + (counter,)


@pytest.mark.parametrize('with_lens', [False, True])
def test_no_training_sample_is_lost(dev, with_lens):
    """H = 32, C = 2, three 32 x 24 frames: the march of every training ray through the all-ones bitfield, and through the same
    bitfield after mark_untrained_grid(poses) at the default margin -- rays, counter, xyzs and deltas bit for bit, although bits
    were cleared.  Once more with rays through a lens whose k1 is not zero."""
    r, intr = _small_renderer(dev)
    poses = cameras(3, r.cfg.flip_camera)
    poses[2] = look_at((-1.2, 1.0, 2.9), (0.3, 0.0, 0.0))                   # instead of the camera that looks away
    poses[2, :, :3] *= np.asarray(U.flips(r.cfg.flip_camera), F32)
    lens = None
    if with_lens:
        from nerfstyle_amd.lens import LensRefiner
        Lr = LensRefiner(intr).to(dev)
        with torch.no_grad():
            Lr.dist.copy_(torch.tensor([0.06, 0.01]))
            Lr.center.copy_(torch.tensor([0.4, -0.3]))
        lens = Lr().detach()
    r.density_bitfield.fill_(0xFF)
    full = _march_all(r, intr, poses, lens)
    n_samples = int(full[3][0])
    assert n_samples > 10000 and not r.density_grid.any()
    n_un, counts = r.mark_untrained_grid(poses, lens=lens, return_counts=True)
    n_un, counts = n_un.cpu().numpy(), counts.cpu().numpy().reshape(-1)
    grid, bits = r.density_grid.cpu().numpy().reshape(-1), r.density_bitfield.cpu().numpy()
    cleared = ~np.unpackbits(bits, bitorder='little').astype(bool)
    assert cleared.any() and np.array_equal(cleared, counts == 0) and np.array_equal(grid == -1, cleared) and (grid[~cleared] == 0).all()
    assert np.array_equal(n_un, cleared.reshape(2, -1).sum(1)) and n_un.dtype == np.int32
    cam = (intr.fx, intr.fy, intr.cx, intr.cy) if lens is None else tuple(lens.cpu().tolist())
    frustum = U.lens_frustum(32, 24, cam + ((0.0, 0.0) if lens is None else ()))
    assert np.array_equal(counts, U.counts(2, 32, 2.0, poses, frustum, r.cfg.flip_camera, 1.5))
    marked = _march_all(r, intr, poses, lens)
    for a, b, what in zip(full, marked, ('xyzs', 'deltas', 'rays', 'the counter')):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), what
    # the marks are checkpoint state, and a second call changes nothing
    sd = r.state_dict()
    assert torch.equal(sd['density_grid'], r.density_grid) and (sd['density_grid'] == -1).any()
    again = r.mark_untrained_grid(torch.as_tensor(poses, device=dev), lens=lens)
    assert np.array_equal(again.cpu().numpy(), n_un) and np.array_equal(r.density_grid.cpu().numpy().reshape(-1), grid)
    assert np.array_equal(r.density_bitfield.cpu().numpy(), bits)
