"""nsr_occ_sample_points and nsr_occ_update (csrc/occupancy.hip, nine kernels) called directly through the C ABI and compared
with their NumPy restatement (occupancy_ref.py): the occupied-cell list, every drawn index, every position bit, the grid after
the update and the bitfield exactly; the mean within occupancy_ref.mean_bound, a counted bound.  No field: the sigmas are
synthetic.

Every call runs twice, on a workspace exactly nsr_occ_workspace_bytes long that was filled with different garbage (the call must
initialise every counter it reads), between guard bands that must stay untouched; the grid, xyzs, indices, the bitfield, the mean
and the sequence counter sit between canary bands of their own, and the outputs are pre-filled with a pattern no result has.

The only tolerances in this file are mean_bound and the chi-square quantile written down at test_uniform_half_chi_square."""
import numpy as np
import pytest
import torch

import occupancy_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 4096                 # bytes on each side of every buffer
NSR_OK = 0
NAN = F32('nan')
DENORM = np.nextafter(F32(0), F32(1))                        # the smallest positive denormal
SHAPES = [(8, 1), (8, 8), (16, 3), (32, 2), (64, 2), (64, 3), (128, 2)]         # (H, C)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _garbage(nbytes, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev, generator=g)


class Banded:
    """`nbytes` device bytes at a 256-byte aligned address between two guard bands of random bytes"""

    def __init__(self, dev, nbytes, seed, fill=None):
        self.buf = _garbage(nbytes + 2 * GUARD + 256, dev, seed)
        self.off = ((self.buf.data_ptr() + GUARD + 255) & ~255) - self.buf.data_ptr()
        self.nbytes = nbytes
        assert self.off >= GUARD and self.buf.numel() - (self.off + nbytes) >= GUARD
        if fill is not None:
            self.bytes()[:] = fill
        self.lo, self.hi = self.buf[:self.off].clone(), self.buf[self.off + nbytes:].clone()

    def bytes(self):
        return self.buf[self.off:self.off + self.nbytes]

    def view(self, dtype):
        return self.bytes().view(dtype)

    def put(self, array):
        self.bytes().copy_(torch.as_tensor(np.ascontiguousarray(array).reshape(-1).view(np.uint8)))

    def ptr(self):
        return self.buf.data_ptr() + self.off

    def check(self, what):
        assert torch.equal(self.buf[:self.off], self.lo), 'write below ' + what
        assert torch.equal(self.buf[self.off + self.nbytes:], self.hi), 'write past the end of ' + what


def _workspace(dev, C, H, seed):
    from nerfstyle_amd import _lib as L
    nbytes = int(L.lib().nsr_occ_workspace_bytes(C, H))
    assert nbytes >= 8 * C * H ** 3
    return Banded(dev, nbytes, seed)


UNWRITTEN = 0x7F                 # 0x7F7F7F7F: no cell index (>= 2^31 - 2^24) and no position (3.4e38)


def run_sample(dev, grid, C, H, bound, full, seed, sequence, seq_dev=None, noise=None):
    """-> (xyzs f32 [P,3], idx i32 [P]) of the device, after the harness checks"""
    from nerfstyle_amd import _lib as L
    P = int(L.lib().nsr_occ_num_points(C, H, int(full)))
    assert P == R.num_points(C, H, full)
    grid = np.ascontiguousarray(grid, F32).reshape(-1)
    assert grid.size == C * H ** 3
    g = Banded(dev, grid.nbytes, 11)
    g.put(grid)
    noise_d = None if noise is None else torch.as_tensor(np.ascontiguousarray(noise, F32), device=dev)
    sq = None
    if seq_dev is not None:
        sq = Banded(dev, 4, 12)
        sq.put(np.array([seq_dev], np.uint32))
    results = []
    for run in (1, 2):
        ws = _workspace(dev, C, H, 20 + run)
        xyzs, idx = Banded(dev, P * 12, 13, UNWRITTEN), Banded(dev, P * 4, 14, UNWRITTEN)
        st = L.lib().nsr_occ_sample_points(g.ptr(), C, H, bound, int(full), seed, sequence, None if sq is None else sq.ptr(),
                                           L.p(noise_d), xyzs.ptr(), idx.ptr(), ws.ptr(), L.stream())
        assert st == NSR_OK
        torch.cuda.synchronize()
        ws.check('the workspace'), g.check('density_grid'), xyzs.check('xyzs'), idx.check('indices')
        assert np.array_equal(g.view(torch.int32).cpu().numpy(), grid.view(np.int32)), 'density_grid was modified'
        if sq is not None:
            sq.check('sequence_dev')
            assert int(sq.view(torch.int32).cpu().numpy().view(np.uint32)[0]) == seq_dev, 'sequence_dev was modified'
        results.append((xyzs.view(torch.float32).cpu().numpy().reshape(P, 3), idx.view(torch.int32).cpu().numpy()))
    assert np.array_equal(results[0][1], results[1][1]) and np.array_equal(_bits(results[0][0]), _bits(results[1][0])), \
        'the result depends on what the workspace held'
    xyz, idx = results[0]
    assert not (idx == 0x7F7F7F7F).any() and not (_bits(xyz) == 0x7F7F7F7F).any(), 'outputs left unwritten'
    return xyz, idx


def check_sample(dev, grid, C, H, bound, full, seed, sequence, seq_dev=None, noise=None):
    xyz, idx = run_sample(dev, grid, C, H, bound, full, seed, sequence, seq_dev, noise)
    want_xyz, want_idx = R.sample_points(grid, C, H, bound, full, seed, sequence + (seq_dev or 0), noise)
    bad = np.flatnonzero(idx != want_idx)
    assert bad.size == 0, 'index of point {}: {} != {} ({} differ)'.format(bad[0], idx[bad[0]], want_idx[bad[0]], bad.size)
    bad = np.flatnonzero((_bits(xyz) != _bits(want_xyz)).any(axis=1))
    assert bad.size == 0, 'position of point {}: {} != {} ({} differ)'.format(bad[0], xyz[bad[0]], want_xyz[bad[0]], bad.size)
    return xyz, idx


# ---------------------------------------------------------------------------------------------
# grids: which cells are occupied
# ---------------------------------------------------------------------------------------------
def _cascade(rng, H3, occupied):
    """the occupied cells hold positive values (every 5th the smallest denormal), all others a mix of what must NOT count:
    -1 (the reference's never-update marker), -0.0, +0.0 and NaN"""
    g = np.array([-1.0, -0.0, 0.0, NAN], F32)[rng.integers(0, 4, H3)]
    occupied = np.asarray(occupied, np.int64)
    vals = (rng.random(occupied.size) * 4 + 0.001).astype(F32)
    vals[::5] = DENORM
    g[occupied] = vals
    return g


PATTERNS = {
    'empty': lambda rng, H3: [],
    'cell0': lambda rng, H3: [0],
    'last_cell': lambda rng, H3: [H3 - 1],
    'all': lambda rng, H3: np.arange(H3),
    'last_block': lambda rng, H3: np.arange(H3 - 256, H3),
    'every_257th': lambda rng, H3: np.arange(0, H3, 257),
    'random_10pct': lambda rng, H3: np.flatnonzero(rng.random(H3) < 0.1),
}
NAMES = list(PATTERNS)


def _blocks_around_1024(rng, H3):
    """H = 128: blocks 1023, 1024, 1025 (the last of k_occ_scan's first trip, the first two of its second) full, everything before
    block 1023 sparse, the rest at 10 %"""
    occ = rng.random(H3) < 0.1
    occ[:1023 * 256] = rng.random(1023 * 256) < 0.001
    occ[1023 * 256:1026 * 256] = True
    return np.flatnonzero(occ)


def _grid(H, C, rot, seed=0):
    """cascade c holds pattern (rot + c) mod 7: different patterns in the cascades of one call, so a count or a carry that
    crosses from one cascade into the next shows"""
    rng = np.random.default_rng(1000 * H + 10 * C + rot + seed)
    H3 = H ** 3
    return np.stack([_cascade(rng, H3, PATTERNS[NAMES[(rot + c) % len(NAMES)]](rng, H3)) for c in range(C)])


PARTIAL_CASES = ([(H, C, 2.0, rot) for H, C in [(8, 1), (8, 8), (16, 3), (32, 2), (64, 2)] for rot in range(len(NAMES))]
                 + [(H, C, 1.5, 6) for H, C in [(8, 1), (8, 8), (16, 3), (32, 2), (64, 2)]]
                 + [(16, 3, 4.0, 3), (8, 1, 0.5, 6), (8, 8, 4.0, 5)])


@pytest.mark.parametrize('H,C,bound,rot', PARTIAL_CASES)
def test_partial_sample_points(dev, H, C, bound, rot):
    check_sample(dev, _grid(H, C, rot), C, H, bound, False, 0x1234ABCD, 7)


@pytest.mark.parametrize('bound,rot', [(2.0, 0), (2.0, 2), (2.0, 4), (1.5, 6), (2.0, 'around_1024')])
def test_partial_sample_points_scan_carry(dev, bound, rot):
    """H = 128: 8192 blocks per cascade, eight trips of k_occ_scan's loop, the running sum carried from trip to trip and started
    again at 0 for cascade 1"""
    H, C, H3 = 128, 2, 128 ** 3
    if rot == 'around_1024':
        rng = np.random.default_rng(5)
        grid = np.stack([_cascade(rng, H3, _blocks_around_1024(rng, H3)), _cascade(rng, H3, np.arange(0, H3, 257))])
        assert R.occupied(grid[0])[:1023 * 256].size < 1023 * 256 and (grid[0][1023 * 256:1026 * 256] > 0).all()
    else:
        grid = _grid(H, C, rot)
    check_sample(dev, grid, C, H, bound, False, 99, 3)


def test_one_cell_and_empty_cascades(dev):
    """stated without the restated draw: with one occupied cell every point of the second half is that cell; an empty cascade's
    second half is -1 while the others' is not; the first half always lies in its own cascade"""
    H, C, H3 = 16, 3, 16 ** 3
    N = H3 // 4
    rng = np.random.default_rng(8)
    grid = np.stack([_cascade(rng, H3, []), _cascade(rng, H3, [0]), _cascade(rng, H3, [H3 - 1])])
    grid[2, H3 - 1] = DENORM
    xyz, idx = check_sample(dev, grid, C, H, 2.0, False, 5, 0)
    ii = idx.reshape(C, 2, N)
    for cas in range(C):
        assert ii[cas, 0].min() >= cas * H3 and ii[cas, 0].max() < (cas + 1) * H3
    assert (ii[0, 1] == -1).all() and (ii[1, 1] == H3).all() and (ii[2, 1] == 3 * H3 - 1).all()


@pytest.mark.parametrize('seed', [0, 1234, (1 << 32) + 5, 0xDEADBEEF00000000, (1 << 64) - 1])
@pytest.mark.parametrize('sequence', [0, (1 << 32) - 1, (1 << 32) - 2])
def test_seeds_and_sequences(dev, seed, sequence):
    """both key words and the whole range of the sequence word are used"""
    check_sample(dev, _grid(16, 3, 4), 3, 16, 2.0, False, seed, sequence)


def test_seed_words_and_sequence_change_the_draw(dev):
    grid = _grid(16, 3, 4)
    base = run_sample(dev, grid, 3, 16, 2.0, False, 5, 9)
    for seed, sequence in ((5 + (1 << 32), 9), (6, 9), (5, 10)):
        other = run_sample(dev, grid, 3, 16, 2.0, False, seed, sequence)
        assert not np.array_equal(base[1], other[1]) and not np.array_equal(_bits(base[0]), _bits(other[0]))


def test_sequence_dev_is_added(dev):
    """sequence = 5 with sequence_dev[0] = 2 draws what sequence = 7 draws, and not what sequence = 5 draws; the sum wraps"""
    grid = _grid(16, 3, 6)
    a = check_sample(dev, grid, 3, 16, 2.0, False, 77, 5, seq_dev=2)
    b = check_sample(dev, grid, 3, 16, 2.0, False, 77, 7)
    c = check_sample(dev, grid, 3, 16, 2.0, False, 77, 5)
    assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
    assert not np.array_equal(a[1], c[1]) and not np.array_equal(_bits(a[0]), _bits(c[0]))
    d = run_sample(dev, grid, 3, 16, 2.0, False, 77, (1 << 32) - 1, seq_dev=8)
    assert np.array_equal(d[1], b[1]) and np.array_equal(_bits(d[0]), _bits(b[0]))
    for full_seq in ((5, 2), (7, None)):
        check_sample(dev, grid, 3, 16, 2.0, True, 77, full_seq[0], seq_dev=full_seq[1])


@pytest.mark.parametrize('H,C', [(8, 1), (16, 3), (32, 2)])
def test_partial_noise_overrides_the_jitter_only(dev, H, C):
    grid = _grid(H, C, 6)
    P = R.num_points(C, H, False)
    noise = np.random.default_rng(H).random((P, 3), dtype=F32)
    noise[:4] = [[0, 0, 0], [0.5, 0.5, 0.5], [np.nextafter(F32(1), F32(0))] * 3, [0, 0.25, 0.75]]
    with_noise = check_sample(dev, grid, C, H, 1.5, False, 31, 2, noise=noise)
    without = check_sample(dev, grid, C, H, 1.5, False, 31, 2)
    assert np.array_equal(with_noise[1], without[1]) and not np.array_equal(_bits(with_noise[0]), _bits(without[0]))


def test_uniform_half_chi_square(dev):
    """A backstop that does not lean on the restated draw: over the uniform half of (H, C) = (32, 1) -- 8192 points, decoded from
    the device's indices alone -- the histogram of each axis' coordinate over its 32 values against the uniform expectation of
    256.  The threshold is the chi-square quantile at 1 - 1e-6 for 31 degrees of freedom, 83.6425 (scipy.stats.chi2.ppf(1 - 1e-6,
    31) = 83.64251584691797); a modulo bias or a stuck bit lands far above it.  The restated draw, computed on the CPU, gives
    26.48, 22.80 and 44.16 for x, y and z at this seed and sequence."""
    H, N = 32, 32 ** 3 // 4
    xyz, idx = run_sample(dev, _grid(H, 1, 6), 1, H, 2.0, False, 2024, 1)
    coords = R.morton_invert(idx[:N].astype(np.uint32)).astype(np.int64)
    assert coords.min() >= 0 and coords.max() < H
    for axis in range(3):
        hist = np.bincount(coords[:, axis], minlength=H)
        chi2 = float(((hist - N / H) ** 2 / (N / H)).sum())
        print('chi-square axis', axis, chi2)
        assert chi2 < 83.6425


# ---------------------------------------------------------------------------------------------
# full update: point p is cell p
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_noise', [False, True])
@pytest.mark.parametrize('H,C,bound', [(8, 1, 0.5), (8, 1, 2.0), (32, 2, 1.5), (64, 3, 4.0), (64, 3, 2.0), (128, 2, 2.0)])
def test_full_sample_points(dev, H, C, bound, with_noise):
    """the contents of density_grid must not matter: it is all NaN"""
    cells = C * H ** 3
    noise = np.random.default_rng(H + C).random((cells, 3), dtype=F32) if with_noise else None
    xyz, idx = check_sample(dev, np.full(cells, NAN, F32), C, H, bound, True, (3 << 32) + 17, 4, noise=noise)
    assert np.array_equal(idx, np.arange(cells, dtype=np.int32))


# ---------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------
MEAN_SHARE = {}


def run_update(dev, grid, sigmas, idx, C, H, full, decay, thresh, seq0=None):
    """runs nsr_occ_update under the harness and holds it to the restatement: the grid exactly, the mean within mean_bound, the
    bitfield exactly packbits(device grid, min(device mean, thresh)), sequence_dev + 1.  -> (grid', mean, bitfield, tmp)"""
    from nerfstyle_amd import _lib as L
    cells = C * H ** 3
    grid = np.ascontiguousarray(grid, F32).reshape(-1)
    sigmas = np.ascontiguousarray(sigmas, F32).reshape(-1)
    P = R.num_points(C, H, full)
    assert grid.size == cells and sigmas.size == P
    sig_d = torch.as_tensor(sigmas, device=dev)
    idx_d = None if idx is None else torch.as_tensor(np.ascontiguousarray(idx, np.int32), device=dev)
    results = []
    for run in (1, 2):
        ws = _workspace(dev, C, H, 30 + run)
        g = Banded(dev, grid.nbytes, 31)
        g.put(grid)
        bits, mean = Banded(dev, cells // 8, 32, 0xA5), Banded(dev, 4, 33, UNWRITTEN)
        sq = None
        if seq0 is not None:
            sq = Banded(dev, 4, 34)
            sq.put(np.array([seq0], np.uint32))
        st = L.lib().nsr_occ_update(g.ptr(), L.p(sig_d), L.p(idx_d), P, C, H, int(full), decay, thresh, bits.ptr(), mean.ptr(),
                                    None if sq is None else sq.ptr(), ws.ptr(), L.stream())
        assert st == NSR_OK
        torch.cuda.synchronize()
        ws.check('the workspace'), g.check('density_grid'), bits.check('the bitfield'), mean.check('mean_density')
        if sq is not None:
            sq.check('sequence_dev')
            assert int(sq.view(torch.int32).cpu().numpy().view(np.uint32)[0]) == (seq0 + 1) & 0xffffffff
        results.append((g.view(torch.float32).cpu().numpy(), mean.view(torch.float32).cpu().numpy()[0],
                        bits.bytes().cpu().numpy()))
    for a, b in zip(results[0], results[1]):
        assert np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8)), \
            'the result depends on what the workspace held'
    got, mean, bitfield = results[0]
    want, mean64, tmp = R.update(grid, sigmas, idx, C, H, full, decay)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, 'cell {}: {} != {} (was {}, tmp {}; {} differ)'.format(bad[0], got[bad[0]], want[bad[0]], grid[bad[0]],
                                                                                 tmp[bad[0]], bad.size)
    bound = R.mean_bound(C, H)
    err = abs(float(mean) - mean64)
    if mean64 > 0:
        share = err / (bound * mean64)
        MEAN_SHARE[(H, C)] = max(MEAN_SHARE.get((H, C), 0.0), share)
        print('mean: device {!r} fp64 {!r} share of mean_bound({}, {}) {:.3f}'.format(float(mean), mean64, C, H, share))
    assert err <= bound * mean64
    assert np.array_equal(bitfield, R.packbits(got, min(F32(mean), F32(thresh))))
    return got, mean, bitfield, tmp


def _update_grid(rng, cells):
    """positive cells, zeros, the never-update marker -1, NaNs with different payloads, denormals"""
    g = np.where(rng.random(cells) < 0.4, rng.random(cells) * 3, 0.0).astype(F32)
    g[rng.random(cells) < 0.1] = -1
    g[rng.random(cells) < 0.02] = DENORM
    nan = np.flatnonzero(rng.random(cells) < 0.03)
    g.view(np.uint32)[nan] = 0x7FC00000 | rng.integers(1, 1 << 22, nan.size).astype(np.uint32) | \
        (rng.integers(0, 2, nan.size).astype(np.uint32) << np.uint32(31))
    return g


def _special_sigmas(rng, n):
    """mostly positive; NaN, negative and +0.0 among them"""
    s = (rng.random(n) * 3).astype(F32)
    s[rng.random(n) < 0.08] = NAN
    s[rng.random(n) < 0.08] = -1
    s[rng.random(n) < 0.04] = -2.5
    s[rng.random(n) < 0.08] = 0.0
    return s


FULL_UPDATE_CASES = ([(H, C, 0.95) for H, C in SHAPES] + [(H, C, d) for H, C in SHAPES[:4] for d in (1.0, 0.0)]
                     + [(64, 3, 1.0), (64, 2, 0.0)])


@pytest.mark.parametrize('H,C,decay', FULL_UPDATE_CASES)
def test_update_full(dev, H, C, decay):
    """indices == NULL and indices = arange give the same result; (64, 2) sits at the 2048-block cap of the grid-stride kernels,
    (64, 3) and (128, 2) above it"""
    cells = C * H ** 3
    rng = np.random.default_rng(H * C)
    grid, sig = _update_grid(rng, cells), _special_sigmas(rng, cells)
    thresh = 0.01 if decay == 0.95 else 5.0                      # below the mean / above it
    a = run_update(dev, grid, sig, None, C, H, True, decay, thresh, seq0=41)
    b = run_update(dev, grid, sig, np.arange(cells, dtype=np.int32), C, H, True, decay, thresh)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert (a[1] > thresh) == (decay == 0.95)
    minus = grid == -1
    assert minus.any() and np.array_equal(a[0][minus], grid[minus])                         # -1 stays -1 under any sigma
    with np.errstate(invalid='ignore'):
        dead = ~(sig >= 0)
    assert dead.any() and np.array_equal(_bits(a[0][dead]), _bits(grid[dead]))              # NaN / negative sigma: unchanged
    zero = (sig == 0) & (grid > 0)
    assert zero.any() and np.array_equal(a[0][zero], grid[zero] * F32(decay))               # +0.0 on a positive cell decays it


@pytest.mark.parametrize('H,C', [(8, 8), (16, 3), (32, 2), (64, 2), (64, 3), (128, 2)])
def test_update_partial_with_drawn_indices(dev, H, C):
    """the indices of a real nsr_occ_sample_points call: cells drawn several times, with different sigmas; the largest wins"""
    cells = C * H ** 3
    rng = np.random.default_rng(H + C)
    grid = _update_grid(rng, cells)
    _, idx = run_sample(dev, grid, C, H, 2.0, False, 99, 3)
    assert idx.min() >= 0 and np.array_equal(idx, R.sample_points(grid, C, H, 2.0, False, 99, 3)[1])
    sig = (rng.random(idx.size) * 3).astype(F32)
    sig[rng.random(idx.size) < 0.1] = 0.0
    smin, smax = np.full(cells, np.inf, F32), np.full(cells, -np.inf, F32)
    np.minimum.at(smin, idx, sig)
    np.maximum.at(smax, idx, sig)
    assert int((smax > smin).sum()) > 100
    got, _, _, tmp = run_update(dev, grid, sig, idx, C, H, False, 0.95, 0.01, seq0=0xFFFFFFFF)
    touched = np.isfinite(smax)
    assert np.array_equal(_bits(got[~touched]), _bits(grid[~touched]))                      # NaN payloads included
    assert np.array_equal(tmp[touched], smax[touched]) and (tmp[~touched] == -1).all()


@pytest.mark.parametrize('decay', [0.95, 1.0, 0.0])
@pytest.mark.parametrize('H,C', [(8, 1), (8, 8), (16, 3), (64, 3)])
def test_update_partial_hand_made_indices(dev, H, C, decay):
    cells, H3 = C * H ** 3, H ** 3
    P = R.num_points(C, H, False)
    rng = np.random.default_rng(H * C + 1)
    grid = _update_grid(rng, cells)
    none = np.full(P, -1, np.int32)
    # all -1: the grid is untouched, not even decayed
    got = run_update(dev, grid, _special_sigmas(rng, P), none, C, H, False, decay, 0.01)[0]
    assert np.array_equal(_bits(got), _bits(grid))
    # all points on one positive cell: the largest sigma lands there, nothing else moves
    cell = int(np.flatnonzero(grid > 1.0)[-1])
    sig = (rng.random(P) * 0.5).astype(F32)
    sig[P // 3] = 7.25
    got = run_update(dev, grid, sig, np.full(P, cell, np.int32), C, H, False, decay, 5.0, seq0=7)[0]
    assert got[cell] == 7.25 and np.array_equal(_bits(np.delete(got, cell)), _bits(np.delete(grid, cell)))
    # each point on a cell of its own -- both ends of every cascade among them -- with NaN, negative, +0.0 and -0.0 sigmas
    ends = np.array([c * H3 + e for c in range(C) for e in (0, 1, H3 - 2, H3 - 1)])
    rest = np.setdiff1d(rng.permutation(cells)[:P], ends)[:P - ends.size - 5]
    idx = none.copy()
    idx[:ends.size + rest.size] = rng.permutation(np.concatenate([ends, rest]))
    sig = _special_sigmas(rng, P)
    sig[rng.random(P) < 0.05] = -0.0
    live = idx >= 0
    got, _, _, tmp = run_update(dev, grid, sig, idx, C, H, False, decay, 0.01)
    hit = np.zeros(cells, bool)
    hit[idx[live]] = True
    assert np.array_equal(_bits(got[~hit]), _bits(grid[~hit]))
    with np.errstate(invalid='ignore'):
        no_write = live & (~(sig >= 0) | np.signbit(sig))
        zero = live & (sig == 0) & ~np.signbit(sig)
    assert no_write.sum() > 5 and np.array_equal(_bits(got[idx[no_write]]), _bits(grid[idx[no_write]]))
    assert (np.signbit(sig) & (sig == 0) & live).any()
    pos = zero & (grid[idx] > 0)
    assert pos.any() and np.array_equal(got[idx[pos]], grid[idx[pos]] * F32(decay))
    marked = live & (grid[idx] == -1) & (sig > 0)
    assert marked.any() and (got[idx[marked]] == -1).all()


@pytest.mark.parametrize('H,C', [(8, 1), (16, 3), (64, 3)])
def test_threshold_below_the_mean_is_strict(dev, H, C):
    """density_thresh below the mean: cells exactly at it, one ulp above and one ulp below, over all eight bit positions of the
    first byte, a middle byte and the last byte of the bitfield; only the cells above are set"""
    cells = C * H ** 3
    rng = np.random.default_rng(H)
    thresh = F32(0.3)
    kinds = [thresh, np.nextafter(thresh, F32(1)), np.nextafter(thresh, F32(0))]
    grid = (rng.random(cells) * 3 + 0.5).astype(F32)
    sig = (rng.random(cells) * 3).astype(F32)
    planted = []
    for k, byte in enumerate((0, 1, cells // 16 + 3, cells // 8 - 2, cells // 8 - 1)):
        for bit in range(8):
            cell = byte * 8 + bit
            grid[cell] = kinds[(bit + k) % 3]
            sig[cell] = 0.0
            planted.append((byte, bit, (bit + k) % 3 == 1))
    got, mean, bitfield, _ = run_update(dev, grid, sig, None, C, H, True, 1.0, float(thresh))
    assert mean > thresh
    for byte, bit, above in planted:
        assert got[byte * 8 + bit] == grid[byte * 8 + bit] and bool(bitfield[byte] >> bit & 1) == above, (byte, bit)


def test_all_zero_grid_and_sigmas(dev):
    """mean 0, threshold min(0, thresh) = 0, and under the strict > no bit is set"""
    for full in (True, False):
        P = R.num_points(2, 16, full)
        idx = None if full else np.random.default_rng(0).integers(0, 2 * 16 ** 3, P).astype(np.int32)
        got, mean, bitfield, _ = run_update(dev, np.zeros(2 * 16 ** 3, F32), np.zeros(P, F32), idx, 2, 16, full, 0.95, 0.01, seq0=0)
        assert mean == 0 and not got.any() and not bitfield.any()


def test_sample_update_sample_chain(dev):
    """sample -> sigma = a function of the cell -> update -> sample again: the second draw's occupied half follows the updated
    grid"""
    H, C, H3 = 32, 2, 32 ** 3
    N = H3 // 4
    grid = np.zeros(C * H3, F32)
    grid[H3 + 77] = 1.0
    _, idx = check_sample(dev, grid, C, H, 2.0, False, 8, 0)
    assert (idx.reshape(C, 2, N)[0, 1] == -1).all() and (idx.reshape(C, 2, N)[1, 1] == H3 + 77).all()
    sig = np.where(idx % 3 == 0, (idx % 1000).astype(F32) / F32(100), F32(0)).astype(F32)       # two thirds of the cells stay empty
    got = run_update(dev, grid, sig, idx, C, H, False, 0.95, 0.01, seq0=0)[0]
    occ = [R.occupied(got[c * H3:(c + 1) * H3]) for c in range(C)]
    assert 100 < occ[0].size < H3 // 4 and 100 < occ[1].size < H3 // 4
    _, idx2 = check_sample(dev, got, C, H, 2.0, False, 8, 1)
    for c in range(C):
        second = idx2.reshape(C, 2, N)[c, 1] - c * H3
        assert np.isin(second, occ[c]).all() and np.unique(second).size > occ[c].size // 2
