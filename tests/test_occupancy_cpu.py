"""tests/occupancy_ref.py (the NumPy restatement tests/test_gpu_occupancy.py compares the kernels with) against the reference's
own torch expressions run on the CPU (renderer.py:130-133, :158/:180, :183-190) and the oracle's Morton code, and the host side of
the occupancy entry points (shape predicate, workspace size, argument checks) through the C-ABI library -- no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import occupancy_ref as R

F32 = np.float32
NSR_ERR_INVALID_ARG = -1
NON_POW2 = (24, 40, 48, 72, 96)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _torch_positions(coords, cas, H, bound, noise):
    """renderer.py:158 (= :180) and :130-133, float32 on the CPU, `noise` in place of torch.rand_like"""
    xyzs = 2 * torch.as_tensor(coords.astype(np.int32)).float() / (H - 1) - 1
    b = min(2 ** cas, bound)
    half_grid_size = b / H
    cas_xyzs = xyzs * (b - half_grid_size)
    cas_xyzs += (torch.as_tensor(noise) * 2 - 1) * half_grid_size
    assert cas_xyzs.dtype == torch.float32
    return cas_xyzs.numpy()


def _grid(rng, C, H3):
    g = np.where(rng.random((C, H3)) < 0.1, rng.random((C, H3)) + 0.01, 0.0).astype(F32)
    g[:, 1::7] = -1
    return g


# ---------------------------------------------------------------------------------------------
# positions and indices against the torch expressions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bound', [0.5, 1.5, 2.0, 4.0])
@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('H', [8, 32])
def test_sample_points_match_torch_expressions(O, H, C, bound):
    """bit for bit: with these bounds and a power-of-two H, bound - bound / H is exact in fp32, so the reference's Python double
    scalars and the kernel's fp32 scalars are the same numbers"""
    H3 = H ** 3
    rng = np.random.default_rng(1000 * H + 10 * C + int(bound * 2))
    # full update: the meshgrid cells, written at their Morton index
    xx, yy, zz = np.meshgrid(np.arange(H), np.arange(H), np.arange(H), indexing='ij')
    coords = np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], axis=1).astype(np.int32)
    where = O.morton3D(coords).astype(np.int64)
    noise = rng.random((C * H3, 3), dtype=F32)
    xyz, idx = R.sample_points(None, C, H, bound, True, 1, 0, noise=noise)
    assert np.array_equal(idx, np.arange(C * H3, dtype=np.int32))
    for cas in range(C):
        want = _torch_positions(coords, cas, H, bound, noise[cas * H3 + where])
        assert np.array_equal(_bits(xyz[cas * H3 + where]), _bits(want))
    # partial update: the drawn cells, their coordinates from the oracle's inverse
    grid = _grid(rng, C, H3)
    P = R.num_points(C, H, False)
    noise = rng.random((P, 3), dtype=F32)
    xyz, idx = R.sample_points(grid, C, H, bound, False, 77, 3, noise=noise)
    per = P // C
    for cas in range(C):
        ii = idx[cas * per:(cas + 1) * per].astype(np.int64)
        assert ii.min() >= cas * H3 and ii.max() < (cas + 1) * H3
        assert np.all(grid[cas][ii[per // 2:] - cas * H3] > 0)
        want = _torch_positions(O.morton3D_invert((ii - cas * H3).astype(np.int32)), cas, H, bound, noise[cas * per:(cas + 1) * per])
        assert np.array_equal(_bits(xyz[cas * per:(cas + 1) * per]), _bits(want))


@pytest.mark.parametrize('H', [8, 32])
def test_sample_points_inexact_bound_within_one_ulp_of_the_span(O, H):
    """bound = 1.3: the reference computes 1.3 - 1.3 / H in double and rounds the difference to fp32 ONCE (when the scalar meets
    the float32 tensor); the kernel receives 1.3 already rounded to fp32 and rounds the difference again, so the two spans can
    differ by one unit in the last place -- of a number in [1, 2), that is s = 2^-23; the spans themselves are held to that.
    b / H is the same number on both sides (a power-of-two H only shifts the exponent).  Cascade 0 (b = 1) stays bit-exact.
    What one ulp of the span does to a position: the exact products xn * span differ by at most s (|xn| <= 1) and rounding is
    monotonic on a grid no coarser than s (|product| <= span < 2), so the rounded products differ by at most s; the same jitter
    term is added to both, and the two sums (below 2 in magnitude) round by at most s / 2 each: 2 s in all."""
    C, bound, H3 = 2, 1.3, H ** 3
    rng = np.random.default_rng(H)
    coords = R.morton_invert(np.arange(H3)).astype(np.int32)
    assert np.array_equal(coords, O.morton3D_invert(np.arange(H3, dtype=np.int32)))
    noise = rng.random((C * H3, 3), dtype=F32)
    xyz, _ = R.sample_points(None, C, H, bound, True, 1, 0, noise=noise)
    span, half = R.cascade_scales(np.array([0, 1]), H, bound)
    span_torch = (torch.ones(1) * (bound - bound / H)).numpy()[0]
    assert 1.0 <= span[1] < 2.0 and abs(float(span[1]) - float(span_torch)) <= 2.0 ** -23
    assert half[1] == (torch.ones(1) * (bound / H)).numpy()[0]
    assert np.array_equal(_bits(xyz[:H3]), _bits(_torch_positions(coords, 0, H, bound, noise[:H3])))
    diff = np.abs(xyz[H3:].astype(np.float64) - _torch_positions(coords, 1, H, bound, noise[H3:]).astype(np.float64))
    assert np.abs(xyz[H3:]).max() < 2.0 and diff.max() <= 2 * 2.0 ** -23


def test_morton_against_the_oracle(O):
    """idx of a full update, inverted through the oracle's morton3D_invert, gives exactly the meshgrid coordinates"""
    for H in (8, 32):
        H3 = H ** 3
        _, idx = R.sample_points(None, 2, H, 2.0, True, 0, 0, noise=np.zeros((2 * H3, 3), F32))
        xx, yy, zz = np.meshgrid(np.arange(H), np.arange(H), np.arange(H), indexing='ij')
        coords = np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], axis=1).astype(np.int32)
        for cas in range(2):
            inv = O.morton3D_invert((idx[cas * H3:(cas + 1) * H3] - cas * H3).astype(np.int32))
            assert np.array_equal(inv[O.morton3D(coords)], coords)
            assert np.array_equal(inv[np.lexsort((inv[:, 2], inv[:, 1], inv[:, 0]))], coords)
        assert np.array_equal(R.morton(coords[:, 0], coords[:, 1], coords[:, 2]).astype(np.int32), O.morton3D(coords))
    # where a Morton index leaves the grid: only a power-of-two H keeps morton(H-1, H-1, H-1) below H^3
    assert int(R.morton(23, 23, 23)) == 29183 >= 24 ** 3
    for H in (8, 16, 32, 64, 128, 256, 512):
        assert int(R.morton(H - 1, H - 1, H - 1)) == H ** 3 - 1
    for H in NON_POW2:
        assert int(R.morton(H - 1, H - 1, H - 1)) >= H ** 3


# ---------------------------------------------------------------------------------------------
# update against renderer.py:183-190
# ---------------------------------------------------------------------------------------------
def _torch_update(grid, tmp, decay):
    g, t = torch.as_tensor(grid.copy()), torch.as_tensor(tmp)
    valid_mask = (g >= 0) & (t >= 0)
    g[valid_mask] = torch.maximum(g[valid_mask] * decay, t[valid_mask])
    return g.numpy(), float(torch.mean(g.double().clamp(min=0)))


def _update_inputs(rng, C, H, with_nan):
    cells = C * H ** 3
    grid = np.where(rng.random(cells) < 0.4, rng.random(cells) * 3, 0.0).astype(F32)
    grid[rng.random(cells) < 0.15] = -1
    if with_nan:
        grid[rng.random(cells) < 0.05] = np.nan
    sig = (rng.random(cells) * 3).astype(F32)
    sig[rng.random(cells) < 0.1] = -1
    sig[rng.random(cells) < 0.1] = np.nan
    sig[rng.random(cells) < 0.1] = 0.0
    sig[rng.random(cells) < 0.05] = -2.5
    return grid, sig


@pytest.mark.parametrize('with_nan', [False, True])
@pytest.mark.parametrize('decay', [0.95, 1.0, 0.0])
@pytest.mark.parametrize('C,H', [(1, 8), (3, 8), (2, 16)])
def test_update_matches_torch_lines(O, C, H, decay, with_nan):
    """a grid holding -1, 0 and positive cells (and NaN), a tmp holding -1 and NaN; index sets without duplicates, where index_put_
    has one legal outcome"""
    rng = np.random.default_rng(C * 100 + H + int(decay * 10))
    cells = C * H ** 3
    grid, sig = _update_inputs(rng, C, H, with_nan)
    # full update: tmp_grid = sigmas
    got, mean64, tmp = R.update(grid, sig, None, C, H, True, decay)
    want, mean_t = _torch_update(grid, sig, decay)
    assert np.array_equal(_bits(tmp), _bits(sig)) and np.array_equal(_bits(got), _bits(want))
    if not with_nan:
        assert abs(mean64 - mean_t) <= 1e-12 * mean_t              # two double sums of <= 8192 addends: 8192 * 2^-53 each
    thr = min(F32(mean64), F32(0.7))
    assert np.array_equal(R.packbits(got, thr), O.packbits(got.reshape(C, -1), thr))
    # partial update: distinct cells, a quarter of the points carrying -1 (no point)
    P = R.num_points(C, H, False)
    idx = rng.permutation(cells)[:P].astype(np.int32)
    s = sig[:P]
    t_tmp = -torch.ones(cells)
    keep = torch.as_tensor(rng.random(P) < 0.75)
    t_tmp[torch.as_tensor(idx.astype(np.int64))[keep]] = torch.as_tensor(s)[keep]
    idx[~keep.numpy()] = -1
    got, mean64, tmp = R.update(grid, s, idx, C, H, False, decay)
    want, mean_t = _torch_update(grid, t_tmp.numpy(), decay)
    assert np.array_equal(_bits(tmp), _bits(t_tmp.numpy())) and np.array_equal(_bits(got), _bits(want))
    if not with_nan:
        assert abs(mean64 - mean_t) <= 1e-12 * mean_t              # two double sums of <= 8192 addends: 8192 * 2^-53 each
    untouched = np.ones(cells, bool)
    untouched[idx[idx >= 0]] = False
    assert np.array_equal(_bits(got[untouched]), _bits(grid[untouched]))


def test_update_duplicates_pick_the_maximum_among_the_legal_outcomes():
    """several writers of one cell: index_put_ lets any of them win; the restatement (like k_occ_scatter) takes the largest"""
    C, H, decay = 2, 8, 0.95
    rng = np.random.default_rng(3)
    cells, P = C * H ** 3, R.num_points(C, H, False)
    grid = np.where(rng.random(cells) < 0.5, rng.random(cells) * 2, 0.0).astype(F32)
    idx = rng.integers(0, cells // 4, P).astype(np.int32)            # P = cells / 2 points on a quarter of the cells
    sig = (rng.random(P) * 2).astype(F32)
    got, _, tmp = R.update(grid, sig, idx, C, H, False, decay)
    writers = {}
    for p in range(P):
        writers.setdefault(int(idx[p]), []).append(sig[p])
    assert sum(len(set(w)) > 1 for w in writers.values()) > 100
    for cell in range(cells):
        if cell not in writers:
            assert got[cell] == grid[cell] and tmp[cell] == -1
            continue
        legal = [max(F32(grid[cell] * F32(decay)), s) for s in writers[cell]]
        assert got[cell] in legal and got[cell] == max(legal) and tmp[cell] == max(writers[cell])


def test_update_signed_zero_sigma():
    """+0.0 is a write (a positive cell decays), -0.0 is none (documented deviation: the cell keeps its value undecayed)"""
    grid = np.full(512, 2.0, F32)
    idx = np.full(256, -1, np.int32)
    idx[:2] = (5, 9)
    sig = np.ones(256, F32)
    sig[:2] = (0.0, -0.0)
    got, _, tmp = R.update(grid, sig, idx, 1, 8, False, 0.5)
    assert got[5] == 1.0 and got[9] == 2.0 and tmp[5] == 0.0 and not np.signbit(tmp[5]) and tmp[9] == -1


def test_packbits_is_strict():
    thr = F32(0.3)
    cells = np.array([thr, np.nextafter(thr, F32(1)), np.nextafter(thr, F32(0)), np.nan, -1, 0, 1, np.inf], F32)
    assert R.packbits(cells, thr).tolist() == [0b11000010]
    assert R.packbits(np.zeros(16, F32), 0.0).tolist() == [0, 0]


def test_mean_bound_counts_the_additions():
    assert R.mean_bound(1, 8) == 2 * (1 + 10 + 1) * 2.0 ** -24            # 2 blocks, one cell per thread
    assert R.mean_bound(2, 64) == 2 * (1 + 10 + 1) * 2.0 ** -24           # 2048 blocks exactly
    assert R.mean_bound(2, 128) == 2 * (8 + 10 + 1) * 2.0 ** -24          # 8 grid-stride trips
    assert R.mean_bound(3, 64) == 2 * (2 + 10 + 1) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------
# host entry points
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def L():
    from nerfstyle_amd import build, _lib
    build.build()
    return _lib.lib()


def _refused_shapes():
    return ([(0, 32), (9, 32), (16, 512), (2, 4), (2, 0), (2, 1024), (8, 1024), (1, 2048), (0xFFFFFFFF, 8), (1, 0xFFFFFFF8)]
            + [(C, H) for H in NON_POW2 for C in (1, 2, 8)] + [(2, 12), (2, 100), (2, 129), (2, 511)])


def test_shape_predicate_and_workspace_size(L):
    """C in 1..8, H a power of two in 8..512.  C * H^3 < 2^31 never binds inside these limits: the largest accepted pair,
    C = 8 and H = 512, has exactly 2^30 cells; the first pair with 2^31 cells, C = 16 and H = 512, already has too many
    cascades"""
    for C, H in _refused_shapes():
        assert L.nsr_occ_workspace_bytes(C, H) == 0, (C, H)
        assert L.nsr_occ_num_points(C, H, 0) == 0 and L.nsr_occ_num_points(C, H, 1) == 0, (C, H)
    for C in range(1, 9):
        for H in (8, 16, 32, 64, 128, 256, 512):
            cells = C * H ** 3
            assert cells <= 1 << 30
            nbytes = L.nsr_occ_workspace_bytes(C, H)
            assert nbytes >= 8 * cells and nbytes % 16 == 0, (C, H)
            assert L.nsr_occ_num_points(C, H, 1) == R.num_points(C, H, True) == cells
            assert L.nsr_occ_num_points(C, H, 0) == R.num_points(C, H, False) == cells // 2
    assert L.nsr_occ_num_points(8, 512, 1) == 1 << 30


def test_entry_points_refuse_before_any_launch(L):
    """every call below must return NSR_ERR_INVALID_ARG from the host checks (there is no device here to launch on); the
    pointers are host memory that is never read"""
    C, H = 2, 8
    cells = C * H ** 3
    buf = np.zeros(8 * 1024 + 16, F32)                               # eight 4 KiB slots
    base = (buf.ctypes.data + 63) & ~63
    g, s, x, i, w, b, m = (ctypes.c_void_p(base + 4096 * k) for k in range(7))
    seq = ctypes.c_void_p(base + 4096 * 7)
    Pp, Pf = R.num_points(C, H, False), R.num_points(C, H, True)

    def sample(grid=g, C=C, H=H, bound=2.0, full=0, xyzs=x, idx=i, ws=w):
        return L.nsr_occ_sample_points(grid, C, H, bound, full, 1, 0, seq, None, xyzs, idx, ws, None)

    def update(grid=g, sig=s, idx=i, P=Pp, C=C, H=H, full=0, bits=b, mean=m, ws=w):
        return L.nsr_occ_update(grid, sig, idx, P, C, H, full, 0.95, 0.01, bits, mean, seq, ws, None)

    for Cx, Hx in _refused_shapes():
        Px = 2 * Cx * (Hx ** 3 // 4) & 0xffffffff
        for full in (0, 1):
            assert sample(C=Cx, H=Hx, full=full) == NSR_ERR_INVALID_ARG, (Cx, Hx)
            assert update(C=Cx, H=Hx, full=full, P=Px) == NSR_ERR_INVALID_ARG, (Cx, Hx)
            assert update(C=Cx, H=Hx, full=full, P=0) == NSR_ERR_INVALID_ARG, (Cx, Hx)
    for bound in (0.0, -0.0, -1.0, float('nan'), -float('inf')):
        assert sample(bound=bound) == NSR_ERR_INVALID_ARG and sample(bound=bound, full=1) == NSR_ERR_INVALID_ARG
    for off in (1, 4, 8, 12):
        misaligned = ctypes.c_void_p(w.value + off)
        assert sample(ws=misaligned) == NSR_ERR_INVALID_ARG
        assert update(ws=misaligned) == NSR_ERR_INVALID_ARG and update(ws=misaligned, full=1, P=Pf, idx=None) == NSR_ERR_INVALID_ARG
        assert update(grid=ctypes.c_void_p(g.value + off)) == NSR_ERR_INVALID_ARG          # packbits reads the grid as float4
    for P, full in ((Pf, 0), (Pp, 1), (0, 0), (0, 1), (Pp - 1, 0), (Pp + 1, 0), (Pf - 1, 1), (Pf + 1, 1)):
        assert update(P=P, full=full) == NSR_ERR_INVALID_ARG
    assert update(idx=None) == NSR_ERR_INVALID_ARG                                          # a partial update needs its indices
    for kw in ('grid', 'xyzs', 'idx', 'ws'):
        assert sample(**{kw: None}) == NSR_ERR_INVALID_ARG and sample(full=1, **{kw: None}) == NSR_ERR_INVALID_ARG
    for kw in ('grid', 'sig', 'bits', 'mean', 'ws'):
        assert update(**{kw: None}) == NSR_ERR_INVALID_ARG and update(full=1, P=Pf, **{kw: None}) == NSR_ERR_INVALID_ARG
    assert not buf.any()
