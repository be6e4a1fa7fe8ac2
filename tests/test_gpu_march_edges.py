"""nsr_march_rays_train (csrc/raymarch.hip) and nsr_march_rays called through the C ABI as raymarching.py calls them, on the
edge rays of march_ref.py, against the sequential oracle on the same arrays -- everything compared exactly, on bit views.
test_march_cpu.py proves on the CPU that these inputs put samples on lanes 0 and 63 of a wave block and bits 0 and 31 of a mask
word, skip whole blocks, are cut by max_steps and by far in mid-block, and start blocks just below a power of two.

Harness: xyzs, dirs and deltas are pre-filled with one NaN pattern and rays with a sentinel, each followed by a guard band that
must keep it; the workspace is exactly nsr_march_rays_train_workspace_bytes long, pre-filled with 0xFF bytes, guard band behind.
Expected buffers: the oracle's rows for every kept ray; without NDC, columns 2 and 3 of deltas keep the NaN (nsr.h: only written
when is_ndc); slots no ray owns and everything from M on keep the NaN; a dropped ray's slots inside [offset, M) are zeros -- the
kernels write them so that no consumer reads uninitialised memory, the reference has a zero-filled buffer there.

Which combinations run (march_ref.CASES) and why not the product: the four kernel routes differ in how they walk the step
sequence, the five (bound, C, H) in the probe's cascade and reciprocal arithmetic, dt_gamma in whether the closed-form step
applies at all.  Every route sees every (bound, C, H) once and both dt_gamma; max_steps follows from what a route needs (slot
capacity 0 for the re-marching emit; <= 514 on the 20 481-ray mask route to keep the oracle near a second, except the two
binade cases at bound 1; the binade values 514, 1028 and the control 1024 on the replay and the mask route).  The probe is one
function shared by all routes, so repeating every max_steps on every route would test the same arithmetic again.
The contract cases (incoming counter, dirs = NULL, capacity M at the edges) and `noises` run once per route they name."""
import numpy as np
import pytest
import torch

import march_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN_BITS = 0x7FC00000
SENTINEL = -7
GUARD = 1024                         # elements behind every buffer
CASE_IDS = [R.case_id(c) for c in R.CASES]


def _dev(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _tile(case_arrays, N):
    """the 769 base rays repeated up to N rays"""
    idx = np.arange(N) % R.N_EDGE
    return [np.ascontiguousarray(a[idx]) for a in case_arrays]


def _inputs(O, case, noises=False):
    route, bound, C, H, ms, g, _ = case
    bf, ro, rd, ne, fa, labels, zh = R.case_inputs(O, case)
    N = R.N_MASK if route == 'mask' else R.N_EDGE
    ro, rd, ne, fa, zh = _tile((ro, rd, ne, fa, zh), N)
    return bf, ro, rd, ne, fa, zh, (R.edge_noises(N) if noises else None)


def _nan_buffer(rows, cols, dev):
    t = torch.full(((rows + GUARD) * cols,), NAN_BITS, dtype=torch.int32, device=dev)
    return t


def gpu_march_train(dev, bf, ro, rd, ne, fa, bound, C, H, ms, g, M, is_ndc=False, z_hats=None, noises=None, counter0=(0, 0),
                    want_dirs=True):
    """-> xyzs [M, 3], dirs [M, 3] | None, deltas [M, 4] as uint32 bit views, rays [N, 3], counter [2]; guard bands checked"""
    from nerfstyle_amd import _lib as L
    N = len(ro)
    xyzs, deltas = _nan_buffer(M, 3, dev), _nan_buffer(M, 4, dev)
    dirs = _nan_buffer(M, 3, dev) if want_dirs else None
    rays = torch.full(((N + GUARD) * 3,), SENTINEL, dtype=torch.int32, device=dev)
    counter = torch.full((2 + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    counter[:2] = torch.tensor(counter0, dtype=torch.int32)
    nbytes = int(L.lib().nsr_march_rays_train_workspace_bytes(N, float(bound), int(ms)))
    assert nbytes % 4 == 0
    ws = torch.full((nbytes + 4 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    t = [_dev(a, dev) for a in (ro, rd, bf, ne, fa)]
    zh = _dev(z_hats, dev) if is_ndc else None
    no = _dev(noises, dev) if noises is not None else None
    st = L.lib().nsr_march_rays_train(L.p(t[0]), L.p(t[1]), L.p(zh), L.p(t[2]), float(bound), float(g), int(ms), int(is_ndc), N, C, H, M,
                                      L.p(t[3]), L.p(t[4]), L.p(xyzs), L.p(dirs), L.p(deltas), L.p(rays), L.p(counter), L.p(no),
                                      L.p(ws), L.stream())
    assert st == 0
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xFF).all()), 'write past the end of the workspace'
    assert bool((rays[N * 3:] == SENTINEL).all()) and bool((counter[2:] == SENTINEL).all())
    out = []
    for buf, cols in ((xyzs, 3), (dirs, 3), (deltas, 4)):
        if buf is None:
            out.append(None)
            continue
        assert bool((buf[M * cols:] == NAN_BITS).all()), 'write behind M'
        out.append(buf[:M * cols].cpu().numpy().view(np.uint32).reshape(M, cols))
    return out[0], out[1], out[2], rays[:N * 3].cpu().numpy().reshape(N, 3), counter[:2].cpu().numpy()


def expected_train(O, bf, ro, rd, ne, fa, bound, C, H, ms, g, M, is_ndc=False, z_hats=None, noises=None, counter0=(0, 0)):
    """the oracle's output laid into NaN-filled buffers by the rules of the module docstring (bit views)"""
    xo, do, dlo, rays, cnt = O.march_rays_train(ro, rd, bound, bf, C, H, ne, fa, ms, dt_gamma=g, M=M, counter=np.array(counter0, np.int32),
                                                z_hats=z_hats, is_ndc=is_ndc, noises=noises)
    exp = [np.full((M, c), NAN_BITS, np.uint32) for c in (3, 3, 4)]
    full = [np.zeros((M, c), np.uint32) for c in (3, 3, 4)]
    m = len(xo)
    for e, a in zip(full, (xo, do, dlo)):
        e[:m] = R.bits(a).reshape(m, -1)
    kept = dropped = 0
    for n, o, c in rays:
        if c == 0:
            continue
        if o + c >= M:                                   # raymarching.cu:517
            dropped += 1
            for e in exp:
                e[o:min(o + c, M)] = 0
            continue
        kept += 1
        exp[0][o:o + c], exp[1][o:o + c] = full[0][o:o + c], full[1][o:o + c]
        exp[2][o:o + c, :4 if is_ndc else 2] = full[2][o:o + c, :4 if is_ndc else 2]
    return exp, rays, cnt, kept, dropped


def check_train(O, dev, case, M=None, slack=64, noises=False, counter0=(0, 0), want_dirs=True, arrays=None):
    route, bound, C, H, ms, g, _ = case
    bf, ro, rd, ne, fa, zh, no = arrays if arrays is not None else _inputs(O, case, noises)
    is_ndc = route == 'ndc'
    if M is None:                                        # every ray kept: the oracle's total + slack
        total = int(O.march_rays_train(ro, rd, bound, bf, C, H, ne, fa, ms, dt_gamma=g, M=1, noises=no)[4][0])
        M = counter0[0] + total + slack
    exp, rays_o, cnt_o, kept, dropped = expected_train(O, bf, ro, rd, ne, fa, bound, C, H, ms, g, M, is_ndc, zh, no, counter0)
    x, d, dl, rays, cnt = gpu_march_train(dev, bf, ro, rd, ne, fa, bound, C, H, ms, g, M, is_ndc, zh, no, counter0, want_dirs)
    assert np.array_equal(cnt, cnt_o), (cnt, cnt_o)
    bad = np.flatnonzero((rays != rays_o).any(1))
    assert bad.size == 0, 'ray {}: {} != {} ({} rays differ)'.format(bad[0], rays[bad[0]], rays_o[bad[0]], bad.size)
    for name, got, want in (('xyzs', x, exp[0]), ('dirs', d, exp[1]), ('deltas', dl, exp[2])):
        if got is None:
            continue
        bad = np.flatnonzero((got != want).any(1))
        if bad.size:
            n = int(np.searchsorted(rays_o[:, 1], bad[0], 'right')) - 1
            raise AssertionError('{} slot {} (ray {}, its sample {}): {} != {}; {} slots differ'.format(
                name, bad[0], n, bad[0] - rays_o[n, 1], got[bad[0]].view(F32), want[bad[0]].view(F32), bad.size))
    return rays_o, kept, dropped


@pytest.mark.parametrize('case', R.CASES, ids=CASE_IDS)
def test_march_train_edge_rays_bit_exact(O, dev, case):
    """every route and configuration, with the binade rays where the case has them (they fail on the closed-form step that only
    checked t_1 .. t_span: max_steps 514 and 1028; 1024 is the control)"""
    rays_o, kept, dropped = check_train(O, dev, case)
    assert kept > 600 and dropped == 0


NOISE_CASES = [R.CASES[0], R.CASES[5], R.CASES[11], R.CASES[19]]         # one per route


@pytest.mark.parametrize('case', NOISE_CASES, ids=[R.case_id(c) for c in NOISE_CASES])
def test_march_train_noises(O, dev, case):
    """noises = 0, 0.5, the float below 1 and uniform random, interleaved: the start moves by that fraction of a step
    (raymarching.cu:452) and every later parameter with it"""
    route, bound, C, H, ms, g, _ = case
    bf, ro, rd, ne, fa, zh, no = _inputs(O, case, noises=True)
    plain = O.march_rays_train(ro, rd, bound, bf, C, H, ne, fa, ms, dt_gamma=g, M=1)[3][:, 2]
    rays_o, kept, dropped = check_train(O, dev, case, noises=True)
    assert (rays_o[:, 2] != plain).any() and dropped == 0


CONTRACT_CASES = [R.CASES[1], R.CASES[10]]                               # the replay route and the mask route


@pytest.mark.parametrize('case', CONTRACT_CASES, ids=[R.case_id(c) for c in CONTRACT_CASES])
def test_march_train_contract(O, dev, case):
    """Incoming counter (37, 0) offsets the allocation as the reference's atomics do; dirs = NULL; a capacity M that the last
    ray fits exactly (dropped: offset + count >= M, raymarching.cu:517) with the ray before it ending at M - 1 (kept); and an M
    that a ray straddles (dropped, zero-filled inside the buffer only, as is nothing behind M)."""
    route, bound, C, H, ms, g, _ = case
    rays_o, kept, dropped = check_train(O, dev, case, counter0=(37, 0))
    assert rays_o[0, 1] == 37 and dropped == 0
    check_train(O, dev, case, want_dirs=False)
    # the last ray: one sample (its far cut to half a step behind its start); the ray before it: one with samples
    bf, ro, rd, ne, fa, zh, _ = [a.copy() if a is not None else None for a in _inputs(O, case)]
    counts = O.march_rays_train(ro, rd, bound, bf, C, H, ne, fa, ms, dt_gamma=g, M=1)[3][:, 2]
    N = len(ro)
    heavy = np.flatnonzero(counts == counts.max())[:2]
    for dst, src in ((N - 1, heavy[0]), (N - 2, heavy[1])):
        for a in (ro, rd, ne, fa, zh):
            a[[dst, src]] = a[[src, dst]]
    fa[N - 1] = ne[N - 1] + F32(0.5) * R.dt_limits(ms, C, H)[0]
    rays_all = O.march_rays_train(ro, rd, bound, bf, C, H, ne, fa, ms, dt_gamma=g, M=1)
    counts, total = rays_all[3][:, 2], int(rays_all[4][0])
    assert counts[N - 1] == 1 and counts[N - 2] > 1
    arrays = (bf, ro, rd, ne, fa, zh, None)
    rays_o, kept, dropped = check_train(O, dev, case, M=total, arrays=arrays)
    assert dropped == 1 and rays_o[N - 1, 1] + 1 == total and rays_o[N - 2, 1] + rays_o[N - 2, 2] == total - 1
    # a ray straddling M: M in the middle of a heavy ray's run
    n = int(np.flatnonzero(counts > 100)[len(counts[counts > 100]) // 2])
    M = int(rays_o[n, 1] + counts[n] // 2)
    rays_o, kept, dropped = check_train(O, dev, case, M=M, arrays=arrays)
    assert dropped >= 2 and kept >= 100 and rays_o[n, 1] < M < rays_o[n, 1] + rays_o[n, 2]


def test_march_train_smallest_grid(O, dev):
    """H = 8, the smallest resolution the entry points accept (and with test_march_cpu.py's refusals the accepting side of the H
    check): one cascade, every cell of the lower half in x occupied"""
    H, C, bound, ms = 8, 1, 1.0, 64
    cells = np.zeros((H, H, H), bool)
    cells[:H // 2] = True
    i = np.arange(H)
    nx, ny, nz = np.meshgrid(i, i, i, indexing='ij')
    flat = np.zeros(H ** 3, bool)
    flat[(R._expand(nx) | (R._expand(ny) << 1) | (R._expand(nz) << 2)).reshape(-1)] = cells.reshape(-1)
    bf = np.packbits(flat.reshape(-1, 8)[:, ::-1], axis=1).reshape(-1)
    rng = np.random.default_rng(5)
    N = 301
    ro = np.concatenate([np.full((N, 1), -1.4), rng.uniform(-0.9, 0.9, (N, 2))], 1).astype(F32)
    rd = np.concatenate([np.ones((N, 1)), rng.uniform(-0.3, 0.3, (N, 2))], 1)
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(F32)
    ne, fa = O.near_far_from_aabb(ro, rd, np.array([-1, -1, -1, 1, 1, 1], F32), 0.2)
    R.check_safe(ro, rd, ne, fa, bound)
    case = ('replay', bound, C, H, ms, 0.0, None)
    rays_o, kept, dropped = check_train(O, dev, case, arrays=(bf, ro, rd, ne, fa, None, None))
    assert kept > 250


@pytest.mark.parametrize('is_ndc', [False, True])
def test_march_rays_inference_noises(O, dev, is_ndc):
    """one step of the inference march (n_step 16) with noises, against the oracle with the same array: positions, directions,
    deltas (all four columns with NDC; the kernel writes a zero step into deltas[:, 0] of a ray's unused slots, which the
    reference has from its zero-filled buffer, and leaves the rest of such a row alone)"""
    from nerfstyle_amd import _lib as L
    case = R.CASES[17] if is_ndc else R.CASES[3]
    route, bound, C, H, ms, g, _ = case
    bf, ro, rd, ne, fa, zh, no = _inputs(O, case, noises=True)
    N, n_step = len(ro), 16
    alive = np.arange(N, dtype=np.int32)[::-1].copy()                     # slot n marches ray N - 1 - n: noises are per slot
    rt = np.stack([ne, ne], 1) if is_ndc else ne.copy()
    xo, do, dlo = O.march_rays(N, n_step, alive, rt, ro, rd, bound, bf, C, H, ne, fa, -1, ms, g, is_ndc=is_ndc, z_hats=zh if is_ndc else None,
                               noises=no)
    plain = O.march_rays(N, n_step, alive, rt, ro, rd, bound, bf, C, H, ne, fa, -1, ms, g, is_ndc=is_ndc, z_hats=zh if is_ndc else None)
    assert not np.array_equal(R.bits(plain[0]), R.bits(xo)) and np.isfinite(dlo).all()
    M = N * n_step
    xyzs, dirs, deltas = _nan_buffer(M, 3, dev), _nan_buffer(M, 3, dev), _nan_buffer(M, 4, dev)
    t = [_dev(a, dev) for a in (alive, rt, ro, rd, bf, ne, fa, no)]
    zh_t = _dev(zh, dev) if is_ndc else None
    st = L.lib().nsr_march_rays(N, n_step, L.p(t[0]), L.p(t[1]), L.p(t[2]), L.p(t[3]), L.p(zh_t), float(bound), float(g), int(ms),
                                int(is_ndc), C, H, L.p(t[4]), L.p(t[5]), L.p(t[6]), L.p(xyzs), L.p(dirs), L.p(deltas), L.p(t[7]),
                                L.stream())
    assert st == 0
    torch.cuda.synchronize()
    used = (dlo[:, 0] != 0)
    assert used.sum() > 2000 and (~used).sum() > 100
    for buf, cols, want in ((xyzs, 3, xo), (dirs, 3, do), (deltas, 4, dlo)):
        assert bool((buf[M * cols:] == NAN_BITS).all()), 'write behind the buffer'
        got = buf[:M * cols].cpu().numpy().view(np.uint32).reshape(M, cols)
        exp = np.full((M, cols), NAN_BITS, np.uint32)
        keep = cols if (cols == 3 or is_ndc) else 2
        exp[used, :keep] = R.bits(want).reshape(M, cols)[used, :keep]
        if cols == 4:
            exp[~used, 0] = 0
        bad = np.flatnonzero((got != exp).any(1))
        assert bad.size == 0, 'slot {}: {} != {} ({} differ)'.format(bad[0], got[bad[0]].view(F32), exp[bad[0]].view(F32), bad.size)
