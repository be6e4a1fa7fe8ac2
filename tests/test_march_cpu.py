"""CPU proof that the inputs of test_gpu_march_edges.py reach the edges they are meant for, the closed-form step rule of
rm_const_step restated, and the host argument checks of the march entry points.  No GPU.

The edge conditions are CONDITIONS on the oracle's output for the rays of march_ref.edge_march_rays, not measurements: whether
random rays put a sample on lane 63 of a wave block is luck, whether these do is asserted here, for every configuration the GPU
file runs (march_ref.CASES).  Three conditions cannot hold everywhere, for reasons of geometry that do not depend on any
kernel, and are asserted exactly where they can:
  * a gap of 192 step indices is 192 * 2 sqrt(3) / max_steps long, and a ray along x is 2 bound long: bound * max_steps >= 512
    (the slabs leave 69 % of it empty), and a constant step (with dt_gamma = 1/64 a whole ray has about 64 ln(far / near) steps);
  * max_steps samples in a row are 2 sqrt(3) of occupied cells, the diagonal of the whole box at bound 1: bound > 1, constant step;
  * the diagonal ray's last step index reaches bound * max_steps only with a constant step."""
import ctypes

import numpy as np
import pytest

import march_ref as R

F32 = np.float32
CASE_IDS = [R.case_id(c) for c in R.CASES]


def _march(O, case, noises=None, max_steps=None):
    route, bound, C, H, ms, g, _ = case
    bf, ro, rd, ne, fa, labels, zh = R.case_inputs(O, case)
    ndc = route == 'ndc'
    total_cap = len(ro) * (max_steps or ms) + 1
    return O.march_rays_train(ro, rd, bound, bf, C, H, ne, fa, max_steps or ms, dt_gamma=g, M=total_cap, z_hats=zh if ndc else None,
                              is_ndc=ndc, noises=noises)


@pytest.mark.parametrize('case', R.CASES, ids=CASE_IDS)
def test_edge_rays_reach_the_edges(O, case):
    route, bound, C, H, ms, g, edge = case
    bf, ro, rd, ne, fa, labels, zh = R.case_inputs(O, case)
    labels = np.array(labels)
    N = len(ro)
    assert N == R.N_EDGE and N % 4 != 0 and N % 256 != 0
    want = set(R.LABELS) | ({'binade'} if edge is not None else set())
    assert set(labels) == want
    # which emit the entry point takes: recorded blocks only while a wave's 64 lanes can hold a ray's records
    slot_cap_zero = (R.step_capacity(bound, ms) + 63) // 64 + 1 > 64
    assert slot_cap_zero == (route == 'remarch') or route in ('mask', 'ndc')

    xyz, dirs, dl, rays, cnt = _march(O, case)
    assert int(cnt[0]) == len(xyz)
    assert np.isfinite(xyz).all() and np.isfinite(dl).all() and np.isfinite(dirs).all()          # NDC: columns 2 and 3 too
    if route == 'ndc':
        assert np.abs(dl[:, 2]).max() > 0 and np.abs(dl[:, 3]).max() > 0
    counts = rays[:, 2]
    assert np.array_equal(rays[:, 0], np.arange(N)) and (counts[list(R.HEAVY)] >= np.percentile(counts, 90)).all()

    dt_min, dt_max = R.dt_limits(ms, C, H)
    K = R.step_capacity(bound, ms)
    ts = R.t_sequence(R.start_t(ne, 0.0, g, dt_min, dt_max), g, dt_min, dt_max, K)
    assert np.isfinite(ts[:, ne < R.FLT_MAX]).all()
    ks = []
    for n in range(N):
        o, c = rays[n, 1], rays[n, 2]
        ks.append(R.step_indices(ts[:, n], ro[n], rd[n], bound, g, dt_min, dt_max, xyz[o:o + c], dl[o:o + c, 0]) if c
                  else np.zeros(0, np.int64))
    allk = np.concatenate(ks)
    assert allk.max() < K - 64                                       # inside the kernels' step capacity, slack unused
    for period in (64, 32):
        assert (allk % period == 0).any() and (allk % period == period - 1).any()
    assert any(R.runs_crossing(k, 64) for k in ks) and any(R.runs_crossing(k, 32) for k in ks)
    # skips that pass whole blocks and words
    gap = max(int(np.diff(k).max()) for k in ks if len(k) > 1)
    if g == 0.0 and bound * ms >= 512:
        assert gap >= 192, gap
    # max_steps cuts a ray while occupied cells remain
    if g == 0.0 and bound > 1.0:
        more = _march(O, case, max_steps=ms + 1)[3][:, 2]
        assert ((counts == ms) & (more > ms)).any()
    # far ends a ray in the middle of a block that holds samples
    n_below_far = (ts < fa[None, :]).sum(0)                          # the first step index with t >= far
    mid = [n for n in np.flatnonzero((counts > 0) & (counts < ms))
           if n_below_far[n] % 64 not in (0, 63) and ks[n][-1] >= n_below_far[n] - n_below_far[n] % 64]
    assert len(mid) > 0
    # rays without samples: through empty space, beside the box (near = far = FLT_MAX), the box behind them
    for lab in ('empty', 'miss', 'behind'):
        assert (counts[labels == lab] == 0).all()
    assert ((ne == R.FLT_MAX) & (fa == R.FLT_MAX))[labels == 'miss'].all() and (fa[labels == 'behind'] < 0).all()
    for lab in ('oblique+x', 'oblique-x', 'inner+x', 'inner-x', 'cut', 'axis'):
        assert (counts[labels == lab] > 0).all(), lab
    # the diagonal: near == 0 (the t > 0 branch of the closed form), samples at the far corner only, up to the last step index
    d = int(np.flatnonzero(labels == 'diagonal')[0])
    assert ne[d] == 0.0 and counts[d] > 0 and np.abs(xyz[rays[d, 1], :2]).min() > 0.8 * bound
    if g == 0.0:
        assert ks[d][-1] >= 0.99 * bound * ms, (ks[d][-1], bound * ms)
    # axis-parallel rays carry a negative zero
    ax = rd[labels == 'axis']
    assert ((ax == 0).sum(1) == 2).all() and (np.signbit(ax) & (ax == 0)).any(1).all()
    # noise moves samples: some ray's count differs from the noiseless run
    noisy = _march(O, case, noises=R.edge_noises(N))[3][:, 2]
    assert (noisy != counts).any()


def _old_rule(t, dt, span):
    """the rule before the fix: t_1 .. t_span in one binade, t_0 anywhere"""
    t1 = (t + dt).astype(F32)
    t2 = (t1 + dt).astype(F32)
    b1, b2 = R.bits(t1).astype(np.int64), R.bits(t2).astype(np.int64)
    cc = b2 - b1
    b_last = b1 + (span - 1) * cc
    return (b2 > b1) & ((b1 >> 23) == (b_last >> 23)) & (cc < (1 << 23)), b1, cc


def _rule(t, dt, span):
    """rm_const_step (csrc/raymarch.hip) restated: two real additions give t_1 and t_2, c = bits(t_2) - bits(t_1), and the closed
    form t_j = bits(t_1) + (j - 1) c is accepted when t_0 and t_span share an exponent (t_1 .. t_span lie between them), c > 0
    and c < 2^23.  -> (accepted, bits(t_1), c)"""
    _, b1, cc = _old_rule(t, dt, span)
    b_last = b1 + (span - 1) * cc
    return (cc > 0) & ((R.bits(t).astype(np.int64) >> 23) == (b_last >> 23)) & (cc < (1 << 23)) & (t > 0), b1, cc


@pytest.mark.parametrize('edge,max_steps,bites', [(2.0, 514, True), (1.0, 1028, True), (1.0, 1024, False), (2.0, 1024, False)])
def test_binade_cases_bite(edge, max_steps, bites):
    """The CPU proof that the binade rays exercise the defect: for max_steps 514 (edge 2.0) and 1028 (edge 1.0) at least one of
    the 8 starts just below the edge has t_1 .. t_3 in one binade with unequal bit increments -- where the closed form with
    c = bits(t_2) - bits(t_1) is not the serial sum -- and for 1024 none has."""
    dt_min, _ = R.dt_limits(max_steps, 1, 32)
    ts = R.t_sequence(R.floats_below(edge, 8), 0.0, dt_min, dt_min, 3)
    b = R.bits(ts).astype(np.int64)
    same = ((b[1] >> 23) == (b[3] >> 23))
    uneven = same & (b[2] - b[1] != b[3] - b[2])
    assert same.all() and uneven.any() == bites
    if bites:
        assert (R.bits(R.floats_below(edge, 8)) & 1).min() == 0 and (R.bits(R.floats_below(edge, 8)) & 1).max() == 1


def test_closed_form_rule_equals_serial_sums():
    """Keeps the ARGUMENT in the comment of rm_const_step honest; it does not bind the kernel (test_gpu_march_edges.py does, bit
    for bit against the sequential oracle).  The acceptance rule restated in NumPy (_rule), for every max_steps in 16..8192, the
    64 floats below each power of two from 2^-2 to 2^3 (block starts in the binade below: where the first rule failed) and the 64
    from it on, spans 32 and 64: wherever the rule accepts, bits(t_1) + (j - 1) c are the floats of `span` serial additions.
    The rule before the fix, on the same inputs, is wrong for max_steps 257, 514 and 1028 and right for 1024."""
    starts = np.concatenate([(np.arange(-64, 64) + int(F32(2.0 ** e).view(np.uint32))).astype(np.uint32).view(F32) for e in range(-2, 4)])
    bad = {(_rule, 32): [], (_rule, 64): [], (_old_rule, 32): [], (_old_rule, 64): []}
    accepted = []
    for lo in range(16, 8193, 512):                                    # in chunks of max_steps: 65 x 512 x 768 sums at a time
        ms = np.arange(lo, min(lo + 512, 8193))
        dt = (F32(2) * R.SQRT3 / ms.astype(F32)).astype(F32)
        t0 = np.broadcast_to(starts[None, :], (len(ms), len(starts))).astype(F32)
        dtb = np.broadcast_to(dt[:, None], t0.shape).astype(F32)
        serial = np.empty((65,) + t0.shape, np.int64)
        t = t0.copy()
        for j in range(65):
            serial[j] = R.bits(t)
            t = (t + dtb).astype(F32)
        for (rule, span), found in bad.items():
            ok, b1, cc = rule(t0, dtb, span)
            wrong = np.zeros(t0.shape, bool)
            for j in range(1, span + 1):
                wrong |= ok & (b1 + (j - 1) * cc != serial[j])
            found += ms[wrong.any(1)].tolist()
            if rule is _rule:
                accepted.append(ok.mean())
    for span in (32, 64):
        assert not bad[(_rule, span)], 'span {}: the closed form differs from the serial sums at max_steps {}'.format(
            span, bad[(_rule, span)][:8])
        old = set(bad[(_old_rule, span)])
        assert {257, 514, 1028} <= old and not ({256, 512, 768, 1000, 1024, 1536, 3000} & old)
    accepted_some = np.mean(accepted) > 0.1                            # ... and the rule is not vacuous
    assert accepted_some


@pytest.fixture(scope='module')
def lib():
    from nerfstyle_amd import _lib, build
    build.build()
    return _lib.lib()


def test_march_entry_points_refuse_h_that_is_no_power_of_two(lib):
    """The probe addresses bit cascade * H^3 + morton(nx, ny, nz): for H = 24, 40, 48, 96 a Morton index exceeds H^3 and the read
    leaves the bitfield, so nsr_march_rays_train, nsr_march_rays and the streaming renders return NSR_ERR_INVALID_ARG (-1) before
    any launch; so do H below 8 and above 512, the limits of the occupancy calls.  The pointers are fakes that are never
    dereferenced: every call here returns on the host.
    That H = 8, 32, 128 pass the check shows on the host only where a later check answers with another status: the streaming
    renders refuse 14 classes with NSR_ERR_UNSUPPORTED (-2) after the H check.  The two march calls have no such later check (a
    good H goes on to launch), so for them the accepting side is test_gpu_march_edges.py, which marches H = 8, 32, 64 and 128."""
    from nerfstyle_amd import _lib
    fake = ctypes.c_void_p(4096)

    def train(H, N=4):
        return lib.nsr_march_rays_train(fake, fake, None, fake, 2.0, 0.0, 1024, 0, N, 2, H, 64, fake, fake, fake, None, fake, fake,
                                        fake, None, fake, None)

    def infer(H, n_alive=4):
        return lib.nsr_march_rays(n_alive, 16, fake, fake, fake, fake, None, 2.0, 0.0, 1024, 0, 2, H, fake, fake, fake, fake, None,
                                  fake, None, None)

    offsets = (np.arange(17, dtype=np.int32) * 4096).copy()
    desc = _lib.FieldDesc()
    desc.L, desc.H, desc.S, desc.num_classes = 16, 16, 0.5, 14          # 14 classes: NSR_ERR_UNSUPPORTED, after the H check
    desc.table_dtype, desc.compute_dtype = _lib.NSR_F16, _lib.NSR_F16
    for i in range(3):
        desc.bbox_min[i], desc.bbox_size[i] = -2.0, 4.0
    desc.density_scale = 1.0
    desc.offsets = offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def stream(H):
        a = lib.nsr_render_rays_infer(ctypes.byref(desc), fake, fake, fake, fake, None, 8, fake, fake, fake, 2.0, 0.0, 1024, 0, 2, H,
                                      1e-4, fake, fake, fake, None, None)
        b = lib.nsr_render_rays_stream(ctypes.byref(desc), fake, fake, fake, fake, None, 8, fake, fake, fake, 2.0, 0.0, 1024, 2, H,
                                       1e-4, 1, fake, fake, fake, None, None, None, None, None, None)
        assert a == b
        return a

    for H in (24, 40, 48, 96, 0, 4, 1024, 3 << 30):
        assert train(H) == -1 and infer(H) == -1 and stream(H) == -1, H
        assert train(H, N=0) == 0 and infer(H, n_alive=0) == 0            # empty work stays a no-op success
    for H in (8, 32, 128, 512):
        assert stream(H) == -2, H
