"""The inputs of test_gpu_infer_composite.py do what infer_composite_ref.py's docstring claims, and its fp32 restatement of
the loop step agrees with the oracle the suite already trusts.  No GPU."""
import numpy as np
import pytest

import infer_composite_ref as R

F32 = np.float32


@pytest.fixture(scope='module')
def infer_all():
    return [(p, R.infer_batches(*p)) for p in R.infer_params()]


@pytest.fixture(scope='module')
def loop_all():
    return [(p, R.loop_batches(*p)) for p in R.loop_params()]


def test_parameter_sets_cover_the_issue_lists():
    ip, lp = R.infer_params(), R.loop_params()
    assert {p[0] for p in ip} == set(R.C_LIST) == {1, 3, 4, 5, 8, 9, 16} and max(R.C_LIST) == R.RM_MAXC
    for C in R.C_LIST:
        want = set(R.N_LIST) | ({R.N_BIG} if C in R.C_BIG else set())
        assert {p[1] for p in ip if p[0] == C} == want
        for n_step in R.N_STEPS:
            for ndc in (False, True):
                sub = [p for p in lp if p[:3] == (C, n_step, ndc)]
                assert {p[3] for p in sub} == want and {p[4] for p in sub} == set(R.T_THRESHES)
    assert {p[2] for p in ip} == {1e-4, 1e-2, 0.0}
    assert [R.lanes_per_ray(C) for C in R.C_LIST] == [4, 4, 4, 8, 8, 16, 16]


def test_thread_counts_stop_where_the_issue_says():
    """N * LPR against the 64-lane wave and the 256-thread block"""
    for lpr_C in (4, 8, 16):
        for N in (15, 17, 63, 65):
            assert R.infer_threads(N, lpr_C) % 64 != 0                     # stops inside a wave
    for N in (16, 64):
        for lpr_C in (4, 16):
            assert R.infer_threads(N, lpr_C) % 64 == 0                     # stops on a wave boundary
    assert R.infer_threads(16, 4) == 64 and R.infer_threads(16, 16) == 256 and R.infer_threads(64, 4) == 256
    for N in (257, 2049):
        for lpr_C in (4, 8, 16):
            assert R.infer_threads(N, lpr_C) > 256 and R.infer_threads(N, lpr_C) % 256 != 0   # more than a block, ends inside one
    for N in R.N_LIST:                                                     # the loop step: one thread per alive slot
        assert (N % 64 == 0) == (N == 64)


def _classes_of(batches):
    return set(np.concatenate([b['cls'] for b in batches]))


def test_single_pass_batches_hold_every_class(infer_all):
    for (C, N, tt), batches in infer_all:
        assert _classes_of(batches) == set(R.INFER_CLASSES)
        counts = set()
        for b in batches:
            ref, rays, cls, M = b['ref'], b['rays'], b['cls'], b['M']
            assert sorted(rays[:, 0]) == list(range(b['N']))
            if b['N'] > 1:
                assert (rays[:, 0] != np.arange(b['N'])).any() and len(set(b['nears'])) > 1
            counts |= set(rays[:, 2])
            end = rays[:, 1] + rays[:, 2]
            assert (end[cls == 'drop'] == M).all() and (end[cls == 'keep'] == M - 1).all()
            assert (~ref['live'][np.isin(cls, ('drop', 'zero'))]).all() and ref['live'][~np.isin(cls, ('drop', 'zero'))].all()
            assert (ref['consumed'][~ref['live']] == 0).all()
            # runs do not overlap, and some pair of neighbours has a gap
            o = np.argsort(rays[:, 1], kind='stable')
            o = o[rays[o, 2] > 0]
            assert (end[o][:-1] <= rays[o, 1][1:]).all()
            if b['N'] >= 15:
                assert (end[o][:-1] < rays[o, 1][1:]).any()
            got, cnt = ref['consumed'], rays[:, 2]
            assert (got[cls == 'a'] == cnt[cls == 'a']).all() and (ref['weights_sum'][rays[cls == 'a', 0]] == 0).all()
            assert (got[np.isin(cls, ('e', 'g', 'keep'))] == cnt[np.isin(cls, ('e', 'g', 'keep'))]).all()
            if tt > 0:
                assert (got[cls == 'b'] == 2).all()                        # the opaque sample, then the sample that sees T = 0
                assert ((got[cls == 'c'] > 2) & (got[cls == 'c'] < cnt[cls == 'c'] - 2)).all()   # in the middle
                assert (got[cls == 'd'] == cnt[cls == 'd']).all()          # ... and the last sample is the one that trips
                for n in np.flatnonzero(cls == 'd'):
                    assert ref['T'][n, cnt[n] - 1] < tt <= ref['T'][n, cnt[n] - 2]
            else:
                assert (got == np.where(ref['live'], cnt, 0)).all()        # nothing ever crosses 0
            for n in np.flatnonzero(cls == 'g'):                           # the zero step adds no weight but the pass goes on
                k = cnt[n] // 2
                assert b['deltas'][rays[n, 1] + k, 0] == 0 and ref['w'][n, k] == 0 and ref['w'][n, k + 1:cnt[n]].sum() > 1e-3
        assert counts == set(R.STEP_COUNTS)


def test_loop_batches_hold_every_class(loop_all):
    for (C, n_step, ndc, N, tt), batches in loop_all:
        assert _classes_of(batches) == set(R.LOOP_CLASSES)
        for b in batches:
            ref, cls, alive = b['ref'], b['cls'], b['alive']
            assert b['n_rays'] > N and len(set(alive)) == N and (N == 1 or (np.diff(alive) < 0).any())
            for name in ('weights_sum', 'depth', 'image', 'rays_t'):
                assert (b[name] != 0).all()
            dl = b['deltas'].reshape(N, n_step, 4)
            if ndc:
                ok = np.isfinite(dl[..., 2])
                assert ((dl[..., 2][ok] > 0) & (dl[..., 2][ok] <= 1)).all()
                assert (dl[..., 1][ok] > 0).all() and (dl[..., 3][ok] > dl[..., 1][ok]).all()
                assert (b['rays_t'][:, 0] != b['rays_t'][:, 1]).all()
            else:
                assert np.isnan(dl[..., 2:]).all()
            s, got = ref['survived'], ref['consumed']
            assert s[np.isin(cls, ('a', 'e'))].all() and not s[np.isin(cls, ('f', 't'))].any()
            assert (got[cls == 'f'] == 0).all() and (got[cls == 't'] <= n_step // 2).all()
            f = np.flatnonzero(cls == 'f')
            assert (dl[f, 0, 0] == 0).all() and np.isnan(b['sig'].reshape(N, n_step)[f]).all()
            assert np.isnan(b['rgb'].reshape(N, n_step, C)[f]).all()
            if tt > 0:
                # (b): alive after a single slot (nothing tests the T it leaves), dead on the slot after the opaque one
                assert (s[cls == 'b'] == (n_step == 1)).all() and (got[cls == 'b'] == min(n_step, 2)).all()
                # (d): the T test fires on the last slot, every slot was composited, the ray is dead all the same
                assert (got[cls == 'd'] == n_step).all() and not s[cls == 'd'].any()
                for n in np.flatnonzero(cls == 'd'):
                    assert ref['T'][n, n_step - 1] < tt and (n_step == 1 or ref['T'][n, n_step - 2] >= tt)
                if n_step == 64:
                    c = cls == 'c'
                    assert (~s[c]).all() and ((got[c] > 1) & (got[c] < n_step - 1)).all()
            else:
                assert s[np.isin(cls, ('a', 'b', 'c', 'd', 'e'))].all()    # (e): nothing crosses 0, the opaque ray included
            assert 0 < s.sum() < N or N == 1


def test_margin_and_its_cap(infer_all, loop_all):
    redraws = soft = 0
    for _, batches in infer_all + loop_all:
        for b in batches:
            assert not R.too_close(b['ref']['T'], b['T_thresh']).any()
            redraws, soft = redraws + b['redraws'], soft + b['n_soft']
    assert soft > 10000 and redraws <= 0.05 * soft
    print('redraws {} of {} soft rays'.format(redraws, soft))
    # the relative part alone, as a condition on T
    tt = float(F32(1e-2))
    assert R.too_close(np.array([[tt * (1 + 0.9e-3)]]), 1e-2)[0] and not R.too_close(np.array([[tt * (1 + 1.1e-3)]]), 1e-2)[0]
    assert not R.too_close(np.array([[0.0]]), 0.0)[0]


def test_opaque_alpha_is_one_in_fp32():
    b = R.infer_case(4, 64, 1e-4)
    for n in np.flatnonzero(b['cls'] == 'b'):
        o = b['rays'][n, 1]
        x = -b['sig'][o] * b['deltas'][o, 0]
        assert x.dtype == F32 and abs(float(x) + 200) < 1e-3
        with np.errstate(under='ignore'):
            alpha = F32(1) - np.exp(x)
        assert alpha.dtype == F32 and alpha == F32(1.0)
    r32 = R.composite_infer_ref(b['sig'], b['rgb'], b['deltas'], b['rays'], b['nears'], b['M'], 4, 1e-4, F32)
    n = np.flatnonzero(b['cls'] == 'b')
    assert (r32['T'][n, 1] == 0).all() and (r32['weights_sum'][b['rays'][n, 0]] == 1).all()
    assert r32['weights_sum'].dtype == F32 and b['ref']['weights_sum'].dtype == np.float64


def test_t_columns_are_exact_in_fp32(infer_all, loop_all):
    """rays_t of the fp32 chain equals the fp64 chain bit for bit: no rounding choice exists"""
    for (C, n_step, ndc, N, tt), batches in loop_all[::7]:
        for b in batches:
            r32 = R.composite_rays_ref(N, n_step, b['alive'], b['rays_t'], b['sig'], b['rgb'], b['deltas'], b['weights_sum'],
                                       b['depth'], b['image'], C, tt, ndc, F32)
            assert r32['rays_t'].dtype == F32 and np.array_equal(r32['rays_t'].astype(np.float64), b['ref']['rays_t'])
            assert np.array_equal(r32['rays_alive'], b['ref']['rays_alive'])


def _floor_update(worst, cls_rows, cls, r32, r64):
    for c in set(cls):
        rows = cls_rows[cls == c]
        v = max(np.abs(r32['weights_sum'][rows] - r64['weights_sum'][rows]).max(),
                np.abs(r32['image'][rows] - r64['image'][rows]).max())
        d = (np.abs(r32['depth'][rows] - r64['depth'][rows]) / np.maximum(np.abs(r64['depth'][rows]), 1)).max()
        worst[c] = (max(worst.get(c, (0, 0))[0], float(v)), max(worst.get(c, (0, 0))[1], float(d)))


def test_fp32_floor(infer_all, loop_all):
    """measures |fp32 restatement - fp64| per class over every batch; FLOOR records it (rounded up), and the values agree on
    every decision"""
    worst = {}
    for (C, N, tt), batches in infer_all:
        for b in batches:
            r32 = R.composite_infer_ref(b['sig'], b['rgb'], b['deltas'], b['rays'], b['nears'], b['M'], C, tt, F32)
            assert np.array_equal(r32['consumed'], b['ref']['consumed'])
            _floor_update(worst, b['rays'][:, 0], b['cls'], r32, b['ref'])
    for (C, n_step, ndc, N, tt), batches in loop_all:
        for b in batches:
            r32 = R.composite_rays_ref(N, n_step, b['alive'], b['rays_t'], b['sig'], b['rgb'], b['deltas'], b['weights_sum'],
                                       b['depth'], b['image'], C, tt, ndc, F32)
            assert np.array_equal(r32['consumed'], b['ref']['consumed']) and np.array_equal(r32['survived'], b['ref']['survived'])
            _floor_update(worst, b['alive'].astype(np.int64), b['cls'], r32, b['ref'])
    for c in sorted(worst):
        print('floor {:5s} value {:.3e} depth {:.3e}'.format(c, *worst[c]))
    assert set(worst) == set(R.FLOOR)
    for c, (v, d) in worst.items():
        assert v <= R.FLOOR[c][0] and d <= R.FLOOR[c][1], (c, v, d)
        assert R.FLOOR[c][0] <= max(2 * v, 1e-12) and R.FLOOR[c][1] <= max(2 * d, 1e-12), (c, v, d)   # recorded, not padded


@pytest.mark.parametrize('C,n_step,ndc,tt', [(8, 8, False, 1e-4), (3, 64, True, 1e-2), (16, 2, False, 0.0), (5, 1, True, 1e-4)])
def test_fp32_restatement_agrees_with_the_oracle(O, C, n_step, ndc, tt):
    """O.composite_rays on one 257-slot batch.  The oracle expresses every class (it stops on the terminator before it reads the
    NaN behind it), so no ray is left out."""
    b = R.loop_case(C, 257, n_step, ndc, tt)
    r32 = R.composite_rays_ref(257, n_step, b['alive'], b['rays_t'], b['sig'], b['rgb'], b['deltas'], b['weights_sum'], b['depth'],
                               b['image'], C, tt, ndc, F32)
    alive, rt, ws, d, im = (b[k].copy() for k in ('alive', 'rays_t', 'weights_sum', 'depth', 'image'))
    O.composite_rays(257, n_step, alive, rt, b['sig'], b['rgb'], b['deltas'], ws, d, im, tt, is_ndc=ndc)
    assert np.array_equal(alive, r32['rays_alive'])
    assert np.array_equal(rt.view(np.uint32), r32['rays_t'].view(np.uint32))
    assert not np.isnan(ws).any() and not np.isnan(im).any()
    assert np.abs(ws - r32['weights_sum']).max() <= 1e-6 and np.abs(im - r32['image']).max() <= 1e-6
    assert np.abs(d - r32['depth']).max() <= 1e-6 * max(1, np.abs(d).max())


def test_chain_cases_build():
    for p in R.CHAIN_PARAMS:
        ch = R.chain_case(*p)
        assert ch['ref']['survived'].any() and not ch['ref']['survived'].all()
        assert set(ch['cls2']) == set(R.LOOP_CLASSES)


def test_compact_ref_and_cases():
    a = np.array([5, -1, 0, -2, R.INT32_MIN, 7, 5 + 1, R.INT32_MAX], np.int32)
    assert R.compact_ref(a).tolist() == [5, 0, 7, 6, R.INT32_MAX]          # stable: the input's order
    assert R.compact_ref(np.zeros(0, np.int32)).size == 0
    assert [R.scan_trips(n) for n in (0, 1, 262144, 262145, 524288, 524545, 762048)] == [0, 1, 1, 2, 2, 3, 3]
    assert -(-524545 // 256) == 2050 and -(-762048 // 256) == 2977 and 762048 == 1008 * 756
    for n in R.COMPACT_SIZES:
        for pat in R.COMPACT_PATTERNS:
            a = R.compact_case(n, pat)
            keep = R.compact_keep(n, pat)
            out = R.compact_ref(a)
            assert a.dtype == np.int32 and a.shape == (n,) and out.size == keep.sum() == (a >= 0).sum()
            assert len(set(out.tolist())) == out.size                      # distinct ids: any misplaced element shows
            if out.size >= 2:
                assert 0 in out and R.INT32_MAX in out
            if n >= 255 and pat == 'none':
                assert {-1, -2, R.INT32_MIN} == set(a.tolist())
    n = 762048
    def blocks(k):
        return k[:n // 256 * 256].reshape(-1, 256)
    keep = R.compact_keep(n, 'dead_waves_blocks')
    assert (~keep.reshape(-1, 64).any(1)).sum() > 3000 and not blocks(keep)[1020:1028].any() and not blocks(keep)[2045:2051].any()
    assert blocks(keep)[1019].any() and blocks(keep)[1028].any()
    assert (blocks(R.compact_keep(n, 'per_block')).sum(1) == 1).all()
    assert R.compact_keep(n, 'all').all() and not R.compact_keep(n, 'none').any()
    assert R.compact_keep(n, 'first').nonzero()[0].tolist() == [0] and R.compact_keep(n, 'last').nonzero()[0].tolist() == [n - 1]
    for pat, dens in (('rand01', 0.01), ('rand50', 0.5), ('rand99', 0.99)):
        assert abs(R.compact_keep(n, pat).mean() - dens) < 0.005
