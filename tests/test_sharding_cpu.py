"""Shard geometry of the sharded optimiser step (nerfstyle_amd/sharded_optim.py), host only: the shards partition the
trained elements, chunks are multiples of 16 floats, padding stays below world * 16, the packed-lane index maps round-trip,
and selections other than the reference trainers' two raise.  Also host only: FusedAdam and ShardedFusedAdam hold the
same state after loading the same one."""
import pytest
import torch

from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig
from nerfstyle_amd.sharded_optim import SHARD_ALIGN, ShardGeometry, ShardedFusedAdam, shard_chunk, trained_lane_mask
from nerfstyle_amd.style_nerf import StyleTCNerf


@pytest.fixture(scope='module', params=[None, torch.float32], ids=['f16_tables', 'f32_tables'])
def model(request):
    return StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=request.param, use_dir=False)


SETS = [(None, 0xF), (['x_color_embedder'], 0xC), (['x_density_embedder'], 0x3)]


@pytest.mark.parametrize('keywords,mask', SETS)
def test_shards_partition_the_trained_elements(model, keywords, mask):
    assert trained_lane_mask(model, keywords) == mask
    total = model.arena.numel() if mask == 0xF else 2 * model.rows
    for world in range(1, 9):
        geos = [ShardGeometry.of(model, keywords, world, k) for k in range(world)]
        c = geos[0].chunk
        assert c % SHARD_ALIGN == 0 and c == shard_chunk(total, world)
        assert geos[0].total == total and geos[0].padded == world * c
        assert 0 <= world * c - total < world * SHARD_ALIGN
        covered = 0
        for k, g in enumerate(geos):
            assert g.chunk == c and g.slot == k * c
            assert g.lo == covered and g.hi - g.lo == g.n <= c
            assert (g.lo, g.hi) == geos[0].bounds(k)
            covered = g.hi
            if mask != 0xF:
                assert g.lo % 2 == 0 and g.hi % 2 == 0 and 0 <= g.row_lo <= g.row_hi <= model.rows
        assert covered == total


@pytest.mark.parametrize('keywords,mask', SETS[1:])
def test_lane_index_maps_round_trip(model, keywords, mask):
    g = ShardGeometry.of(model, keywords, 3, 1)
    j = torch.arange(g.total, dtype=torch.int64)
    i = g.lane_to_arena(j)
    assert torch.equal(g.arena_to_lane(i), j)
    assert int(i.max()) < model.table_elems
    lanes = i % 4
    assert bool(((1 << lanes) & mask).bool().all())                # only trained lanes
    assert torch.equal(i.view(-1, 2) // 4, torch.arange(model.rows)[:, None].expand(-1, 2))
    # the rank's rows hold exactly its packed elements
    assert g.row_lo * 2 == g.lo and g.row_hi * 2 == g.hi


def test_half_copy_ranges_cover_the_tables(model):
    te = model.table_elems
    for world in range(1, 9):
        for k in range(world):
            g = ShardGeometry.of(model, None, world, k)
            seen = torch.zeros(te, dtype=torch.int32)
            for (o, n) in [g.half_own()] + g.half_refresh():
                assert o % 4 == 0 and n % 4 == 0          # 16-byte aligned fp32 / 8-byte aligned f16 pointers, whole rows
                seen[o:o + n] += 1
            assert bool((seen == 1).all()), (world, k)


@pytest.mark.parametrize('keywords', [['x_color_embedder', 'color2_net'], ['_net'], ['embedder'], ['density']])
def test_other_selections_raise(model, keywords):
    with pytest.raises(NotImplementedError, match='ShardedFusedAdam supports'):
        ShardedFusedAdam(model, keywords=keywords)


def test_unknown_keywords_still_raise_value_error(model):
    with pytest.raises(ValueError):
        ShardedFusedAdam(model, keywords=['no_such_parameter'])


@pytest.mark.parametrize('keywords', [None, ['x_color_embedder']], ids=['everything', 'colour_table'])
def test_both_optimisers_hold_the_same_state_after_loading_it(keywords):
    """The reference's optimiser state (torch.optim.Adam.state_dict() over the trained parameters + torch_ema's dict over all
    of them) loaded into a FusedAdam and into a ShardedFusedAdam of world 1 gives the same state_dict(), key by key, and the
    state_dict() of either loads into the other.  CPU model, no process group: no collective, no kernel."""
    from nerfstyle_amd.config import PosEncConfig
    from nerfstyle_amd.optim import FusedAdam
    ncfg = NetworkConfig(pos_enc=PosEncConfig(hashmap_size=14))

    def fresh(cls):
        m = StyleTCNerf(ncfg, BBox.from_radius(2.0), 5)
        with torch.no_grad():
            m.arena.copy_(torch.rand(m.arena.shape, generator=torch.Generator().manual_seed(1)) - 0.5)
        return cls(m, lr=1e-2, keywords=keywords, ema_decay=0.95)
    m = StyleTCNerf(ncfg, BBox.from_radius(2.0), 5)
    g = torch.Generator().manual_seed(3)
    trained = [(n, v) for n, v in m.named_views() if keywords is None or any(k in n for k in keywords)]
    assert len(trained) == (6 if keywords is None else 1)
    optim_sd = {'state': {i: {'step': torch.tensor(41.), 'exp_avg': torch.randn(v.shape, generator=g),
                              'exp_avg_sq': torch.rand(v.shape, generator=g)} for i, (n, v) in enumerate(trained)},
                'param_groups': [{'lr': 0.0097, 'initial_lr': 0.01, 'betas': (0.9, 0.999), 'eps': 1e-15,
                                  'params': list(range(len(trained)))}]}
    ema_sd = {'decay': 0.95, 'num_updates': 37, 'shadow_params': [torch.randn(v.shape, generator=g) for _, v in m.named_views()],
              'collected_params': None}
    KEYS = ['step', 'exp_avg', 'exp_avg_sq', 'ema', 'ema_updates', 'lr']

    def same(a, b):
        assert sorted(a) == sorted(b) == sorted(KEYS)
        for k in KEYS:
            if torch.is_tensor(a[k]):
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
    fa, sh = fresh(FusedAdam), fresh(ShardedFusedAdam)
    fa.load_reference_state(optim_sd, ema_sd)
    sh.load_reference_state(optim_sd, ema_sd)
    sd_f, sd_s = fa.state_dict(), sh.state_dict()
    same(sd_f, sd_s)
    assert sd_f['step'] == 41 and sd_f['ema_updates'] == 37 and sd_f['lr'] == 0.0097
    assert fa.param_groups[0]['initial_lr'] == sh.param_groups[0]['initial_lr'] == 0.01
    # the loaded values are there: not two optimisers that both ignored their input
    views = dict(m.named_views())
    name0 = trained[0][0]
    off = views[name0].storage_offset()
    assert sd_f['exp_avg'].flatten()[off] == optim_sd['state'][0]['exp_avg'].flatten()[0] != 0
    assert sd_f['ema'][0] == ema_sd['shadow_params'][0].flatten()[0]
    # one's state into the other
    sh2, fa2 = fresh(ShardedFusedAdam), fresh(FusedAdam)
    sh2.load_state_dict(sd_f)
    fa2.load_state_dict(sd_s)
    same(sh2.state_dict(), sd_f)
    same(fa2.state_dict(), sd_s)
    # ... and the reference's state through load_state_dict, as checkpoint.restore may hand it over
    sh3, fa3 = fresh(ShardedFusedAdam), fresh(FusedAdam)
    sh3.load_state_dict(optim_sd)
    fa3.load_state_dict(optim_sd)
    same(sh3.state_dict(), fa3.state_dict())
