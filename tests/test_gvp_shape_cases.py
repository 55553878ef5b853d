"""CPU: every case of gvp_shape_cases.py has the property it is named for, shown with the oracle alone: tile spans of the destination
runs, E mod 64 and tile counts, neighbour caps, rows without in-edge, a relative gap of at least 1e-3 behind every edge list, and the
float32-against-float64 oracle figures behind the loosened constants of the GPU modules.  Without this the GPU comparisons of
test_gvp_shapes_gpu.py / test_recenc_shapes_gpu.py could pass on inputs that never leave the first tile."""
import pytest
import torch

from . import gvp_shape_cases as gc
from . import util


def test_tile_spans_helper():
    dst = torch.tensor([0] * 70 + [2] * 58 + [3] * 1 + [4] * 130)          # runs [0, 70) [128, 128) [70, 128) [128, 129) [129, 259)
    assert util.tile_spans(dst, 6, 64).tolist() == [2, 0, 1, 1, 3, 0]


@pytest.mark.parametrize('bname', list(gc.BATCHES))
def test_denoiser_batch_property(bname):
    gap = gc.check_batch(bname)
    st = gc.den_stats(bname)
    print(f'{bname}: gap {gap:.2e}', {et: (st[et]['E'], st[et]['tiles'], int(st[et]['spans'].max()) if st[et]['E'] else 0) for et in gc.ETYPES})
    g = gc.den_batch(bname)
    for et in gc.ETYPES:                                                   # the lists are what the kernels' CSR layout assumes
        s, d = gc.den_edges(bname)[et]
        assert s.numel() == d.numel() and (d.numel() == 0 or int(d.max()) < g.num_nodes(gc.DST_NT[et]))
    assert gc.den_stats(bname)['kl']['E'] == gc.den_stats(bname)['lk']['E']


def test_every_denoiser_case_names_a_checked_batch():
    for name, c in gc.DEN.items():
        assert c['batch'] in gc.BATCHES, name
    long_batches = {gc.DEN[n]['batch'] for n in gc.LONG}
    assert long_batches == {gc.DENSE_RAD, gc.LIG230, gc.KP600}
    for b in long_batches:                                                 # both widths of the segmented sum, all three norm modes, both vector sizes
        grid = {(gc.DEN[n]['cfg']['n_hidden_scalars'], gc.DEN[n]['cfg']['message_norm']) for n in gc.LONG if gc.DEN[n]['batch'] == b}
        assert grid >= {(S, mn) for S in (128, 256) for mn in ('mean', 0, 10.0)}
        assert {gc.DEN[n]['cfg']['vector_size'] for n in gc.LONG if gc.DEN[n]['batch'] == b} == {16, 5}


def test_long_runs_exist_where_the_suite_had_none():
    """Runs over at least 3 tiles in every edge type, at least 4 in ll and kl, 5 (the ll cap) and 10 (kl) somewhere."""
    st = {b: gc.den_stats(b) for b in (gc.DENSE_RAD, gc.LIG230, gc.KP600)}
    for et in gc.ETYPES:
        assert int((st[gc.DENSE_RAD][et]['spans'] >= 3).sum()) >= 50
    assert int(st[gc.LIG230]['ll']['spans'].max()) == 5 and int(st[gc.KP600]['kl']['spans'].max()) >= 10


def test_tile_edge_coverage():
    rem, tiles = gc.tile_coverage()
    for et in gc.ETYPES:
        assert 0 in rem[et] and rem[et] & {1, 2}, (et, rem[et])
    assert tiles >= set(range(1, 10)), tiles
    widths = {gc.DEN[n]['cfg']['n_hidden_scalars'] for n in gc.TILES}
    assert widths == {128, 256}


def test_chain_and_narrow_configs():
    chains = {(c['n_message_gvps'], c['n_update_gvps'], c['n_noise_gvps'], c['n_hidden_scalars']) for c in (gc.DEN[n]['cfg'] for n in gc.CHAINS)}
    assert chains == {(m, u, n, S) for (m, u, n) in ((1, 1, 1), (4, 4, 4), (1, 4, 2), (4, 1, 1)) for S in (128, 256)}
    assert max(max(c[:3]) for c in chains) == gc.GVP_MAX_CHAIN
    assert gc.DEN['S1']['cfg']['n_hidden_scalars'] == 1 and gc.DEN['S2_V1']['cfg']['vector_size'] == 1
    assert gc.DEN['conv1_no_kp']['cfg']['n_convs'] == 1 and not gc.DEN['conv1_no_kp']['cfg']['update_kp']
    assert gc.DEN['B300']['cfg']['n_convs'] == 1 and gc.DEN[gc.SYM]['cfg']['n_convs'] == 3
    assert all(gc.DEN[n]['cfg']['n_hidden_scalars'] == 256 for n in gc.TRAIN)


@pytest.mark.parametrize('mn', ['mean', 0, 10.0])
def test_isolated_atom_gets_zero_eps_x(mn):
    """No in-edge of any type: the atom's vectors stay zero through every conv and the noise head, so the float64 oracle gives
    eps_x = 0 exactly, in every norm mode ('mean' divides by no count: oracle/graph_ops.py scatter_mean), and a finite eps_h."""
    ref = gc.den_reference(f'isolated_{gc._norm_tag(mn)}')
    assert torch.equal(ref['eps_x'][gc.ISOLATED_ROW], torch.zeros(3, dtype=torch.float64))
    assert torch.isfinite(ref['eps_h']).all() and torch.isfinite(ref['eps_x']).all()
    assert float(ref['eps_x'].abs().min(dim=1).values[:gc.ISOLATED_ROW].min()) > 0


def test_rigid_motions_are_proper_and_short():
    for R, t in gc.rigid_motions(3):
        assert torch.allclose(R @ R.T, torch.eye(3, dtype=torch.float64), atol=1e-12) and float(torch.linalg.det(R)) > 0
        assert 0 < float(t.norm()) <= 20.0 + 1e-9


# ---- the float32 oracle against the float64 oracle: the margins behind the bounds of the GPU modules -----------------------------------
def _excess(name, key, atol_rel=1e-6):
    a, b = gc.den_reference(name, torch.float32)[key], gc.den_reference(name)[key]
    return util.elementwise_excess(a, b, rtol=1e-4, atol_rel=atol_rel)


@pytest.mark.parametrize('name', [f'{b}_S{S}_n0' for b in (gc.DENSE_RAD, gc.LIG230, gc.KP600) for S in (128, 256)])
def test_long_runs_hold_the_plain_bound_in_fp32(name):
    """No long-run case may carry a loosened bound: fp32 itself (the float32 oracle) stays well inside the elementwise one."""
    ex = max(_excess(name, 'eps_h'), _excess(name, 'eps_x'))
    print(f'{name}: float32 oracle elementwise excess {ex:.3f}')
    assert ex <= 0.55


# ---- encoder -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(gc.REC))
def test_encoder_case_property(name):
    gap = gc.check_rec(name)
    ref = gc.rec_reference(name)
    print(f'{name}: gap {gap:.2e}, rk {ref["rk"][0].numel()} kk {ref["kk"][0].numel()} edges')
    assert all(torch.isfinite(ref[k]).all() and ref[k].dtype == torch.float64 for k in gc.REC_KEYS)


def test_encoder_cases_cover_the_issue():
    kws = {n: gc.REC[n]['kw'] for n in gc.REC}
    assert {kws[n]['out_scalar_size'] for n in ('out1', 'out127', 'out129')} == {1, 127, 129}
    assert kws['in1']['in_scalar_size'] == 1 and (kws['in256_out255']['in_scalar_size'], kws['in256_out255']['out_scalar_size']) == (256, 255)
    assert kws['rr0']['n_rr_convs'] == 0 and kws['k1']['k_closest'] == 1 and kws['k16_n16']['k_closest'] == gc.KL_KMAX
    assert (kws['chains44']['n_message_gvps'], kws['chains44']['n_update_gvps']) == (gc.GVP_MAX_CHAIN,) * 2
    assert {kws[n]['vector_size'] for n in ('V1', 'V15')} == {1, 15}
    assert {kws[f'dense_rr_{t}']['message_norm'] for t in ('mean', 'n0', 'n10')} == {'mean', 0, 10.0}
    b300 = kws['B300']
    assert (b300['n_keypoints'], b300['k_closest'], b300['n_rr_convs'], b300['message_norm']) == (2, 1, 1, 0)
    assert set(gc.REC_TRAIN) <= set(gc.REC)
