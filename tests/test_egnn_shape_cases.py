"""CPU: every case of egnn_shape_cases.py names a batch whose stated property holds (gvp_shape_cases.check_batch, from the oracle alone),
the table covers what test_egnn_shapes_gpu.py claims to cover, and the float32 oracle's distance from the float64 oracle is printed
per case and asserted to stay well inside the plain bounds: no case of the GPU module carries a loosened one."""
import pytest
import torch

from . import egnn_shape_cases as ec
from . import gvp_shape_cases as gc
from . import util

ALL = ec.LONG + ec.WIDE + ec.TILES + ec.EDGE + [ec.SYM] + ec.TRAIN
# The float32 oracle against the float64 oracle, as a share of the bounds of the GPU module.  A bound of the GPU module is loosened
# only where the figure here comes within a factor 2 of it (half the bound); none does: the largest elementwise excess of any case is
# 0.41 of the bound (lig230_h64_n5_nonorm_notanh), the largest gradient error 1.8e-5 of the tensor's largest entry against the bound of
# 2e-4 (coord_mlp.lk.0.weight of layer 0 in tr_dense_n0).
MAX_EXCESS_F32 = 0.55            # test_gvp_shape_cases.py uses the same for the same purpose
GRAD_TOL = 2e-4
MAX_GRAD_F32 = GRAD_TOL / 2


def test_every_case_names_a_checked_batch():
    assert set(ALL) == set(ec.EGNN) and len(ALL) == len(set(ALL))
    for name in ALL:
        c = ec.EGNN[name]
        assert gc.check_batch(c['batch']) >= gc.GAP, name
        b = gc.BATCHES[c['batch']]
        assert (c['cfg']['ll_k'], c['cfg']['kl_k']) == (b['ll_k'], b['kl_k']), name
    used = {ec.EGNN[n]['batch'] for n in ALL}
    at256 = {ec.EGNN[n]['batch'] for n in ALL if ec.EGNN[n]['cfg']['hidden_nf'] == 256}
    assert used == at256, used - at256                                     # every batch at the full width once
    assert all(ec.EGNN[n]['cfg']['n_layers'] == 2 for n in ec.LONG + ec.TILES)


def test_long_grid_shows_every_switch_on_every_batch():
    assert {ec.EGNN[n]['batch'] for n in ec.LONG} == set(ec.LONG_BATCHES) == {gc.DENSE_RAD, gc.LIG230, gc.KP600}
    for b in ec.LONG_BATCHES:
        cfgs = [ec.EGNN[n]['cfg'] for n in ec.LONG if ec.EGNN[n]['batch'] == b]
        assert {c['message_norm'] for c in cfgs} == {0, ec.MN_CONST}
        for sw in ('norm', 'use_tanh', 'update_kp_feat'):
            assert {bool(c[sw]) for c in cfgs} == {True, False}, (b, sw)
        assert {c['hidden_nf'] for c in cfgs} >= {64, 100, 256}
    assert {(ec.EGNN[n]['batch'], ec.EGNN[n]['cfg']['hidden_nf']) for n in ec.WIDE} == {(gc.DENSE_RAD, 257), (gc.LIG230, 257)}


def test_both_keypoint_paths():
    """dense_rad and kp600_lig3 run layer 0 from the class table (as generated: one-hot kp_h, B * rec_nf <= n_kp / 2) and from the
    per-atom projection (kp_h replaced by randn); in f16x2 mode the table is never used."""
    for b in (gc.DENSE_RAD, gc.KP600):
        paths = {ec.kp_path(n) for n in ec.LONG if ec.EGNN[n]['batch'] == b}
        assert paths == {'table', 'per_atom'}, (b, paths)
    for n in ec.LONG:
        want = 'per_atom' if ec.EGNN[n]['randn_kp'] or ec.EGNN[n]['batch'] == gc.LIG230 else 'table'      # lig230: 20 class rows for 29 keypoints
        assert ec.kp_path(n) == want and ec.kp_path(n, 'f16x2') == 'per_atom', n
    assert all(ec.kp_path(n) == 'wide' for n in ec.WIDE)
    assert all(ec.kp_path(n) == 'per_atom' for n in ec.TILES)              # hand-built batches carry randn kp_h
    print({n: ec.kp_path(n) for n in ALL})


def test_tile_and_node_count_coverage():
    rem, tiles = gc.tile_coverage()
    for et in gc.ETYPES:
        assert 0 in rem[et] and rem[et] & {1, 2}, (et, rem[et])
    assert tiles >= set(range(1, 10)), tiles
    assert {ec.EGNN[n]['batch'] for n in ec.TILES} == set(gc.TILE) | set(gc.NODES)
    tile_cases = [n for n in ec.TILES if ec.EGNN[n]['batch'] in gc.TILE]
    assert [bool(ec.EGNN[n]['cfg']['update_kp_feat']) for n in tile_cases] == [i % 2 == 0 for i in range(len(tile_cases))]
    n_kp, n_lig = gc.node_coverage()
    assert n_kp == {32, 33, 64, 65} and n_lig == {32, 33, 64, 65}
    # the counts against the row blocks they were chosen for: on a block edge and one past it
    for blk in (4, 8, 16, 32):
        assert {n % blk for n in n_kp} == {0, 1} and {n % blk for n in n_lig} == {0, 1}
    assert {-(-n // 64) for n in n_lig} == {1, 2} and {-(-n // 32) for n in n_kp} == {1, 2, 3}
    assert {ec.EGNN[n]['batch'] for n in ec.TRAIN} >= set(gc.NODES) | {'t_ll64', 't_kl65_kk65', 't_T1'}


def test_edge_sym_and_train_cases():
    cfg = {n: ec.EGNN[n]['cfg'] for n in ALL}
    assert [ec.EGNN[n]['batch'] for n in ec.EDGE] == [gc.EMPTY_KK, gc.ISOLATED, gc.ISOLATED, gc.B1, gc.B300, gc.ONE_ATOM]
    assert {cfg[n]['message_norm'] for n in ec.ISOLATED_CASES} == {0, ec.MN_CONST}
    assert cfg['B300']['n_layers'] == cfg['tr_B300']['n_layers'] == 1
    assert ec.EGNN[ec.SYM]['batch'] == gc.RAGGED and cfg[ec.SYM]['n_layers'] == 3
    # engine reuse: the long batch, two whose every edge type has fewer tiles, the long one again
    assert ec.REUSE_CASE in ec.LONG and ec.REUSE_BATCHES[0] == ec.REUSE_BATCHES[-1] == ec.EGNN[ec.REUSE_CASE]['batch'] == gc.DENSE_RAD
    for b in ec.REUSE_BATCHES[1:-1]:
        assert all(gc.den_batch(b).num_nodes(nt) < gc.den_batch(gc.DENSE_RAD).num_nodes(nt) for nt in ('lig', 'kp'))
    E = lambda n, et: gc.den_stats(ec.EGNN[n]['batch'])[et]['E']
    assert any(E(n, 'll') == 0 for n in ec.TRAIN) and any(E(n, 'kk') == 0 for n in ec.TRAIN)
    assert E('tr_one_atom', 'll') == 0 and E('tr_t_T1', 'll') == 0 and E('tr_empty_kk', 'kk') == 0
    assert all(cfg[n]['hidden_nf'] == 256 for n in ec.TRAIN if n != 'tr_dense_h100') and cfg['tr_dense_h100']['hidden_nf'] == 100
    assert {cfg[n]['message_norm'] for n in ('tr_dense_n0', 'tr_dense_n5')} == {0, ec.MN_CONST}
    assert not cfg['tr_dense_nokp']['update_kp_feat']
    for n in ec.TRAIN_LONG:                                                  # a tile wholly inside one run, in the trainer's cases too
        st = gc.den_stats(ec.EGNN[n]['batch'])
        assert max(int(st[et]['spans'].max()) for et in ('ll', 'kl')) >= 3, n


@pytest.mark.parametrize('name', ALL)
def test_reference_and_float32_margin(name):
    """The float64 reference is finite and float64; the float32 oracle on the same edge lists stays inside MAX_EXCESS_F32 of the
    elementwise bounds (rtol 1e-4; atol 1e-6 max |ref| for eps_h, 1e-5 for eps_x) and, for the trainer's cases, inside MAX_GRAD_F32
    per gradient tensor."""
    grad = name in ec.TRAIN
    ref, r32 = ec.reference(name, torch.float64, grad), ec.reference(name, torch.float32, grad)
    assert all(ref[k].dtype == torch.float64 and torch.isfinite(ref[k]).all() for k in ('eps_h', 'eps_x'))
    bname = ec.EGNN[name]['batch']
    st = gc.den_stats(bname)
    ex_h = util.elementwise_excess(r32['eps_h'], ref['eps_h'], rtol=1e-4, atol_rel=1e-6)
    ex_x = util.elementwise_excess(r32['eps_x'], ref['eps_x'], rtol=1e-4, atol_rel=1e-5)
    print(f'{name}: gap {gc.check_batch(bname):.2e}', {et: (st[et]['E'], st[et]['tiles'], int(st[et]['spans'].max()) if st[et]['E'] else 0) for et in gc.ETYPES},
          f'kp path {ec.kp_path(name)}; float32 oracle elementwise excess eps_h {ex_h:.3f} eps_x {ex_x:.3f}')
    assert float(ref['eps_x'].abs().max()) > 1e-3 * float(ref['eps_h'].abs().max())        # the coordinate head carries weight
    assert max(ex_h, ex_x) <= MAX_EXCESS_F32
    if grad:
        assert all(ref['inputs'][k] is not None and torch.isfinite(ref['inputs'][k]).all() for k in ec.INPUT_KEYS)
        errs = ec.grad_errors(r32['params'], r32['inputs'], ref)
        worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
        print(f'{name}: float32 autograd, worst gradient errors of {len(errs)} tensors', [(n, f'{e:.2e}') for n, e in worst])
        assert len(errs) > 10 and worst[0][1] <= MAX_GRAD_F32, worst


@pytest.mark.parametrize('name', ec.ISOLATED_CASES)
def test_isolated_atom_gets_zero_eps_x(name):
    """No in-edge of any type: x_neigh of the atom is an empty sum in every layer, so the float64 oracle gives eps_x = 0 exactly, in
    both norm modes, and a finite eps_h; every other atom of that ligand moves."""
    ref = ec.reference(name)
    assert torch.equal(ref['eps_x'][gc.ISOLATED_ROW], torch.zeros(3, dtype=torch.float64))
    assert torch.isfinite(ref['eps_h']).all() and torch.isfinite(ref['eps_x']).all()
    assert float(ref['eps_x'].abs().max(dim=1).values[:gc.ISOLATED_ROW].min()) > 0
    g = ec.reference('tr_isolated', torch.float64, True)['inputs']
    assert float(g['lx'][gc.ISOLATED_ROW].abs().max()) == 0.0            # and its position reaches no output


def test_sym_edge_lists_survive_the_rigid_motions():
    """The moved batch of the symmetry test has the float64 oracle's edge lists of the unmoved one: a rigid motion changes a
    distance by rounding only, and every deciding distance has a relative gap of 1e-3."""
    from oracle import egnn as oegnn
    g, _ = ec.inputs(ec.SYM)
    moved = ec.moved_batch(g)
    ob = util.to_obatch64(moved)
    with torch.no_grad(), util.float64_oracle():
        e = oegnn.lig_edges(ob, gc.graph_cfg(gc.RAGGED))
    for et in ('ll', 'kl', 'lk'):
        assert torch.equal(e[et][0], gc.den_edges(gc.RAGGED)[et][0]) and torch.equal(e[et][1], gc.den_edges(gc.RAGGED)[et][1]), et
    # 20 A away from the origin fp32 holds the coordinates, and so eps_x = x_out - x_0, less finely: the plain bounds still hold
    sd, t = ec.model(ec.SYM).state_dict(), ec.inputs(ec.SYM)[1]
    ref, r32 = ec.oracle(sd, ec.SYM, moved, t), ec.oracle(sd, ec.SYM, moved, t, torch.float32)
    ex_h = util.elementwise_excess(r32['eps_h'], ref['eps_h'], rtol=1e-4, atol_rel=1e-6)
    ex_x = util.elementwise_excess(r32['eps_x'], ref['eps_x'], rtol=1e-4, atol_rel=1e-5)
    print(f'sym moved: float32 oracle elementwise excess eps_h {ex_h:.3f} eps_x {ex_x:.3f}')
    assert max(ex_h, ex_x) <= MAX_EXCESS_F32
    unmoved = ec.reference(ec.SYM)
    assert float((ref['eps_h'] - unmoved['eps_h']).abs().max()) < 1e-5 * float(unmoved['eps_h'].abs().max())      # (the moved positions are fp32)
