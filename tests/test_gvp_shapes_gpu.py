"""The GVP denoiser (kpd_gvp_* and kpd_gvp_trainer_*, through LigRecDynamicsGVP) away from the shipped shapes: destination runs that
span three to eleven 64-edge tiles (the continuation loop of the node kernels over ms_cont / mv_cont), edge counts at the tile edges
and launches of 1 .. 9 tiles, empty edge types and rows without in-edge, every chain length 1 and GVP_MAX_CHAIN = 4, the narrowest
models, and the symmetries of the function.  Every engine case runs in both node-side forms (register-chained and cooperative).

The cases, their batches and the properties they are named for live in gvp_shape_cases.py (checked on the CPU by
test_gvp_shape_cases.py and asserted again here before anything is compared).  The reference is oracle/gvp.py run in float64;
gradients are torch autograd through it.  Bounds are the project's own: util.assert_parity at 1e-4 (all three measures) for values,
2e-4 of the largest entry per tensor for gradients.  No case carries a loosened bound.  Exact fp32 mode only: the f16x2 forms share
the segmented-sum and launch code, and test_gvp_gpu.py / test_gvp_train_gpu.py keep their two-mode runs."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip
from keypoint_diffusion_amd import synth
from keypoint_diffusion_amd.dynamics_gvp import LigRecDynamicsGVP

from . import gvp_shape_cases as gc
from . import util

pytestmark = pytest.mark.gpu
TOL = 1e-4
GRAD_TOL = 2e-4     # test_gvp_train_gpu.py: relative to the largest entry of each gradient tensor
# two runs of the engine on inputs that an exact symmetry of the function maps onto each other: each is within TOL of that function
SYM_TOL = 2 * TOL
FORMS = (('chained', -1), ('cooperative', 1 << 30))       # engine switch `coop_rows=`: -1 never, 1 << 30 always cooperative


def _gpu_model(name, cuda):
    model = gc.den_model(name).to(cuda)
    model.gemm_mode = 'f32'
    return model


def _forward(model, g, t, cuda):
    with torch.no_grad():
        h, x = model(g.to(cuda), t.to(cuda), None)
    torch.cuda.synchronize()
    return h.cpu(), x.cpu()


def _check(h, x, ref_h, ref_x, n_lig, what, tol=TOL):
    assert torch.isfinite(h).all() and torch.isfinite(x).all(), f'{what}: not finite'
    util.assert_parity(h, ref_h, n_lig, tol, f'{what}: eps_h')
    util.assert_parity(x, ref_x, n_lig, tol, f'{what}: eps_x')


def _edge_set(s, d):
    return set(zip(s.tolist(), d.tolist()))


def _check_edge_lists(bname, cuda):
    """The engine's graph build on the batch against the float64 oracle's lists: ll and lk in order, kl (destination-major here,
    keypoint-major there) and kk as sets with the same in-degree per destination."""
    b, ref = gc.BATCHES[bname], gc.den_edges(bname)
    g = gc.den_batch(bname).to(cuda)
    pb = g.prepared()
    out = hip.build_lig_graph(pb, g.nodes['lig'].data['x_0'], g.nodes['kp'].data['x_0'], float(b['cutoffs']['ll']), b['kl_k'], ll_k=b['ll_k'],
                              kl_cutoff=float(b['cutoffs']['kl']))
    torch.cuda.synchronize()
    E_ll, E_kl = int(out['counts'][0]), int(out['counts'][1])
    assert (E_ll, E_kl) == (ref['ll'][0].numel(), ref['kl'][0].numel()), f'{bname}: edge counts'
    got = {et: (out[f'{et}_src'][:E].long().cpu(), out[f'{et}_dst'][:E].long().cpu()) for et, E in (('ll', E_ll), ('kl', E_kl), ('lk', E_kl))}
    got['kk'] = (pb.kk_src.long().cpu(), pb.kk_dst.long().cpu())
    for et in ('ll', 'lk'):
        assert torch.equal(got[et][0], ref[et][0]) and torch.equal(got[et][1], ref[et][1]), f'{bname}: {et} edges'
    for et in ('kl', 'kk'):
        assert _edge_set(*got[et]) == _edge_set(*ref[et]) and got[et][0].numel() == ref[et][0].numel(), f'{bname}: {et} edges'
        n = g.num_nodes(gc.DST_NT[et])
        assert torch.equal(torch.bincount(got[et][1], minlength=n), torch.bincount(ref[et][1], minlength=n)), f'{bname}: {et} in-degrees'
    assert bool((got['kl'][1][1:] >= got['kl'][1][:-1]).all()), f'{bname}: kl is not destination-major'


def _check_counts(model, name):
    """What the engine's last forward counted against the oracle's lists: edges per type and tiles per launch."""
    c = gc.DEN[name]
    st, (t_all, t_last) = gc.den_stats(c['batch']), gc.launch_tiles(c['batch'])
    got = model.engine().last_counts()
    assert (got['E_ll'], got['E_kl']) == (st['ll']['E'], st['kl']['E']), got
    assert got['tiles_last'] == t_last and got['E_last'] == st['ll']['E'] + st['kl']['E'], got
    if c['cfg']['update_kp'] and c['cfg']['n_convs'] > 1:             # some conv runs all four edge types
        assert (got['E_lk'], got['E_kk'], got['tiles']) == (st['lk']['E'], st['kk']['E'], t_all), got
    return got


def _case(name, cuda):
    """One case in both node-side forms against the float64 oracle; returns form -> (eps_h, eps_x)."""
    bname = gc.DEN[name]['batch']
    gc.check_batch(bname)                                             # the gap and the stated property, from the oracle alone
    _check_edge_lists(bname, cuda)
    ref = gc.den_reference(name)
    g, t = gc.den_inputs(name)
    n_lig = g.batch_num_nodes('lig').tolist()
    model, outs, failed = _gpu_model(name, cuda), {}, []
    try:
        for form, rows in FORMS:
            model.engine().debug(f'coop_rows={rows}')
            h, x = _forward(model, g, t, cuda)
            outs[form] = (h, x)
            try:                                                      # both forms run and report, whichever fails first
                _check_counts(model, name)
                _check(h, x, ref['eps_h'], ref['eps_x'], n_lig, f'{name} {form}')
            except AssertionError as ex:
                failed.append(str(ex).splitlines()[0])
    finally:
        model.engine().debug('coop_rows=0')
    assert not failed, ' | '.join(failed)
    return outs


# ---- 1. long destination runs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', gc.LONG)
def test_long_runs(cuda, name):
    """dense_rad: at least 50 destinations per edge type whose run spans 3 or 4 tiles; lig230: the 200-neighbour ll cap, runs over 4 and
    5 tiles; kp600_lig3: three ligand rows whose kl run spans 10 or 11 tiles, beside keypoints of lk in-degree 3.  At both widths of the
    segmented sum (vt = S < 256 ? tid - 192 : tid), in all three norm modes."""
    _case(name, cuda)


# ---- 2. tile edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', gc.TILES)
def test_tile_edges(cuda, name):
    """E_et mod 64 in {0} and {1, 2} for every edge type and launches of T = 1 .. 9 tiles (gvp_shape_cases.tile_coverage): the XCD map
    chunk_tiles = (T + 7) >> 3 leaves workgroups without a tile below 8.  T is what the engine itself counted."""
    _case(name, cuda)


# ---- 3. empty and isolated --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', gc.EDGE)
def test_empty_and_isolated(cuda, name):
    outs = _case(name, cuda)
    if name.startswith('isolated'):            # no in-edge of any type: the oracle's eps_x of that atom is exactly zero, in every norm mode
        ref = gc.den_reference(name)
        assert torch.equal(ref['eps_x'][gc.ISOLATED_ROW], torch.zeros(3, dtype=torch.float64))
        for form, (h, x) in outs.items():
            assert torch.isfinite(h[gc.ISOLATED_ROW]).all() and torch.isfinite(x[gc.ISOLATED_ROW]).all(), form


# ---- 4. chain lengths, 5. narrow models -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', gc.CHAINS)
def test_chain_lengths(cuda, name):
    """Head stage + n_gvps - 1 generic stages + a weight ring of n0 + (n_gvps - 1) (NTS + 2) slots: a single-stage noise chain and
    four-stage message / update chains, at both widths."""
    _case(name, cuda)


@pytest.mark.parametrize('name', gc.NARROW)
def test_narrow_models(cuda, name):
    _case(name, cuda)


# ---- 6. symmetry ------------------------------------------------------------------------------------------------------------------------
def _sym(cuda):
    gc.check_batch(gc.RAGGED)
    g, t = gc.den_inputs(gc.SYM)
    model = _gpu_model(gc.SYM, cuda)
    base = _forward(model, g, t, cuda)
    n_lig = g.batch_num_nodes('lig').tolist()
    ref = gc.den_reference(gc.SYM)
    _check(*base, ref['eps_h'], ref['eps_x'], n_lig, 'sym')
    return model, g, t, base, n_lig


def test_same_call_twice_same_bits(cuda):
    model, g, t, base, _ = _sym(cuda)
    again = _forward(model, g, t, cuda)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])


def test_rotation_and_translation_per_complex(cuda):
    """A proper rotation and a translation of at most 20 A of each complex (positions and the keypoints' vector features): eps_h
    stays, eps_x turns with its complex.  The edge lists cannot change: every deciding distance has a relative gap of 1e-3."""
    model, g, t, base, n_lig = _sym(cuda)
    g2 = g.to('cpu')
    lp, kp = g.node_ptr('lig').tolist(), g.node_ptr('kp').tolist()
    lx, kx, kv = (g.nodes[nt].data[k].double().clone() for nt, k in (('lig', 'x_0'), ('kp', 'x_0'), ('kp', 'v_0')))
    want_x = base[1].double().clone()
    for b, (R, tr) in enumerate(gc.rigid_motions(g.batch_size)):
        lx[lp[b]:lp[b + 1]] = lx[lp[b]:lp[b + 1]] @ R.T + tr
        kx[kp[b]:kp[b + 1]] = kx[kp[b]:kp[b + 1]] @ R.T + tr
        kv[kp[b]:kp[b + 1]] = kv[kp[b]:kp[b + 1]] @ R.T
        want_x[lp[b]:lp[b + 1]] = want_x[lp[b]:lp[b + 1]] @ R.T
    g2.nodes['lig'].data['x_0'], g2.nodes['kp'].data['x_0'], g2.nodes['kp'].data['v_0'] = lx.float(), kx.float(), kv.float()
    h, x = _forward(model, g2, t, cuda)
    _check(h, x, base[0], want_x, n_lig, 'moved', SYM_TOL)


def test_order_of_complexes(cuda):
    model, g, t, base, n_lig = _sym(cuda)
    gs, perm = gc.den_complexes(gc.RAGGED), [2, 0, 1]
    h, x = _forward(model, G.batch([gs[i] for i in perm]), t[perm], cuda)
    lp, off = g.node_ptr('lig').tolist(), 0
    for i in perm:
        n = n_lig[i]
        _check(h[off:off + n], x[off:off + n], base[0][lp[i]:lp[i + 1]], base[1][lp[i]:lp[i + 1]], None, f'complex {i} reordered', SYM_TOL)
        off += n


def test_alone_and_batched(cuda):
    model, g, t, base, n_lig = _sym(cuda)
    gs, lp = gc.den_complexes(gc.RAGGED), g.node_ptr('lig').tolist()
    for i, gi in enumerate(gs):
        h, x = _forward(model, G.batch([gi]), t[i:i + 1], cuda)
        _check(h, x, base[0][lp[i]:lp[i + 1]], base[1][lp[i]:lp[i + 1]], None, f'complex {i} alone', SYM_TOL)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('over,message', gc.REFUSALS)
def test_refusals(cuda, over, message):
    """kpd_gvp_create's host-side checks: nothing is launched for a config outside the kernels' limits, and the error names the value."""
    over = dict(over)
    n_lig_scalars = over.pop('n_lig_scalars', 10)
    model = synth.fill_state_dict_(LigRecDynamicsGVP(n_lig_scalars, 10, graph_cutoffs=gc.CUT, **dict(gc.BASE, **over)), 7).eval().to(cuda)
    with pytest.raises(hip.KpdError, match=message):
        model.engine()
    for k, v in over.items():
        with pytest.raises(hip.KpdError, match=f'{k}={v}'):
            model.engine()


# ---- trainer ----------------------------------------------------------------------------------------------------------------------------
def _train_step(model, g, t, cuda):
    gd, ins = g.to(cuda), {}
    for key, nt, k in (('lh', 'lig', 'h_0'), ('kh', 'kp', 'h_0'), ('kv', 'kp', 'v_0'), ('lx', 'lig', 'x_0'), ('kx', 'kp', 'x_0')):
        ins[key] = gd.nodes[nt].data[k].detach().clone().requires_grad_(True)
        gd.nodes[nt].data[k] = ins[key]
    model.zero_grad(set_to_none=True)
    eh, ex = model(gd, t.to(cuda), None)
    w_h, w_x = gc.loss_weights(eh.shape[0])
    ((eh * w_h.to(cuda)).sum() + (ex * w_x.to(cuda)).sum()).backward()
    torch.cuda.synchronize()
    return (eh.detach().cpu(), ex.detach().cpu(), {k: v.grad.cpu() for k, v in ins.items()},
            {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})


@pytest.mark.parametrize('name', gc.TRAIN)
def test_trainer(cuda, name):
    """kpd_gvp_trainer_* on the long-run batches (k_gvp_chain<., 0, 1>, k_gvp_chain_bwd and k_gvp_node_chain_bwd over runs of at least
    3 tiles), the shortest and longest chains and the atom without in-edge: parameter and input gradients against float64 autograd,
    the training forward against the oracle and against the inference engine, two backward passes bit for bit."""
    gc.check_batch(gc.DEN[name]['batch'])
    ref = gc.den_reference(name, torch.float64, True)
    g, t = gc.den_inputs(name)
    n_lig = g.batch_num_nodes('lig').tolist()
    model = _gpu_model(name, cuda)
    eng = _forward(model, g, t, cuda)
    _check(*eng, ref['eps_h'], ref['eps_x'], n_lig, f'{name} engine')
    eh, ex, d_in, d_par = _train_step(model, g, t, cuda)
    assert model._trainer()[0].message_path() == 1                     # hidden width 256: the register-chained message kernels
    _check(eh, ex, ref['eps_h'], ref['eps_x'], n_lig, f'{name} trainer')
    _check(eh, ex, eng[0], eng[1], n_lig, f'{name} trainer against engine')
    util.assert_param_grads(model, ref['params'], GRAD_TOL)
    for k, r in ref['inputs'].items():
        assert torch.isfinite(d_in[k]).all(), k
        err = float((d_in[k].double() - r).abs().max() / r.abs().max())
        assert err < GRAD_TOL, f'{name}: gradient of input {k}: {err:.3e} of its largest entry'
    if name == 'tr_isolated':                  # the atom without in-edge sends nothing and receives nothing: position and noise decouple
        assert float(ref['inputs']['lx'][gc.ISOLATED_ROW].abs().max()) == 0.0 and float(d_in['lx'][gc.ISOLATED_ROW].abs().max()) == 0.0
    eh2, ex2, d_in2, d_par2 = _train_step(model, g, t, cuda)
    assert torch.equal(eh, eh2) and torch.equal(ex, ex2) and d_par.keys() == d_par2.keys()
    for n in d_par:
        assert torch.equal(d_par[n], d_par2[n]), f'{name}: gradient of {n} differs between two backward passes'
    for k in d_in:
        assert torch.equal(d_in[k], d_in2[k]), f'{name}: gradient of input {k} differs between two backward passes'
