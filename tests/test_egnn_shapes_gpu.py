"""The EGNN denoiser (kpd_egnn_* and kpd_egnn_trainer_*, through LigRecDynamics) away from the shipped shapes: destination runs that
span three to eleven 64-edge tiles in every edge type (main[dst] / cont[tile] of the edge kernels, the continuation walk of the node
update, the final-layer head and the backward edge pieces), both keypoint paths of layer 0, hidden_nf 257 (egnn_wide.hip), edge counts
at the tile edges and launches of 1 .. 9 tiles, node counts on and one past the row blocks of the node-side kernels, empty edge types,
an atom without in-edge, B = 300, the symmetries of the function, and one engine / trainer reused across batches of different tile
layouts (a stale cont row would be read silently).  Every test runs in both GEMM modes (conftest.py's gemm_mode).

The cases, their batches and the properties they are named for live in egnn_shape_cases.py / gvp_shape_cases.py (checked on the CPU by
test_egnn_shape_cases.py and asserted again here before anything is compared).  The reference is oracle/egnn.py run in float64 on the
float64 oracle's edge lists; gradients are torch autograd through it.  Bounds are the project's own: util.assert_parity at 1e-4 (all
three measures; atol 1e-5 of max |ref| for eps_x, as test_egnn_gpu.py) for values, 2e-4 of the largest entry per tensor for gradients,
1e-5 between a complex reordered and in its batch (test_batch_independence).  No case carries a loosened bound.

Measured on an MI355X, worst over both GEMM modes (whole-tensor relative error of eps_h / eps_x; share of the elementwise bound):
long runs 1.2e-6 / 9.7e-7 (0.46), hidden 257 4.3e-7 / 7.7e-7 (0.21), tile edges and node counts 7.0e-7 / 7.0e-7 (0.22), empty and
isolated 5.0e-7 / 6.8e-7 (0.14), symmetry 1.1e-6 / 5.6e-7 (0.32; reordered complexes 5.8e-7 of the 1e-5), trainer forward
9.4e-7 / 8.4e-7 (0.65), worst gradient 1.65e-5 of its tensor's largest entry (coord_mlp.kk.2.bias of layer 0 on lig230; bound 2e-4).
With the first continuation tile of every run over three or more tiles skipped in k_node_update8 / k_node_update8_h and
k_edge_pieces_set (a local experiment), every long-run case, every long-run trainer case and the reuse test fail, while
test_egnn_train_gpu.py's gradient comparison does not notice and test_egnn_gpu.py fails only where a kl run is that long (a small
ligand in a large pocket): its ll, lk and kk runs never are."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G

from . import egnn_shape_cases as ec
from . import gvp_shape_cases as gc
from . import util

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('gemm_mode')]   # both GEMM modes of the EGNN kernels (conftest.py)
TOL = 1e-4          # BASELINE.json north_star: "within 1e-4 rel fp32"
X_ATOL = 1e-5       # eps_x = x_out - x_0, the difference of two O(1) coordinates: its absolute floor is that of the coordinates
GRAD_TOL = 2e-4     # test_egnn_train_gpu.py: relative to the largest entry of each gradient tensor
BATCH_TOL = 1e-5    # test_egnn_gpu.py::test_batch_independence
# two runs of the engine on inputs that an exact symmetry of the function maps onto each other: each is within TOL of that function
SYM_TOL = 2 * TOL


def _gpu_model(name, cuda, gemm_mode):
    model = ec.model(name).to(cuda)
    if ec.EGNN[name]['cfg']['hidden_nf'] <= 256:                       # (above 256 the engine has the exact fp32 path only)
        assert model.engine().gemm_mode() == gemm_mode
    return model


def _forward(model, g, t, cuda):
    with torch.no_grad():
        h, x = model(g.to(cuda), t.to(cuda), None)
    torch.cuda.synchronize()
    return h.cpu(), x.cpu()


def _check(h, x, ref_h, ref_x, n_lig, what, tol=TOL):
    assert torch.isfinite(h).all() and torch.isfinite(x).all(), f'{what}: not finite'
    print(f'{what}: rel err eps_h {util.rel_err(h, ref_h):.2e} eps_x {util.rel_err(x, ref_x):.2e}, elementwise excess '
          f'{util.elementwise_excess(h, ref_h, tol):.3f} {util.elementwise_excess(x, ref_x, tol, X_ATOL):.3f}')
    util.assert_parity(h, ref_h, n_lig, tol, f'{what}: eps_h')
    util.assert_parity(x, ref_x, n_lig, tol, f'{what}: eps_x', atol_rel=X_ATOL)


def _check_counts(handle, name):
    """What the engine's last forward counted against the oracle's lists: edges per type and tiles per launch."""
    got, want = handle.last_counts(), ec.expected_counts(name)
    assert got == want, (name, got, want)


def _check_kp_path(model, name, gemm_mode, cuda):
    """Layer 0's keypoint path as the engine reports it against the case table's (decided from the inputs by the engine's rule)."""
    path = ec.kp_path(name, gemm_mode)
    if path != 'wide':
        assert float(model.engine().debug('kp_table_ok', 1, device=cuda)[0]) == (1.0 if path == 'table' else 0.0), (name, path)


def _case(name, cuda, gemm_mode):
    """One case against the float64 oracle; returns (eps_h, eps_x)."""
    gc.check_batch(ec.EGNN[name]['batch'])                             # the gap and the stated property, from the oracle alone
    ref = ec.reference(name)
    g, t = ec.inputs(name)
    model = _gpu_model(name, cuda, gemm_mode)
    h, x = _forward(model, g, t, cuda)
    _check_counts(model.engine(), name)
    _check_kp_path(model, name, gemm_mode, cuda)
    _check(h, x, ref['eps_h'], ref['eps_x'], g.batch_num_nodes('lig').tolist(), name)
    return h, x


# ---- 1. long destination runs, 2. hidden_nf 257 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ec.LONG)
def test_long_runs(cuda, gemm_mode, name):
    """dense_rad: at least 50 destinations per edge type whose run spans 3 or 4 tiles; lig230: the 200-neighbour ll cap, runs over 4 and
    5 tiles; kp600_lig3: three ligand rows whose kl run spans 10 or 11 tiles.  Every switch of the layer on every batch, every batch
    at hidden_nf 256, dense_rad and kp600_lig3 on both keypoint paths of layer 0."""
    _case(name, cuda, gemm_mode)


@pytest.mark.parametrize('name', ec.WIDE)
def test_long_runs_hidden_257(cuda, gemm_mode, name):
    _case(name, cuda, gemm_mode)


# ---- 3. tile edges and node counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ec.TILES)
def test_tile_edges_and_node_counts(cuda, gemm_mode, name):
    """E_et mod 64 in {0} and {1, 2} for every edge type, launches of 1 .. 9 tiles, E_ll = 0 (t_T1), update_kp_feat alternating; node
    counts 32, 33, 64, 65 of either type: on and one past the 32-row node update and the 64-row projection tile."""
    _case(name, cuda, gemm_mode)


# ---- 4. empty and isolated --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ec.EDGE)
def test_empty_and_isolated(cuda, gemm_mode, name):
    h, x = _case(name, cuda, gemm_mode)
    if name in ec.ISOLATED_CASES:              # no in-edge of any type: eps_x of that atom is exactly zero, here as in the oracle
        assert torch.equal(ec.reference(name)['eps_x'][gc.ISOLATED_ROW], torch.zeros(3, dtype=torch.float64))
        assert torch.equal(x[gc.ISOLATED_ROW], torch.zeros(3)) and torch.isfinite(h[gc.ISOLATED_ROW]).all()


# ---- 5. symmetry ------------------------------------------------------------------------------------------------------------------------
def _sym(cuda, gemm_mode):
    gc.check_batch(gc.RAGGED)
    g, t = ec.inputs(ec.SYM)
    model = _gpu_model(ec.SYM, cuda, gemm_mode)
    base = _forward(model, g, t, cuda)
    n_lig = g.batch_num_nodes('lig').tolist()
    ref = ec.reference(ec.SYM)
    _check(*base, ref['eps_h'], ref['eps_x'], n_lig, 'sym')
    return model, g, t, base, n_lig


def test_same_call_twice_same_bits(cuda, gemm_mode):
    model, g, t, base, _ = _sym(cuda, gemm_mode)
    again = _forward(model, g, t, cuda)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])


def test_rotation_and_translation_per_complex(cuda, gemm_mode):
    """A proper rotation and a translation of at most 20 A of each complex: against the float64 oracle on the moved batch at the
    plain bounds, and against the turned output of the unmoved batch.  The moved batch has the unmoved one's edge lists
    (test_egnn_shape_cases.py recomputes them), so the oracle takes those; the kk index list is the caller's anyway."""
    model, g, t, base, n_lig = _sym(cuda, gemm_mode)
    moved = ec.moved_batch(g)
    h, x = _forward(model, moved, t, cuda)
    ref = ec.oracle(ec.model(ec.SYM).state_dict(), ec.SYM, moved, t)
    _check(h, x, ref['eps_h'], ref['eps_x'], n_lig, 'moved')
    _check(h, x, base[0], ec.rotated_rows(base[1], g), n_lig, 'moved against unmoved', SYM_TOL)


def test_order_of_complexes(cuda, gemm_mode):
    model, g, t, base, n_lig = _sym(cuda, gemm_mode)
    gs, perm = gc.den_complexes(gc.RAGGED), [2, 0, 1]
    h, x = _forward(model, G.batch([gs[i] for i in perm]), t[perm], cuda)
    lp, off = g.node_ptr('lig').tolist(), 0
    for i in perm:
        n = n_lig[i]
        eh, ex = util.rel_err(h[off:off + n], base[0][lp[i]:lp[i + 1]]), util.rel_err(x[off:off + n], base[1][lp[i]:lp[i + 1]])
        print(f'complex {i} reordered: {eh:.2e} {ex:.2e}')
        assert eh < BATCH_TOL and ex < BATCH_TOL, (i, eh, ex)
        off += n


def test_order_of_atoms_in_a_ligand(cuda, gemm_mode):
    """The atoms of one ligand permuted: its rows come out permuted, within the plain bounds of the float64 oracle on the permuted
    batch (which builds its own edge lists: the distances, and so the gaps, are the same)."""
    model, g, t, base, n_lig = _sym(cuda, gemm_mode)
    lp = g.node_ptr('lig').tolist()
    perm = torch.arange(g.num_nodes('lig'))
    perm[lp[2]:lp[3]] = lp[2] + torch.randperm(n_lig[2], generator=torch.Generator().manual_seed(4))
    assert not torch.equal(perm, torch.arange(perm.numel()))
    g2 = g.to('cpu')
    for k in ('x_0', 'h_0'):
        g2.nodes['lig'].data[k] = g.nodes['lig'].data[k][perm]
    ref = ec.oracle(ec.model(ec.SYM).state_dict(), ec.SYM, g2, t, edges=None)
    full = ec.reference(ec.SYM)
    assert float((ref['eps_h'] - full['eps_h'][perm]).abs().max()) < 1e-11 and float((ref['eps_x'] - full['eps_x'][perm]).abs().max()) < 1e-11
    h, x = _forward(model, g2, t, cuda)
    _check(h, x, ref['eps_h'], ref['eps_x'], n_lig, 'atoms permuted')
    _check(h, x, base[0][perm], base[1][perm], n_lig, 'atoms permuted against the rows of the unpermuted run', SYM_TOL)


# ---- 6. engine reuse --------------------------------------------------------------------------------------------------------------------
def _train_step(model, g, t, cuda):
    gd, ins = g.to(cuda), {}
    for key, nt, k in (('lx', 'lig', 'x_0'), ('lh', 'lig', 'h_0'), ('kx', 'kp', 'x_0'), ('kh', 'kp', 'h_0')):
        ins[key] = gd.nodes[nt].data[k].detach().clone().requires_grad_(True)
        gd.nodes[nt].data[k] = ins[key]
    model.zero_grad(set_to_none=True)
    eh, ex = model(gd, t.to(cuda), None)
    assert eh.requires_grad and ex.requires_grad
    w_h, w_x = gc.loss_weights(eh.shape[0])
    ((eh * w_h.to(cuda)).sum() + (ex * w_x.to(cuda)).sum()).backward()
    torch.cuda.synchronize()
    return (eh.detach().cpu(), ex.detach().cpu(), {k: v.grad.cpu() for k, v in ins.items()},
            {n: p.grad.cpu().clone() for n, p in model.named_parameters()})


def test_engine_reuse(cuda, gemm_mode):
    """One model on dense_rad, small, t_T1, dense_rad: the workspace is carved for the first batch and every later one writes fewer
    cont rows.  Every output is what a fresh model gives on that batch, bit for bit."""
    name = ec.REUSE_CASE
    model, outs = _gpu_model(name, cuda, gemm_mode), []
    for b in ec.REUSE_BATCHES:
        g, t = ec.inputs(name, b)
        outs.append(_forward(model, g, t, cuda))
        fresh = _forward(_gpu_model(name, cuda, gemm_mode), g, t, cuda)
        assert torch.equal(outs[-1][0], fresh[0]) and torch.equal(outs[-1][1], fresh[1]), f'{b} on a used engine'
    ref = ec.reference(name)
    _check(*outs[-1], ref['eps_h'], ref['eps_x'], gc.den_batch(gc.DENSE_RAD).batch_num_nodes('lig').tolist(), 'dense_rad on a used engine')
    assert torch.equal(outs[0][0], outs[-1][0]) and torch.equal(outs[0][1], outs[-1][1])


def test_trainer_reuse(cuda, gemm_mode):
    """The same for the trainer, forward and backward: outputs, input gradients and parameter gradients (after zero_grad) of a used
    trainer against a fresh one's, bit for bit."""
    name = ec.REUSE_CASE
    model = _gpu_model(name, cuda, gemm_mode)
    for b in ec.REUSE_BATCHES:
        g, t = ec.inputs(name, b)
        used, fresh = _train_step(model, g, t, cuda), _train_step(_gpu_model(name, cuda, gemm_mode), g, t, cuda)
        assert torch.equal(used[0], fresh[0]) and torch.equal(used[1], fresh[1]), f'{b} on a used trainer'
        for k in ec.INPUT_KEYS:
            assert torch.equal(used[2][k], fresh[2][k]), f'{b} on a used trainer: gradient of input {k}'
        diff = [n for n in fresh[3] if not torch.equal(used[3][n], fresh[3][n])]
        assert not diff, f'{b} on a used trainer: gradients of {diff[:6]}'


# ---- 7. trainer -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ec.TRAIN)
def test_trainer(cuda, gemm_mode, name):
    """kpd_egnn_trainer_* on the long-run batches (k_egnn_edge_train and k_egnn_edge_bwd over runs of at least 3 tiles, the
    source-grouped sums over as many out-edges), the tile-edge and node-count batches, empty ll and kk lists, the atom without
    in-edge and B = 300: the training forward against the oracle and against the inference engine, every parameter and input gradient
    against float64 autograd, two passes bit for bit."""
    gc.check_batch(ec.EGNN[name]['batch'])
    ref = ec.reference(name, torch.float64, True)
    g, t = ec.inputs(name)
    n_lig = g.batch_num_nodes('lig').tolist()
    model = _gpu_model(name, cuda, gemm_mode)
    eng = _forward(model, g, t, cuda)
    _check(*eng, ref['eps_h'], ref['eps_x'], n_lig, f'{name} engine')
    eh, ex, d_in, d_par = _train_step(model, g, t, cuda)
    _check(eh, ex, ref['eps_h'], ref['eps_x'], n_lig, f'{name} trainer')
    _check(eh, ex, eng[0], eng[1], n_lig, f'{name} trainer against engine')
    errs = ec.grad_errors(d_par, d_in, ref)
    print(f'{name}: worst gradient errors of {len(errs)} tensors', [(n, f'{e:.2e}') for n, e in sorted(errs.items(), key=lambda kv: -kv[1])[:3]])
    util.assert_param_grads(model, ref['params'], GRAD_TOL)           # (its rules: a lone bias on its weight's scale, exact zero without a path)
    for n, r in ref['params'].items():
        if r is None:                                                  # no path to the loss (keypoint side of the last layer): exactly zero
            assert float(d_par[n].abs().max()) == 0.0, n
    for k in ec.INPUT_KEYS:
        assert torch.isfinite(d_in[k]).all(), k
        assert errs[f'input {k}'] < GRAD_TOL, f'{name}: gradient of input {k}: {errs[f"input {k}"]:.3e} of its largest entry'
    if name == 'tr_isolated':                  # the atom without in-edge sends nothing and receives nothing: its position reaches no output
        assert float(ref['inputs']['lx'][gc.ISOLATED_ROW].abs().max()) == 0.0 and float(d_in['lx'][gc.ISOLATED_ROW].abs().max()) == 0.0
        assert torch.equal(ex[gc.ISOLATED_ROW], torch.zeros(3))
    eh2, ex2, d_in2, d_par2 = _train_step(model, g, t, cuda)
    assert torch.equal(eh, eh2) and torch.equal(ex, ex2)
    for n in d_par:
        assert torch.equal(d_par[n], d_par2[n]), f'{name}: gradient of {n} differs between two backward passes'
    for k in d_in:
        assert torch.equal(d_in[k], d_in2[k]), f'{name}: gradient of input {k} differs between two backward passes'
