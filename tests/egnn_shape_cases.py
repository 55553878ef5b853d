"""Case table of test_egnn_shapes_gpu.py: the EGNN denoiser (csrc/egnn.hip, egnn_kernels.hip, egnn_wide.hip, egnn_train.hip) away from
the shipped shapes.  A case is a batch of gvp_shape_cases.py (the edge lists of oracle.egnn.lig_edges are the same for both denoisers,
and so are the properties stated there from the oracle alone: tile spans of the destination runs, E mod 64, tile counts, empty edge
types, rows without in-edge, a relative gap of at least 1e-3 behind every list) plus a LigRecDynamics config based on util.EGNN_C2.

The reference everywhere is oracle/egnn.py run in float64 (weights, positions, features, t and the oracle's own constants) on the
edge lists of gc.den_edges, so it is a high-precision one and not a second fp32 rounding of the same sums; gradients are torch
autograd through the same run.  (The one fp32 step left in it is the quotient edges / nodes of message_norm = 0, which the oracle
casts itself: 6e-8 of z.)  References are computed once (lru_cache) and never written to afterwards.

To keep the float64 oracle affordable the grid runs at n_layers = 2 (one full layer and the pruned last one) and mostly at a narrow
hidden_nf (100 or 64: zero-padded onto the same 256-wide kernels, so segment and tile logic is the same); every batch appears at
hidden_nf = 256 at least once."""
import functools

import torch

from keypoint_diffusion_amd import synth
from oracle import egnn as oegnn

from . import gvp_shape_cases as gc
from . import util

BASE = dict(util.EGNN_C2, n_layers=2)        # hidden 256, tanh, message_norm 0, update_kp_feat, LayerNorm
ATOM_NF = REC_NF = 10
MN_CONST = 5.0
EGNN = {}


def _egnn(name, bname, randn_kp=False, **over):
    """`randn_kp`: kp_h replaced by seeded randn (not one-hot: layer 0 takes the per-atom keypoint projection)."""
    b = gc.BATCHES[bname]
    assert name not in EGNN, name
    EGNN[name] = dict(batch=bname, randn_kp=randn_kp, cfg=dict(BASE, **over, ll_k=b['ll_k'], kl_k=b['kl_k']))
    return name


# ---- 1. long destination runs: main[dst] / cont[tile] of k_egnn_edge and the walk lo / 64 + 1 .. (hi - 1) / 64 of the node kernels -----
LONG_BATCHES = (gc.DENSE_RAD, gc.LIG230, gc.KP600)
SWITCHES = ('message_norm', 'norm', 'use_tanh', 'update_kp_feat')
LONG = []
for _b in LONG_BATCHES:
    LONG += [_egnn(f'{_b}_h100', _b, hidden_nf=100),
             _egnn(f'{_b}_h64_n5_nonorm_notanh', _b, hidden_nf=64, message_norm=MN_CONST, norm=False, use_tanh=False),
             _egnn(f'{_b}_h100_nokp_notanh', _b, hidden_nf=100, update_kp_feat=False, use_tanh=False),      # meta: tile offsets of ll + kl only
             _egnn(f'{_b}_h256', _b)]
# layer 0's other keypoint path: as generated kp_h is one-hot (the class table where B * rec_nf <= n_kp / 2, fp32 mode)
LONG += [_egnn(f'{gc.DENSE_RAD}_h64_randn_kp', gc.DENSE_RAD, randn_kp=True, hidden_nf=64, message_norm=MN_CONST),
         _egnn(f'{gc.KP600}_h100_randn_kp', gc.KP600, randn_kp=True, hidden_nf=100)]

# ---- 2. hidden_nf 257: the gather, head and segmented-sum kernels of egnn_wide.hip (inference only) -------------------------------
WIDE = [_egnn(f'{gc.DENSE_RAD}_h257', gc.DENSE_RAD, hidden_nf=257), _egnn(f'{gc.LIG230}_h257', gc.LIG230, hidden_nf=257)]

# ---- 3. tile edges (E mod 64 in {0, 1, 2} per edge type, launches of 1 .. 9 tiles, E_ll = 0) and node counts on / one past the row
# blocks of the node-side kernels: TN = 32 (node update), TM = 64 (projection), 8 (LayerNorm backward), 16 (k_dx_gather), 4 (k_segsum264)
# (t_ll64 and t_T1 run at 256 in TRAIN, the node-count batches too)
TILES = [_egnn(b, b, hidden_nf={'t_ll64': 100, 't_T1': 64}.get(b, 256), update_kp_feat=i % 2 == 0) for i, b in enumerate(gc.TILE)]
TILES += [_egnn(b, b, hidden_nf=256 if i == 1 else 64, update_kp_feat=i % 2 == 1) for i, b in enumerate(gc.NODES)]

# ---- 4. empty and isolated ---------------------------------------------------------------------------------------------------------
EDGE = [_egnn('empty_kk', gc.EMPTY_KK, hidden_nf=100),
        _egnn('isolated_n0', gc.ISOLATED, hidden_nf=100), _egnn('isolated_n5', gc.ISOLATED, hidden_nf=100, message_norm=MN_CONST),
        _egnn('B1', gc.B1),
        _egnn('B300', gc.B300, hidden_nf=100, n_layers=1),           # k_egnn_meta strides 256 threads over B
        _egnn('one_atom', gc.ONE_ATOM, hidden_nf=100)]               # E_ll = 0 in every complex: z of message_norm 0 from kl alone
ISOLATED_CASES = ('isolated_n0', 'isolated_n5')

# ---- 5. symmetry, 6. engine reuse ---------------------------------------------------------------------------------------------------
SYM = _egnn('sym', gc.RAGGED, n_layers=3)
# one model (an engine's graph config is fixed: dense_rad's radius kl graph for all) on a long batch, two short ones, the long one again:
# the short batches leave tiles of the long one's cont rows unwritten
REUSE_CASE, REUSE_BATCHES = f'{gc.DENSE_RAD}_h256', (gc.DENSE_RAD, gc.SMALL, 't_T1', gc.DENSE_RAD)

# ---- 7. trainer: k_egnn_edge_train / k_egnn_edge_bwd, the source-grouped sums, the by-destination pieces, LayerNorm backward --------
TRAIN = [_egnn('tr_dense_n0', gc.DENSE_RAD), _egnn('tr_dense_n5', gc.DENSE_RAD, message_norm=MN_CONST),
         _egnn('tr_lig230', gc.LIG230), _egnn('tr_kp600', gc.KP600),
         _egnn('tr_t_ll64', 't_ll64'), _egnn('tr_t_kl65_kk65', 't_kl65_kk65'), _egnn('tr_t_T1', 't_T1'),
         *[_egnn(f'tr_{b}', b) for b in gc.NODES],
         _egnn('tr_empty_kk', gc.EMPTY_KK), _egnn('tr_isolated', gc.ISOLATED), _egnn('tr_one_atom', gc.ONE_ATOM),
         _egnn('tr_B300', gc.B300, n_layers=1), _egnn('tr_dense_nokp', gc.DENSE_RAD, update_kp_feat=False),
         _egnn('tr_dense_h100', gc.DENSE_RAD, hidden_nf=100, norm=False, use_tanh=False, message_norm=MN_CONST)]   # the padded wide copies
TRAIN_LONG = ('tr_dense_n0', 'tr_dense_n5', 'tr_lig230', 'tr_kp600', 'tr_dense_nokp', 'tr_dense_h100')
INPUT_KEYS = ('lx', 'lh', 'kx', 'kh')


def cutoffs(name):
    return gc.BATCHES[EGNN[name]['batch']]['cutoffs']


def model(name):
    """A fresh CPU module of a case: the seeded weight fill, with the coordinate head (xavier-small in the fill) scaled up so that
    eps_x and the position gradients are not noise (as test_egnn_train_gpu.py does)."""
    from keypoint_diffusion_amd.dynamics import LigRecDynamics
    m = synth.fill_state_dict_(LigRecDynamics(ATOM_NF, REC_NF, graph_cutoffs=cutoffs(name), **EGNN[name]['cfg']), 21)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('.4.weight'):
                p.mul_(20.0)
    return m.eval()


def inputs(name, bname=None):
    """(batch on the CPU, t) of a case (`bname`: another batch for the case's model); a fresh batch object each call (its tensors are
    not shared with the cached complexes)."""
    c = EGNN[name]
    g = gc.den_batch(bname or c['batch'])
    if c['randn_kp']:
        gen = torch.Generator().manual_seed(23)
        g.nodes['kp'].data['h_0'] = torch.randn(g.num_nodes('kp'), REC_NF, generator=gen)
    B = g.batch_size
    return g, (torch.arange(B, dtype=torch.float32) + 1) / (B + 1)


def kp_path(name, gemm_mode='f32'):
    """'table' | 'per_atom' | 'wide': which keypoint path layer 0 takes, from the inputs alone by the engine's stated rule (egnn.hip at
    kp_tab): the class table for one-hot kp_h where B * rec_nf <= n_kp / 2, in fp32 mode, at hidden_nf <= 256."""
    c = EGNN[name]
    if c['cfg']['hidden_nf'] > 256:
        return 'wide'
    g, _ = inputs(name)
    h = g.nodes['kp'].data['h_0']
    one_hot = bool(((h == 0) | (h == 1)).all()) and bool((h.sum(1) == 1).all())
    return 'table' if one_hot and gemm_mode == 'f32' and g.batch_size * REC_NF <= g.num_nodes('kp') // 2 else 'per_atom'


def expected_counts(name):
    """What engine().last_counts() must report after a forward of the case, from the oracle's lists."""
    c = EGNN[name]
    st, (t_all, t_last) = gc.den_stats(c['batch']), gc.launch_tiles(c['batch'])
    upd = c['cfg']['update_kp_feat']
    return dict(E_ll=st['ll']['E'], E_kl=st['kl']['E'], E_lk=st['lk']['E'] if upd else 0, E_kk=st['kk']['E'] if upd else 0,
                tiles=t_all if upd else t_last, tiles_last=t_last, E_last=st['ll']['E'] + st['kl']['E'])


def oracle(sd, name, g, t, dtype=torch.float64, grad=False, edges='batch'):
    """The oracle on batch `g` in `dtype` with the state dict `sd`: dict(eps_h, eps_x) and, with `grad`, the gradients of
    sum(eps_h w_h) + sum(eps_x w_x) (gc.loss_weights) in every parameter (`params`) and input (`inputs`: lx, lh, kx, kh).
    `edges`: 'batch' = gc.den_edges of the case's batch, None = built by the oracle from `g` in `dtype`."""
    c = EGNN[name]
    ocfg = dict(c['cfg'], graph_cutoffs=cutoffs(name))
    ob = util.to_obatch(g)
    for d in (ob.x, ob.h):
        for nt in d:
            d[nt] = d[nt].to(dtype)
    sd = {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in sd.items()}
    ins = {}
    if grad:
        ins = {k: v.clone().requires_grad_(True) for k, v in (('lx', ob.x['lig']), ('lh', ob.h['lig']), ('kx', ob.x['kp']), ('kh', ob.h['kp']))}
        ob.x['lig'], ob.h['lig'], ob.x['kp'], ob.h['kp'] = ins['lx'], ins['lh'], ins['kx'], ins['kh']
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        if edges == 'batch':
            edges = gc.den_edges(c['batch'])
        elif edges is None:
            with torch.no_grad():
                edges = oegnn.lig_edges(ob, ocfg)
        with torch.enable_grad() if grad else torch.no_grad():
            eh, ex = oegnn.egnn_dynamics_forward(sd, ocfg, ob, t.to(dtype), edges={et: edges[et] for et in ('ll', 'kl', 'lk')})
        out = dict(eps_h=eh.detach(), eps_x=ex.detach())
        if grad:
            w_h, w_x = gc.loss_weights(eh.shape[0])
            ((eh * w_h.to(dtype)).sum() + (ex * w_x.to(dtype)).sum()).backward()
            out['params'] = {k: v.grad for k, v in sd.items()}
            out['inputs'] = {k: v.grad for k, v in ins.items()}
    finally:
        torch.set_default_dtype(old)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, grad):
    g, t = inputs(name)
    return oracle(model(name).state_dict(), name, g, t, dtype, grad)


def reference(name, dtype=torch.float64, grad=False):
    """The oracle's result for a case, computed once and shared (not to be written to)."""
    return _reference(name, dtype, grad)


def grad_errors(got_params, got_inputs, ref):
    """name -> max |g - ref| / scale of every parameter and input gradient with a path to the loss: scale is the largest entry of the
    reference tensor; a lone bias (the attention bias: one cancelling sum over all edges) is judged on the scale of its weight's
    gradient, as test_egnn_train_gpu.py does."""
    out = {}
    for n, r in ref['params'].items():
        if r is None or float(r.abs().max()) == 0.0:
            continue
        scale = float(r.abs().max())
        if r.numel() == 1 and n.endswith('.bias'):
            scale = max(scale, float(ref['params'][n[:-4] + 'weight'].abs().max()))
        out[n] = float((got_params[n].double() - r).abs().max()) / scale
    for k, r in ref['inputs'].items():
        out[f'input {k}'] = float((got_inputs[k].double() - r).abs().max()) / max(float(r.abs().max()), 1e-300)
    return out


def moved_batch(g):
    """A copy of the CPU batch `g` with every complex rotated and translated by gc.rigid_motions (float64 arithmetic on the fp32
    positions, stored as fp32 again); the kk index list is kept: it is the caller's."""
    g2 = g.to('cpu')
    lp, kp = g.node_ptr('lig').tolist(), g.node_ptr('kp').tolist()
    lx, kx = g.nodes['lig'].data['x_0'].double().clone(), g.nodes['kp'].data['x_0'].double().clone()
    for b, (R, tr) in enumerate(gc.rigid_motions(g.batch_size)):
        lx[lp[b]:lp[b + 1]] = lx[lp[b]:lp[b + 1]] @ R.T + tr
        kx[kp[b]:kp[b + 1]] = kx[kp[b]:kp[b + 1]] @ R.T + tr
    g2.nodes['lig'].data['x_0'], g2.nodes['kp'].data['x_0'] = lx.float(), kx.float()
    return g2


def rotated_rows(x, g):
    """The ligand rows `x` [n_lig, 3] of batch `g` turned by the rotation of their complex (float64)."""
    lp, out = g.node_ptr('lig').tolist(), x.double().clone()
    for b, (R, _) in enumerate(gc.rigid_motions(g.batch_size)):
        out[lp[b]:lp[b + 1]] = out[lp[b]:lp[b + 1]] @ R.T
    return out
