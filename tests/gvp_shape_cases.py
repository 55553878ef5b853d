"""Case tables of test_gvp_shapes_gpu.py and test_recenc_shapes_gpu.py: the GVP denoiser (csrc/gvp_chain.hip, gvp_coop.hip, gvp.hip,
gvp_train.hip) and the GVP receptor encoder (csrc/rec_encoder.hip, recenc_train.hip) away from the shipped shapes, with the functions
that state, from the oracle alone, the property each case exists for: how many 64-edge tiles (TM) a destination's run of in-edges
spans, E mod 64, the tile count of a launch, neighbour caps, rows without in-edge, and a relative gap of at least GAP = 1e-3 between
any two distances that decide an edge list.  test_gvp_shape_cases.py checks all of it without a GPU; the GPU modules assert it again
before they compare, so a changed generator fails loudly instead of quietly testing something else.

The reference everywhere is oracle/gvp.py / oracle/rec_encoder.py run in float64 (weights, positions, features, v_0, t and the
oracle's own constants), so it is a high-precision one and not a second fp32 rounding of the same sums; gradients are torch autograd
through it.  References are computed once (lru_cache) and never written to afterwards.

The denoiser batches (the edge lists of oracle.egnn.lig_edges, the same for both denoisers) also serve egnn_shape_cases.py."""
import functools
import math

import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import synth
from oracle import egnn as oegnn
from oracle import gvp as ogvp
from oracle import rec_encoder as orec

from . import util
from .golden.make_golden_cfgs import GVP_CFGS, RECENC_CFGS

CUT = util.CUTOFFS_ALL_ATOM
TM = 64             # edges per tile of k_gvp_chain (gvp_kernels.h)
GAP = 1e-3          # ten times the value tolerance
LL_MAX_NN, KL_MAX_NN, RR_MAX_NN, KL_KMAX, KPE_MAX, GVP_MAX_CHAIN = 200, 100, 100, 16, 10240, 4
ETYPES = ('ll', 'kl', 'lk', 'kk')
DST_NT = {'ll': 'lig', 'kl': 'lig', 'lk': 'kp', 'kk': 'kp'}


def rotation(angle=0.7, axis=(1.0, 2.0, 3.0)):
    """A proper rotation (Rodrigues), float64."""
    ax = torch.tensor(axis, dtype=torch.float64)
    ax = ax / ax.norm()
    Kx = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


def rigid_motions(B):
    """One proper rotation and one translation of at most 20 A per complex."""
    gen = torch.Generator().manual_seed(17)
    out = []
    for b in range(B):
        R = rotation(0.7 + 0.9 * b, (1.0 + b, 2.0, 3.0 - b))
        t = torch.randn(3, generator=gen, dtype=torch.float64)
        t = t / t.norm() * (20.0 - 4.0 * b)
        assert abs(float(torch.linalg.det(R)) - 1.0) < 1e-12 and float(t.norm()) <= 20.0 + 1e-9
        out.append((R, t))
    return out


# ======================================================================================================================== denoiser
# ---- batches: what the edge lists depend on (sizes, seed, cutoffs, ll_k / kl_k); a case adds a model config ------------------------
BATCHES = {}


def _batch(name, n_rec=None, n_lig=None, seed=1234, cutoffs=CUT, kl_k=5, ll_k=0, move=None, hand=None):
    """`hand`: (n_kp, n_lig, kk in-degree) per complex of a batch built by hand (below) instead of synth + the fixed encoder;
    `move`: index of one ligand atom moved 60 A away."""
    BATCHES[name] = dict(n_rec=n_rec, n_lig=n_lig, seed=seed, cutoffs=cutoffs, kl_k=kl_k, ll_k=ll_k, move=move, hand=hand)
    return name


def _hand_complex(n_kp, n_lig, deg, seed):
    """As test_gvp_40kp_shape builds its complexes: keypoints without receptor, a kk graph given as data.  Keypoint i receives
    kk edges from i + 1 .. i + deg (mod n_kp): E_kk = n_kp * deg exactly."""
    gen = torch.Generator().manual_seed(seed)
    kp_pos = torch.randn(n_kp, 3, generator=gen) * 2.5
    dst = torch.arange(n_kp).repeat_interleave(deg)
    src = (dst + torch.arange(1, deg + 1).repeat(n_kp)) % n_kp
    g = G.heterograph({('kp', 'kk', 'kp'): (src, dst)}, {'rec': 0, 'kp': n_kp, 'lig': n_lig})
    g.nodes['kp'].data['x_0'] = kp_pos
    g.nodes['kp'].data['h_0'] = torch.randn(n_kp, 10, generator=gen)
    lx = torch.randn(n_lig, 3, generator=gen)
    g.nodes['lig'].data['x_0'] = lx - lx.mean(0, keepdim=True)
    g.nodes['lig'].data['h_0'] = torch.randn(n_lig, 10, generator=gen)
    g.nodes['rec'].data['x_0'] = torch.zeros(0, 3)
    g.nodes['rec'].data['h_0'] = torch.zeros(0, 10)
    return g


@functools.lru_cache(maxsize=None)
def den_complexes(bname, nv=16):
    """The complexes of a batch, one graph each, with v_0 of `nv` channels on the keypoints (a tuple: not to be written to)."""
    b = BATCHES[bname]
    if b['hand'] is not None:
        gs = [_hand_complex(nk, nl, deg, b['seed'] + i) for i, (nk, nl, deg) in enumerate(b['hand'])]
    else:
        gs = synth.synth_complexes(b['n_rec'], b['n_lig'], 20, b['cutoffs'], seed=b['seed'])
        if b['move'] is not None:
            gs[0].nodes['lig'].data['x_0'][b['move']] += torch.tensor([60.0, 0.0, 0.0])
        gs = [util.fixed_encode(g, n_vec=nv) for g in gs]
    for i, g in enumerate(gs):
        gen = torch.Generator().manual_seed(3 + i)
        g.nodes['kp'].data['v_0'] = 0.5 * torch.randn(g.num_nodes('kp'), nv, 3, generator=gen)
    return tuple(gs)


def den_batch(bname, nv=16):
    return G.batch(list(den_complexes(bname, nv)))


def graph_cfg(bname):
    b = BATCHES[bname]
    return dict(graph_cutoffs=b['cutoffs'], ll_k=b['ll_k'], kl_k=b['kl_k'])


@functools.lru_cache(maxsize=None)
def den_edges(bname):
    """The float64 oracle's edge lists of a batch: et -> (src, dst)."""
    ob = util.to_obatch64(den_batch(bname))
    with torch.no_grad(), util.float64_oracle():
        e = oegnn.lig_edges(ob, graph_cfg(bname))
    e['kk'] = ob.edges['kk']
    return e


@functools.lru_cache(maxsize=None)
def den_stats(bname):
    """et -> dict(E, tiles, deg [n_dst], spans [n_dst]) of the oracle's edge lists, stored destination-major in tiles of TM."""
    g, out = den_batch(bname), {}
    for et, (s, d) in den_edges(bname).items():
        n = g.num_nodes(DST_NT[et])
        out[et] = dict(E=int(d.numel()), tiles=-(-int(d.numel()) // TM), deg=torch.bincount(d, minlength=n), spans=util.tile_spans(d, n, TM))
    return out


def launch_tiles(bname):
    """(tiles of a conv over all four edge types, tiles of a conv over ll + kl): what engine().last_counts() reports."""
    st = den_stats(bname)
    return sum(st[et]['tiles'] for et in ETYPES), st['ll']['tiles'] + st['kl']['tiles']


def den_gap(bname):
    """Smallest relative gap of the distances that decide the oracle's ll and kl / lk lists.  The kk list of the denoiser is the
    caller's: the same index lists go to the oracle and to the engine, so no distance decides it on either side."""
    b, g = BATCHES[bname], den_batch(bname)
    lx, kx = g.nodes['lig'].data['x_0'], g.nodes['kp'].data['x_0']
    nl, nk = g.batch_num_nodes('lig'), g.batch_num_nodes('kp')
    cut = b['cutoffs']
    return min(util.knn_rel_gap(lx, lx, b['ll_k'] + 1, nl, nl) if b['ll_k'] else util.radius_rel_gap(lx, lx, cut['ll'], nl, nl),
               util.knn_rel_gap(lx, kx, b['kl_k'], nl, nk) if b['kl_k'] else util.radius_rel_gap(lx, kx, cut['kl'], nl, nk))


def _n_span(st, et, k):
    return int((st[et]['spans'] >= k).sum())


# ---- 1. long destination runs: the loop `for t = lo / TM + 1 .. (hi - 1) / TM` of the node kernels over ms_cont / mv_cont ----------
# the small complex behind the large one: a long run is followed by short ones in the same tile
DENSE_RAD = _batch('dense_rad', [150, 9], [140, 3], cutoffs=dict(CUT, rr=30.0, kl=30.0), kl_k=0)
# (where every atom sits at the cap all runs start at multiples of 8 and none spans a fifth tile, as with seed 1234: this seed has an
# outlying atom with fewer neighbours in front of capped ones)
LIG230 = _batch('lig230', [20, 9], [230, 3], seed=1299)
KP600 = _batch('kp600_lig3', [600, 12], [3, 5], kl_k=16, seed=1612)
DENSE_RAD_TABLE = {'ll': (19452, 139, 4, 140), 'kl': (15027, 150, 4, 100), 'lk': (15027, 100, 3, 75), 'kk': (15072, 100, 3, 75)}


def prop_dense_rad(st):
    """Every edge type has at least 50 destinations whose run spans at least 3 tiles (E, max in-degree, longest run in tiles and
    destinations over >= 3 tiles as measured with seed 1234)."""
    for et in ETYPES:
        got = (st[et]['E'], int(st[et]['deg'].max()), int(st[et]['spans'].max()), _n_span(st, et, 3))
        assert got == DENSE_RAD_TABLE[et], (et, got)
        assert got[3] >= 50
    assert int(st['ll']['deg'][-3:].max()) == 2 and int(st['kk']['deg'][-9:].max()) == 8          # short runs behind the long ones


def prop_lig230(st):
    """The 200-neighbour ll cap is reached (229 candidates inside 6 A for most atoms) and some run spans 5 tiles."""
    deg = st['ll']['deg']
    assert int(deg.max()) == LL_MAX_NN and int((deg[:230] == LL_MAX_NN).sum()) >= 100
    assert int(st['ll']['spans'].max()) == 5 and _n_span(st, 'll', 4) >= 100


def prop_kp600(st):
    """Three ligand rows of kl in-degree 600 (at least 10 tiles each) beside keypoints of lk in-degree 3 or less."""
    assert st['kl']['deg'][:3].tolist() == [600, 600, 600] and int(st['kl']['spans'][:3].min()) >= 10
    assert int(st['lk']['deg'][:600].max()) == 3 and int(st['lk']['deg'][600:].max()) == 5


# ---- 2. tile edges: E_et mod 64 in {0} and {1, 2} per edge type; launches of T = 1 .. 9 tiles (chunk_tiles = (T + 7) >> 3 leaves
# workgroups of the XCD map without a tile below 8).  Built by hand: (n_kp, n_lig, kk in-degree) per complex; complete ll graphs
# of n (n - 1) edges, kl / lk of n_kp * min(kl_k, n_lig) edges, kk of n_kp * deg edges
TILE = {
    _batch('t_ll64', hand=((3, 8, 2), (3, 3, 2), (3, 2, 2)), kl_k=2, seed=500): dict(E=(64, 18, 18, 18), T=(4, 2)),
    _batch('t_ll66', hand=((3, 8, 2), (3, 3, 2), (3, 2, 2), (3, 2, 2)), kl_k=2, seed=510): dict(E=(66, 24, 24, 24), T=(5, 3)),
    _batch('t_kl64_kk64', hand=((16, 5, 4),), kl_k=4, seed=520): dict(E=(20, 64, 64, 64), T=(4, 2)),
    _batch('t_kl65_kk65', hand=((13, 6, 5),), kl_k=5, seed=531): dict(E=(30, 65, 65, 65), T=(7, 3)),
    _batch('t_T1', hand=((5, 1, 2),), kl_k=5, seed=540): dict(E=(0, 5, 5, 10), T=(3, 1)),
    _batch('t_T6', hand=((9, 8, 8), (3, 3, 2), (3, 2, 2), (3, 2, 2)), kl_k=2, seed=550): dict(E=(66, 36, 36, 90), T=(6, 3)),
    _batch('t_T8', hand=((20, 11, 4),), kl_k=4, seed=564): dict(E=(110, 80, 80, 80), T=(8, 4)),
    _batch('t_T9', hand=((20, 12, 4),), kl_k=4, seed=570): dict(E=(132, 80, 80, 80), T=(9, 5)),
}


def prop_tile(bname, st):
    want = TILE[bname]
    assert tuple(st[et]['E'] for et in ETYPES) == want['E'], [st[et]['E'] for et in ETYPES]
    assert launch_tiles(bname) == want['T']


def tile_coverage():
    """What the tile-edge cases cover together: per edge type the remainders E mod 64 that occur, and the tile counts of all launches."""
    rem = {et: {TILE[b]['E'][i] % TM for b in TILE if TILE[b]['E'][i]} for i, et in enumerate(ETYPES)}
    return rem, {t for b in TILE for t in TILE[b]['T']}


# ---- 3. empty and isolated ----------------------------------------------------------------------------------------------------------
EMPTY_KK = _batch('empty_kk', [26, 19], [7, 10], cutoffs=dict(CUT, rr=0.05), seed=31)
ISOLATED, ISOLATED_ROW = _batch('isolated', [26, 19], [9, 7], seed=49, move=4), 4
B1 = _batch('B1', [26], [7], seed=31)
B300 = _batch('B300', [6] * 300, [2] * 300, seed=2265)
SMALL = _batch('small', [26, 19], [7, 10], seed=31)                 # chain lengths and narrow models: the shapes of test_gvp_small_configs
RAGGED = _batch('ragged', [40, 9, 25], [9, 3, 12], seed=51)         # symmetry


def prop_empty_kk(st):
    assert st['kk']['E'] == 0 and st['ll']['E'] > 0 and st['kl']['E'] == st['lk']['E'] == 45 * 5


def prop_isolated(st):
    """Row ISOLATED_ROW of the ligand has no in-edge of any type (and no out-edge); every other ligand atom has some."""
    e = den_edges(ISOLATED)
    for et in ('ll', 'kl'):
        assert int(st[et]['deg'][ISOLATED_ROW]) == 0
    assert int((e['ll'][0] == ISOLATED_ROW).sum()) == 0 and int((e['lk'][0] == ISOLATED_ROW).sum()) == 0
    both = st['ll']['deg'] + st['kl']['deg']
    assert int((both == 0).sum()) == 1


def prop_b1(st):
    assert den_batch(B1).batch_size == 1


def prop_b300(st):
    assert den_batch(B300).batch_size == 300 > 256 and st['ll']['E'] == 600 and st['kl']['E'] == 300 * 6 * 2


# ---- 4. node counts on and one past the row blocks of the EGNN denoiser's node-side kernels (egnn_shape_cases.py): 32 rows of the node
# update, 64 of the projection launch, 8 / 16 / 4 of the trainer's LayerNorm backward, k_dx_gather and k_segsum264.  (n_kp, n_lig)
NODES = {
    _batch('n_kp64_lig32', hand=((64, 32, 3),), seed=622): (64, 32),
    _batch('n_kp65_lig33', hand=((65, 33, 3),), seed=1229): (65, 33),
    _batch('n_kp32_lig64', hand=((32, 64, 3),), seed=639): (32, 64),
    _batch('n_kp33_lig65', hand=((33, 65, 3),), seed=630): (33, 65),
}
# one-atom ligands only: no ll edge in any complex while every keypoint keeps its one kl edge
ONE_ATOM = _batch('one_atom_ligs', [26, 19, 30], [1, 1, 1], seed=31)


def prop_nodes(bname, st):
    g = den_batch(bname)
    assert (g.num_nodes('kp'), g.num_nodes('lig')) == NODES[bname] and g.batch_size == 1
    assert st['kk']['E'] == 3 * NODES[bname][0] and st['kl']['E'] == st['lk']['E'] == 5 * NODES[bname][0] and st['ll']['E'] > 0


def node_coverage():
    """The total keypoint and ligand node counts of the node-count batches."""
    return {nk for nk, _ in NODES.values()}, {nl for _, nl in NODES.values()}


def prop_one_atom(st):
    g = den_batch(ONE_ATOM)
    assert g.batch_num_nodes('lig').tolist() == [1, 1, 1] and st['ll']['E'] == 0
    assert st['kl']['E'] == st['lk']['E'] == g.num_nodes('kp') == 75 and st['kl']['deg'].tolist() == [26, 19, 30]


PROPS = {DENSE_RAD: prop_dense_rad, LIG230: prop_lig230, KP600: prop_kp600, EMPTY_KK: prop_empty_kk, ISOLATED: prop_isolated,
         B1: prop_b1, B300: prop_b300, ONE_ATOM: prop_one_atom, **{b: functools.partial(prop_tile, b) for b in TILE},
         **{b: functools.partial(prop_nodes, b) for b in NODES}}


@functools.lru_cache(maxsize=None)
def check_batch(bname):
    """The gap of at least GAP and the stated property of a batch, from the oracle alone; returns the gap."""
    gap = den_gap(bname)
    assert gap >= GAP, f'{bname}: the oracle has a near-tie (relative gap {gap:.2e}): pick another seed'
    if bname in PROPS:
        PROPS[bname](den_stats(bname))
    return gap


# ---- the cases: a batch and a model config ------------------------------------------------------------------------------------------
BASE = dict(GVP_CFGS['gvp_norm0'])          # 2 convs, 128 hidden scalars, message_norm 0, update_kp, chains (2, 1, 3), 16 vector channels
DEN = {}


def _den(name, bname, **over):
    DEN[name] = dict(batch=bname, cfg=dict(BASE, **over, ll_k=BATCHES[bname]['ll_k'], kl_k=BATCHES[bname]['kl_k']))
    return name


def _norm_tag(mn):
    return {'mean': 'mean', 0: 'n0', 10.0: 'n10'}[mn]


# the segmented sum carries the 48 vector columns on the last wave's spare lanes at S < 256 and on threads 0 .. 47 at S = 256
LONG = [_den(f'{b}_S{S}_{_norm_tag(mn)}', b, n_hidden_scalars=S, message_norm=mn)
        for b in (DENSE_RAD, LIG230, KP600) for S in (128, 256) for mn in ('mean', 0, 10.0)]
# vector_size 5 (zero-padded channels in the same sums) once per batch and width: the grid is cut here, not the shapes
LONG += [_den(f'{DENSE_RAD}_S256_mean_V5', DENSE_RAD, n_hidden_scalars=256, message_norm='mean', vector_size=5),
         _den(f'{LIG230}_S128_n0_V5', LIG230, n_hidden_scalars=128, message_norm=0, vector_size=5),
         _den(f'{KP600}_S128_n10_V5', KP600, n_hidden_scalars=128, message_norm=10.0, vector_size=5)]
TILES = [_den(b, b, n_hidden_scalars=256 if i % 2 else 128) for i, b in enumerate(TILE)]
EDGE = [_den('empty_kk', EMPTY_KK)] + [_den(f'isolated_{_norm_tag(mn)}', ISOLATED, message_norm=mn) for mn in ('mean', 0, 10.0)] + \
       [_den('B1', B1), _den('B300', B300, n_convs=1)]
CHAINS = [_den(f'chain{m}{u}{n}_S{S}', SMALL, n_message_gvps=m, n_update_gvps=u, n_noise_gvps=n, n_hidden_scalars=S)
          for (m, u, n) in ((1, 1, 1), (4, 4, 4), (1, 4, 2), (4, 1, 1)) for S in (128, 256)]
NARROW = [_den('S1', SMALL, n_hidden_scalars=1), _den('S2_V1', SMALL, n_hidden_scalars=2, vector_size=1),
          _den('conv1_no_kp', SMALL, n_convs=1, update_kp=False)]
SYM = _den('sym', RAGGED, n_convs=3)
# trainer: hidden width 256 takes the register-chained message kernels (k_gvp_chain<., 0, 1>, k_gvp_chain_bwd, k_gvp_node_chain_bwd)
TRAIN = [_den('tr_dense_mean', DENSE_RAD, n_hidden_scalars=256, message_norm='mean'), _den('tr_dense_n0', DENSE_RAD, n_hidden_scalars=256),
         _den('tr_lig230', LIG230, n_hidden_scalars=256), _den('tr_chain111', SMALL, n_message_gvps=1, n_update_gvps=1, n_noise_gvps=1, n_hidden_scalars=256),
         _den('tr_chain444', SMALL, n_message_gvps=4, n_update_gvps=4, n_noise_gvps=4, n_hidden_scalars=256),
         _den('tr_isolated', ISOLATED, n_hidden_scalars=256, message_norm='mean')]
# (config override, the value the message must name): refused by kpd_gvp_create's host-side checks
REFUSALS = [(dict(n_noise_gvps=5), r'1\.\.4'), (dict(n_message_gvps=5), r'1\.\.4'), (dict(vector_size=17), 'vector_size=17'),
            (dict(ll_k=17), 'll_k=17'), (dict(n_lig_scalars=256), 'n_lig_scalars=256')]


def den_model(name):
    """A fresh CPU module of a case with the seeded weight fill."""
    from keypoint_diffusion_amd.dynamics_gvp import LigRecDynamicsGVP
    c = DEN[name]
    model = LigRecDynamicsGVP(10, 10, graph_cutoffs=BATCHES[c['batch']]['cutoffs'], **c['cfg'])
    return synth.fill_state_dict_(model, 7).eval()


def den_inputs(name):
    """(batch on the CPU, t) of a case."""
    c = DEN[name]
    g = den_batch(c['batch'], c['cfg'].get('vector_size', 16))
    B = g.batch_size
    return g, (torch.arange(B, dtype=torch.float32) + 1) / (B + 1)


def loss_weights(n_lig):
    gen = torch.Generator().manual_seed(2)
    f32 = dict(generator=gen, dtype=torch.float32)          # (the same draws whatever the default dtype is when this is called)
    return torch.randn(n_lig, 10, **f32), torch.randn(n_lig, 3, **f32)


def den_oracle(sd, name, g, t, dtype=torch.float64, grad=False):
    """The oracle on batch `g` in `dtype` with the state dict `sd`: dict(eps_h, eps_x) and, with `grad`, the gradients of
    sum(eps_h w_h) + sum(eps_x w_x) (loss_weights) in every parameter (`params`) and input (`inputs`: lh, kh, kv, lx, kx)."""
    c = DEN[name]
    ocfg = dict(c['cfg'], graph_cutoffs=BATCHES[c['batch']]['cutoffs'])
    ob = util.to_obatch(g)
    for d in (ob.x, ob.h, ob.v):
        for nt in d:
            d[nt] = d[nt].to(dtype)
    sd = {k: v.detach().to(dtype).clone().requires_grad_(grad and v.numel() > 0) for k, v in sd.items()}
    ins = {}
    if grad:
        ins = {'lh': ob.h['lig'], 'kh': ob.h['kp'], 'kv': ob.v['kp'], 'lx': ob.x['lig'], 'kx': ob.x['kp']}
        ins = {k: v.clone().requires_grad_(True) for k, v in ins.items()}
        ob.h['lig'], ob.h['kp'], ob.v['kp'], ob.x['lig'], ob.x['kp'] = ins['lh'], ins['kh'], ins['kv'], ins['lx'], ins['kx']
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            edges = oegnn.lig_edges(ob, ocfg)
        with torch.enable_grad() if grad else torch.no_grad():
            eh, ex = ogvp.gvp_dynamics_forward(sd, ocfg, ob, t.to(dtype), edges=edges)
        out = dict(eps_h=eh.detach(), eps_x=ex.detach())
        if grad:
            w_h, w_x = loss_weights(eh.shape[0])
            ((eh * w_h.to(dtype)).sum() + (ex * w_x.to(dtype)).sum()).backward()
            out['params'] = {k: v.grad for k, v in sd.items()}
            out['inputs'] = {k: v.grad for k, v in ins.items()}
    finally:
        torch.set_default_dtype(old)
    return out


@functools.lru_cache(maxsize=None)
def _den_reference(name, dtype, grad):
    g, t = den_inputs(name)
    return den_oracle(den_model(name).state_dict(), name, g, t, dtype, grad)


def den_reference(name, dtype=torch.float64, grad=False):
    """The oracle's result for a case, computed once and shared (not to be written to)."""
    return _den_reference(name, dtype, grad)


# ========================================================================================================================= encoder
REC = {}
REC_BASE = dict(RECENC_CFGS['recenc_norm10'])   # in 10, out 128, chains (1, 1), 16 channels, 3 rr + 2 rk convs, norm 10, k_closest 4, K = 5


def _rec(name, n_rec=(33, 21), seed=17, cutoffs=CUT, isolate=None, **over):
    REC[name] = dict(kw=dict(REC_BASE, **over, graph_cutoffs=cutoffs), n_rec=list(n_rec), seed=seed, isolate=isolate)
    return name


REC_SHAPES = [
    _rec('K1', n_keypoints=1),                                                   # no kk edges
    _rec('K40_out256', n_keypoints=40, out_scalar_size=256, seed=27),            # n_keypoints * out_scalar_size = KPE_MAX exactly
    _rec('k1', k_closest=1),
    _rec('k16_n16', n_rec=(16, 40), k_closest=16, seed=23),                      # a pocket of exactly KL_KMAX atoms: every atom is a neighbour
    _rec('rr0', n_rr_convs=0),
    _rec('out1', out_scalar_size=1),                                             # LayerNorm over one entry
    _rec('out127', out_scalar_size=127), _rec('out129', out_scalar_size=129, seed=18),    # either side of the 128 / 256 kernel switch
    _rec('in1', in_scalar_size=1),
    _rec('in256_out255', in_scalar_size=256, out_scalar_size=255),
    _rec('n256_n257', n_rec=(256, 257)), _rec('n513_n6', n_rec=(513, 6)),        # the attention strides a pocket 256 atoms at a time
    _rec('mod4_is2', n_rec=(33, 21)), _rec('mod4_is3', n_rec=(33, 22)),          # k_rec_embed / k_linear_rows: 4 rows per block
    _rec('isolated', isolate=11),                                                # an atom without rr in-edge
    _rec('dense_rr_mean', n_rec=(150, 9), cutoffs=dict(CUT, rr=30.0), message_norm='mean'),
    _rec('dense_rr_n0', n_rec=(150, 9), cutoffs=dict(CUT, rr=30.0), message_norm=0),
    _rec('dense_rr_n10', n_rec=(150, 9), cutoffs=dict(CUT, rr=30.0), message_norm=10.0),
    _rec('kp_rad', n_rec=(60, 8), k_closest=0, kp_rad=1.3),                      # keypoints without any rk edge
    _rec('B1', n_rec=(33,)),
    _rec('B300', n_rec=(6,) * 300, n_keypoints=2, k_closest=1, n_rr_convs=1, message_norm=0, seed=2000),
    _rec('chains44', n_message_gvps=4, n_update_gvps=4),
    _rec('V1', vector_size=1, seed=18), _rec('V15', vector_size=15),
]
REC_SYM = _rec('sym', n_rec=(40, 9, 25))
REC_TRAIN = ['dense_rr_n0', 'K40_out256', 'k16_n16', 'out129', 'isolated', 'chains44']
REC_KEYS = ('kp_x', 'kp_h', 'kp_v')


@functools.lru_cache(maxsize=None)
def rec_complexes(name):
    c = REC[name]
    kw, n_rec = c['kw'], c['n_rec']
    gs = synth.synth_complexes(n_rec, [1] * len(n_rec), kw['n_keypoints'], kw['graph_cutoffs'], seed=c['seed'], n_rec_feat=kw['in_scalar_size'])
    if c['isolate'] is not None:                   # one atom of pocket 0 moved 40 A away BEFORE the rr graph is built
        pos, feat = synth.synth_pocket(n_rec[0], c['seed'], kw['in_scalar_size'])
        pos[c['isolate']] += torch.tensor([40.0, 0.0, 0.0])
        gs[0] = synth.build_complex_graph(pos, feat, kw['n_keypoints'], kw['graph_cutoffs'], n_lig=1)
    return tuple(gs)


def rec_batch(name):
    return G.batch(list(rec_complexes(name)))


def rec_model(name):
    from keypoint_diffusion_amd.receptor_encoder_gvp import ReceptorEncoderGVP
    return synth.fill_state_dict_(ReceptorEncoderGVP(**REC[name]['kw']), 61).eval()


def rec_loss_weights(n_kp, S, V):
    gen = torch.Generator().manual_seed(5)
    f32 = dict(generator=gen, dtype=torch.float32)          # (the same draws whatever the default dtype is when this is called)
    return torch.randn(n_kp, 3, **f32), torch.randn(n_kp, S, **f32) / S ** 0.5, torch.randn(n_kp, V, 3, **f32) / 4


def rec_oracle(sd, name, g, dtype=torch.float64, grad=False):
    """The oracle on batch `g` in `dtype`: dict(kp_x, kp_h, kp_v, rk, kk) and, with `grad`, `params`: the gradients of
    sum(x w_x) + sum(h w_h) + sum(v w_v) (rec_loss_weights)."""
    kw = REC[name]['kw']
    ob = util.to_obatch(g)
    ob.x['rec'], ob.h['rec'] = ob.x['rec'].to(dtype), ob.h['rec'].to(dtype)
    sd = {k: v.detach().to(dtype).clone().requires_grad_(grad and v.numel() > 0) for k, v in sd.items()}
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.enable_grad() if grad else torch.no_grad():
            ref = orec.rec_encoder_gvp_forward(sd, kw, ob)
        out = dict(kp_x=ref.x['kp'].detach(), kp_h=ref.h['kp'].detach(), kp_v=ref.v['kp'].detach(), rk=ref.edges['rk'], kk=ref.edges['kk'])
        if grad:
            w = rec_loss_weights(ref.x['kp'].shape[0], kw['out_scalar_size'], kw['vector_size'])
            sum((a * b.to(dtype)).sum() for a, b in zip((ref.x['kp'], ref.h['kp'], ref.v['kp']), w)).backward()
            out['params'] = {k: v.grad for k, v in sd.items()}
    finally:
        torch.set_default_dtype(old)
    return out


@functools.lru_cache(maxsize=None)
def _rec_reference(name, dtype, grad):
    return rec_oracle(rec_model(name).state_dict(), name, rec_batch(name), dtype, grad)


def rec_reference(name, dtype=torch.float64, grad=False):
    """The oracle's result for a case, computed once and shared (not to be written to)."""
    return _rec_reference(name, dtype, grad)


def rec_gap(name, ref=None):
    """Smallest relative gap of the distances that decide the oracle's rk list (kNN or radius around its keypoints) and kk list."""
    kw, g = REC[name]['kw'], rec_batch(name)
    ref = ref or rec_reference(name)
    x0, kp, n_rec = g.nodes['rec'].data['x_0'], ref['kp_x'], g.batch_num_nodes('rec')
    n_kp = torch.full_like(n_rec, kw['n_keypoints'])
    rk = (util.knn_rel_gap(x0, kp, kw['k_closest'], n_rec, n_kp) if kw['k_closest'] else util.radius_rel_gap(x0, kp, kw['kp_rad'], n_rec, n_kp))
    return min(rk, util.radius_rel_gap(kp, kp, kw['graph_cutoffs']['kk'], n_kp, n_kp))


def rec_property(name, ref=None):
    """The property the case is named for, from the config and the oracle's lists alone."""
    c, g = REC[name], rec_batch(name)
    kw, n_rec = c['kw'], c['n_rec']
    ref = ref or rec_reference(name)
    K, S, B, N = kw['n_keypoints'], kw['out_scalar_size'], len(n_rec), sum(n_rec)
    rs, rd = g.edges(etype='rr')
    rr_deg, rk_deg = torch.bincount(rd, minlength=N), torch.bincount(ref['rk'][1], minlength=B * K)
    if name == 'K1':
        assert K == 1 and ref['kk'][0].numel() == 0
    if name == 'K40_out256':
        assert K * S == KPE_MAX and (K + 1) * S > KPE_MAX
    if name == 'k16_n16':
        assert kw['k_closest'] == KL_KMAX == n_rec[0] and sorted(ref['rk'][0][:16].tolist()) == list(range(16))
    if name in ('mod4_is2', 'mod4_is3'):
        assert N % 4 == int(name[-1])
    if name == 'n256_n257':
        assert n_rec == [256, 257]
    if name == 'n513_n6':
        assert n_rec[0] == 2 * 256 + 1
    if name == 'isolated':
        assert int(rr_deg[c['isolate']]) == 0 and int((rs == c['isolate']).sum()) == 0 and int((rr_deg == 0).sum()) == 1
    if name.startswith('dense_rr'):                # the 100-neighbour cap of the rr graph is reached and runs span 3 tiles
        spans = util.tile_spans(rd, N, TM)
        assert int(rr_deg.max()) == RR_MAX_NN and int((rr_deg[:150] == RR_MAX_NN).sum()) == 150 and int((spans >= 3).sum()) >= 50
        assert int(rr_deg[150:].max()) == 8
    if name == 'kp_rad':                           # the degree assertions of test_receptor_encoder
        assert int(rk_deg.max()) <= 10 and int(rk_deg.min()) == 0 and int(rk_deg.max()) > 0
    if name == 'B1':
        assert B == 1
    if name == 'B300':
        assert B == 300 > 256
    if kw['k_closest']:
        assert ref['rk'][0].numel() == sum(K * min(kw['k_closest'], n) for n in n_rec)


def check_rec(name, ref=None):
    gap = rec_gap(name, ref)
    assert gap >= GAP, f'{name}: the oracle has a near-tie (relative gap {gap:.2e}): pick another seed'
    rec_property(name, ref)
    return gap
