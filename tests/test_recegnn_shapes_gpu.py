"""The EGNN keypoint receptor encoder (kpd_recegnn_* and kpd_recegnn_trainer_*, through models/receptor_encoder.py's ReceptorEncoder)
away from the shipped shapes: every feature width on its own anywhere in 1..256, the shape edges of its kernels, its invariances, and
the trainer against the engine.  The reference everywhere is oracle/rec_encoder_egnn.py run in float64 (weights, positions, features
and same_res), so it is a high-precision one and not a second fp32 rounding of the same sums; gradients are torch autograd through it.

Exact comparison of the rk edge lists needs the float64 oracle to have no near-tie: every case asserts, from the oracle alone, that
the smallest relative gap between consecutive distances among a keypoint's k + 1 nearest atoms (kNN), or between any distance and
kp_rad / the kk cutoff (radius), exceeds GAP = 1e-3, ten times the value tolerance.  The batch seeds below were chosen on the CPU for
that; a change of the generator fails the gap assertion loudly instead of flipping an edge."""
import copy
import functools
import math

import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import synth
from keypoint_diffusion_amd.receptor_encoder import ReceptorEncoder
from oracle import rec_encoder_egnn as orec

from . import util
from .golden.make_golden_cfgs import RECEGNN_CFGS, same_res_feature

pytestmark = pytest.mark.gpu
CUT = util.CUTOFFS_ALL_ATOM
TOL = 1e-4
GRAD_TOL = 2e-4     # test_recegnn_train_gpu.py: relative to the largest entry of each gradient tensor
GAP = 1e-3
KEYS = ('kp_x', 'kp_h', 'rec_h', 'rec_x')
EDGES = ('rk_src', 'rk_dst', 'kk_src', 'kk_dst')
CASES = {}
# Where fp32 itself cannot hold a bound, the bound is four times what the float32 oracle shows against the float64 oracle on the CPU:
# all256, kp x_0: three 256-long fp32 sums in a row leave entries near zero 0.293 of the elementwise bound away in the float32 oracle
MAX_EXCESS = {('all256', 'kp_x'): 4 * 0.293}
# w1, coordinate branch: every atom carries the same single feature, so SiLU(coord_mlp.0) is the same on an edge and its reverse while
# x_diff changes sign: the gradients of the three coordinate tensors are what is left of a sum that cancels.  float32 autograd through
# the oracle is off by 1.51e-3 (coord_mlp.0.weight), 4.39e-4 (coord_mlp.0.bias), 2.50e-3 (coord_mlp.2.weight) of the largest entry
GRAD_TOL_OF = {'w1': {'rec_convs.0.coord_mlp.0.weight': 4 * 1.51e-3, 'rec_convs.0.coord_mlp.0.bias': 4 * 4.39e-4,
                      'rec_convs.0.coord_mlp.2.weight': 4 * 2.50e-3}}


def _case(name, base, widths, n_rec=(33, 21, 7), seed=19, K=5, isolate=None, **over):
    """`base` of RECEGNN_CFGS ('recegnn_small': no LayerNorm, no same_res, no tanh, message_norm 5; 'recegnn_20kp': all of them,
    message_norm 0) at widths (in, hid, out, n_convs) with K keypoints, on pockets `n_rec` drawn with `seed`."""
    i, h, o, L = widths
    CASES[name] = dict(kw=dict(RECEGNN_CFGS[base], in_n_node_feat=i, hidden_n_node_feat=h, out_n_node_feat=o, n_convs=L, n_keypoints=K,
                               graph_cutoffs=CUT, **over), n_rec=list(n_rec), seed=seed, isolate=isolate)
    return name


# ---- 1. width grid: k_rc_conv's masks on = tid < hid, oon = tid < out, tid < in; block_sum2 / block_layernorm with a partial last wave
WIDTHS = [
    _case('w1', 'recegnn_small', (1, 1, 1, 1)),                     # every mask at one thread
    _case('w1_norm', 'recegnn_20kp', (1, 1, 1, 1)),                # block_layernorm over n = 1: d = 0, the result is the bias, no NaN
    _case('out130_hid48', 'recegnn_20kp', (10, 48, 130, 2), seed=20),        # out > hid: `oon` threads past `on` read s_f[k < hid] only
    _case('out65_hid63', 'recegnn_small', (10, 63, 65, 3)),         # hid one below, out one above a wave: block_sum2's second wave holds one lane
    _case('in200_hid64', 'recegnn_20kp', (200, 64, 64, 2)),         # in > hid: s_f[tid < in] loaded by threads that are not `on`; k_rc_proj packs 4 x 200
    _case('all256', 'recegnn_20kp', (256, 256, 256, 2), seed=20),            # s_in[4][RW], s_f[2 RW], s_m[RW] full; We_t rows 2 in, 2 in + 1 = 512, 513
    _case('in65_hid129_out33', 'recegnn_small', (65, 129, 33, 3)),  # three widths off the 16-grid, the middle conv is hid -> hid
    _case('hid255_out100', 'recegnn_20kp', (10, 255, 100, 2)),      # last wave one lane short; LayerNorm over 255 then 100
    _case('single_conv', 'recegnn_small', (17, 200, 256, 1)),       # one conv: c.in = in and c.out = D in the same ConvW
    # one switch each at in = 17, so the rows 2 in = 34 and 2 in + 1 = 35 of We_t / Wc_t are read where 2 in != 20
    _case('fix_pos', 'recegnn_small', (17, 40, 24, 2), fix_pos=True),               # Wc_t null: k_rc_proj skips parts 2, 3; x_out = x
    _case('no_tanh', 'recegnn_20kp', (17, 40, 24, 2), seed=22, use_tanh=False),              # c = cpart, with wae / wac (same_res) live
    _case('no_sameres', 'recegnn_20kp', (17, 40, 24, 2), use_sameres_feat=False),   # a.ef = 0: row 2 in + 1 does not exist and is not read
    _case('mnorm0', 'recegnn_small', (17, 40, 24, 2), message_norm=0.0),            # zinv = 1 / z[bidx[v]]
    _case('mnorm5', 'recegnn_20kp', (17, 40, 24, 2), seed=21, message_norm=5.0),             # zinv = 1 / norm_const, a.z null
]

# ---- 2. shape edges on one narrow config (in 10, hid 32, out 24), LayerNorm and same_res on
NARROW = (10, 32, 24, 2)
SHAPES = [
    _case('k1', 'recegnn_20kp', NARROW, n_rec=(16, 40), k_closest=1),              # k_rc_kp_feat: s_f[D + tid] for tid < 1, reduction over D + 1
    _case('k16', 'recegnn_20kp', NARROW, seed=112, n_rec=(16, 40), k_closest=16),            # a pocket of exactly k atoms: every atom is a neighbour
    _case('k16_out256', 'recegnn_20kp', (10, 32, 256, 2), seed=68, n_rec=(16, 40), k_closest=16),   # s_f[RW + 32]: D + k = 272 entries
    _case('K1', 'recegnn_20kp', NARROW, K=1),                                      # cap_kk = 0: no kk edges; D K = 24 < one block of k_rc_kp_embed
    _case('K3', 'recegnn_20kp', NARROW, seed=20, K=3),                                      # D K = 72 < 256: j >= DK threads leave after the barrier
    _case('K11_out100', 'recegnn_20kp', (10, 32, 100, 2), seed=20, K=11),                   # D K = 1100: grid.y = 5, the last block 76 wide
    _case('mod4_is3', 'recegnn_20kp', NARROW, seed=20, n_rec=(33, 21, 9)),                  # 63 atoms: k_rc_proj / k_linear_rows tail of 3 (61 = 1 mod 4 is everywhere else)
    _case('n256_n257', 'recegnn_20kp', NARROW, n_rec=(256, 257)),                  # k_kp_attention strides r += 256: exactly one pass, then one atom in the second
    _case('n513', 'recegnn_20kp', NARROW, seed=20, n_rec=(513, 6)),                         # three passes, 519 = 3 mod 4
    _case('isolated', 'recegnn_20kp', NARROW, n_rec=(33, 21), isolate=11, message_norm=5.0),   # rowptr[v] == rowptr[v + 1]: k_rc_conv's edge loop and its barriers skipped
    _case('B1', 'recegnn_20kp', NARROW, seed=20, n_rec=(33,)),                              # one graph: every per-batch kernel with one live thread
    # k_z_indegree / k_iota_scaled / k_node_graph_index: 256 threads per block over B, a second block at B = 300; z read for every graph
    _case('B300', 'recegnn_20kp', (10, 16, 24, 2), seed=1247, n_rec=(6,) * 300, K=2, k_closest=1, message_norm=0.0),
]

# ---- 3. invariances
INV = _case('inv', 'recegnn_20kp', (10, 63, 65, 2), n_rec=(40, 9, 25))
REUSE = [_case(f'reuse{i}', 'recegnn_20kp', (10, 63, 65, 2), n_rec=n, seed=sd) for i, (n, sd) in enumerate([((120, 60), 19), ((7,), 19), ((300, 150, 40), 20)])]

# ---- 4. trainer
TRAIN = ['out130_hid48', 'in65_hid129_out33', 'in200_hid64', 'w1',
         _case('single_conv_fix_pos', 'recegnn_small', (17, 200, 256, 1), fix_pos=True),
         _case('train_k16', 'recegnn_20kp', (10, 63, 65, 2), seed=231, n_rec=(33, 21, 16), k_closest=16),     # k_rk_feat_in / _dx / _dh at k = KL_KMAX
         _case('train_rad5', 'recegnn_20kp', (10, 63, 65, 2), seed=22, k_closest=0, kp_rad=5.0)]           # k_rk_radfeat_in / _dh at D = 65


def _complexes(c):
    kw, n_rec = c['kw'], c['n_rec']
    gs = synth.synth_complexes(n_rec, [1] * len(n_rec), kw['n_keypoints'], CUT, seed=c['seed'], n_rec_feat=kw['in_n_node_feat'])
    if c['isolate'] is not None:                   # one atom of pocket 0 moved 40 A away BEFORE the rr graph is built
        pos, feat = synth.synth_pocket(n_rec[0], c['seed'], kw['in_n_node_feat'])
        pos[c['isolate']] += torch.tensor([40.0, 0.0, 0.0])
        gs[0] = synth.build_complex_graph(pos, feat, kw['n_keypoints'], CUT, n_lig=1)
    for g in gs:                                   # per complex, so that a complex carries the same column alone and batched
        s, d = g.edges(etype='rr')
        g.edges['rr'].data['same_res'] = same_res_feature(s, d).bool()
    return gs


def _model(kw):
    model = synth.fill_state_dict_(ReceptorEncoder(**kw), 71).eval()
    with torch.no_grad():                          # the synthetic fill leaves the tiny xavier coordinate head: give it some weight
        for n, p in model.named_parameters():
            if 'coord_mlp.2.weight' in n:
                p.mul_(5.0)
    return model


def _oracle(model, kw, g, grad=False):
    """float64 oracle on the CPU batch `g`: (batch with kp x / h and the rk / kk edges, rec h, rec x, the float64 state dict)."""
    sd = {k: v.detach().double().clone().requires_grad_(grad) for k, v in model.state_dict().items()}
    ob = util.to_obatch(g)
    ob.x['rec'], ob.h['rec'] = ob.x['rec'].double(), ob.h['rec'].double()
    a = g.edges['rr'].data['same_res'].double().view(-1, 1) if kw['use_sameres_feat'] else None
    with torch.enable_grad() if grad else torch.no_grad():
        ref, ref_h, ref_x = orec.rec_encoder_egnn_forward(sd, kw, ob, a, return_rec=True)
    return ref, ref_h, ref_x, sd


def _gap(ref, kw, g):
    """Smallest relative distance gap of the oracle's rk and kk edge lists (module docstring)."""
    x0, kp = g.nodes['rec'].data['x_0'], ref.x['kp']
    n_rec, n_kp = g.batch_num_nodes('rec'), ref.n['kp']
    rk = (util.knn_rel_gap(x0, kp, kw['k_closest'], n_rec, n_kp) if kw['k_closest'] else
          util.radius_rel_gap(x0, kp, kw['kp_rad'], n_rec, n_kp))
    return min(rk, util.radius_rel_gap(kp, kp, CUT['kk'], n_kp, n_kp))


@functools.lru_cache(maxsize=None)
def _setup(name):
    """Model, complexes and float64 reference of a case (with its autograd graph for the trainer's cases), built once and shared by
    the tests that use the case; nothing here is written to afterwards: what runs are device copies (`_gpu`, `g.to(cuda)`)."""
    c, grad = CASES[name], name in TRAIN
    model, gs = _model(c['kw']), _complexes(c)
    g = G.batch(gs)
    ref = _oracle(model, c['kw'], g, grad)
    gap = _gap(ref[0], c['kw'], g)
    assert gap > GAP, f'{name}: the oracle has a near-tie (relative gap {gap:.2e}): pick another seed'
    return model, gs, g, ref


def _gpu(model, cuda):
    return copy.deepcopy(model).to(cuda)


def _run(model, g, cuda):
    """One forward of `model` (already on the GPU) on a fresh device copy of the CPU batch `g`: outputs and edge lists, on the CPU."""
    out = model(g.to(cuda), None)
    torch.cuda.synchronize()
    rec, kp = out.nodes['rec'].data, out.nodes['kp'].data
    res = dict(kp_x=kp['x_0'], kp_h=kp['h_0'], rec_h=rec['h'], rec_x=rec['x'])
    res['rk_src'], res['rk_dst'] = out.edges(etype='rk')
    res['kk_src'], res['kk_dst'] = out.edges(etype='kk')
    res['bne_rk'], res['bne_kk'] = out.batch_num_edges('rk'), out.batch_num_edges('kk')
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _engine(model, g, cuda):
    with torch.no_grad():
        return _run(model, g, cuda)


def _edge_set(s, d):
    return set(zip(s.tolist(), d.tolist()))


def _check(out, ref, name, what):
    kw, n_rec = CASES[name]['kw'], CASES[name]['n_rec']
    ref, ref_h, ref_x = ref[0], ref[1].detach(), ref[2].detach()
    K, B = kw['n_keypoints'], len(n_rec)
    for k in KEYS:
        assert torch.isfinite(out[k]).all(), f'{what}: {k} is not finite'
    # h leaves a LayerNorm when norm is set: an entry near zero carries the absolute error of its whole row, hence atol_rel = 1e-5
    # there (as test_infer_widths_gpu.py does for its normalised outputs); 1e-6 otherwise
    ln = 1e-5 if kw['norm'] else 1e-6
    util.assert_parity(out['kp_x'], ref.x['kp'].detach(), [K] * B, TOL, f'{what}: kp x_0', max_excess=MAX_EXCESS.get((name, 'kp_x'), 1.0))
    util.assert_parity(out['kp_h'], ref.h['kp'].detach(), [K] * B, TOL, f'{what}: kp h_0', atol_rel=ln)
    util.assert_parity(out['rec_h'], ref_h, n_rec, TOL, f'{what}: rec h', atol_rel=ln)
    util.assert_parity(out['rec_x'], ref_x, n_rec, TOL, f'{what}: rec x')
    assert torch.equal(out['rk_src'], ref.edges['rk'][0]) and torch.equal(out['rk_dst'], ref.edges['rk'][1]), f'{what}: rk edges'
    assert _edge_set(out['kk_src'], out['kk_dst']) == _edge_set(*ref.edges['kk']), f'{what}: kk edges'
    assert out['kk_src'].numel() == ref.edges['kk'][0].numel()
    assert torch.equal(out['bne_rk'], torch.bincount(ref.edges['rk'][1] // K, minlength=B)), f'{what}: rk edges per complex'
    assert torch.equal(out['bne_kk'], torch.bincount(ref.edges['kk'][1] // K, minlength=B)), f'{what}: kk edges per complex'


def _case_parity(name, cuda):
    model, _, g, ref = _setup(name)
    out = _engine(_gpu(model, cuda), g, cuda)
    _check(out, ref, name, f'{name} engine')
    return out, ref


@pytest.mark.parametrize('name', WIDTHS)
def test_width_grid(cuda, name):
    out, ref = _case_parity(name, cuda)
    if name == 'w1_norm':                  # LayerNorm over one element is its bias, exactly
        lb = _setup(name)[0].state_dict()['rec_convs.0.layer_norm.bias'].cpu()
        assert torch.equal(out['rec_h'], lb.expand_as(out['rec_h']))


@pytest.mark.parametrize('name', SHAPES)
def test_shape_edges(cuda, name):
    out, ref = _case_parity(name, cuda)
    c = CASES[name]
    if name == 'K1':
        assert out['kk_src'].numel() == 0 and int(out['bne_kk'].sum()) == 0
    if name == 'isolated':                 # the case exists only while the moved atom really has no rr edge
        s, d = _setup(name)[2].edges(etype='rr')
        assert int((d == c['isolate']).sum()) == 0 and int((s == c['isolate']).sum()) == 0
    if name == 'k16':
        assert sorted(out['rk_src'][:16].tolist()) == list(range(16))


# ---- 3. invariances ---------------------------------------------------------------------------------------------------------------
def test_same_batch_twice_same_bits(cuda):
    model, _, g, _ = _setup(INV)
    model = _gpu(model, cuda)
    a, b = _engine(model, g, cuda), _engine(model, g, cuda)
    for k in KEYS + EDGES:
        assert torch.equal(a[k], b[k]), k


def test_alone_and_batched(cuda):
    """Nothing in these kernels spans complexes (one workgroup per node or keypoint, per-graph loops in index order), so a complex
    alone and inside a batch gives the same bits; measured so on an MI355X before this was pinned to torch.equal."""
    model, gs, g, _ = _setup(INV)
    model = _gpu(model, cuda)
    full = _engine(model, g, cuda)
    n_rec, K, k = CASES[INV]['n_rec'], CASES[INV]['kw']['n_keypoints'], CASES[INV]['kw']['k_closest']
    r0 = 0
    for i, n in enumerate(n_rec):
        one = _engine(model, G.batch([gs[i]]), cuda)
        kk = (full['kk_dst'] >= i * K) & (full['kk_dst'] < (i + 1) * K)
        assert torch.equal(one['rk_src'] + r0, full['rk_src'][i * K * k:(i + 1) * K * k])
        assert torch.equal(one['rk_dst'] + i * K, full['rk_dst'][i * K * k:(i + 1) * K * k])
        assert _edge_set(one['kk_src'] + i * K, one['kk_dst'] + i * K) == _edge_set(full['kk_src'][kk], full['kk_dst'][kk])
        for key, lo, hi in (('kp_x', i * K, (i + 1) * K), ('kp_h', i * K, (i + 1) * K), ('rec_h', r0, r0 + n), ('rec_x', r0, r0 + n)):
            assert torch.equal(one[key], full[key][lo:hi]), f'complex {i} {key}'
        r0 += n


def _rotation():
    """A fixed proper rotation: 0.7 rad about (1, 2, 3) (Rodrigues)."""
    ax = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    ax = ax / ax.norm()
    Kx = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(0.7) * Kx + (1 - math.cos(0.7)) * Kx @ Kx


def test_rotation_and_translation(cuda):
    model, _, g, _ = _setup(INV)
    model = _gpu(model, cuda)
    base = _engine(model, g, cuda)
    R, t = _rotation(), torch.tensor([3.0, -2.0, 1.5], dtype=torch.float64)
    assert abs(float(torch.linalg.det(R)) - 1.0) < 1e-12
    move = lambda x: (x.double() @ R.T + t).float()
    g2 = g.to('cpu')                                   # same rr edges (a rigid motion keeps every distance), moved positions
    g2.nodes['rec'].data['x_0'] = move(g.nodes['rec'].data['x_0'])
    out = _engine(model, g2, cuda)
    n_rec, K = CASES[INV]['n_rec'], CASES[INV]['kw']['n_keypoints']
    util.assert_parity(out['kp_x'], move(base['kp_x']), [K] * 3, TOL, 'kp x_0 moved')
    util.assert_parity(out['rec_x'], move(base['rec_x']), n_rec, TOL, 'rec x moved')
    util.assert_parity(out['kp_h'], base['kp_h'], [K] * 3, TOL, 'kp h_0 unchanged', atol_rel=1e-5)      # LayerNorm outputs, as in _check
    util.assert_parity(out['rec_h'], base['rec_h'], n_rec, TOL, 'rec h unchanged', atol_rel=1e-5)
    assert torch.equal(out['rk_src'], base['rk_src']) and torch.equal(out['rk_dst'], base['rk_dst'])
    assert _edge_set(out['kk_src'], out['kk_dst']) == _edge_set(base['kk_src'], base['kk_dst'])


def test_order_of_complexes(cuda):
    model, gs, g, _ = _setup(INV)
    model = _gpu(model, cuda)
    base = _engine(model, g, cuda)
    perm = [2, 0, 1]
    out = _engine(model, G.batch([gs[i] for i in perm]), cuda)
    n_rec, K, k = CASES[INV]['n_rec'], CASES[INV]['kw']['n_keypoints'], CASES[INV]['kw']['k_closest']
    off = [sum(n_rec[:i]) for i in range(3)]
    r0 = 0
    for j, i in enumerate(perm):
        n = n_rec[i]
        util.assert_parity(out['kp_x'][j * K:(j + 1) * K], base['kp_x'][i * K:(i + 1) * K], None, TOL, f'complex {i} kp x_0')
        util.assert_parity(out['kp_h'][j * K:(j + 1) * K], base['kp_h'][i * K:(i + 1) * K], None, TOL, f'complex {i} kp h_0', atol_rel=1e-5)
        util.assert_parity(out['rec_h'][r0:r0 + n], base['rec_h'][off[i]:off[i] + n], None, TOL, f'complex {i} rec h', atol_rel=1e-5)
        util.assert_parity(out['rec_x'][r0:r0 + n], base['rec_x'][off[i]:off[i] + n], None, TOL, f'complex {i} rec x')
        assert torch.equal(out['rk_src'][j * K * k:(j + 1) * K * k] - r0, base['rk_src'][i * K * k:(i + 1) * K * k] - off[i])
        assert int(out['bne_kk'][j]) == int(base['bne_kk'][i])
        r0 += n


def test_engine_reuse(cuda):
    """kpd_recegnn_reserve re-carves the workspace when a later batch is larger: big, small, bigger, small on ONE module."""
    model = _gpu(_setup(REUSE[0])[0], cuda)
    small = []
    for name in (REUSE[0], REUSE[1], REUSE[2], REUSE[1]):
        _, _, g, ref = _setup(name)
        out = _engine(model, g, cuda)
        _check(out, ref, name, f'{name} engine')
        if name == REUSE[1]:
            small.append(out)
    for k in KEYS + EDGES:
        assert torch.equal(small[0][k], small[1][k]), k


# ---- 4. trainer -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_grads(name):
    """Gradients of the loss of test_encoder_gradients_match_oracle_autograd (random fixed weights on kp x_0 and kp h_0) through the
    float64 oracle: (name -> gradient, w_x, w_h)."""
    ref, _, _, sd = _setup(name)[3]
    n_kp, D = ref.x['kp'].shape[0], CASES[name]['kw']['out_n_node_feat']
    gen = torch.Generator().manual_seed(5)
    w_x, w_h = torch.randn(n_kp, 3, generator=gen), torch.randn(n_kp, D, generator=gen) / D ** 0.5
    ((ref.x['kp'] * w_x.double()).sum() + (ref.h['kp'] * w_h.double()).sum()).backward()
    return {n: t.grad for n, t in sd.items()}, w_x, w_h


@pytest.mark.parametrize('name', TRAIN)
def test_trainer_widths(cuda, name):
    model, _, g, ref = _setup(name)
    kw, n_rec = CASES[name]['kw'], CASES[name]['n_rec']
    ref_grads, w_x, w_h = _ref_grads(name)
    model = _gpu(model, cuda)
    eng = _engine(model, g, cuda)
    _check(eng, ref, name, f'{name} engine')

    def train():
        model.zero_grad(set_to_none=True)
        out = model(g.to(cuda), None)
        kp, rec = out.nodes['kp'].data, out.nodes['rec'].data
        assert kp['x_0'].requires_grad and kp['h_0'].requires_grad
        ((kp['x_0'] * w_x.to(cuda)).sum() + (kp['h_0'] * w_h.to(cuda)).sum()).backward()
        torch.cuda.synchronize()
        res = dict(kp_x=kp['x_0'], kp_h=kp['h_0'], rec_h=rec['h'], rec_x=rec['x'], bne_rk=out.batch_num_edges('rk'), bne_kk=out.batch_num_edges('kk'))
        res['rk_src'], res['rk_dst'] = out.edges(etype='rk')
        res['kk_src'], res['kk_dst'] = out.edges(etype='kk')
        return ({k: v.detach().cpu().clone() for k, v in res.items()},
                {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})

    tr, grads = train()
    _check(tr, ref, name, f'{name} trainer')
    K, B, ln = kw['n_keypoints'], len(n_rec), 1e-5 if kw['norm'] else 1e-6
    for k, counts in (('kp_x', [K] * B), ('kp_h', [K] * B), ('rec_h', n_rec), ('rec_x', n_rec)):
        util.assert_parity(tr[k], eng[k], counts, TOL, f'{name}: trainer vs engine {k}', atol_rel=ln if k.endswith('_h') else 1e-6)
    for k in EDGES[:2]:
        assert torch.equal(tr[k], eng[k]), k
    util.assert_param_grads(model, ref_grads, GRAD_TOL, tol_of=GRAD_TOL_OF.get(name))
    _, again = train()
    assert again.keys() == grads.keys()
    for n in grads:
        assert torch.equal(grads[n], again[n]), f'{name}: gradient of {n} differs between two backward passes'
