"""The GVP keypoint receptor encoder (kpd_recenc_* and kpd_recenc_trainer_*, through ReceptorEncoderGVP) at the edges of its kernels:
K = 1, n_keypoints * out_scalar_size at KPE_MAX exactly, k_closest 1 and KL_KMAX on a pocket of exactly 16 atoms, no rr conv,
out_scalar_size 1 / 127 / 129 / 255, in_scalar_size 1 / 256, pockets of 256 / 257 / 513 atoms, atom totals 2 and 3 mod 4, an atom
without rr in-edge, rr runs over 3 tiles at the 100-neighbour cap in every norm mode, keypoints without rk edge, B = 1 and B = 300,
chains (4, 4), 1 and 15 vector channels; its symmetries; the trainer against float64 autograd and against the engine.

The cases and the properties they are named for live in gvp_shape_cases.py (checked on the CPU by test_gvp_shape_cases.py and
asserted again here before anything is compared).  The reference is oracle/rec_encoder.py run in float64.  Exact comparison of the
rk lists (and of the kk sets) needs that oracle to have no near-tie: every case asserts a relative gap of at least 1e-3 between
consecutive distances among a keypoint's k + 1 nearest atoms, and between any distance and kp_rad / the kk cutoff.  Bounds are the
project's own: util.assert_parity at 1e-4 (all three measures), gradients within 2e-4 of the largest entry per tensor; no case
carries a loosened bound."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip
from keypoint_diffusion_amd import synth
from keypoint_diffusion_amd.receptor_encoder_gvp import ReceptorEncoderGVP

from . import gvp_shape_cases as gc
from . import util

pytestmark = pytest.mark.gpu
TOL = 1e-4
GRAD_TOL = 2e-4     # test_recenc_train_gpu.py: relative to the largest entry of each gradient tensor
# two runs of the engine on inputs that an exact symmetry of the function maps onto each other: each is within TOL of that function
SYM_TOL = 2 * TOL
KEYS = gc.REC_KEYS
EDGES = ('rk_src', 'rk_dst', 'kk_src', 'kk_dst')


def _collect(out):
    kp = out.nodes['kp'].data
    res = dict(kp_x=kp['x_0'], kp_h=kp['h_0'], kp_v=kp['v_0'], bne_rk=out.batch_num_edges('rk'), bne_kk=out.batch_num_edges('kk'))
    res['rk_src'], res['rk_dst'] = out.edges(etype='rk')
    res['kk_src'], res['kk_dst'] = out.edges(etype='kk')
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _engine(model, g, cuda):
    """One forward of `model` (on the GPU) on a fresh device copy of the CPU batch `g`: outputs and edge lists, on the CPU."""
    with torch.no_grad():
        out = model(g.to(cuda), None)
    torch.cuda.synchronize()
    return _collect(out)


def _edge_set(s, d):
    return set(zip(s.tolist(), d.tolist()))


def _check(out, ref, name, what):
    kw, n_rec = gc.REC[name]['kw'], gc.REC[name]['n_rec']
    K, B = kw['n_keypoints'], len(n_rec)
    for k in KEYS:
        assert torch.isfinite(out[k]).all(), f'{what}: {k} is not finite'
        util.assert_parity(out[k], ref[k], [K] * B, TOL, f'{what}: {k}')
    assert torch.equal(out['rk_src'], ref['rk'][0]) and torch.equal(out['rk_dst'], ref['rk'][1]), f'{what}: rk edges'
    assert _edge_set(out['kk_src'], out['kk_dst']) == _edge_set(*ref['kk']) and out['kk_src'].numel() == ref['kk'][0].numel(), f'{what}: kk edges'
    assert torch.equal(out['bne_rk'], torch.bincount(ref['rk'][1] // K, minlength=B)), f'{what}: rk edges per complex'
    assert torch.equal(out['bne_kk'], torch.bincount(ref['kk'][1] // K, minlength=B)), f'{what}: kk edges per complex'


def _setup(name, cuda, grad=False):
    ref = gc.rec_reference(name, torch.float64, grad)
    gc.check_rec(name, ref)                                           # the gap and the stated property, from the oracle alone
    return gc.rec_model(name).to(cuda), gc.rec_batch(name), ref


@pytest.mark.parametrize('name', gc.REC_SHAPES)
def test_shape_edges(cuda, name):
    model, g, ref = _setup(name, cuda)
    out = _engine(model, g, cuda)
    _check(out, ref, name, f'{name} engine')
    kw = gc.REC[name]['kw']
    if name == 'K1':
        assert out['kk_src'].numel() == 0 and int(out['bne_kk'].sum()) == 0
    if name == 'k16_n16':
        assert sorted(out['rk_src'][:16].tolist()) == list(range(16))
    if name == 'kp_rad':                       # the degree assertions of test_receptor_encoder
        deg = torch.bincount(out['rk_dst'], minlength=len(gc.REC[name]['n_rec']) * kw['n_keypoints'])
        assert int(deg.max()) <= 10 and int(deg.min()) == 0
        assert torch.equal(out['bne_rk'], torch.bincount(out['rk_dst'] // kw['n_keypoints'], minlength=len(gc.REC[name]['n_rec'])))
    if name == 'out1':                         # GVPLayerNorm over one scalar is its bias, exactly
        lb = gc.rec_model(name).state_dict()['rk_conv_layers.1.update_layer_norm.feat_norm.bias']
        assert torch.equal(out['kp_h'], lb.expand_as(out['kp_h']))


def test_one_keypoint_past_the_limit_is_refused(cuda):
    """n_keypoints * out_scalar_size = 41 * 256 > KPE_MAX: refused by kpd_recenc_create's host-side check, naming the value."""
    kw = dict(gc.REC['K40_out256']['kw'], n_keypoints=41)
    model = synth.fill_state_dict_(ReceptorEncoderGVP(**kw), 61).eval().to(cuda)
    with pytest.raises(hip.KpdError, match='n_keypoints=41'):
        model.engine()


# ---- symmetry ---------------------------------------------------------------------------------------------------------------------------
def _sym(cuda):
    model, g, ref = _setup(gc.REC_SYM, cuda)
    base = _engine(model, g, cuda)
    _check(base, ref, gc.REC_SYM, 'sym engine')
    return model, g, base


def _close(got, want, what):
    for k in KEYS:
        util.assert_parity(got[k], want[k], None, SYM_TOL, f'{what}: {k}')


def test_same_batch_twice_same_bits(cuda):
    model, g, base = _sym(cuda)
    again = _engine(model, g, cuda)
    for k in KEYS + EDGES:
        assert torch.equal(base[k], again[k]), k


def test_rotation_and_translation_per_complex(cuda):
    """A proper rotation and a translation of at most 20 A of each pocket: kp x_0 moves with it, h_0 stays, v_0 turns; the rr edges
    are the caller's (a rigid motion keeps every distance) and the rk / kk lists cannot change at a relative gap of 1e-3."""
    model, g, base = _sym(cuda)
    n_rec, K = gc.REC[gc.REC_SYM]['n_rec'], gc.REC[gc.REC_SYM]['kw']['n_keypoints']
    g2, rp = g.to('cpu'), g.node_ptr('rec').tolist()
    x = g.nodes['rec'].data['x_0'].double().clone()
    want = {k: base[k].double().clone() for k in KEYS}
    for b, (R, tr) in enumerate(gc.rigid_motions(len(n_rec))):
        x[rp[b]:rp[b + 1]] = x[rp[b]:rp[b + 1]] @ R.T + tr
        want['kp_x'][b * K:(b + 1) * K] = want['kp_x'][b * K:(b + 1) * K] @ R.T + tr
        want['kp_v'][b * K:(b + 1) * K] = want['kp_v'][b * K:(b + 1) * K] @ R.T
    g2.nodes['rec'].data['x_0'] = x.float()
    out = _engine(model, g2, cuda)
    for k in KEYS:
        util.assert_parity(out[k], want[k], [K] * len(n_rec), SYM_TOL, f'moved: {k}')
    assert torch.equal(out['rk_src'], base['rk_src']) and torch.equal(out['rk_dst'], base['rk_dst'])
    assert _edge_set(out['kk_src'], out['kk_dst']) == _edge_set(base['kk_src'], base['kk_dst'])


def _complex_slice(res, i, K, k, r0):
    """Complex i of a result: its keypoint rows, its rk sources relative to its first atom `r0`, its kk set relative to its keypoints."""
    kk = (res['kk_dst'] >= i * K) & (res['kk_dst'] < (i + 1) * K)
    return ({key: res[key][i * K:(i + 1) * K] for key in KEYS}, res['rk_src'][i * K * k:(i + 1) * K * k] - r0,
            _edge_set(res['kk_src'][kk] - i * K, res['kk_dst'][kk] - i * K))


def test_order_of_complexes(cuda):
    model, g, base = _sym(cuda)
    c = gc.REC[gc.REC_SYM]
    n_rec, K, k = c['n_rec'], c['kw']['n_keypoints'], c['kw']['k_closest']
    gs, perm = gc.rec_complexes(gc.REC_SYM), [2, 0, 1]
    out = _engine(model, G.batch([gs[i] for i in perm]), cuda)
    off, r0 = [sum(n_rec[:i]) for i in range(3)], 0
    for j, i in enumerate(perm):
        got, want = _complex_slice(out, j, K, k, r0), _complex_slice(base, i, K, k, off[i])
        _close(got[0], want[0], f'complex {i} reordered')
        assert torch.equal(got[1], want[1]) and got[2] == want[2], f'complex {i} reordered: edges'
        r0 += n_rec[i]


def test_alone_and_batched(cuda):
    model, g, base = _sym(cuda)
    c = gc.REC[gc.REC_SYM]
    n_rec, K, k = c['n_rec'], c['kw']['n_keypoints'], c['kw']['k_closest']
    r0 = 0
    for i, gi in enumerate(gc.rec_complexes(gc.REC_SYM)):
        got, want = _complex_slice(_engine(model, G.batch([gi]), cuda), 0, K, k, 0), _complex_slice(base, i, K, k, r0)
        _close(got[0], want[0], f'complex {i} alone')
        assert torch.equal(got[1], want[1]) and got[2] == want[2], f'complex {i} alone: edges'
        r0 += n_rec[i]


# ---- trainer ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', gc.REC_TRAIN)
def test_trainer(cuda, name):
    """kpd_recenc_trainer_*: every parameter gradient against float64 autograd for a loss through all three outputs, the training
    forward against the oracle and against the engine, two backward passes bit for bit."""
    model, g, ref = _setup(name, cuda, grad=True)
    kw, n_rec = gc.REC[name]['kw'], gc.REC[name]['n_rec']
    K, B = kw['n_keypoints'], len(n_rec)
    eng = _engine(model, g, cuda)
    _check(eng, ref, name, f'{name} engine')
    w = [t.to(cuda) for t in gc.rec_loss_weights(B * K, kw['out_scalar_size'], kw['vector_size'])]

    def train():
        model.zero_grad(set_to_none=True)
        out = model(g.to(cuda), None)
        kp = out.nodes['kp'].data
        assert kp['x_0'].requires_grad and kp['h_0'].requires_grad and kp['v_0'].requires_grad
        sum((a * b).sum() for a, b in zip((kp['x_0'], kp['h_0'], kp['v_0']), w)).backward()
        torch.cuda.synchronize()
        return _collect(out), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    tr, grads = train()
    _check(tr, ref, name, f'{name} trainer')
    for k in KEYS:
        util.assert_parity(tr[k], eng[k], [K] * B, TOL, f'{name}: trainer against engine {k}')
    for k in EDGES[:2]:
        assert torch.equal(tr[k], eng[k]), k
    util.assert_param_grads(model, ref['params'], GRAD_TOL, min_checked=20)
    tr2, again = train()
    assert again.keys() == grads.keys() and all(torch.equal(tr[k], tr2[k]) for k in KEYS + EDGES)
    for n in grads:
        assert torch.equal(grads[n], again[n]), f'{name}: gradient of {n} differs between two backward passes'
