"""The EGNN denoiser at hidden_nf 257 .. 1024 (inference, csrc/egnn_wide.hip): oracle parity, determinism, bitwise batch invariance,
the captured step, sampling through KeypointDiffusion, and the refusals that name the limits."""
import os

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip, synth
from keypoint_diffusion_amd.dynamics import LigRecDynamics
from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
from oracle import diffusion as odiff
from oracle import egnn as oegnn

from . import util
from .golden.make_golden_cfgs import RECEGNN_CFGS, same_res_feature

pytestmark = pytest.mark.gpu
CUT = util.CUTOFFS_ALL_ATOM
TOL = 1e-4


def _model(cfg, rec_nf=10, seed=3):
    m = LigRecDynamics(10, rec_nf, graph_cutoffs=CUT, **cfg)
    synth.fill_state_dict_(m, seed)
    return m.eval()


def _t(B):
    return (torch.arange(B, dtype=torch.float32) + 1) / (B + 1)


def _oracle(model, cfg, g, layers=None):
    ocfg = dict(cfg, graph_cutoffs=CUT)
    if layers is not None:
        ocfg['n_layers'] = layers
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return oegnn.egnn_dynamics_forward(sd, ocfg, util.to_obatch(g), _t(g.batch_size))


def _hip(model, g, cuda, layers=None):
    gd = g.to(cuda)
    with torch.no_grad():
        if layers is not None:
            model.engine().debug(f'layers={layers}')
        h, x = model(gd, _t(g.batch_size).to(cuda), None)
    torch.cuda.synchronize()
    return h.cpu(), x.cpu()


CASES = [
    # hidden_nf, config overrides, pockets, ligands, debug layers
    (257, dict(n_layers=2), [300, 150, 40], [25, 9, 3], None),
    (384, dict(n_layers=3, norm=False, use_tanh=False, message_norm=5.0, update_kp_feat=False, ll_k=3, kl_k=0), [7, 600], [5, 30], None),
    (512, dict(n_layers=3, kl_k=0), [120, 77], [14, 6], 1),
    (512, dict(n_layers=3), [90, 45], [11, 4], 0),
    (512, dict(n_layers=3, update_kp_feat=False, message_norm=0), [7, 600, 60], [3, 25, 9], None),
    (1024, dict(n_layers=2), [60, 30], [10, 4], None),
]


@pytest.mark.parametrize('hidden_nf,over,n_rec,n_lig,layers', CASES)
def test_oracle_parity(cuda, hidden_nf, over, n_rec, n_lig, layers):
    cfg = dict(util.EGNN_C2, hidden_nf=hidden_nf, **over)
    g = util.fixed_encode(util.make_batch(n_rec, n_lig))
    model = _model(cfg)
    rh, rx = _oracle(model, cfg, g, layers)
    h, x = _hip(model.to(cuda), g, cuda, layers)
    util.assert_parity(h, rh, n_lig, TOL, 'eps_h')
    if layers == 0:
        assert float(x.abs().max()) == 0.0
    else:
        util.assert_parity(x, rx, n_lig, TOL, 'eps_x', atol_rel=1e-5)


def _fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'egnn_wide.npz'))


@pytest.mark.parametrize('tag', ['h257_kp', 'h257_nokp', 'h512_kp', 'h512_nokp'])
def test_upstream_fixture_parity(cuda, tag):
    """One forward against upstream's own LigRecConv sub-modules in float64 (make_egnn_wide_golden.py): the [h, t] column order
    and the src / dst / distance split of the first Linear are upstream's, not only the project oracle's."""
    z = _fixture()
    n_rec, n_lig = [int(v) for v in z['n_rec']], [int(v) for v in z['n_lig']]
    g = util.fixed_encode(util.make_batch(n_rec, n_lig, seed=int(z['batch_seed'])))
    ob = util.to_obatch(g)
    for got, key in ((ob.x['lig'], 'lig_x'), (ob.h['lig'], 'lig_h'), (ob.x['kp'], 'kp_x'), (ob.h['kp'], 'kp_h'),
                     (ob.edges['kk'][0], 'kk_src'), (ob.edges['kk'][1], 'kk_dst')):
        assert np.array_equal(got.numpy(), z[key]), key                    # the stored inputs are the ones rebuilt here
    H = 257 if tag.startswith('h257') else 512
    cfg = dict(util.EGNN_C2, hidden_nf=H, n_layers=2, update_kp_feat=tag.endswith('_kp'))
    model = _model(cfg, seed=int(z[f'{tag}_seed'])).to(cuda)
    gd = g.to(cuda)
    with torch.no_grad():
        h, x = model(gd, torch.tensor(z['t'], device=cuda), None)
        c = model.engine().last_counts()
    torch.cuda.synchronize()
    assert (c['E_ll'], c['E_kl']) == (len(z[f'{tag}_ll_src']), len(z[f'{tag}_kl_src']))
    util.assert_parity(h.cpu(), torch.tensor(z[f'{tag}_eps_h']), n_lig, TOL, 'eps_h')
    util.assert_parity(x.cpu(), torch.tensor(z[f'{tag}_eps_x']), n_lig, TOL, 'eps_x', atol_rel=1e-5)


def test_pruning_and_repeat_are_bit_identical(cuda):
    cfg = dict(util.EGNN_C2, hidden_nf=512, n_layers=2)
    g = util.fixed_encode(util.make_batch([300, 150, 40], [25, 9, 3])).to(cuda)
    model = _model(cfg).to(cuda)
    t = _t(3).to(cuda)
    eng = model.engine()
    with torch.no_grad():
        eng.debug('prune=0')
        h0, x0 = model(g, t, None)
        eng.debug('prune=1')
        h1, x1 = model(g, t, None)
        h2, x2 = model(g, t, None)
    torch.cuda.synchronize()
    assert torch.equal(h0, h1) and torch.equal(x0, x1)
    assert torch.equal(h1, h2) and torch.equal(x1, x2)


def test_batch_invariance_bitwise(cuda):
    """kl_k = 1 on all-atom keypoints: E_kl = E_lk = keypoints, 129 alone and 385 in the batch -- both 1 (mod 128), the GEMM shapes
    whose last row the product would otherwise compute as a fringe row."""
    n_rec, n_lig = [129, 200, 56], [9, 17, 5]
    cfg = dict(util.EGNN_C2, hidden_nf=384, n_layers=2, kl_k=1)
    model = _model(cfg).to(cuda)
    gs = synth.synth_complexes(n_rec, n_lig, 20, CUT, seed=1234)
    g = util.fixed_encode(G.batch(gs)).to(cuda)
    t = torch.tensor([0.2, 0.5, 0.8], device=cuda)
    with torch.no_grad():
        h, x = model(g, t, None)
        assert model.engine().last_counts()['E_kl'] == 385
        off = 0
        for i, nl in enumerate(n_lig):
            g1 = util.fixed_encode(G.batch([synth.synth_complexes(n_rec, n_lig, 20, CUT, seed=1234)[i]])).to(cuda)
            h1, x1 = model(g1, t[i:i + 1], None)
            if i == 0:
                assert model.engine().last_counts()['E_kl'] == 129
            assert torch.equal(h1, h[off:off + nl]) and torch.equal(x1, x[off:off + nl]), i
            off += nl


def _diffusion(hidden_nf, learned=False, T=10):
    dyn = dict(util.EGNN_C2, hidden_nf=hidden_nf, n_layers=2)
    if learned:
        rec_cfg = {k: v for k, v in RECEGNN_CFGS['recegnn_20kp'].items() if k not in ('in_n_node_feat', 'n_keypoints')}
        m = KeypointDiffusion(10, 128, None, n_timesteps=T, architecture='egnn', rec_encoder_type='learned',
                              graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dyn,
                              rec_encoder_config=dict(rec_cfg, in_n_node_feat=10), precision=1e-5)
    else:
        m = KeypointDiffusion(10, 10, None, n_timesteps=T, architecture='egnn', rec_encoder_type='fixed',
                              graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dyn,
                              rec_encoder_config={'vector_size': 16}, precision=1e-5)
    synth.fill_state_dict_(m, 13)
    return m.eval()


def _pocket_batch(model, n_rec, n_lig, seed, learned, cuda=None):
    gs = synth.synth_complexes(n_rec, n_lig, 20, CUT, seed=seed)
    if learned:
        for gg in gs:
            s, d = gg.edges(etype='rr')
            gg.edges['rr'].data['same_res'] = same_res_feature(s, d).bool()
    g = G.batch(gs)
    return model.encode_receptors(g.to(cuda) if cuda is not None else g)


@pytest.mark.parametrize('learned', [False, True])
def test_reverse_steps_match_oracle(cuda, learned):
    """Ten reverse steps at hidden_nf = 512 with fixed per-step noise against the oracle's sample_step chain, with the fixed
    encoder and with the learned EGNN keypoint encoder (keypoints encoded once, as the sampler does)."""
    T = 10
    model = _diffusion(512, learned=learned, T=T).to(cuda)
    with torch.no_grad():
        gd = _pocket_batch(model, [90, 140], [11, 17], 3, learned, cuda)
    ob = util.to_obatch(gd)
    sd = {k[len('dynamics.'):]: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.startswith('dynamics.')}
    ocfg = dict(util.EGNN_C2, hidden_nf=512, n_layers=2, graph_cutoffs=CUT)
    gen = torch.Generator().manual_seed(1)
    noise = [(torch.randn(ob.x['lig'].shape, generator=gen), torch.randn(ob.h['lig'].shape, generator=gen)) for _ in range(T)]
    table = odiff.gamma_table(T, 1e-5)
    ones = torch.ones(2)
    for i, sidx in enumerate(range(T - 1, -1, -1)):
        s, t = ones * (sidx / T), ones * ((sidx + 1) / T)
        eh, ex = oegnn.egnn_dynamics_forward(sd, ocfg, ob, t)
        ob = odiff.sample_step(ob.clone(), eh, ex, s, t, table, T, *noise[i])
        with torch.no_grad():
            model.sample_p_zs_given_zt(s.to(cuda), t.to(cuda), gd, G.get_batch_idxs(gd), noise=tuple(n.to(cuda) for n in noise[i]))
    torch.cuda.synchronize()
    assert util.rel_err(gd.nodes['lig'].data['x_0'], ob.x['lig']) < 1e-3
    assert util.rel_err(gd.nodes['lig'].data['h_0'], ob.h['lig']) < 1e-3


@pytest.mark.parametrize('learned', [False, True])
def test_step_graph_and_sampling(cuda, learned):
    """At hidden_nf = 512 the captured reverse step (StepGraph) equals the eager step bit for bit for several timesteps, with the
    fixed and with the learned EGNN keypoint encoder (rec_nf = 128 != hidden_nf); sampling runs end to end with both."""
    T = 10
    model = _diffusion(512, learned=learned, T=T).to(cuda)
    with torch.no_grad():
        g1 = _pocket_batch(model, [60, 45], [9, 13], 5, learned, cuda)
        g2 = _pocket_batch(model, [60, 45], [9, 13], 5, learned, cuda)
        gen = torch.Generator().manual_seed(1)
        nx = torch.randn(g1.num_nodes('lig'), 3, generator=gen).to(cuda)
        nh = torch.randn(g1.num_nodes('lig'), 10, generator=gen).to(cuda)
        sg = model.capture_step(g1, noise=(nx, nh))
        ones = torch.ones(2, device=cuda)
        for s in (9, 8, 3):
            sg.step(s / T, (s + 1) / T)
            model.sample_p_zs_given_zt(ones * (s / T), ones * ((s + 1) / T), g2, noise=(nx, nh))
            for nt, k in (('lig', 'x_0'), ('lig', 'h_0'), ('kp', 'x_0')):
                assert torch.equal(g1.nodes[nt].data[k], g2.nodes[nt].data[k]), (s, nt, k)
            assert torch.isfinite(g1.nodes['lig'].data['x_0']).all()
        pocket = synth.synth_complexes([70], [1], 20, CUT, seed=9)[0].to(cuda)
        pocket.remove_nodes(pocket.nodes('lig'), ntype='lig')
        if learned:
            s, d = pocket.edges(etype='rr')
            pocket.edges['rr'].data['same_res'] = same_res_feature(s.cpu(), d.cpu()).bool().to(cuda)
        pos, feat = model.sample_given_pocket(pocket, torch.tensor([6, 9]), diff_batch_size=2)
    assert [p.shape for p in pos] == [(6, 3), (9, 3)] and all(torch.isfinite(p).all() for p in pos)


def test_feature_width_mismatch_is_refused(cuda):
    """Keypoint features narrower than rec_nf would be read past their end: refused, as upstream's encoder Linear refuses them."""
    cfg = dict(util.EGNN_C2, hidden_nf=512, n_layers=1)
    g = util.fixed_encode(util.make_batch([40], [5])).to(cuda)
    model = _model(cfg, rec_nf=16).to(cuda)
    with torch.no_grad(), pytest.raises(hip.KpdError, match='rec_nf=16'):
        model(g, torch.tensor([0.5], device=cuda), None)


def test_refusals_name_the_limits(cuda, monkeypatch):
    with pytest.raises(ValueError, match='1 .. 1024'):
        LigRecDynamics(10, 10, hidden_nf=1025, graph_cutoffs=CUT, kl_k=5)
    cfg = dict(util.EGNN_C2, hidden_nf=512, n_layers=1)
    g = util.fixed_encode(util.make_batch([40], [5])).to(cuda)
    model = _model(cfg).to(cuda)
    t = torch.tensor([0.5], device=cuda)
    with pytest.raises(hip.KpdError, match='training above 256 is not implemented'):
        model(g, t, None)                                           # grad enabled, parameters require grad
    model.gemm_mode = 'f16x2'
    with torch.no_grad(), pytest.raises(hip.KpdError, match='f16x2'):
        model(g, t, None)
    monkeypatch.setenv('KPD_GEMM', 'f16x2')
    model = _model(cfg).to(cuda)
    with torch.no_grad():
        h, _ = model(g, t, None)
    assert model.engine().gemm_mode() == 'f32' and torch.isfinite(h).all()
