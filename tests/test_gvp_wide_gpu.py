"""The GVP denoiser at n_hidden_scalars 257 .. 1024 (inference, csrc/gvp_wide.hip): fixture and oracle parity, per-conv parity,
determinism, bitwise batch invariance, the captured step, sampling through KeypointDiffusion, and the refusals that name the limits."""
import os

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip, synth
from keypoint_diffusion_amd.dynamics_gvp import LigRecDynamicsGVP
from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
from oracle import diffusion as odiff
from oracle import gvp as ogvp

from . import util
from .golden.make_golden_cfgs import RECENC_CFGS

pytestmark = pytest.mark.gpu
CUT = util.CUTOFFS_ALL_ATOM
TOL = 1e-4
BASE = dict(vector_size=16, n_convs=2, message_norm=10.0, update_kp=True, ll_k=0, kl_k=7, n_message_gvps=3, n_update_gvps=2,
            n_noise_gvps=4, dropout=0.0)


def _model(cfg, seed=7):
    m = LigRecDynamicsGVP(10, 10, graph_cutoffs=CUT, **cfg)
    synth.fill_state_dict_(m, seed)
    return m.eval()


def _t(B):
    return (torch.arange(B, dtype=torch.float32) + 1) / (B + 1)


def _batch(n_rec, n_lig, V, seed=31):
    g = util.fixed_encode(util.make_batch(n_rec, n_lig, seed=seed), n_vec=V)
    gen = torch.Generator().manual_seed(3)
    g.nodes['kp'].data['v_0'] = 0.5 * torch.randn(g.num_nodes('kp'), V, 3, generator=gen)
    return g


def _oracle(model, cfg, g, convs=None):
    ocfg = dict(cfg, graph_cutoffs=CUT)
    if convs is not None:
        ocfg['n_convs'] = convs
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return ogvp.gvp_dynamics_forward(sd, ocfg, util.to_obatch(g), _t(g.batch_size))


def _hip(model, g, cuda, convs=None):
    gd = g.to(cuda)
    with torch.no_grad():
        if convs is not None:
            model.engine().debug(f'convs={convs}')
        h, x = model(gd, _t(g.batch_size).to(cuda), None)
    torch.cuda.synchronize()
    return h.cpu(), x.cpu()


CASES = [
    # n_hidden_scalars, config overrides, pockets, ligands
    (257, dict(), [60, 30], [10, 4]),
    (320, dict(vector_size=5, message_norm=0, kl_k=0, n_message_gvps=1, n_noise_gvps=3), [7, 600], [1, 25]),
    (384, dict(vector_size=1, message_norm='mean', n_convs=1, update_kp=False, kl_k=5), [120, 45], [14, 6]),
    (512, dict(message_norm='mean', n_convs=3), [90, 45, 7], [11, 4, 1]),
    (512, dict(vector_size=5, message_norm=0, kl_k=0, n_message_gvps=3, n_noise_gvps=3, n_update_gvps=1), [40, 30], [9, 5]),
    (1024, dict(vector_size=1, kl_k=3, n_message_gvps=1), [60, 30], [10, 4]),
]


@pytest.mark.parametrize('S,over,n_rec,n_lig', CASES)
def test_oracle_parity(cuda, S, over, n_rec, n_lig):
    cfg = dict(BASE, n_hidden_scalars=S, **over)
    g = _batch(n_rec, n_lig, cfg['vector_size'])
    model = _model(cfg)
    rh, rx = _oracle(model, cfg, g)
    h, x = _hip(model.to(cuda), g, cuda)
    util.assert_parity(h, rh, n_lig, TOL, 'eps_h')
    util.assert_parity(x, rx, n_lig, TOL, 'eps_x')


@pytest.mark.parametrize('convs', [0, 1, 2])
def test_per_conv_parity(cuda, convs):
    """The first `convs` convs of a 3-conv model against the oracle run with that many: the ligand outputs of a truncated stack do
    not depend on whether its last conv also updates the keypoints."""
    cfg = dict(BASE, n_hidden_scalars=384, n_convs=3, message_norm='mean')
    g = _batch([70, 40], [12, 5], 16)
    model = _model(cfg, seed=11)
    rh, rx = _oracle(model, cfg, g, convs)
    h, x = _hip(model.to(cuda), g, cuda, convs)
    util.assert_parity(h, rh, [12, 5], TOL, 'eps_h')
    if convs == 0:
        assert float(x.abs().max()) == 0.0                     # ligand vectors start at zero: nothing to gate
    else:
        util.assert_parity(x, rx, [12, 5], TOL, 'eps_x')


def _fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gvp_wide.npz'))


FIXTURE_CFG = dict(vector_size=16, n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4, ll_k=0, kl_k=7, dropout=0.0)


@pytest.mark.parametrize('tag', ['s320_kp', 's320_mean', 's512_kp', 's512_mean'])
def test_upstream_fixture_parity(cuda, tag):
    """One forward against upstream's own GVP sub-modules in float64 (make_gvp_wide_golden.py): the [s_src | rbf | |Vh|] column
    order of the message head and the GVPLayerNorm placement are upstream's, not only the project oracle's."""
    z = _fixture()
    n_rec, n_lig = [int(v) for v in z['n_rec']], [int(v) for v in z['n_lig']]
    g = util.fixed_encode(util.make_batch(n_rec, n_lig, seed=int(z['batch_seed'])), n_vec=16)
    g.nodes['kp'].data['v_0'] = torch.tensor(z['kp_v'])
    ob = util.to_obatch(g)
    for got, key in ((ob.x['lig'], 'lig_x'), (ob.h['lig'], 'lig_h'), (ob.x['kp'], 'kp_x'), (ob.h['kp'], 'kp_h'),
                     (ob.edges['kk'][0], 'kk_src'), (ob.edges['kk'][1], 'kk_dst')):
        assert np.array_equal(got.numpy(), z[key]), key                    # the stored inputs are the ones rebuilt here
    S = 320 if tag.startswith('s320') else 512
    over = dict(n_convs=2, update_kp=True, message_norm=10.0) if tag.endswith('_kp') else \
        dict(n_convs=1, update_kp=False, message_norm='mean')
    model = _model(dict(FIXTURE_CFG, n_hidden_scalars=S, **over), seed=int(z[f'{tag}_seed'])).to(cuda)
    gd = g.to(cuda)
    with torch.no_grad():
        h, x = model(gd, torch.tensor(z['t'], device=cuda), None)
        c = model.engine().last_counts()
    torch.cuda.synchronize()
    assert (c['E_ll'], c['E_kl']) == (len(z[f'{tag}_ll_src']), len(z[f'{tag}_kl_src']))
    util.assert_parity(h.cpu(), torch.tensor(z[f'{tag}_eps_h']).float(), n_lig, TOL, 'eps_h')
    util.assert_parity(x.cpu(), torch.tensor(z[f'{tag}_eps_x']).float(), n_lig, TOL, 'eps_x')


def test_repeat_and_batch_invariance_bitwise(cuda):
    """A forward repeated gives the same bits, and every complex alone gives the bits it gets inside the batch (kl_k = 1: E_kl = 129
    alone, 385 in the batch; node and edge counts that are not multiples of 4 or of the GEMM tiles)."""
    n_rec, n_lig = [129, 200, 56], [9, 17, 5]
    cfg = dict(BASE, n_hidden_scalars=384, kl_k=1)
    model = _model(cfg).to(cuda)
    gs = synth.synth_complexes(n_rec, n_lig, 20, CUT, seed=1234)
    g = util.fixed_encode(G.batch(gs), n_vec=16).to(cuda)
    t = torch.tensor([0.2, 0.5, 0.8], device=cuda)
    with torch.no_grad():
        h, x = model(g, t, None)
        h2, x2 = model(g, t, None)
        assert torch.equal(h, h2) and torch.equal(x, x2)
        assert model.engine().last_counts()['E_kl'] == 385
        off = 0
        for i, nl in enumerate(n_lig):
            g1 = util.fixed_encode(G.batch([synth.synth_complexes(n_rec, n_lig, 20, CUT, seed=1234)[i]]), n_vec=16).to(cuda)
            h1, x1 = model(g1, t[i:i + 1], None)
            if i == 0:
                assert model.engine().last_counts()['E_kl'] == 129
            assert torch.equal(h1, h[off:off + nl]) and torch.equal(x1, x[off:off + nl]), i
            off += nl


def _diffusion(S, learned=False, T=10):
    dyn = dict(BASE, n_hidden_scalars=S, message_norm='mean')
    if learned:
        rec_cfg = {k: v for k, v in RECENC_CFGS['recenc_mean'].items() if k not in ('in_scalar_size', 'n_keypoints')}
        m = KeypointDiffusion(10, 128, None, n_timesteps=T, architecture='gvp', rec_encoder_type='learned',
                              graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dyn,
                              rec_encoder_config=dict(rec_cfg, in_scalar_size=10), precision=1e-5)
    else:
        m = KeypointDiffusion(10, 10, None, n_timesteps=T, architecture='gvp', rec_encoder_type='fixed',
                              graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dyn,
                              rec_encoder_config={'vector_size': 16}, precision=1e-5)
    synth.fill_state_dict_(m, 13)
    return m.eval()


def _pocket_batch(model, n_rec, n_lig, seed, cuda=None):
    g = G.batch(synth.synth_complexes(n_rec, n_lig, 20, CUT, seed=seed))
    return model.encode_receptors(g.to(cuda) if cuda is not None else g)


@pytest.mark.parametrize('learned', [False, True])
def test_reverse_steps_match_oracle(cuda, learned):
    """Ten reverse steps at n_hidden_scalars = 512 with fixed per-step noise against the oracle's sample_step chain, with the fixed
    encoder and with the learned GVP keypoint encoder (keypoints encoded once, as the sampler does; its widths stay 128)."""
    T = 10
    model = _diffusion(512, learned=learned, T=T).to(cuda)
    with torch.no_grad():
        gd = _pocket_batch(model, [90, 140], [11, 17], 3, cuda)
    ob = util.to_obatch(gd)
    sd = {k[len('dynamics.'):]: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.startswith('dynamics.')}
    ocfg = dict(BASE, n_hidden_scalars=512, message_norm='mean', graph_cutoffs=CUT)
    gen = torch.Generator().manual_seed(1)
    noise = [(torch.randn(ob.x['lig'].shape, generator=gen), torch.randn(ob.h['lig'].shape, generator=gen)) for _ in range(T)]
    table = odiff.gamma_table(T, 1e-5)
    ones = torch.ones(2)
    for i, sidx in enumerate(range(T - 1, -1, -1)):
        s, t = ones * (sidx / T), ones * ((sidx + 1) / T)
        eh, ex = ogvp.gvp_dynamics_forward(sd, ocfg, ob, t)
        ob = odiff.sample_step(ob.clone(), eh, ex, s, t, table, T, *noise[i])
        with torch.no_grad():
            model.sample_p_zs_given_zt(s.to(cuda), t.to(cuda), gd, G.get_batch_idxs(gd), noise=tuple(n.to(cuda) for n in noise[i]))
    torch.cuda.synchronize()
    assert util.rel_err(gd.nodes['lig'].data['x_0'], ob.x['lig']) < 1e-3
    assert util.rel_err(gd.nodes['lig'].data['h_0'], ob.h['lig']) < 1e-3


@pytest.mark.parametrize('learned', [False, True])
def test_step_graph_and_sampling(cuda, learned):
    """At n_hidden_scalars = 512 the captured reverse step (StepGraph) equals the eager step bit for bit for several timesteps, with
    the fixed and with the learned GVP keypoint encoder; sampling runs end to end with both."""
    T = 10
    model = _diffusion(512, learned=learned, T=T).to(cuda)
    with torch.no_grad():
        g1 = _pocket_batch(model, [60, 45], [9, 13], 5, cuda)
        g2 = _pocket_batch(model, [60, 45], [9, 13], 5, cuda)
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
        pos, feat = model.sample_given_pocket(pocket, torch.tensor([6, 9]), diff_batch_size=2)
    assert [p.shape for p in pos] == [(6, 3), (9, 3)] and all(torch.isfinite(p).all() for p in pos)


def test_refusals_name_the_limits(cuda, monkeypatch):
    with pytest.raises(ValueError, match='1 .. 1024'):
        LigRecDynamicsGVP(10, 10, n_hidden_scalars=1025, graph_cutoffs=CUT, update_kp=True, kl_k=5)
    g = _batch([40], [5], 17)
    with torch.no_grad(), pytest.raises(hip.KpdError, match='vector_size=17'):
        _model(dict(BASE, n_hidden_scalars=512, vector_size=17)).to(cuda)(g.to(cuda), torch.tensor([0.5], device=cuda), None)
    cfg = dict(BASE, n_hidden_scalars=512, n_convs=1, update_kp=False)
    g = _batch([40], [5], 16).to(cuda)
    model = _model(cfg).to(cuda)
    t = torch.tensor([0.5], device=cuda)
    with pytest.raises(hip.KpdError, match='training above 256 is not implemented'):
        model(g, t, None)                                           # grad enabled, parameters require grad
    with pytest.raises(hip.KpdError, match='kpd_gvp_profile'):
        model.engine().profile(True)
    model.gemm_mode = 'f16x2'
    with torch.no_grad(), pytest.raises(hip.KpdError, match='f16x2'):
        model(g, t, None)
    monkeypatch.setenv('KPD_GEMM', 'f16x2')
    model = _model(cfg).to(cuda)
    with torch.no_grad():
        h, _ = model(g, t, None)
    assert model.engine().gemm_mode() == 'f32' and torch.isfinite(h).all()
