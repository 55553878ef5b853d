"""Every width a trainer accepts also runs for inference: the EGNN denoiser at rec_nf 129 .. 255, with the identity keypoint encoder
below hidden_nf 256 and at atom_nf 33 .. 256; the GVP denoiser at n_lig_scalars 65 .. 255; the GVP keypoint encoder at any
out_scalar_size / in_scalar_size up to 256.  Limits agree (eval runs wherever training runs), oracle parity, train / eval agreement,
a complex alone and batched, and train-then-sample through KeypointDiffusion."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip, synth
from keypoint_diffusion_amd.dynamics import LigRecDynamics
from keypoint_diffusion_amd.dynamics_gvp import LigRecDynamicsGVP
from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
from keypoint_diffusion_amd.optim import Adam
from keypoint_diffusion_amd.receptor_encoder_gvp import ReceptorEncoderGVP
from oracle import egnn as oegnn
from oracle import gvp as ogvp
from oracle import rec_encoder as orec

from . import util
from .golden.make_golden_cfgs import GVP_CFGS, RECEGNN_CFGS, RECENC_CFGS, same_res_feature

pytestmark = pytest.mark.gpu
CUT = util.CUTOFFS_ALL_ATOM
TOL = 1e-4
EGNN = dict(util.EGNN_C2, n_layers=2)
GVP = dict(GVP_CFGS['gvp_norm0'], n_hidden_scalars=256)
RECENC = dict(RECENC_CFGS['recenc_norm10'], n_rr_convs=2)


def _t(B):
    return (torch.arange(B, dtype=torch.float32) + 1) / (B + 1)


def _lig_feats(g, width, seed=4):
    g.nodes['lig'].data['h_0'] = torch.randn(g.num_nodes('lig'), width, generator=torch.Generator().manual_seed(seed))
    return g


def _egnn(atom_nf, rec_nf, hidden_nf, seed=3):
    m = LigRecDynamics(atom_nf, rec_nf, graph_cutoffs=CUT, **dict(EGNN, hidden_nf=hidden_nf))
    synth.fill_state_dict_(m, seed)
    return m


def _egnn_batch(atom_nf, rec_nf, n_rec=(50, 30), n_lig=(8, 5), seed=5):
    gs = synth.synth_complexes(list(n_rec), list(n_lig), 20, CUT, seed=seed, n_rec_feat=rec_nf)
    return _lig_feats(util.fixed_encode(G.batch(gs)), atom_nf)


def _gvp(n_lig, S, seed=7):
    m = LigRecDynamicsGVP(n_lig, 10, graph_cutoffs=CUT, **dict(GVP, n_hidden_scalars=S))
    synth.fill_state_dict_(m, seed)
    return m


def _gvp_batch(n_lig_feat, n_rec=(26, 19), n_lig=(7, 10), seed=31):
    g = util.fixed_encode(util.make_batch(list(n_rec), list(n_lig), seed=seed), n_vec=16)
    g.nodes['kp'].data['v_0'] = 0.5 * torch.randn(g.num_nodes('kp'), 16, 3, generator=torch.Generator().manual_seed(3))
    return _lig_feats(g, n_lig_feat)


def _recenc(out_s, in_s, seed=61):
    return synth.fill_state_dict_(ReceptorEncoderGVP(**dict(RECENC, out_scalar_size=out_s, in_scalar_size=in_s, graph_cutoffs=CUT)), seed)


def _recenc_batch(in_s, n_rec=(33, 21), seed=17):
    return util.make_batch(list(n_rec), [4] * len(n_rec), seed=seed, n_keypoints=RECENC['n_keypoints'], n_rec_feat=in_s)


def _train_then_eval(model, make, fwd):
    """The grad-enabled forward (training engine), then the eval forward (inference engine) on the same weights.  Each forward gets
    its own copy of the batch from `make()`, and its outputs `fwd(model, batch)` are cloned at once: an encoder writes its outputs
    into the graph it was given and returns that graph."""
    model = model.cuda().train()
    tr = {k: v.detach().clone() for k, v in fwd(model, make()).items()}
    model.eval()
    with torch.no_grad():
        ev = {k: v.clone() for k, v in fwd(model, make()).items()}
    torch.cuda.synchronize()
    return tr, ev


def _denoise(t):
    return lambda model, g: dict(zip(('eps_h', 'eps_x'), model(g, t, None)))


def _encode(model, g):
    kp = model(g, G.get_batch_idxs(g)).nodes['kp'].data
    return {k: kp[k] for k in ('x_0', 'h_0', 'v_0')}


# ---- limits agree, and eval matches the trainer's forward --------------------------------------------------------------------------
EGNN_GRID = ([(10, r, 256) for r in (1, 128, 129, 192, 255, 256)] + [(10, h, h) for h in (7, 100, 255)] +
             [(a, 10, 256) for a in (32, 33, 100, 256)])


@pytest.mark.parametrize('atom_nf,rec_nf,hidden_nf', EGNN_GRID)
def test_egnn_eval_runs_wherever_training_runs(cuda, atom_nf, rec_nf, hidden_nf):
    model = _egnn(atom_nf, rec_nf, hidden_nf)
    tr, ev = _train_then_eval(model, lambda: _egnn_batch(atom_nf, rec_nf).to(cuda), _denoise(_t(2).to(cuda)))
    assert ev['eps_h'].shape == (13, atom_nf)
    for k in ('eps_h', 'eps_x'):
        assert torch.isfinite(ev[k]).all(), k
        util.assert_parity(ev[k], tr[k], tol=TOL, what=f'{k} eval vs train')


@pytest.mark.parametrize('n_lig', [64, 65, 255])
def test_gvp_eval_runs_wherever_training_runs(cuda, n_lig):
    model = _gvp(n_lig, 256)
    tr, ev = _train_then_eval(model, lambda: _gvp_batch(n_lig).to(cuda), _denoise(_t(2).to(cuda)))
    assert ev['eps_h'].shape == (17, n_lig)
    for k in ('eps_h', 'eps_x'):
        assert torch.isfinite(ev[k]).all(), k
        util.assert_parity(ev[k], tr[k], tol=TOL, what=f'{k} eval vs train')


@pytest.mark.parametrize('n_lig', [65, 255])
def test_gvp_wide_eval_at_new_lig_widths(cuda, n_lig):
    """S = 320: training stays refused, the eval forward runs."""
    model = _gvp(n_lig, 320).cuda().eval()
    gd = _gvp_batch(n_lig).to(cuda)
    with torch.no_grad():
        eh, ex = model(gd, _t(2).to(cuda), None)
    assert eh.shape == (gd.num_nodes('lig'), n_lig) and torch.isfinite(eh).all() and torch.isfinite(ex).all()


@pytest.mark.parametrize('out_s,in_s', [(o, 10) for o in (16, 64, 100, 129, 192, 255)] + [(128, i) for i in (64, 65, 256)])
def test_recenc_eval_runs_wherever_training_runs(cuda, out_s, in_s):
    model = _recenc(out_s, in_s)
    tr, ev = _train_then_eval(model, lambda: _recenc_batch(in_s).to(cuda), _encode)
    assert ev['h_0'].shape == (2 * RECENC['n_keypoints'], out_s)
    for k in ('x_0', 'h_0', 'v_0'):
        assert torch.isfinite(ev[k]).all(), k
        util.assert_parity(ev[k], tr[k], tol=TOL, what=f'kp {k} eval vs train', atol_rel=1e-5 if k == 'v_0' else 1e-6)


# ---- oracle parity, one case per new width ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('atom_nf,rec_nf,hidden_nf', [(10, 192, 256), (10, 100, 100), (40, 10, 256), (40, 10, 384)])
def test_egnn_oracle_parity(cuda, atom_nf, rec_nf, hidden_nf):
    model = _egnn(atom_nf, rec_nf, hidden_nf).eval()
    g = _egnn_batch(atom_nf, rec_nf, n_rec=(90, 40, 7), n_lig=(12, 5, 3))
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    ref_h, ref_x = oegnn.egnn_dynamics_forward(sd, dict(EGNN, hidden_nf=hidden_nf, graph_cutoffs=CUT), util.to_obatch(g), _t(3))
    model = model.to(cuda)
    with torch.no_grad():
        h, x = model(g.to(cuda), _t(3).to(cuda), None)
    counts = g.batch_num_nodes('lig')
    util.assert_parity(h, ref_h, counts, TOL, 'eps_h')
    util.assert_parity(x, ref_x, counts, TOL, 'eps_x')


@pytest.mark.parametrize('S', [256, 384])
def test_gvp_oracle_parity(cuda, S):
    model = _gvp(100, S).eval()
    g = _gvp_batch(100, n_rec=(40, 19, 60), n_lig=(9, 4, 12))
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    ref_h, ref_x = ogvp.gvp_dynamics_forward(sd, dict(GVP, n_hidden_scalars=S, graph_cutoffs=CUT), util.to_obatch(g), _t(3))
    model = model.to(cuda)
    with torch.no_grad():
        h, x = model(g.to(cuda), _t(3).to(cuda), None)
    counts = g.batch_num_nodes('lig')
    util.assert_parity(h, ref_h, counts, TOL, 'eps_h')
    util.assert_parity(x, ref_x, counts, TOL, 'eps_x')


@pytest.mark.parametrize('out_s', [64, 192])
def test_recenc_oracle_parity(cuda, out_s):
    model = _recenc(out_s, 100).eval()
    g = _recenc_batch(100, n_rec=(50, 3, 27))
    kw = dict(RECENC, out_scalar_size=out_s, in_scalar_size=100, graph_cutoffs=CUT)
    ref = orec.rec_encoder_gvp_forward({k: v.clone() for k, v in model.state_dict().items()}, kw, util.to_obatch(g))
    model = model.to(cuda)
    with torch.no_grad():
        out = model(g.to(cuda), G.get_batch_idxs(g.to(cuda)))
    kp = out.nodes['kp'].data
    assert kp['h_0'].shape == ref.h['kp'].shape
    util.assert_parity(kp['x_0'], ref.x['kp'], tol=TOL, what='kp x')
    util.assert_parity(kp['h_0'], ref.h['kp'], tol=TOL, what='kp h')
    # the vectors leave a GVPLayerNorm: entries near zero carry the absolute error of the whole row (test_recenc_gpu.py judges
    # them by the whole-tensor measure alone)
    util.assert_parity(kp['v_0'], ref.v['kp'], tol=TOL, what='kp v', atol_rel=1e-5)
    rs, rd = out.edges(etype='rk')
    assert torch.equal(rs.cpu(), ref.edges['rk'][0]) and torch.equal(rd.cpu(), ref.edges['rk'][1])


# ---- a complex alone and inside a batch -------------------------------------------------------------------------------------------
# The new widths run on the engines' fused kernels (hidden width <= 256), whose edge tiles span complexes: a complex's sums are split
# where the tiles fall, so alone and batched agree to rounding, not bit for bit (bitwise batch invariance is a property of the wide
# paths, test_egnn_wide_gpu.py / test_gvp_wide_gpu.py).  A repeat of the same batch gives the same bits.
def test_recenc_alone_and_batched(cuda):
    model = _recenc(96, 10).to(cuda).eval()
    n_rec, K = [40, 9, 25], RECENC['n_keypoints']
    gs = synth.synth_complexes(n_rec, [4] * 3, K, CUT, seed=17, n_rec_feat=10)
    with torch.no_grad():
        full = {k: v.clone() for k, v in _encode(model, G.batch(gs).to(cuda)).items()}
        again = _encode(model, G.batch(gs).to(cuda))
        for i in range(len(n_rec)):
            one = _encode(model, G.batch([gs[i]]).to(cuda))
            for k in ('x_0', 'h_0', 'v_0'):
                assert torch.equal(full[k], again[k]), k
                util.assert_parity(one[k], full[k][i * K:(i + 1) * K], tol=TOL, what=f'complex {i} {k}', atol_rel=1e-5)


def test_egnn_alone_and_batched(cuda):
    model = _egnn(10, 192, 256).to(cuda).eval()
    n_rec, n_lig = [60, 35, 48], [9, 14, 6]
    gs = synth.synth_complexes(n_rec, n_lig, 20, CUT, seed=8, n_rec_feat=192)
    t = _t(3).to(cuda)
    with torch.no_grad():
        g = util.fixed_encode(G.batch(gs)).to(cuda)
        h, x = model(g, t, None)
        h2, x2 = model(g, t, None)
        assert torch.equal(h, h2) and torch.equal(x, x2)
        off = 0
        for i in range(3):
            gi = util.fixed_encode(G.batch([gs[i]])).to(cuda)
            hi, xi = model(gi, t[i:i + 1], None)
            util.assert_parity(hi, h[off:off + n_lig[i]], tol=TOL, what=f'complex {i} eps_h')
            util.assert_parity(xi, x[off:off + n_lig[i]], tol=TOL, what=f'complex {i} eps_x')
            off += n_lig[i]


# ---- f16x2 at a new width is refused with the width in the message ------------------------------------------------------------------
def test_f16x2_refused_at_new_widths(cuda):
    g = _egnn_batch(40, 10).to(cuda)
    model = _egnn(40, 10, 256).to(cuda).eval()
    model.gemm_mode = 'f16x2'
    with torch.no_grad(), pytest.raises(hip.KpdError, match='atom_nf = 40'):
        model(g, _t(2).to(cuda), None)
    g = _gvp_batch(100).to(cuda)
    model = _gvp(100, 256).to(cuda).eval()
    model.gemm_mode = 'f16x2'
    with torch.no_grad(), pytest.raises(hip.KpdError, match='n_lig_scalars = 100'):
        model(g, _t(2).to(cuda), None)


# ---- train, then sample ------------------------------------------------------------------------------------------------------------
def _diffusion(kind):
    T = 10
    if kind == 'gvp':
        rec = {k: v for k, v in RECENC_CFGS['recenc_norm10'].items() if k not in ('in_scalar_size', 'n_keypoints')}
        m = KeypointDiffusion(10, 64, None, n_timesteps=T, architecture='gvp', rec_encoder_type='learned',
                              graph_config=dict(n_keypoints=5, graph_cutoffs=CUT), dynamics_config=dict(GVP_CFGS['gvp_norm0']),
                              rec_encoder_config=dict(rec, in_scalar_size=10, out_scalar_size=64), precision=1e-5)
    else:
        D = 192 if kind == 'egnn192' else 100
        rec = {k: v for k, v in RECEGNN_CFGS['recegnn_20kp'].items() if k not in ('in_n_node_feat', 'n_keypoints', 'out_n_node_feat')}
        rec['n_convs'] = 2
        dyn = dict(EGNN, hidden_nf=256 if kind == 'egnn192' else 100)
        m = KeypointDiffusion(10, D, None, n_timesteps=T, architecture='egnn', rec_encoder_type='learned',
                              graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dyn,
                              rec_encoder_config=dict(rec, in_n_node_feat=10, out_n_node_feat=D), precision=1e-5)
    synth.fill_state_dict_(m, 13)
    return m


def _complexes(kind, n_rec, n_lig, seed):
    gs = synth.synth_complexes(n_rec, n_lig, 5 if kind == 'gvp' else 20, CUT, seed=seed)
    if kind != 'gvp':
        for gg in gs:
            s, d = gg.edges(etype='rr')
            gg.edges['rr'].data['same_res'] = same_res_feature(s, d).bool()
    return gs


@pytest.mark.parametrize('kind', ['gvp', 'egnn192', 'egnn_identity100'])
def test_train_then_sample(cuda, kind):
    model = _diffusion(kind).to(cuda).train()
    opt = Adam(model.parameters(), lr=1e-4)
    gen = torch.Generator().manual_seed(0)
    for step in range(2):
        # a fresh batch per step: the keypoint encoders append the kk edges to the graph they are given
        gk = model.encode_receptors(G.batch(_complexes(kind, [40, 30], [7, 5], 3 + step)).to(cuda))
        t = torch.tensor([0.3, 0.7], device=cuda)
        eh, ex = model.dynamics(gk, t, G.get_batch_idxs(gk))
        loss = (eh - torch.randn(eh.shape, generator=gen).to(cuda)).square().mean() + ex.square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        g1 = model.encode_receptors(G.batch(_complexes(kind, [40, 30], [7, 5], 5)).to(cuda))
        g2 = model.encode_receptors(G.batch(_complexes(kind, [40, 30], [7, 5], 5)).to(cuda))
        nx = torch.randn(g1.num_nodes('lig'), 3, generator=gen).to(cuda)
        nh = torch.randn(g1.num_nodes('lig'), 10, generator=gen).to(cuda)
        sg = model.capture_step(g1, noise=(nx, nh))
        ones = torch.ones(2, device=cuda)
        for s in (9, 4):
            sg.step(s / 10, (s + 1) / 10)
            model.sample_p_zs_given_zt(ones * (s / 10), ones * ((s + 1) / 10), g2, noise=(nx, nh))
            for nt, k in (('lig', 'x_0'), ('lig', 'h_0'), ('kp', 'x_0')):
                assert torch.equal(g1.nodes[nt].data[k], g2.nodes[nt].data[k]), (s, nt, k)
        pocket = _complexes(kind, [60], [1], 9)[0].to(cuda)
        pocket.remove_nodes(pocket.nodes('lig'), ntype='lig')
        pos, feat = model.sample_given_pocket(pocket, torch.tensor([6, 9]), diff_batch_size=2)
    assert [p.shape for p in pos] == [(6, 3), (9, 3)] and all(torch.isfinite(p).all() for p in pos)
    assert [f.shape[0] for f in feat] == [6, 9] and all(torch.isfinite(f).all() for f in feat)
