"""`KeypointDiffusion.forward` with the receptor-ligand hinge term (rl_dist_threshold > 0, models/ligand_diffuser.py:44-49, 109-112,
137-156): its value against a float64 restatement of upstream's steps (per-complex loop, exact-difference cdist), its parameter
gradients against the chain rule through eps_x_pred and against central finite differences, the fixed encoder's differentiable zero,
the unchanged path at threshold 0, and a few optimizer steps that pull the denoised ligands out of the pocket atoms."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import optim, synth
from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion

from . import util
from .golden.make_golden_cfgs import same_res_feature

pytestmark = pytest.mark.gpu
CUT = util.CUTOFFS_ALL_ATOM
T = 50
THR = 4.0
N_REC, N_LIG = [60, 45, 52], [14, 20, 12]


def _egnn_learned(cuda, thr=THR):
    rec_cfg = dict(coords_range=10, fix_pos=False, hidden_n_node_feat=64, k_closest=4, kp_feat_scale=1.0, kp_rad=0.0, message_norm=0.0,
                   n_convs=2, n_kk_convs=0, n_kk_heads=4, no_cg=False, norm=True, out_n_node_feat=64, use_sameres_feat=True, use_tanh=True,
                   in_n_node_feat=10)
    cut = dict(CUT, kl=8, ll=5)
    kw = dict(rl_dist_threshold=thr) if thr is not None else {}
    m = KeypointDiffusion(10, 64, None, n_timesteps=T, architecture='egnn', rec_encoder_type='learned',
                          graph_config=dict(n_keypoints=8, graph_cutoffs=cut), dynamics_config=dict(util.EGNN_C2, n_layers=2, message_norm=0.0),
                          rec_encoder_config=rec_cfg, rec_encoder_loss_config=dict(loss_type='optimal_transport'), precision=1e-5, **kw)
    synth.fill_state_dict_(m, 3)

    def mk():
        g = G.batch(synth.synth_complexes(N_REC, N_LIG, 8, cut, seed=11))
        s, d = g.edges(etype='rr')
        g.edges['rr'].data['same_res'] = same_res_feature(s, d).bool()
        return g.to(cuda)
    return m.to(cuda).eval(), mk


def _gvp_learned(cuda, thr=THR):
    from .test_gvp_gpu import GVP_40KP
    rec_cfg = dict(out_scalar_size=128, n_message_gvps=2, n_update_gvps=1, vector_size=16, n_rr_convs=2, n_rk_convs=2, message_norm=10.0,
                   k_closest=4, kp_rad=0, dropout=0.0, in_scalar_size=10)
    cut = dict(CUT, kl=8, ll=6.0)
    m = KeypointDiffusion(10, 128, None, n_timesteps=T, architecture='gvp', rec_encoder_type='learned',
                          graph_config=dict(n_keypoints=8, graph_cutoffs=cut), dynamics_config=dict(GVP_40KP, n_convs=2, dropout=0.0),
                          rec_encoder_config=rec_cfg, rec_encoder_loss_config=dict(loss_type='optimal_transport'), precision=1e-5,
                          rl_dist_threshold=thr)
    synth.fill_state_dict_(m, 3)
    return m.to(cuda).eval(), lambda: G.batch(synth.synth_complexes(N_REC, N_LIG, 8, cut, seed=11)).to(cuda)


def _egnn_fixed(cuda, thr=THR):
    kw = dict(rl_dist_threshold=thr) if thr is not None else {}
    m = KeypointDiffusion(10, 10, None, n_timesteps=T, architecture='egnn', rec_encoder_type='fixed',
                          graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dict(util.EGNN_C2, n_layers=2),
                          precision=1e-5, **kw)
    synth.fill_state_dict_(m, 3)
    return m.to(cuda).eval(), lambda: G.batch(synth.synth_complexes(N_REC, N_LIG, 20, CUT, seed=11)).to(cuda)


def _seed(cuda):
    """A seed whose timestep draw (the first draw of the training step on the GPU generator) is small for every complex, so the
    denoised ligands lie inside their pockets and the hinge has many active pairs."""
    for s in range(200):
        torch.manual_seed(s)
        if int(torch.randint(0, T, size=(len(N_REC),), device=cuda).max()) <= T // 5:
            return s
    raise AssertionError('no seed with small timesteps')


def _forward(model, mk, seed, with_grad):
    """One forward under `seed`, with the tensors the restatement needs: receptor atoms and keypoints after the encoder, the noised
    ligand and keypoints the denoiser sees, its timesteps and its eps_x prediction."""
    cap = {}

    def enc_hook(mod, inp, out):
        cap['rec'] = out.nodes['rec'].data['x_0'].detach().clone()
        cap['kp0'] = out.nodes['kp'].data['x_0'].detach().clone()
        cap['n_rec'] = out.batch_num_nodes('rec').cpu()
        cap['n_kp'] = out.batch_num_nodes('kp').cpu()

    def dyn_hook(mod, inp, out):
        g, t = inp[0], inp[1]
        cap['z'] = g.nodes['lig'].data['x_0'].detach().clone()
        cap['kp2'] = g.nodes['kp'].data['x_0'].detach().clone()
        cap['n_lig'] = g.batch_num_nodes('lig').cpu()
        cap['t'] = t.detach().clone()
        cap['eps_x'] = out[1]

    hs = [model.rec_encoder.register_forward_hook(enc_hook), model.dynamics.register_forward_hook(dyn_hook)]
    try:
        torch.manual_seed(seed)
        with torch.enable_grad() if with_grad else torch.no_grad():
            out = model(mk(), None)
    finally:
        for h in hs:
            h.remove()
    return out, cap


def _restate(model, cap, thr):
    """Upstream's steps 3-4 in float64, one complex at a time: x_hat = (z - sigma_t eps) / alpha_t, minus the current keypoint mean,
    plus the keypoint mean after the encoder, then DistanceHingeLoss against the receptor atoms.  Returns (loss, dL/d eps [N,3]
    float32, active pairs)."""
    eps = cap['eps_x'].detach().double().cpu().requires_grad_(True)
    gamma = model.gamma(cap['t']).double().cpu()
    alpha, sigma = torch.sqrt(torch.sigmoid(-gamma)), torch.sqrt(torch.sigmoid(gamma))
    z, kp2, kp0, rec = (cap[k].double().cpu() for k in ('z', 'kp2', 'kp0', 'rec'))
    loss, active = torch.zeros((), dtype=torch.float64), 0
    lo = ko = ro = 0
    for b in range(len(cap['n_lig'])):
        nl, nk, nr = int(cap['n_lig'][b]), int(cap['n_kp'][b]), int(cap['n_rec'][b])
        x_hat = (z[lo:lo + nl] - sigma[b] * eps[lo:lo + nl]) / alpha[b]
        x_hat = x_hat - kp2[ko:ko + nk].mean(0) + kp0[ko:ko + nk].mean(0)
        r = rec[ro:ro + nr]
        if nr:
            d = torch.cdist(x_hat, r, compute_mode='donot_use_mm_for_euclid_dist')
            loss = loss + torch.max(thr - d, torch.zeros_like(d)).sum()
            active += int((d < thr).sum())
        lo, ko, ro = lo + nl, ko + nk, ro + nr
    if loss.requires_grad:
        loss.backward()
    g = eps.grad if eps.grad is not None else torch.zeros_like(eps)
    return float(loss.detach()), g.float(), active


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('setup', ['egnn_learned', 'gvp_learned'])
def test_value_chain_and_finite_differences(cuda, setup):
    model, mk = {'egnn_learned': _egnn_learned, 'gvp_learned': _gvp_learned}[setup](cuda)
    seed = _seed(cuda)
    out, cap = _forward(model, mk, seed, True)
    assert set(out) == {'l2', 'pos', 'feat', 'rec_encoder', 'rl_hinge'}
    ref, G_eps, active = _restate(model, cap, THR)
    got = float(out['rl_hinge'].detach())
    print(f'{setup}: rl_hinge {got:.6f} restated {ref:.6f}, {active} active pairs')
    assert active >= 300
    assert abs(got - ref) <= 2e-5 * ref, (got, ref)

    # chain rule: rl_hinge.backward() == eps_x_pred.backward(dL/d eps) for every parameter, encoder included (the keypoint
    # terms of the frame shift cancel, so eps_x_pred is the only way in)
    out['rl_hinge'].backward()
    g_hinge = _grads(model)
    model.zero_grad(set_to_none=True)
    out2, cap2 = _forward(model, mk, seed, True)
    assert torch.equal(cap2['eps_x'].detach(), cap['eps_x'].detach())
    cap2['eps_x'].backward(G_eps.to(cuda))
    g_chain = _grads(model)
    model.zero_grad(set_to_none=True)
    assert set(g_hinge) == set(g_chain) and any(n.startswith('rec_encoder.') for n in g_hinge)
    for n, ref_g in g_chain.items():
        scale = float(ref_g.abs().max())
        assert float((g_hinge[n] - ref_g).abs().max()) <= 1e-4 * scale + 1e-12, n

    # central finite differences of the term alone along random directions, for the two denoiser tensors and the encoder tensor
    # with the largest gradients (one tensor at a time, inference engines for the perturbed evaluations; each perturbed value is
    # the float64 restatement of the product's eps_x prediction, so the fp32 rounding of the summed loss does not swamp the
    # difference).  The encoder reaches the term only through the keypoints the denoiser sees.
    params = dict(model.named_parameters())
    by_norm = lambda prefix: sorted((n for n in g_hinge if n.startswith(prefix)), key=lambda n: -float(g_hinge[n].norm()))
    pick = by_norm('dynamics.')[:2] + by_norm('rec_encoder.')[:1]
    gen = torch.Generator().manual_seed(3)
    strong = 0
    for n in pick:
        d = torch.randn(params[n].shape, generator=gen).to(cuda)
        analytic = float((g_hinge[n].double() * d.double()).sum())
        numeric = []
        for h in (1e-3, 3e-4):
            vals = []
            with torch.no_grad():
                for sign in (1.0, -1.0):
                    params[n].add_(sign * h * d)
                    vals.append(_restate(model, _forward(model, mk, seed, False)[1], THR)[0])
                    params[n].sub_(sign * h * d)
            numeric.append((vals[0] - vals[1]) / (2 * h))
        print(f'{n}: analytic {analytic:+.5e} numeric {numeric[0]:+.5e} {numeric[1]:+.5e}')
        assert min(abs(analytic - v) - 5e-2 * max(abs(analytic), abs(v)) for v in numeric) <= 1e-3, (n, analytic, numeric)
        strong += abs(analytic) > 0.05
    assert strong >= 2


def test_fixed_encoder_term_is_a_differentiable_zero(cuda):
    model, mk = _egnn_fixed(cuda)
    seed = _seed(cuda)
    out, cap = _forward(model, mk, seed, True)
    assert 'rl_hinge' in out and float(out['rl_hinge'].detach()) == 0.0 and out['rl_hinge'].requires_grad
    assert cap['rec'].shape[0] == 0
    (out['l2'] + 2.0 * out['rl_hinge']).backward()
    with_term = _grads(model)
    model.zero_grad(set_to_none=True)
    out2, _ = _forward(model, mk, seed, True)
    out2['l2'].backward()
    alone = _grads(model)
    assert torch.equal(out['l2'], out2['l2'])
    assert set(with_term) == set(alone) and all(torch.equal(with_term[n], alone[n]) for n in alone)


@pytest.mark.parametrize('build', [_egnn_fixed, _egnn_learned])
def test_threshold_zero_is_todays_path(cuda, build):
    m0, mk = build(cuda, thr=0)
    m_default, _ = build(cuda, thr=None)
    seed = _seed(cuda)
    a, _ = _forward(m0, mk, seed, False)
    b, _ = _forward(m_default, mk, seed, False)
    assert 'rl_hinge' not in a and set(a) == set(b) == {'l2', 'pos', 'feat', 'rec_encoder'}
    for k in ('l2', 'pos', 'feat'):
        assert torch.equal(a[k], b[k]), k


def test_adam_steps_lower_the_hinge(cuda):
    model, mk = _egnn_learned(cuda)
    model.train()
    opt = optim.Adam(model.parameters(), lr=1e-3)
    seed = _seed(cuda)
    totals, actives = [], []
    for it in range(6):
        out, cap = _forward(model, mk, seed, True)
        total = out['l2'] + 1.0 * out['rl_hinge']
        actives.append(_restate(model, cap, THR)[2])
        opt.zero_grad(set_to_none=True)
        total.backward()
        opt.step()
        totals.append(float(total.detach()))
    print('totals', totals, 'active pairs', actives)
    assert all(v == v for v in totals) and totals[-1] < totals[0] and actives[-1] < actives[0], (totals, actives)
