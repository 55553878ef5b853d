"""Inpainting on the GPU: the fused update kernel around fixed atoms (kpd_sample_update_inpaint) and its re-noise mode against an
fp64 restatement of the algorithm of include/kpd.h written here, the bitwise guarantees (no fixed atom = the plain kernel;
independent of batch composition; repeatable), the coefficient kernel, an anchored step with a real denoiser, and the public
loop: frame bookkeeping, overwrite, determinism, resampling, captured step, sharded job."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip, synth
from keypoint_diffusion_amd.ligand_diffuser import InpaintContext, KeypointDiffusion
from oracle import egnn as oegnn

from . import util
from .test_gvp_gpu import GVP_ALL_ATOM
from .test_inpaint_config import oracle_coefficients
from .test_trajectory_gpu import CUT_DEV

pytestmark = pytest.mark.gpu
CUT = util.CUTOFFS_ALL_ATOM
N_LIG, N_KP = [1, 5, 90, 3], [20, 1, 65, 300]       # 3 * 90 and 5 * 90 exceed the 256 threads, 300 keypoints are strided over


# ---- the fp64 restatement (steps 1-5 of include/kpd.h, "Inpainting") ---------------------------------------------------
def ref_update(n_lig, n_kp, lig_x, lig_h, kp_x, eps_x, eps_h, nx, nh, coef6, fixed, X, Hn, com0, kx, kh):
    d = lambda t: t.detach().cpu().double()
    lig_x, lig_h, kp_x, eps_x, eps_h, nx, nh, coef6, X, Hn, com0, kx, kh = map(d, (lig_x, lig_h, kp_x, eps_x, eps_h, nx, nh, coef6, X, Hn,
                                                                                  com0, kx, kh))
    fixed = fixed.cpu().bool()
    ox, oh, ok, lo, ko = [], [], [], 0, 0
    for b, (nl, nk) in enumerate(zip(n_lig, n_kp)):
        L, K = slice(lo, lo + nl), slice(ko, ko + nk)
        a_ts, var, sg, a_s, s_s, _ = coef6[b]
        ux = lig_x[L] / a_ts - var * eps_x[L] + sg * nx[L]                        # 1. candidate
        uh = lig_h[L] / a_ts - var * eps_h[L] + sg * nh[L]
        k0 = (X[L] - com0[b]) + kp_x[K].mean(0)                                   # 2. frame
        k, kh_ = a_s * k0 + s_s * kx[L], a_s * Hn[L] + s_s * kh[L]                # 3. noised known part
        f = fixed[L][:, None]
        zx, zh = torch.where(f, k, ux), torch.where(f, kh_, uh)                   # 4. merge
        c = zx.mean(0)                                                            # 5. COM removal
        ox.append(zx - c), oh.append(zh), ok.append(kp_x[K] - c)
        lo, ko = lo + nl, ko + nk
    return torch.cat(ox), torch.cat(oh), torch.cat(ok)


def ref_renoise(n_lig, n_kp, lig_x, lig_h, kp_x, nx, nh, coef6):
    d = lambda t: t.detach().cpu().double()
    lig_x, lig_h, kp_x, nx, nh, coef6 = map(d, (lig_x, lig_h, kp_x, nx, nh, coef6))
    ox, oh, ok, lo, ko = [], [], [], 0, 0
    for b, (nl, nk) in enumerate(zip(n_lig, n_kp)):
        L, K = slice(lo, lo + nl), slice(ko, ko + nk)
        zx = coef6[b, 0] * lig_x[L] + coef6[b, 5] * nx[L]
        c = zx.mean(0)
        ox.append(zx - c), oh.append(coef6[b, 0] * lig_h[L] + coef6[b, 5] * nh[L]), ok.append(kp_x[K] - c)
        lo, ko = lo + nl, ko + nk
    return torch.cat(ox), torch.cat(oh), torch.cat(ok)


def _mask(pattern, n):
    return {0: torch.zeros(n, dtype=torch.bool), 1: torch.ones(n, dtype=torch.bool), 2: torch.arange(n) == n // 2,
            3: torch.arange(n) % 2 == 0}[pattern]


def _inputs(F, rotation, dev, seed=0):
    """State, denoiser output, draws and known part of one step for the shapes above.  The known positions sit ~100 A from the
    origin of the state frame, with kp_com0 to match, so (X - kp_com0) + m only works in that order."""
    gen = torch.Generator().manual_seed(100 * seed + 10 * F + rotation)
    r = lambda *s: torch.randn(*s, generator=gen)
    nl, nk = sum(N_LIG), sum(N_KP)
    kp_x = 6.0 * r(nk, 3) + torch.repeat_interleave(2.0 * r(4, 3), torch.tensor(N_KP), 0)
    m = torch.stack([p.mean(0) for p in kp_x.split(N_KP)])
    com0 = torch.tensor([[100.0, -80.0, 120.0]]) + 20.0 * r(4, 3)
    lig_b = torch.repeat_interleave(torch.arange(4), torch.tensor(N_LIG))
    X = 2.0 * r(nl, 3) - m[lig_b] + com0[lig_b]                  # about 2 A from the state origin, in the input frame
    _, _, table = oracle_coefficients(10, 1e-4)
    t = dict(lig_x=2.0 * r(nl, 3), lig_h=r(nl, F), kp_x=kp_x, eps_x=r(nl, 3), eps_h=r(nl, F), nx=r(nl, 3), nh=r(nl, F),
             coef6=table[[9, 0, 4, 7]].contiguous(), fixed=torch.cat([_mask((b + rotation) % 4, n) for b, n in enumerate(N_LIG)]),
             X=X, Hn=r(nl, F), com0=com0, kx=r(nl, 3), kh=r(nl, F))
    return {k: v.to(dev) for k, v in t.items()}


def _pb(n_lig, n_kp, dev):
    e = torch.zeros(0, dtype=torch.long)
    return hip.PreparedBatch(torch.tensor(n_lig), torch.tensor(n_kp), e, e, dev)


def _run(pb, F, t, rows=(slice(None), slice(None), slice(None))):
    """kpd_sample_update_inpaint on clones of the inputs `t` (restricted to the ligand rows / keypoint rows / complexes `rows`)."""
    L, K, Bs = rows
    x, h, k = t['lig_x'][L].clone(), t['lig_h'][L].clone(), t['kp_x'][K].clone()
    hip.sample_update_inpaint(pb, F, x, h, k, t['eps_x'][L], t['eps_h'][L], t['nx'][L], t['nh'][L], t['coef6'][Bs], t['fixed'][L],
                              t['X'][L], t['Hn'][L], t['com0'][Bs], t['kx'][L], t['kh'][L])
    return x, h, k


@pytest.mark.parametrize('F', [1, 5, 10])
def test_update_kernel_matches_fp64_restatement_and_bitwise_contracts(cuda, F):
    pb = _pb(N_LIG, N_KP, cuda)
    for rotation in range(4):                                    # every complex meets every mask: none, all, one atom, alternating
        t = _inputs(F, rotation, cuda)
        x, h, k = _run(pb, F, t)
        rx, rh, rk = ref_update(N_LIG, N_KP, t['lig_x'], t['lig_h'], t['kp_x'], t['eps_x'], t['eps_h'], t['nx'], t['nh'], t['coef6'],
                                t['fixed'], t['X'], t['Hn'], t['com0'], t['kx'], t['kh'])
        errs = (util.rel_err(x, rx), util.rel_err(h, rh), util.rel_err(k, rk))
        print(f'F={F} rotation={rotation}: rel err x {errs[0]:.2e} h {errs[1]:.2e} kp {errs[2]:.2e}')
        assert max(errs) < 1e-4, errs
        lx, lk = x.cpu().split(N_LIG), k.cpu().split(N_KP)
        for b in range(4):                                       # the ligand COM is gone, per complex, at the scale of its coordinates
            assert float(lx[b].mean(0).abs().max()) < 1e-5 * max(1.0, float(lx[b].abs().max()))
        # a second call on cloned inputs: the same bits
        x2, h2, k2 = _run(pb, F, t)
        assert torch.equal(x, x2) and torch.equal(h, h2) and torch.equal(k, k2)
        # the plain kernel on the same inputs: the complex without a fixed atom has its bits
        px, ph, pk = t['lig_x'].clone(), t['lig_h'].clone(), t['kp_x'].clone()
        hip.sample_update(pb, F, px, ph, pk, t['eps_x'], t['eps_h'], t['nx'], t['nh'], t['coef6'][:, :3].contiguous())
        free = (-rotation) % 4
        assert not bool(t['fixed'].cpu().split(N_LIG)[free].any())
        for got, plain, sizes in ((x, px, N_LIG), (h, ph, N_LIG), (k, pk, N_KP)):
            assert torch.equal(got.cpu().split(sizes)[free], plain.cpu().split(sizes)[free])
        # every complex alone: its rows of the batch
        lo, ko = 0, 0
        for b, (nl, nk) in enumerate(zip(N_LIG, N_KP)):
            rows = (slice(lo, lo + nl), slice(ko, ko + nk), slice(b, b + 1))
            ax, ah, ak = _run(_pb([nl], [nk], cuda), F, t, rows)
            assert torch.equal(ax, x[rows[0]]) and torch.equal(ah, h[rows[0]]) and torch.equal(ak, k[rows[1]]), (rotation, b)
            lo, ko = lo + nl, ko + nk


@pytest.mark.parametrize('F', [1, 5, 10])
def test_renoise_kernel_matches_fp64_restatement_and_bitwise_contracts(cuda, F):
    pb = _pb(N_LIG, N_KP, cuda)
    t = _inputs(F, 0, cuda, seed=1)

    def run(pb_, L=slice(None), K=slice(None), Bs=slice(None)):
        x, h, k = t['lig_x'][L].clone(), t['lig_h'][L].clone(), t['kp_x'][K].clone()
        hip.sample_renoise(pb_, F, x, h, k, t['nx'][L], t['nh'][L], t['coef6'][Bs])
        return x, h, k

    x, h, k = run(pb)
    rx, rh, rk = ref_renoise(N_LIG, N_KP, t['lig_x'], t['lig_h'], t['kp_x'], t['nx'], t['nh'], t['coef6'])
    errs = (util.rel_err(x, rx), util.rel_err(h, rh), util.rel_err(k, rk))
    print(f'renoise F={F}: rel err x {errs[0]:.2e} h {errs[1]:.2e} kp {errs[2]:.2e}')
    assert max(errs) < 1e-4, errs
    assert all(torch.equal(a, b) for a, b in zip((x, h, k), run(pb)))
    lo, ko = 0, 0
    for b, (nl, nk) in enumerate(zip(N_LIG, N_KP)):
        ax, ah, ak = run(_pb([nl], [nk], cuda), slice(lo, lo + nl), slice(ko, ko + nk), slice(b, b + 1))
        assert torch.equal(ax, x[lo:lo + nl]) and torch.equal(ah, h[lo:lo + nl]) and torch.equal(ak, k[ko:ko + nk]), b
        lo, ko = lo + nl, ko + nk


def test_wrappers_refuse_tensors_that_do_not_fit_the_batch(cuda):
    pb, t = _pb(N_LIG, N_KP, cuda), _inputs(5, 3, cuda)
    for key in ('eps_x', 'kh', 'fixed', 'com0', 'coef6'):
        bad = dict(t)
        bad[key] = t[key][:-1].contiguous()
        with pytest.raises(hip.KpdError):
            _run(pb, 5, bad)
    with pytest.raises(hip.KpdError):
        hip.sample_renoise(pb, 5, t['lig_x'].clone(), t['lig_h'].clone(), t['kp_x'].clone(), t['nx'], t['nh'], t['coef6'][:, :3].contiguous())
    with pytest.raises(hip.KpdError):
        _run(pb, 5, {k: v.cpu() for k, v in t.items()})


@pytest.mark.parametrize('T,precision', [(10, 1e-4), (10, 1e-5), (1000, 1e-4), (1000, 1e-5)])
def test_inpaint_coefficients_kernel(cuda, T, precision):
    s, t, ref = oracle_coefficients(T, precision)
    from oracle import diffusion as odiff
    table = odiff.gamma_table(T, precision).to(cuda)
    got = hip.inpaint_coefficients(table, s.to(cuda), t.to(cuda))
    assert got.shape == (T, 6)
    assert torch.equal(got[:, :3], hip.step_coefficients(table, s.to(cuda), t.to(cuda)))
    assert float(((got.cpu() - ref).abs() / ref.abs().clamp_min(1e-6)).max()) < 1e-4
    m = _model('egnn', T, precision).to(cuda)
    assert torch.equal(m.inpaint_coefficients(s.to(cuda), t.to(cuda)), hip.inpaint_coefficients(m.gamma.gamma, s.to(cuda), t.to(cuda)))


# ---- with a denoiser -------------------------------------------------------------------------------------------------
def _model(arch, T=10, precision=1e-4, norm=1.0):
    dyn = util.EGNN_C2 if arch == 'egnn' else dict(GVP_ALL_ATOM, n_convs=3)
    m = KeypointDiffusion(10, 10, None, n_timesteps=T, architecture=arch, rec_encoder_type='fixed',
                          graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dyn,
                          rec_encoder_config={'vector_size': 16}, precision=precision, lig_feat_norm_constant=norm)
    synth.fill_state_dict_(m, 13)
    return m.eval()


def test_anchored_inpainting_steps_with_the_egnn_denoiser(cuda, gemm_mode):
    """configs/dev_config.yml model, one complex of 60 x 20, T = 10, half the atoms fixed: every one of the 10 steps is taken on
    the GPU from the state of a CPU trajectory (oracle denoiser + the fp64 restatement, same injected noise) and must agree
    with that trajectory's next state to 1e-4."""
    T = 10
    model = KeypointDiffusion(10, 20, None, n_timesteps=T, architecture='egnn', rec_encoder_type='fixed',
                              graph_config=dict(n_keypoints=20, graph_cutoffs=CUT_DEV), dynamics_config=util.EGNN_DEV, precision=1e-5)
    synth.fill_state_dict_(model, 21)
    model.eval()
    gs = synth.synth_complexes([60], [20], 20, CUT_DEV, seed=77, n_rec_feat=20, density=synth.CA_DENSITY)
    shift = torch.tensor([[100.0, -80.0, 120.0]])
    gs[0].nodes['rec'].data['x_0'] += shift
    X = 3.0 * gs[0].nodes['lig'].data['x_0'] + shift             # known positions, input frame
    Hn = gs[0].nodes['lig'].data['h_0'].clone()
    fixed = torch.arange(20) % 2 == 0
    g = model.encode_receptors(G.batch(gs))
    com0 = g.nodes['kp'].data['x_0'].mean(0, keepdim=True)
    gen = torch.Generator().manual_seed(5)
    g.nodes['kp'].data['x_0'] = g.nodes['kp'].data['x_0'] - X[fixed].mean(0, keepdim=True)
    x0 = torch.randn(20, 3, generator=gen)
    c = x0.mean(0, keepdim=True)
    g.nodes['lig'].data['x_0'], g.nodes['lig'].data['h_0'] = x0 - c, torch.randn(20, 10, generator=gen)
    g.nodes['kp'].data['x_0'] = g.nodes['kp'].data['x_0'] - c
    ob = util.to_obatch(g)
    sd = {k[len('dynamics.'):]: v.clone() for k, v in model.state_dict().items() if k.startswith('dynamics.')}
    cfg = dict(util.EGNN_DEV, graph_cutoffs=CUT_DEV)
    _, _, table = oracle_coefficients(T, 1e-5)
    model = model.to(cuda)
    ga = g.to(cuda)
    bidx = G.get_batch_idxs(ga)
    ctx = InpaintContext(fixed.to(cuda), X.to(cuda), Hn.to(cuda), com0.to(cuda))
    one, worst = torch.ones(1), 0.0
    with torch.no_grad():
        for si in reversed(range(T)):
            s, t = one * (si / T), one * ((si + 1) / T)
            noise = [torch.randn(20, w, generator=gen) for w in (3, 10, 3, 10)]
            for key, src in (('x_0', ob.x['lig']), ('h_0', ob.h['lig'])):
                ga.nodes['lig'].data[key].copy_(src.to(cuda))
            ga.nodes['kp'].data['x_0'].copy_(ob.x['kp'].to(cuda))
            model.sample_p_zs_given_zt(s.to(cuda), t.to(cuda), ga, bidx, noise=tuple(n.to(cuda) for n in noise), inpaint=ctx)
            eh, ex = oegnn.egnn_dynamics_forward(sd, cfg, ob, t)
            rx, rh, rk = ref_update([20], [g.num_nodes('kp')], ob.x['lig'], ob.h['lig'], ob.x['kp'], ex, eh, noise[0], noise[1],
                                    table[si:si + 1], fixed, X, Hn, com0, noise[2], noise[3])
            errs = (util.rel_err(ga.nodes['lig'].data['x_0'], rx), util.rel_err(ga.nodes['lig'].data['h_0'], rh),
                    util.rel_err(ga.nodes['kp'].data['x_0'], rk))
            worst = max(worst, *errs)
            assert max(errs) < 1e-4, f's = {si}: rel err x {errs[0]:.3e} h {errs[1]:.3e} kp {errs[2]:.3e}'
            ob.x['lig'], ob.h['lig'], ob.x['kp'] = rx.float(), rh.float(), rk.float()
    print(f'anchored inpainting steps: worst rel err {worst:.3e}')


N_REC3, N_LIG3 = [90, 140, 60], [11, 17, 6]


def _encoded(model, dev, far=True, seed=3):
    """B = 3 ragged complexes with their reference ligands, moved ~100 A away from the origin (each complex elsewhere)."""
    gs = synth.synth_complexes(N_REC3, N_LIG3, 20, CUT, seed=seed)
    for i, g in enumerate(gs):
        shift = torch.tensor([[100.0 + 30 * i, -80.0, 120.0 - 50 * i]]) if far else torch.zeros(1, 3)
        g.nodes['rec'].data['x_0'] = g.nodes['rec'].data['x_0'] + shift
        g.nodes['lig'].data['x_0'] = 2.5 * g.nodes['lig'].data['x_0'] + shift
    return model.encode_receptors(G.batch(gs).to(dev))


@pytest.mark.parametrize('arch,norm', [('egnn', 1.0), ('gvp', 4.0)])
def test_frame_bookkeeping_end_to_end(cuda, arch, norm):
    """All atoms fixed, no overwrite: a fixed atom comes back as X + (alpha_0 - 1) k0 + sigma_0 n', so every returned position lies
    within 7 sigma_0 + (1 - alpha_0) R + 1e-3 A of its known position (|n'| <= 6.66 for a 32-bit Box-Muller draw; R = largest
    distance of a known atom from its ligand's centroid, which is the state-frame origin up to the noise of the last step).  A
    wrong frame is an error of Angstroms.  Features: the same bound times lig_feat_norm_constant."""
    model = _model(arch, 10, 1e-4, norm).to(cuda).use_complex_noise(1234)
    g = _encoded(model, cuda)
    X, H = g.nodes['lig'].data['x_0'].cpu().split(N_LIG3), g.nodes['lig'].data['h_0'].cpu().split(N_LIG3)
    c0 = model.inpaint_coefficients(torch.zeros(1, device=cuda), torch.full((1,), 0.1, device=cuda)).cpu()
    alpha_0, sigma_0 = float(c0[0, 3]), float(c0[0, 4])
    assert abs(sigma_0 - 0.01) < 1e-4 and abs(alpha_0 - 0.99995) < 1e-5
    pos, feat = model.inpaint_from_encoded_receptors(g, torch.ones(sum(N_LIG3), dtype=torch.bool, device=cuda),
                                                     complex_ids=torch.tensor([7, 8, 9]), overwrite_fixed=False)
    for p, f, x, h in zip(pos, feat, X, H):
        R = float((x - x.mean(0)).norm(dim=1).max())
        bound = 7 * sigma_0 + (1 - alpha_0) * R + 1e-3
        dx, dh = float((p - x).norm(dim=1).max()), float((f - h).abs().max())
        print(f'{arch}: |dx| {dx:.4f} A (bound {bound:.4f}), |dh| {dh:.4f} (bound {norm * bound:.4f})')
        assert dx <= bound and dh <= norm * bound
        assert dx > 0                                            # not overwritten


def test_loop_properties(cuda):
    T = 10
    model = _model('egnn', T).to(cuda).use_complex_noise(99)
    ids = torch.tensor([40, 41, 42])
    n = sum(N_LIG3)
    fixed = (torch.arange(n) % 3 == 0).to(cuda)
    g = _encoded(model, cuda)
    X, H = g.nodes['lig'].data['x_0'].cpu(), g.nodes['lig'].data['h_0'].cpu()
    pos, feat = model.inpaint_from_encoded_receptors(g, fixed, complex_ids=ids)
    assert [tuple(p.shape) for p in pos] == [(k, 3) for k in N_LIG3] and [tuple(f.shape) for f in feat] == [(k, 10) for k in N_LIG3]
    px, ph, fx = torch.cat(pos), torch.cat(feat), fixed.cpu()
    assert torch.equal(px[fx], X[fx]) and torch.equal(ph[fx], H[fx])                     # the caller's values, bit for bit
    assert torch.isfinite(px).all() and torch.isfinite(ph).all()
    assert float((px[~fx] - X[~fx]).abs().max()) > 1e-3                                   # the free rows were generated
    # the same seed twice
    pos2, feat2 = model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed.to(torch.uint8), complex_ids=ids)
    assert all(torch.equal(a, b) for a, b in zip(pos + feat, pos2 + feat2))
    # nothing fixed: the plain sampler of the same seed and ids, bit for bit
    zero = torch.zeros(n, dtype=torch.bool, device=cuda)
    ip, if_ = model.inpaint_from_encoded_receptors(_encoded(model, cuda), zero, complex_ids=ids)
    sp, sf = model.sample_from_encoded_receptors(_encoded(model, cuda), complex_ids=ids)
    assert all(torch.equal(a, b) for a, b in zip(ip + if_, sp + sf))
    # resampling: r T denoiser forwards, fixed rows still exact
    calls = []
    hook = model.dynamics.register_forward_hook(lambda *a: calls.append(1))
    try:
        rp, rf = model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed, resamplings=2, complex_ids=ids)
        assert len(calls) == 2 * T
        del calls[:]
        model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed, complex_ids=ids)
        assert len(calls) == T
    finally:
        hook.remove()
    rx, rh = torch.cat(rp), torch.cat(rf)
    assert torch.equal(rx[fx], X[fx]) and torch.equal(rh[fx], H[fx]) and torch.isfinite(rx).all() and torch.isfinite(rh).all()
    assert not torch.equal(rx, px)
    # trajectories: T + 1 frames per ligand, the last one is the result
    vx, vh = model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed, visualize=True, complex_ids=ids)
    assert len(vx) == 3 and all(len(tr) == T + 1 for tr in vx) and len(vh) == 3 and all(len(tr) == T + 1 for tr in vh)
    assert all(torch.equal(tr[-1], p) for tr, p in zip(vx, pos)) and all(torch.equal(tr[-1], f) for tr, f in zip(vh, feat))
    # the global torch.randn noise works too (the default)
    model.use_complex_noise(None)
    gp, gf = model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed)
    assert torch.equal(torch.cat(gp)[fx], X[fx]) and torch.isfinite(torch.cat(gp)).all()


def _pocket(dev, n_rec=70, seed=9):
    pocket = synth.synth_complexes([n_rec], [1], 20, CUT, seed=seed)[0].to(dev)
    pocket.remove_nodes(pocket.nodes('lig'), ntype='lig')
    return pocket


def test_inpaint_given_pocket(cuda):
    T = 10
    model = _model('egnn', T).to(cuda)
    gen = torch.Generator().manual_seed(2)
    kpos, kfeat = 1.5 * torch.randn(4, 3, generator=gen), torch.randn(4, 10, generator=gen)
    pos, feat = model.inpaint_given_pocket(_pocket(cuda), kpos, kfeat, torch.tensor([6, 4, 9]), diff_batch_size=2)
    assert [tuple(p.shape) for p in pos] == [(6, 3), (4, 3), (9, 3)] and [tuple(f.shape) for f in feat] == [(6, 10), (4, 10), (9, 10)]
    for p, f in zip(pos, feat):
        assert torch.equal(p[:4], kpos) and torch.equal(f[:4], kfeat) and torch.isfinite(p).all() and torch.isfinite(f).all()
        assert p.device.type == 'cpu'
    fx, fh = model.inpaint_given_pocket(_pocket(cuda), kpos, kfeat, torch.tensor([7]), resamplings=2, visualize=True)
    assert len(fx) == 1 and len(fx[0]) == T + 1 and fx[0][0].shape == (7, 3) and torch.equal(fx[0][-1][:4], kpos)


@pytest.mark.parametrize('arch', ['egnn', 'gvp'])
def test_step_graph_replays_the_eager_inpainting_step(cuda, arch):
    T = 20
    model = _model(arch, T, 1e-5).to(cuda)
    g1, g2 = _encoded(model, cuda, far=False), _encoded(model, cuda, far=False)
    n = sum(N_LIG3)
    gen = torch.Generator().manual_seed(1)
    noise = tuple(torch.randn(n, w, generator=gen).to(cuda) for w in (3, 10, 3, 10))
    ctx = InpaintContext((torch.arange(n) % 2 == 1).to(cuda), torch.randn(n, 3, generator=gen).to(cuda),
                         torch.randn(n, 10, generator=gen).to(cuda), torch.randn(3, 3, generator=gen).to(cuda))
    with torch.no_grad():
        sg = model.capture_step(g1, noise=noise, inpaint=ctx)
        ones = torch.ones(3, device=cuda)
        for s in (19, 18, 7):
            sg.step(s / T, (s + 1) / T)
            model.sample_p_zs_given_zt(ones * (s / T), ones * ((s + 1) / T), g2, noise=noise, inpaint=ctx)
            for nt, k in (('lig', 'x_0'), ('lig', 'h_0'), ('kp', 'x_0')):
                assert torch.equal(g1.nodes[nt].data[k], g2.nodes[nt].data[k]), (s, nt, k)
    fixed = ctx.fixed.bool()
    g = _encoded(model, cuda)
    X = g.nodes['lig'].data['x_0'].cpu()
    pos, feat = model.inpaint_from_encoded_receptors(g, fixed, use_graph=True)            # global noise, one repetition
    assert torch.equal(torch.cat(pos)[fixed.cpu()], X[fixed.cpu()]) and torch.isfinite(torch.cat(pos)).all()
    with pytest.raises(ValueError, match='resamplings'):
        model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed, use_graph=True, resamplings=2)
    model.use_complex_noise(5)
    with pytest.raises(ValueError, match='per-complex'):
        model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed, use_graph=True, complex_ids=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError):
        model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed, use_graph=True, resamplings=2,
                                             complex_ids=torch.tensor([0, 1, 2]))


def test_sample_with_known_atoms_sharded_equals_single_process(cuda):
    """`_sample(..., known=...)` on two thread ranks: every rank returns all ligands in input order, equal to the single-process
    run of the same seed under the comparison the plain sharded tests apply; the known rows are exact everywhere."""
    from . import sharded_worker as W
    from .test_sampler_gpu import _assert_samples_equal
    gen = torch.Generator().manual_seed(8)
    known = [(torch.randn(3, 3, generator=gen), torch.randn(3, 10, generator=gen)), None,
             (torch.randn(5, 3, generator=gen), torch.randn(5, 10, generator=gen)), None,
             (torch.randn(1, 3, generator=gen), torch.randn(1, 10, generator=gen))]

    def run(rank=None):
        model = W.build_model(cuda).use_complex_noise(W.SEED)
        return model._sample(W.pockets(cuda), W.N_LIG, rec_enc_batch_size=2, diff_batch_size=2, known=known)

    ref = run()
    assert [len(r['positions']) for r in ref] == [len(sizes) for sizes in W.N_LIG]
    for got in [ref] + util.run_threaded_world(2, run):
        _assert_samples_equal(got, ref)
        for r, k, sizes in zip(got, known, W.N_LIG):
            assert [p.shape[0] for p in r['positions']] == sizes
            for p, f in zip(r['positions'], r['features']):
                if k is not None:
                    assert torch.equal(p[:k[0].shape[0]], k[0]) and torch.equal(f[:k[1].shape[0]], k[1])
    with pytest.raises(ValueError, match='n_lig_atoms'):
        W.build_model(cuda)._sample(W.pockets(cuda), W.N_LIG, known=[None, (torch.zeros(10, 3), torch.zeros(10, 10)), None, None, None])
