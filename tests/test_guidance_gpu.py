"""Clash guidance on the GPU: the fused guided update (kpd_sample_update_guided), its coefficient kernel and the clash report
(kpd_clash_score) against an fp64 restatement of the algorithm of include/kpd.h written here; the bitwise guarantees (a neutral
complex = the plain / inpainting kernel; independent of batch composition; repeatable); anchored steps with real denoisers; the
captured step; the public loop, alone, with known atoms and sharded; the refusals."""
import math

import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip, synth
from keypoint_diffusion_amd.ligand_diffuser import ClashGuidance, GuidanceContext, InpaintContext, KeypointDiffusion
from oracle import diffusion as odiff
from oracle import egnn as oegnn
from oracle import gvp as ogvp

from . import util
from .test_guidance_config import GRID, fp64_guided_coefficients, max_rel
from .test_gvp_gpu import GVP_ALL_ATOM
from .test_trajectory_gpu import CUT_DEV

pytestmark = pytest.mark.gpu
CUT = util.CUTOFFS_ALL_ATOM
THR = 3.0
N_LIG, N_KP = [1, 5, 14, 25], [3, 40, 64, 130]      # a one-atom ligand (its COM removal zeroes it); 130 keypoints are strided over
_BASE = [0, 1, 65, 130]                             # wall atoms per complex: none, one, one past a wavefront, two strides and two
WALLS = [_BASE[r:] + _BASE[:r] for r in range(4)] + [[63, 64, 130, 0], [64, 63, 0, 65]]      # and both sides of the lane-stride edge


# ---- the fp64 restatement (steps 1-7 of include/kpd.h, "Clash guidance") -------------------------------------------------
def ref_guided(n_lig, n_kp, n_wall, lig_x, lig_h, kp_x, eps_x, eps_h, nx, nh, coef9, wall_x, com0, thr, fixed=None, X=None, Hn=None,
               kx=None, kh=None):
    """Returns (x, h, kp, info): info = per-atom contact counts, the smallest pair distance per complex, the smallest
    |threshold - d| over all pairs, the per-atom shift w F and x-hat, all in fp64."""
    d = lambda t: None if t is None else t.detach().cpu().double()
    lig_x, lig_h, kp_x, eps_x, eps_h, nx, nh, coef9, wall_x, com0, X, Hn, kx, kh = map(d, (lig_x, lig_h, kp_x, eps_x, eps_h, nx, nh, coef9,
                                                                                         wall_x, com0, X, Hn, kx, kh))
    fixed = None if fixed is None else fixed.cpu().bool()
    ox, oh, ok, lo, ko, wo = [], [], [], 0, 0, 0
    info = dict(contacts=[], dmin=[], margin=math.inf, shift=[], xhat=[], energy=[])
    for b, (nl, nk, nw) in enumerate(zip(n_lig, n_kp, n_wall)):
        L, K, W = slice(lo, lo + nl), slice(ko, ko + nk), slice(wo, wo + nw)
        a_ts, var, sg, a_s, s_s, _, a_t, s_t, w = coef9[b]
        ux = lig_x[L] / a_ts - var * eps_x[L] + sg * nx[L]                        # 1. candidate
        uh = lig_h[L] / a_ts - var * eps_h[L] + sg * nh[L]
        xh = (lig_x[L] - s_t * eps_x[L]) / a_t                                    # 2. denoised positions
        m = kp_x[K].mean(0)                                                       # 3. frame
        r = (wall_x[W] - com0[b]) + m
        diff = xh[:, None, :] - r[None, :, :]                                     # 4. force
        dist = diff.norm(dim=2)
        h = (thr - dist).clamp_min(0.0)
        Fc = (torch.where(dist >= 1e-6, h / dist.clamp_min(1e-300), torch.zeros_like(h))[:, :, None] * diff).sum(1)
        ux = ux + w * Fc                                                          # 5. shift
        free = torch.ones(nl, dtype=torch.bool)
        if fixed is not None:                                                     # 6. inpainting merge
            k0 = (X[L] - com0[b]) + m
            f = fixed[L][:, None]
            ux, uh = torch.where(f, a_s * k0 + s_s * kx[L], ux), torch.where(f, a_s * Hn[L] + s_s * kh[L], uh)
            free = ~fixed[L]
        c = ux.mean(0)                                                            # 7. COM removal
        ox.append(ux - c), oh.append(uh), ok.append(kp_x[K] - c)
        info['contacts'].append(((dist < thr).sum(1) * free).long())
        info['dmin'].append(float(dist.min()) if nw else math.inf)
        info['energy'].append(float(0.5 * (h ** 2).sum()))
        info['shift'].append(w * Fc * free[:, None])
        info['xhat'].append(xh)
        if nw:
            info['margin'] = min(info['margin'], float((thr - dist).abs().min()))
        lo, ko, wo = lo + nl, ko + nk, wo + nw
    return torch.cat(ox), torch.cat(oh), torch.cat(ok), info


def _mask(pattern, n):
    return {0: torch.zeros(n, dtype=torch.bool), 1: torch.arange(n) % 2 == 0, 2: torch.arange(n) == n // 2,
            3: torch.arange(n) % 3 == 1}[pattern]


_TABLE = {}


def _table(T=10, precision=1e-4, scale=1.0, t_max=1.0):
    key = (T, precision, scale, t_max)
    if key not in _TABLE:
        _TABLE[key] = fp64_guided_coefficients(T, precision, scale, t_max)[2].float()
    return _TABLE[key]


def _inputs(F, walls, dev, seed=0, rows=(9, 0, 4, 7)):
    """State, denoiser output, draws, wall and known part of one guided step for the shapes above.  The wall (and the known
    positions) sit ~100 A from the origin of the state frame, with kp_com0 to match, so (r - kp_com0) + m only works in that
    order.  In the state frame the wall atoms are ~ 4 N(0,1); every ligand atom's denoised position is aimed at a random wall atom
    of its complex plus a random direction times U(0.4, threshold + 1), and the state is alpha_t x-hat + sigma_t eps.  The
    coefficient rows are steps 9 (t = 1), 0 (s = 0), 4 and 7 of T = 10."""
    gen = torch.Generator().manual_seed(1000 * seed + 10 * F + sum((i + 1) * w for i, w in enumerate(walls)))
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    nl, nk = sum(N_LIG), sum(N_KP)
    kp_x = (6.0 * r(nk, 3) + torch.repeat_interleave(2.0 * r(4, 3), torch.tensor(N_KP), 0)).float()
    m = torch.stack([p.double().mean(0) for p in kp_x.split(N_KP)])
    com0 = (torch.tensor([[100.0, -80.0, 120.0]]) + 20.0 * r(4, 3)).float()
    lig_b = torch.repeat_interleave(torch.arange(4), torch.tensor(N_LIG))
    coef9 = _table()[list(rows)].contiguous()
    wall_state, xhat = [], []
    for b, (n, nw) in enumerate(zip(N_LIG, walls)):
        ws = 4.0 * r(nw, 3)
        wall_state.append(ws)
        if nw:
            aim = ws[torch.randint(nw, (n,), generator=gen)]
            u = r(n, 3)
            rad = 0.4 + (THR + 1.0 - 0.4) * torch.rand(n, 1, generator=gen, dtype=torch.float64)
            xhat.append(aim + rad * u / u.norm(dim=1, keepdim=True))
        else:
            xhat.append(4.0 * r(n, 3))
    wall_x = torch.cat([(ws - m[b]) + com0[b].double() for b, ws in enumerate(wall_state)]).float()
    eps_x = r(nl, 3).float()
    lig_x = (coef9[lig_b, 6:7].double() * torch.cat(xhat) + coef9[lig_b, 7:8].double() * eps_x.double()).float()
    X = (2.0 * r(nl, 3) - m[lig_b] + com0[lig_b].double()).float()
    f32 = lambda *s: r(*s).float()
    t = dict(lig_x=lig_x, lig_h=f32(nl, F), kp_x=kp_x, eps_x=eps_x, eps_h=f32(nl, F), nx=f32(nl, 3), nh=f32(nl, F), coef9=coef9,
             wall_x=wall_x, wall_ptr=torch.tensor([0] + list(walls)).cumsum(0).int(), com0=com0,
             fixed=torch.cat([_mask((b + seed) % 4, n) for b, n in enumerate(N_LIG)]), X=X, Hn=f32(nl, F), kx=f32(nl, 3), kh=f32(nl, F))
    return {k: v.to(dev) for k, v in t.items()}


def _ref(t, walls, masked=False, n_lig=N_LIG, n_kp=N_KP):
    kw = dict(fixed=t['fixed'], X=t['X'], Hn=t['Hn'], kx=t['kx'], kh=t['kh']) if masked else {}
    return ref_guided(n_lig, n_kp, walls, t['lig_x'], t['lig_h'], t['kp_x'], t['eps_x'], t['eps_h'], t['nx'], t['nh'], t['coef9'],
                      t['wall_x'], t['com0'], THR, **kw)


def _pb(n_lig, n_kp, dev):
    e = torch.zeros(0, dtype=torch.long)
    return hip.PreparedBatch(torch.tensor(n_lig), torch.tensor(n_kp), e, e, dev)


def _run(pb, F, t, masked=False, rows=None, coef9=None):
    """kpd_sample_update_guided on clones of the inputs `t`, or of its ligand / keypoint / wall rows and complexes `rows`."""
    L, K, W, Bs = rows or (slice(None),) * 4
    x, h, k = t['lig_x'][L].clone(), t['lig_h'][L].clone(), t['kp_x'][K].clone()
    wall_ptr = t['wall_ptr'] if rows is None else (t['wall_ptr'][Bs.start:Bs.stop + 1] - t['wall_ptr'][Bs.start]).contiguous()
    kw = dict(fixed=t['fixed'][L], known_x=t['X'][L], known_h=t['Hn'][L], known_noise_x=t['kx'][L], known_noise_h=t['kh'][L]) if masked else {}
    hip.sample_update_guided(pb, F, x, h, k, t['eps_x'][L], t['eps_h'][L], t['nx'][L], t['nh'][L], (t['coef9'] if coef9 is None else coef9)[Bs],
                             t['wall_x'][W].contiguous(), wall_ptr, t['com0'][Bs], THR, **kw)
    return x, h, k


def _plain(pb, F, t, masked=False):
    x, h, k = t['lig_x'].clone(), t['lig_h'].clone(), t['kp_x'].clone()
    if masked:
        hip.sample_update_inpaint(pb, F, x, h, k, t['eps_x'], t['eps_h'], t['nx'], t['nh'], t['coef9'][:, :6].contiguous(), t['fixed'],
                                  t['X'], t['Hn'], t['com0'], t['kx'], t['kh'])
    else:
        hip.sample_update(pb, F, x, h, k, t['eps_x'], t['eps_h'], t['nx'], t['nh'], t['coef9'][:, :3].contiguous())
    return x, h, k


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


_SEEDS = {(10, 0): 1}                               # (F, row of WALLS) -> input seed, 0 otherwise: where check_construction holds


def check_construction(info, walls):
    """The conditions on the inputs, on the fp64 side: no pair closer than 0.3 A; at least a third of ALL atoms in contact; one
    atom with two contacts or more; and, among the complexes that have a wall, one atom with none (the atom that is not written
    inside a complex that is pushed)."""
    contacts = torch.cat(info['contacts'])
    walled = torch.cat([c for c, nw in zip(info['contacts'], walls) if nw])
    assert min(info['dmin']) >= 0.3, info['dmin']
    assert 3 * int((contacts > 0).sum()) >= contacts.numel(), contacts.tolist()
    assert int(contacts.max()) >= 2 and int(walled.min()) == 0, walled.tolist()


@pytest.mark.parametrize('F', [1, 10])
def test_update_kernel_matches_fp64_restatement_and_bitwise_contracts(cuda, F):
    pb = _pb(N_LIG, N_KP, cuda)
    zero_w = None
    for ci, walls in enumerate(WALLS):
        t = _inputs(F, walls, cuda, seed=_SEEDS.get((F, ci), 0))
        for masked in (False, True):
            got = _run(pb, F, t, masked)
            rx, rh, rk, info = _ref(t, walls, masked)
            if not masked:
                check_construction(info, walls)
            errs = tuple(util.rel_err(a, b) for a, b in zip(got, (rx, rh, rk)))
            print(f'F={F} walls={walls} masked={masked}: rel err x {errs[0]:.2e} h {errs[1]:.2e} kp {errs[2]:.2e}; contacts per atom '
                  f'0..{int(torch.cat(info["contacts"]).max())}, smallest distance {min(info["dmin"]):.2f} A')
            assert max(errs) < 1e-4, errs
            lx = got[0].cpu().split(N_LIG)
            for b in range(4):                                   # the ligand COM is gone, per complex, at the scale of its coordinates
                assert float(lx[b].mean(0).abs().max()) < 1e-5 * max(1.0, float(lx[b].abs().max()))
            assert _same(got, _run(pb, F, t, masked))            # a second call on cloned inputs: the same bits
            # the complexes without wall atoms leave with the bits of the plain (with a mask: the inpainting) kernel
            plain = _plain(pb, F, t, masked)
            for b, nw in enumerate(walls):
                if nw == 0:
                    for a, p, sizes in zip(got, plain, (N_LIG, N_LIG, N_KP)):
                        assert torch.equal(a.cpu().split(sizes)[b], p.cpu().split(sizes)[b]), (walls, masked, b)
            assert not _same(got, plain)                         # ... and the others were pushed
            # scale = 0: every complex is neutral
            zero_w = t['coef9'].clone()
            zero_w[:, 8] = 0.0
            assert _same(_run(pb, F, t, masked, coef9=zero_w), plain)
            # every complex alone: its rows of the batch
            lo, ko = 0, 0
            for b, (nl, nk) in enumerate(zip(N_LIG, N_KP)):
                wlo, whi = int(t['wall_ptr'][b]), int(t['wall_ptr'][b + 1])
                rows = (slice(lo, lo + nl), slice(ko, ko + nk), slice(wlo, whi), slice(b, b + 1))
                ax, ah, ak = _run(_pb([nl], [nk], cuda), F, t, masked, rows)
                assert torch.equal(ax, got[0][rows[0]]) and torch.equal(ah, got[1][rows[0]]) and torch.equal(ak, got[2][rows[1]]), (walls, b)
                lo, ko = lo + nl, ko + nk


def test_no_pair_under_the_threshold_is_neutral(cuda):
    """A wall further than the threshold from every denoised position, w > 0: the bits of the plain kernel."""
    walls = WALLS[2]
    t = _inputs(5, walls, cuda, seed=7)
    t['wall_x'] = t['wall_x'] + 60.0
    _, _, _, info = _ref(t, walls)
    assert int(torch.cat(info['contacts']).sum()) == 0 and bool((t['coef9'][:, 8] > 0).all())
    pb = _pb(N_LIG, N_KP, cuda)
    assert _same(_run(pb, 5, t), _plain(pb, 5, t)) and _same(_run(pb, 5, t, True), _plain(pb, 5, t, True))


def test_single_contact_lands_on_the_threshold_sphere(cuda):
    """scale = 1, no noise, one wall atom: the shift of the candidate is w (threshold - d) along the contact direction, i.e. the
    implied x-hat moves exactly onto the sphere.  The shift is recovered from the guided and the plain output (the keypoints carry
    minus the COM), each good to 1e-4 of the largest coordinate, so the implied x-hat shift is good to twice that over w."""
    n_lig, n_kp, walls = [6], [7], [1]
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    coef9 = _table()[[4]].contiguous()
    a_t, s_t, w = (float(v) for v in coef9[0, 6:9].double())
    kp_x, com0, wall_state = (5.0 * r(7, 3)).float(), torch.tensor([[100.0, -80.0, 120.0]]), r(1, 3)
    wall_x = ((wall_state - kp_x.double().mean(0)) + com0.double()).float()
    u = r(6, 3)
    xhat = wall_state + torch.tensor([[0.5], [1.0], [1.7], [2.4], [2.9], [3.6]]) * u / u.norm(dim=1, keepdim=True)
    eps_x = r(6, 3).float()
    t = dict(lig_x=(a_t * xhat + s_t * eps_x.double()).float(), lig_h=r(6, 4).float(), kp_x=kp_x, eps_x=eps_x, eps_h=r(6, 4).float(),
             nx=torch.zeros(6, 3), nh=torch.zeros(6, 4), coef9=coef9, wall_x=wall_x, wall_ptr=torch.tensor([0, 1], dtype=torch.int32),
             com0=com0)
    t = {k: v.to(cuda) for k, v in t.items()}
    pb = _pb(n_lig, n_kp, cuda)
    gx, _, gk = _run(pb, 4, t)
    px, _, pk = _plain(pb, 4, t)
    _, _, _, info = ref_guided(n_lig, n_kp, walls, t['lig_x'], t['lig_h'], t['kp_x'], t['eps_x'], t['eps_h'], t['nx'], t['nh'], coef9,
                               t['wall_x'], t['com0'], THR)
    assert info['contacts'][0].tolist() == [1, 1, 1, 1, 1, 0]
    shift = ((gx - px) - (gk - pk)[:1]).cpu().double() / w       # implied move of x-hat
    xh = info['xhat'][0]
    rp = (t['wall_x'].cpu().double() - com0.double()) + t['kp_x'].cpu().double().mean(0)
    d = (xh - rp).norm(dim=1, keepdim=True)
    want = (THR - d).clamp_min(0.0) * (xh - rp) / d
    tol = 2e-4 * float(px.abs().max()) / w
    err = float((shift - want).abs().max())
    print(f'single contact: |shift - (threshold - d) n| <= {err:.2e} A (tolerance {tol:.2e}), w = {w:.4f}')
    assert err <= tol
    landed = (xh + shift - rp).norm(dim=1)
    assert float((landed[:5] - THR).abs().max()) <= tol and abs(float(landed[5]) - float(d[5])) <= tol


def test_largest_ligand_the_lds_holds(cuda):
    """max_lig = 4096: 96 KB of dynamic LDS (positions and x-hat), more than the 64 KB a kernel gets without asking."""
    n_lig, n_kp, walls = [4096], [3], [70]
    gen = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=gen)
    coef9 = _table()[[6]].contiguous()
    t = dict(lig_x=3.0 * r(4096, 3), lig_h=r(4096, 2), kp_x=r(3, 3), eps_x=r(4096, 3), eps_h=r(4096, 2), nx=r(4096, 3), nh=r(4096, 2),
             coef9=coef9, wall_x=4.0 * r(70, 3), wall_ptr=torch.tensor([0, 70], dtype=torch.int32), com0=torch.zeros(1, 3))
    t = {k: v.to(cuda) for k, v in t.items()}
    got = _run(_pb(n_lig, n_kp, cuda), 2, t)
    rx, rh, rk, info = ref_guided(n_lig, n_kp, walls, t['lig_x'], t['lig_h'], t['kp_x'], t['eps_x'], t['eps_h'], t['nx'], t['nh'], coef9,
                                  t['wall_x'], t['com0'], THR)
    assert int((info['contacts'][0] > 0).sum()) > 100
    errs = tuple(util.rel_err(a, b) for a, b in zip(got, (rx, rh, rk)))
    print(f'4096 atoms: rel err x {errs[0]:.2e} h {errs[1]:.2e} kp {errs[2]:.2e}')
    assert max(errs) < 1e-4, errs


@pytest.mark.parametrize('T,precision', GRID)
def test_guided_coefficients_kernel(cuda, T, precision):
    s, t, ref = fp64_guided_coefficients(T, precision, scale=0.75, t_max=0.5)
    table = odiff.gamma_table(T, precision).to(cuda)
    got = hip.guided_coefficients(table, s.to(cuda), t.to(cuda), 0.75, 0.5)
    assert got.shape == (T, 9)
    assert torch.equal(got[:, :6], hip.inpaint_coefficients(table, s.to(cuda), t.to(cuda)))
    assert torch.equal(got[:, :3], hip.step_coefficients(table, s.to(cuda), t.to(cuda)))
    err = max_rel(got.cpu(), ref)
    print(f'T={T} precision={precision}: max rel err {err:.2e}')
    assert err < 1e-4
    assert torch.equal(got[T // 2:, 8].cpu(), torch.zeros(T - T // 2)) and bool((got[:T // 2, 8] > 0).all())
    assert torch.equal(hip.guided_coefficients(table, s.to(cuda), t.to(cuda), 0.0, 1.0)[:, 8].cpu(), torch.zeros(T))
    m = _model('egnn', T, precision).to(cuda)
    assert torch.equal(m.guided_coefficients(s.to(cuda), t.to(cuda), 0.75, 0.5), got)


@pytest.mark.parametrize('ci', range(len(WALLS)))
def test_clash_score_matches_fp64(cuda, ci):
    """Ligand = the denoised positions of the update test, wall = its wall, both in the state frame."""
    walls = WALLS[ci]
    t = _inputs(1, walls, torch.device("cpu"), seed=0)
    _, _, _, info = _ref(t, walls)
    m = torch.stack([p.double().mean(0) for p in t['kp_x'].split(N_KP)])
    wall_b = torch.repeat_interleave(torch.arange(4), torch.tensor(walls))
    lig = torch.cat(info['xhat']).float()
    wall = ((t['wall_x'].double() - t['com0'].double()[wall_b]) + m[wall_b]).float()
    e, n, dmin, margin = [], [], [], math.inf
    for x, w in zip(lig.double().split(N_LIG), wall.double().split(walls)):
        d = (x[:, None] - w[None]).norm(dim=2)
        e.append(float(0.5 * ((THR - d).clamp_min(0) ** 2).sum())), n.append(int((d < THR).sum()))
        dmin.append(float(d[d < THR].min()) if n[-1] else math.inf)
        margin = min(margin, float((THR - d).abs().min()) if w.shape[0] else math.inf)
    assert margin > 1e-4, margin                                 # no pair within 1e-4 A of the threshold: the count is exact
    lig_ptr = torch.tensor([0] + N_LIG).cumsum(0).int().to(cuda)
    got = hip.clash_score(lig.to(cuda), lig_ptr, wall.to(cuda), t['wall_ptr'].to(cuda), THR).cpu()
    assert got.shape == (4, 3)
    assert torch.equal(got, hip.clash_score(lig.to(cuda), lig_ptr, wall.to(cuda), t['wall_ptr'].to(cuda), THR).cpu())
    print(f'walls={walls}: energy {[round(v, 3) for v in e]} pairs {n} smallest {[round(v, 3) for v in dmin]}')
    for b in range(4):
        assert int(got[b, 1]) == n[b], (b, got[b], n[b])
        if n[b] == 0:
            assert float(got[b, 0]) == 0.0 and float(got[b, 2]) == math.inf
        else:
            assert abs(float(got[b, 0]) - e[b]) <= 1e-4 * e[b] and abs(float(got[b, 2]) - dmin[b]) <= 1e-4 * dmin[b], (b, got[b], e[b], dmin[b])
    sizes = [(N_LIG[b], walls[b]) for b in range(4)]
    assert (0, 0.0, math.inf) in [(n[b], e[b], dmin[b]) for b in range(4) if walls[b] == 0], sizes
    # a complex alone: its row of the batch
    lo, wo = 0, 0
    for b in range(4):
        one = hip.clash_score(lig[lo:lo + N_LIG[b]].to(cuda), torch.tensor([0, N_LIG[b]], dtype=torch.int32, device=cuda),
                              wall[wo:wo + walls[b]].contiguous().to(cuda), torch.tensor([0, walls[b]], dtype=torch.int32, device=cuda), THR)
        assert torch.equal(one.cpu()[0], got[b]), b
        lo, wo = lo + N_LIG[b], wo + walls[b]


# ---- with a denoiser -------------------------------------------------------------------------------------------------
def _model(arch, T=10, precision=1e-4):
    dyn = util.EGNN_C2 if arch == 'egnn' else dict(GVP_ALL_ATOM, n_convs=3)
    m = KeypointDiffusion(10, 10, None, n_timesteps=T, architecture=arch, rec_encoder_type='fixed',
                          graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dyn,
                          rec_encoder_config={'vector_size': 16}, precision=precision)
    synth.fill_state_dict_(m, 13)
    return m.eval()


def anchored_setup(arch, weights=21):
    """One complex of 60 x 20, T = 10, the receptor ~100 A from the origin; the wall is the pocket's 60 atoms, threshold 3 A.
    Returns what the CPU side of the anchored test needs (the GPU side only copies it)."""
    T = 10
    if arch == 'egnn':                                           # configs/dev_config.yml
        model = KeypointDiffusion(10, 20, None, n_timesteps=T, architecture='egnn', rec_encoder_type='fixed',
                                  graph_config=dict(n_keypoints=20, graph_cutoffs=CUT_DEV), dynamics_config=util.EGNN_DEV, precision=1e-5)
        cut, n_rec_feat, cfg = CUT_DEV, 20, dict(util.EGNN_DEV, graph_cutoffs=CUT_DEV)
        forward = oegnn.egnn_dynamics_forward
        start = 1.0
    else:
        model = KeypointDiffusion(10, 10, None, n_timesteps=T, architecture='gvp', rec_encoder_type='fixed',
                                  graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dict(GVP_ALL_ATOM, n_convs=3),
                                  rec_encoder_config={'vector_size': 16}, precision=1e-5)
        cut, n_rec_feat, cfg = CUT, 10, dict(GVP_ALL_ATOM, n_convs=3, graph_cutoffs=CUT)
        forward = ogvp.gvp_dynamics_forward
        # with synthetic weights this denoiser's eps_x is small, so x-hat ~ z_t / alpha_t: a unit-variance start would put the
        # denoised ligand ~300 A wide and nowhere near the pocket.  Start at alpha_1 (~0.0032) times a 3 A cloud instead.
        start = 0.0032 * 3.0
    synth.fill_state_dict_(model, weights)
    model.eval()
    gs = synth.synth_complexes([60], [20], 20, cut, seed=77, n_rec_feat=n_rec_feat, density=synth.CA_DENSITY)
    shift = torch.tensor([[100.0, -80.0, 120.0]])
    gs[0].nodes['rec'].data['x_0'] += shift
    wall = gs[0].nodes['rec'].data['x_0'].clone()
    centre = gs[0].nodes['lig'].data['x_0'].mean(0, keepdim=True) + shift        # the state frame starts at the reference ligand
    g = model.encode_receptors(G.batch(gs))
    com0 = g.nodes['kp'].data['x_0'].mean(0, keepdim=True)
    gen = torch.Generator().manual_seed(5)
    g.nodes['kp'].data['x_0'] = g.nodes['kp'].data['x_0'] - centre
    x0 = start * torch.randn(20, 3, generator=gen)
    c = x0.mean(0, keepdim=True)
    g.nodes['lig'].data['x_0'], g.nodes['lig'].data['h_0'] = x0 - c, torch.randn(20, 10, generator=gen)
    g.nodes['kp'].data['x_0'] = g.nodes['kp'].data['x_0'] - c
    sd = {k[len('dynamics.'):]: v.clone() for k, v in model.state_dict().items() if k.startswith('dynamics.')}
    return model, g, wall, com0, gen, lambda ob, t: forward(sd, cfg, ob, t)


@pytest.mark.parametrize('arch', ['egnn', 'gvp'])
def test_anchored_guided_steps_with_a_real_denoiser(cuda, gemm_mode, arch):
    """Every one of the 10 steps is taken on the GPU from the state of a CPU trajectory (oracle denoiser + the fp64 restatement,
    same injected noise) and must agree with that trajectory's next state to 1e-4."""
    T = 10
    model, g, wall, com0, gen, denoise = anchored_setup(arch)
    ob = util.to_obatch(g)
    table = _table(T, 1e-5)
    model = model.to(cuda)
    ga = g.to(cuda)
    bidx = G.get_batch_idxs(ga)
    ctx = GuidanceContext(wall.to(cuda), torch.tensor([0, 60], device=cuda), com0.to(cuda), THR)
    one, worst, contacts = torch.ones(1), 0.0, []
    with torch.no_grad():
        for si in reversed(range(T)):
            s, t = one * (si / T), one * ((si + 1) / T)
            noise = [torch.randn(20, w, generator=gen) for w in (3, 10)]
            for key, src in (('x_0', ob.x['lig']), ('h_0', ob.h['lig'])):
                ga.nodes['lig'].data[key].copy_(src.to(cuda))
            ga.nodes['kp'].data['x_0'].copy_(ob.x['kp'].to(cuda))
            model.sample_p_zs_given_zt(s.to(cuda), t.to(cuda), ga, bidx, noise=tuple(n.to(cuda) for n in noise), guidance=ctx)
            eh, ex = denoise(ob, t)
            rx, rh, rk, info = ref_guided([20], [g.num_nodes('kp')], [60], ob.x['lig'], ob.h['lig'], ob.x['kp'], ex, eh, noise[0], noise[1],
                                          table[si:si + 1], wall, com0, THR)
            contacts.append(int((info['contacts'][0] > 0).sum()))
            errs = (util.rel_err(ga.nodes['lig'].data['x_0'], rx), util.rel_err(ga.nodes['lig'].data['h_0'], rh),
                    util.rel_err(ga.nodes['kp'].data['x_0'], rk))
            worst = max(worst, *errs)
            assert max(errs) < 1e-4, f's = {si}: rel err x {errs[0]:.3e} h {errs[1]:.3e} kp {errs[2]:.3e}'
            ob.x['lig'], ob.h['lig'], ob.x['kp'] = rx.float(), rh.float(), rk.float()
    print(f'anchored guided steps ({arch}): worst rel err {worst:.3e}; atoms in contact per step {contacts}')
    assert max(contacts) > 0                                     # the guidance had something to do


N_REC3, N_LIG3 = [90, 140, 60], [11, 17, 6]


def _encoded(model, dev, far=True, seed=3):
    """B = 3 ragged complexes with their reference ligands, moved ~100 A away from the origin (each complex elsewhere)."""
    gs = synth.synth_complexes(N_REC3, N_LIG3, 20, CUT, seed=seed)
    for i, g in enumerate(gs):
        shift = torch.tensor([[100.0 + 30 * i, -80.0, 120.0 - 50 * i]]) if far else torch.zeros(1, 3)
        g.nodes['rec'].data['x_0'] = g.nodes['rec'].data['x_0'] + shift
        g.nodes['lig'].data['x_0'] = 2.5 * g.nodes['lig'].data['x_0'] + shift
    return model.encode_receptors(G.batch(gs).to(dev))


@pytest.mark.parametrize('arch', ['egnn', 'gvp'])
def test_step_graph_replays_the_eager_guided_step(cuda, arch):
    T = 20
    model = _model(arch, T, 1e-5).to(cuda)
    g1, g2 = _encoded(model, cuda, far=False), _encoded(model, cuda, far=False)
    n = sum(N_LIG3)
    gen = torch.Generator().manual_seed(1)
    noise = tuple(torch.randn(n, w, generator=gen).to(cuda) for w in (3, 10))
    wx, wp = model.resolve_wall(g1)
    ctx = GuidanceContext(wx, wp, G.readout_nodes(g1, feat='x_0', op='mean', ntype='kp', ordered=True), THR)
    with torch.no_grad():
        sg = model.capture_step(g1, noise=noise, guidance=ctx)
        ones = torch.ones(3, device=cuda)
        for s in (19, 18, 7):
            sg.step(s / T, (s + 1) / T)
            model.sample_p_zs_given_zt(ones * (s / T), ones * ((s + 1) / T), g2, noise=noise, guidance=ctx)
            for nt, k in (('lig', 'x_0'), ('lig', 'h_0'), ('kp', 'x_0')):
                assert torch.equal(g1.nodes[nt].data[k], g2.nodes[nt].data[k]), (s, nt, k)
    pos, _ = model.sample_from_encoded_receptors(_encoded(model, cuda), use_graph=True, guidance=ClashGuidance(THR))
    assert all(torch.isfinite(p).all() for p in pos)


def _as_wall(pos, dev):
    """Ligands as a wall for a batch: (wall_x, wall_ptr)."""
    return torch.cat(pos).to(dev), torch.tensor([0] + [p.shape[0] for p in pos]).cumsum(0)


def test_loop_properties(cuda):
    """With synthetic weights the sampler does not put its ligands into the pocket, so the pocket's atoms never meet them.  The
    wall that is sure to be met is the unguided result itself: the denoised positions end up there, within the 10 A used here."""
    T, thr = 10, 10.0
    model = _model('egnn', T).to(cuda).use_complex_noise(99)
    ids = torch.tensor([40, 41, 42])
    run = lambda **kw: model.sample_from_encoded_receptors(_encoded(model, cuda), complex_ids=ids, **kw)
    pos, feat = run()
    # scale = 0: the unguided run
    zp, zf = run(guidance=ClashGuidance(THR, scale=0.0))
    assert _same(pos + feat, zp + zf)
    # scale > 0: finite, different ligands; the same seed twice gives the same bits
    obstacle = _as_wall(pos, cuda)
    gp, gf = run(guidance=ClashGuidance(thr, wall=obstacle))
    assert all(torch.isfinite(p).all() for p in gp + gf) and not _same(pos, gp)
    assert [tuple(p.shape) for p in gp] == [(k, 3) for k in N_LIG3]
    assert _same(gp + gf, sum(run(guidance=ClashGuidance(thr, wall=obstacle)), []))
    s0, s1 = model.clash_score(pos, pos, thr), model.clash_score(gp, pos, thr)
    print(f'clash energy against the unguided ligands: unguided {s0[:, 0].tolist()}, guided {s1[:, 0].tolist()}')
    assert s0.shape == (3, 3) and s1.shape == (3, 3) and s0[:, 1].tolist() >= [float(k) for k in N_LIG3]      # every atom meets itself
    gp, gf = run(guidance=ClashGuidance(THR))                    # the default wall, for the comparison below
    # an explicit wall: the keypoints of the batch (what None resolves to after the fixed encoder) give the run above
    g = _encoded(model, cuda)
    wall = (g.nodes['kp'].data['x_0'].clone(), g.node_ptr('kp'))
    ep, ef = model.sample_from_encoded_receptors(g, complex_ids=ids, guidance=ClashGuidance(THR, wall=wall))
    assert _same(gp + gf, ep + ef)
    # t_max = 0.5: the first half of the trajectory is the unguided one (frames 0 .. T / 2: the start and steps t = 1 .. 0.6)
    vx, vh = run(visualize=True)
    hx, hh = run(visualize=True, guidance=ClashGuidance(thr, t_max=0.5, wall=obstacle))
    assert all(len(tr) == T + 1 for tr in hx)
    for a, b in zip(vx + vh, hx + hh):
        assert _same(a[:T // 2 + 1], b[:T // 2 + 1])
    assert not _same([tr[-1] for tr in vx], [tr[-1] for tr in hx])
    # guided, around known atoms: the known rows come back exactly, the free rows differ from the unguided inpainting
    n = sum(N_LIG3)
    fixed = (torch.arange(n) % 3 == 0).to(cuda)
    g = _encoded(model, cuda)
    X, H = g.nodes['lig'].data['x_0'].cpu(), g.nodes['lig'].data['h_0'].cpu()
    up, _ = model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed, complex_ids=ids, resamplings=2)
    ip, if_ = model.inpaint_from_encoded_receptors(g, fixed, complex_ids=ids, guidance=ClashGuidance(thr, wall=_as_wall(up, cuda)),
                                                   resamplings=2)
    fx = fixed.cpu()
    assert torch.equal(torch.cat(ip)[fx], X[fx]) and torch.equal(torch.cat(if_)[fx], H[fx]) and torch.isfinite(torch.cat(ip)).all()
    assert not torch.equal(torch.cat(ip), torch.cat(up))
    zp, _ = model.inpaint_from_encoded_receptors(_encoded(model, cuda), fixed, complex_ids=ids, resamplings=2,
                                                 guidance=ClashGuidance(THR, scale=0.0))
    assert _same(zp, up)


def _pocket(dev, n_rec=70, seed=9):
    pocket = synth.synth_complexes([n_rec], [1], 20, CUT, seed=seed)[0].to(dev)
    pocket.remove_nodes(pocket.nodes('lig'), ntype='lig')
    return pocket


def test_pocket_entry_points(cuda):
    model = _model('egnn', 10).to(cuda).use_complex_noise(4)
    sizes = torch.tensor([6, 4, 9])
    base = model.sample_given_pocket(_pocket(cuda), sizes, diff_batch_size=2)
    none = model.sample_given_pocket(_pocket(cuda), sizes, diff_batch_size=2, guidance=ClashGuidance(THR, scale=0.0))
    assert _same(base[0] + base[1], none[0] + none[1])
    met = model.sample_given_pocket(_pocket(cuda), sizes, diff_batch_size=2, guidance=ClashGuidance(10.0, wall=torch.cat(base[0])))
    assert all(torch.isfinite(p).all() for p in met[0]) and not _same(met[0], base[0])       # a wall where the ligands end up is met
    pos, feat = model.sample_given_pocket(_pocket(cuda), sizes, diff_batch_size=2, guidance=ClashGuidance(THR))
    assert [tuple(p.shape) for p in pos] == [(6, 3), (4, 3), (9, 3)] and all(torch.isfinite(p).all() for p in pos)
    # wall=None is the pocket's receptor atoms as given
    rec = _pocket(cuda).nodes['rec'].data['x_0'].clone()
    same = model.sample_given_pocket(_pocket(cuda), sizes, diff_batch_size=2, guidance=ClashGuidance(THR, wall=rec))
    assert _same(pos + feat, same[0] + same[1])
    gen = torch.Generator().manual_seed(2)
    kpos, kfeat = 1.5 * torch.randn(4, 3, generator=gen), torch.randn(4, 10, generator=gen)
    ip, if_ = model.inpaint_given_pocket(_pocket(cuda), kpos, kfeat, torch.tensor([6, 9]), guidance=ClashGuidance(THR, wall=rec.cpu()))
    for p, f in zip(ip, if_):
        assert torch.equal(p[:4], kpos) and torch.equal(f[:4], kfeat) and torch.isfinite(p).all()
    score = model.clash_score(pos, rec, THR)
    assert score.shape == (3, 3) and score.device.type == 'cpu' and bool((score[:, 1] == score[:, 1].round()).all())


def test_guided_sample_sharded_equals_single_process(cuda):
    """`_sample(..., guidance=...)` on two thread ranks: every rank returns all ligands in input order, equal to the single-process
    run of the same seed under the comparison the plain sharded tests apply."""
    from . import sharded_worker as W
    from .test_sampler_gpu import _assert_samples_equal

    def run(rank=None, **kw):
        model = W.build_model(cuda).use_complex_noise(W.SEED)
        return model._sample(W.pockets(cuda), W.N_LIG, rec_enc_batch_size=2, diff_batch_size=2, **kw)

    plain = run()
    guide = ClashGuidance(10.0, wall=[torch.cat(p['positions']) for p in plain])     # per pocket: where its unguided ligands ended up
    ref = run(guidance=guide)
    assert [len(r['positions']) for r in ref] == [len(sizes) for sizes in W.N_LIG]
    assert any(not torch.equal(a, b) for r, p in zip(ref, plain) for a, b in zip(r['positions'], p['positions']))
    for got in util.run_threaded_world(2, lambda rank: run(rank, guidance=guide)):
        _assert_samples_equal(got, ref)
    with pytest.raises(ValueError, match='per pocket'):
        run(guidance=ClashGuidance(THR, wall=[torch.zeros(3, 3)]))


def test_refusals(cuda):
    pb, t = _pb(N_LIG, N_KP, cuda), _inputs(5, WALLS[2], cuda)
    model = _model('egnn').to(cuda)
    # a CPU graph
    with pytest.raises(hip.KpdError, match='GPU'):
        host = _model('egnn')
        host.sample_from_encoded_receptors(_encoded(host, 'cpu'), guidance=ClashGuidance(THR))
    with pytest.raises(hip.KpdError):
        _run(pb, 5, {k: v.cpu() for k, v in t.items()})
    # a wall that does not fit the batch
    for key in ('wall_ptr', 'com0', 'coef9', 'eps_x'):
        bad = dict(t)
        bad[key] = t[key][:-1].contiguous()
        with pytest.raises(hip.KpdError):
            _run(pb, 5, bad)
    with pytest.raises(hip.KpdError, match='wall_x'):
        _run(pb, 5, dict(t, wall_x=t['wall_x'][:, :2].contiguous()))
    with pytest.raises(hip.KpdError, match='wall_ptr'):
        _run(pb, 5, dict(t, wall_ptr=t['wall_ptr'].long()))
    g = _encoded(model, cuda)
    with pytest.raises(hip.KpdError, match='wall_ptr'):
        model.sample_from_encoded_receptors(g, guidance=ClashGuidance(THR, wall=(torch.zeros(4, 3), torch.tensor([0, 4]))))
    with pytest.raises(hip.KpdError, match='all or none'):
        hip.sample_update_guided(pb, 5, t['lig_x'].clone(), t['lig_h'].clone(), t['kp_x'].clone(), t['eps_x'], t['eps_h'], t['nx'], t['nh'],
                                 t['coef9'], t['wall_x'], t['wall_ptr'], t['com0'], THR, fixed=t['fixed'])
    # wall_ptr not ascending: refused by the wrapper itself, before any launch
    with pytest.raises(hip.KpdError, match='ascend'):
        _run(pb, 5, dict(t, wall_ptr=t['wall_ptr'].flip(0).contiguous()))
    down = torch.tensor([0, 3, 2, 4], device=cuda)
    with pytest.raises(hip.KpdError, match='ascend'):
        model.sample_from_encoded_receptors(g, guidance=ClashGuidance(THR, wall=(torch.zeros(4, 3, device=cuda), down)))
    with pytest.raises(hip.KpdError, match='ascend'):
        GuidanceContext(torch.zeros(4, 3, device=cuda), down, torch.zeros(3, 3, device=cuda), THR)
    lig_ptr = torch.tensor([0, 2, 3, 5], dtype=torch.int32, device=cuda)
    with pytest.raises(hip.KpdError, match='ascend'):
        hip.clash_score(torch.zeros(5, 3, device=cuda), lig_ptr, torch.zeros(4, 3, device=cuda), down.int(), THR)
    # a non-positive threshold
    for thr in (0.0, -1.0):
        with pytest.raises(ValueError, match='threshold'):
            ClashGuidance(thr)
        with pytest.raises(hip.KpdError, match='threshold'):
            hip.sample_update_guided(pb, 5, t['lig_x'].clone(), t['lig_h'].clone(), t['kp_x'].clone(), t['eps_x'], t['eps_h'], t['nx'],
                                     t['nh'], t['coef9'], t['wall_x'], t['wall_ptr'], t['com0'], thr)
        with pytest.raises(hip.KpdError, match='threshold'):
            hip.clash_score(torch.zeros(5, 3, device=cuda), lig_ptr, torch.zeros(4, 3, device=cuda), down.int().sort().values, thr)
    with pytest.raises(hip.KpdError):                            # the C side checks too
        hip.check(hip.lib().kpd_clash_score(3, lig_ptr.data_ptr(), t['lig_x'].data_ptr(), lig_ptr.data_ptr(), t['wall_x'].data_ptr(), 0.0,
                                            t['lig_x'].data_ptr(), None))
