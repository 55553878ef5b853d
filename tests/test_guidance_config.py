"""Clash guidance, the parts that need no GPU: the host mirror of the guided-step coefficients against an independent fp64
formula, the validation of `ClashGuidance`, the wall-resolution rules, and that a host graph is refused, never computed."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip, synth
from keypoint_diffusion_amd.ligand_diffuser import ClashGuidance, GuidanceContext, KeypointDiffusion
from oracle import diffusion as odiff

from . import util

CUT = util.CUTOFFS_ALL_ATOM
GRID = [(10, 1e-4), (10, 1e-5), (1000, 1e-4), (1000, 1e-5)]


def _model(T=10, precision=1e-4):
    m = KeypointDiffusion(10, 10, None, n_timesteps=T, architecture='egnn', rec_encoder_type='fixed',
                          graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dict(util.EGNN_C2, n_layers=1),
                          precision=precision)
    return m.eval()


def fp64_guided_coefficients(T, precision, scale=1.0, t_max=1.0):
    """[T,9] in fp64 for (s, t) = (i / T, (i + 1) / T), from the variance-preserving identities alpha^2 = sigmoid(-gamma),
    sigma^2 = sigmoid(gamma), alpha_t|s = alpha_t / alpha_s, sigma^2_t|s = sigma_t^2 - alpha_t|s^2 sigma_s^2 -- not the
    softplus / expm1 route the product takes.  Column 8 = scale alpha_s sigma^2_t|s / sigma_t^2 up to round(t_max T)."""
    table = odiff.gamma_table(T, precision).double()
    i = torch.arange(T)
    g_s, g_t = table[i], table[i + 1]
    a_s, a_t, s_s, s_t = (torch.sqrt(torch.sigmoid(x)) for x in (-g_s, -g_t, g_s, g_t))
    a_ts = a_t / a_s
    s2_ts = s_t ** 2 - a_ts ** 2 * s_s ** 2
    w = torch.where(i + 1 <= round(t_max * T), scale * a_s * s2_ts / s_t ** 2, torch.zeros_like(a_s))
    ref = torch.stack([a_ts, s2_ts / a_ts / s_t, torch.sqrt(s2_ts) * s_s / s_t, a_s, s_s, torch.sqrt(s2_ts), a_t, s_t, w], dim=1)
    return i.float() / T, (i.float() + 1) / T, ref


def max_rel(got, ref):
    return float(((got.double() - ref).abs() / ref.abs().clamp_min(1e-6)).max())


@pytest.mark.parametrize('T,precision', GRID)
def test_host_guided_coefficients_all_timesteps(T, precision):
    m = _model(T, precision)
    s, t, ref = fp64_guided_coefficients(T, precision, scale=0.75)
    got = m.guided_coefficients(s, t, 0.75, 1.0)
    assert got.shape == (T, 9) and got.dtype == torch.float32 and got.is_contiguous()
    err = max_rel(got, ref)
    print(f'T={T} precision={precision}: max rel err {err:.2e}, weight / scale in [{float(ref[:, 8].min()) / 0.75:.4g}, '
          f'{float(ref[:, 8].max()) / 0.75:.4g}]')
    assert err < 1e-4
    assert torch.equal(got[:, :6], m.inpaint_coefficients(s, t)) and torch.equal(got[:, :3], m.step_coefficients(s, t))
    # the weight of x-hat in the posterior mean stays of order one: nothing blows up at t ~ 1 (include/kpd.h quotes the range)
    lo, hi = (0.19, 0.9995) if T == 10 else (3.9e-4, 0.36)
    w = ref[:, 8] / 0.75
    assert lo * 0.99 <= float(w.min()) and float(w.max()) <= hi * 1.01


@pytest.mark.parametrize('T', [10, 1000])
def test_weight_is_exactly_zero_above_t_max_and_for_scale_zero(T):
    m = _model(T)
    s, t, _ = fp64_guided_coefficients(T, 1e-4)
    on = m.guided_coefficients(s, t, 1.0, 1.0)
    assert bool((on[:, 8] > 0).all())
    half = m.guided_coefficients(s, t, 1.0, 0.5)
    idx = torch.round(t * T).long()
    assert torch.equal(half[idx > T // 2, 8], torch.zeros(int((idx > T // 2).sum())))
    assert torch.equal(half[idx <= T // 2, 8], on[idx <= T // 2, 8])
    assert torch.equal(half[:, :8], on[:, :8])
    off = m.guided_coefficients(s, t, 0.0, 1.0)
    assert torch.equal(off[:, 8], torch.zeros(T)) and torch.equal(off[:, :8], on[:, :8])
    assert torch.equal(m.guided_coefficients(s, t, 2.0, 1.0)[:, 8], 2.0 * on[:, 8])


def test_clash_guidance_validates_its_numbers():
    c = ClashGuidance(3)
    assert (c.threshold, c.scale, c.t_max, c.wall) == (3.0, 1.0, 1.0, None)
    assert ClashGuidance(2.5, scale=0, t_max=1).scale == 0.0
    for bad in (0, -1.0, float('nan'), float('inf'), '3', None, True):
        with pytest.raises(ValueError, match='threshold'):
            ClashGuidance(bad)
    for bad in (-0.1, float('nan'), 'x'):
        with pytest.raises(ValueError, match='scale'):
            ClashGuidance(3.0, scale=bad)
    for bad in (0, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError, match='t_max'):
            ClashGuidance(3.0, t_max=bad)
    m = _model()
    s, t = torch.tensor([0.3]), torch.tensor([0.4])
    with pytest.raises(ValueError, match='scale'):
        m.guided_coefficients(s, t, -1.0, 1.0)
    with pytest.raises(ValueError, match='t_max'):
        m.guided_coefficients(s, t, 1.0, 0.0)
    w = c.with_wall([torch.zeros(2, 3)])
    assert w.wall is not None and c.wall is None and (w.threshold, w.scale, w.t_max) == (3.0, 1.0, 1.0)


def _encoded(m, n_rec=(30, 22), n_lig=(5, 7)):
    return m.encode_receptors(G.batch(synth.synth_complexes(list(n_rec), list(n_lig), 20, CUT, seed=4)))


def test_wall_resolution_on_encoded_batches():
    m = _model()
    g = G.batch(synth.synth_complexes([30, 22], [5, 7], 20, CUT, seed=4))
    rec = g.nodes['rec'].data['x_0'].clone()
    wx, wp = m.resolve_wall(g)                                   # None: the receptor rows of the batch
    assert torch.equal(wx, rec) and wp.dtype == torch.int32 and wp.tolist() == [0, 30, 52] and wx.dtype == torch.float32
    wx[0, 0] += 1.0
    assert torch.equal(g.nodes['rec'].data['x_0'], rec)          # a copy: the loop may not move the caller's atoms
    g = _encoded(m)                                              # the fixed encoder made the atoms keypoints: no receptor rows left
    assert g.num_nodes('rec') == 0
    kx, kp_ptr = m.resolve_wall(g)
    assert torch.equal(kx, g.nodes['kp'].data['x_0']) and kp_ptr.tolist() == [0] + g.batch_num_nodes('kp').cumsum(0).tolist()
    mine = (torch.randn(7, 3, dtype=torch.float64), torch.tensor([0, 0, 7]))
    wx, wp = m.resolve_wall(g, mine)                             # explicit: checked against the batch, a complex may have none
    assert torch.equal(wx, mine[0].float()) and wp.tolist() == [0, 0, 7] and wp.dtype == torch.int32
    with pytest.raises(hip.KpdError, match='wall_ptr'):
        m.resolve_wall(g, (mine[0], torch.tensor([0, 7])))       # does not fit the batch of two
    with pytest.raises(hip.KpdError, match='ascend'):
        m.resolve_wall(g, (mine[0], torch.tensor([0, 8, 7])))
    with pytest.raises(hip.KpdError, match='ascend'):
        m.resolve_wall(g, (mine[0], torch.tensor([0, 3, 6])))    # does not end at n_wall
    with pytest.raises(hip.KpdError, match='ascend'):
        m.resolve_wall(g, (mine[0], torch.tensor([1, 3, 7])))
    with pytest.raises(hip.KpdError, match='wall_x'):
        m.resolve_wall(g, (torch.zeros(7, 2), torch.tensor([0, 0, 7])))
    with pytest.raises(ValueError, match='wall'):
        m.resolve_wall(g, mine[0])


def test_wall_resolution_per_pocket():
    m = _model()
    pockets = synth.synth_complexes([30, 22], [1, 1], 20, CUT, seed=9)
    walls = m.resolve_pocket_walls(pockets)                      # None: each pocket's receptor atoms as given
    assert len(walls) == 2 and all(torch.equal(w, p.nodes['rec'].data['x_0']) for w, p in zip(walls, pockets))
    mine = [torch.randn(4, 3), torch.zeros(0, 3)]
    assert all(torch.equal(a, b) for a, b in zip(m.resolve_pocket_walls(pockets, mine), mine))
    with pytest.raises(ValueError, match='per pocket'):
        m.resolve_pocket_walls(pockets, mine[:1])
    with pytest.raises(ValueError, match='per pocket'):
        m.resolve_pocket_walls(pockets, mine[0])
    with pytest.raises(ValueError, match=r'wall\[1\]'):
        m.resolve_pocket_walls(pockets, [mine[0], torch.zeros(3)])


def test_guidance_context_checks_the_wall():
    ctx = GuidanceContext(torch.zeros(5, 3), torch.tensor([0, 2, 5]), torch.zeros(2, 3), 3.0, 0.5, 0.25)
    assert ctx.wall_ptr.dtype == torch.int32 and (ctx.threshold, ctx.scale, ctx.t_max) == (3.0, 0.5, 0.25)
    with pytest.raises(hip.KpdError, match='wall_ptr'):
        GuidanceContext(torch.zeros(5, 3), torch.tensor([0, 2, 5]), torch.zeros(3, 3), 3.0)
    with pytest.raises(hip.KpdError, match='ascend'):
        GuidanceContext(torch.zeros(5, 3), torch.tensor([0, 6, 5]), torch.zeros(2, 3), 3.0)
    with pytest.raises(ValueError, match='threshold'):
        GuidanceContext(torch.zeros(5, 3), torch.tensor([0, 2, 5]), torch.zeros(2, 3), 0.0)
    with pytest.raises(ValueError, match='kp_com0'):
        GuidanceContext(torch.zeros(5, 3), torch.tensor([0, 2, 5]), torch.zeros(2), 3.0)


def test_host_graphs_are_refused_not_computed():
    m = _model()
    guide = ClashGuidance(3.0)
    with pytest.raises(hip.KpdError, match='GPU'):
        m.sample_from_encoded_receptors(_encoded(m), guidance=guide)
    g = _encoded(m)
    with pytest.raises(hip.KpdError, match='GPU'):
        m.inpaint_from_encoded_receptors(g, torch.zeros(g.num_nodes('lig'), dtype=torch.bool), guidance=guide)
    pocket = synth.synth_complexes([30], [1], 20, CUT, seed=9)[0]
    pocket.remove_nodes(pocket.nodes('lig'), ntype='lig')
    with pytest.raises(hip.KpdError, match='GPU'):
        m.sample_given_pocket(pocket, torch.tensor([6]), guidance=guide)
    with pytest.raises(hip.KpdError, match='GPU'):
        m.inpaint_given_pocket(pocket, torch.zeros(2, 3), torch.zeros(2, 10), torch.tensor([6]), guidance=guide)
    g = _encoded(m)
    ctx = GuidanceContext(*m.resolve_wall(g), torch.zeros(2, 3), 3.0)
    with pytest.raises(hip.KpdError, match='GPU'):
        m.sample_p_zs_given_zt(torch.tensor([0.3, 0.3]), torch.tensor([0.4, 0.4]), g, guidance=ctx)
    with pytest.raises(hip.KpdError, match='GPU'):
        m.clash_score([torch.zeros(4, 3)], torch.zeros(5, 3), 3.0)
    for bad in (3.0, ctx):                                       # the loop takes a ClashGuidance, the step a GuidanceContext
        with pytest.raises(ValueError, match='guidance'):
            m.sample_from_encoded_receptors(_encoded(m), guidance=bad)
    with pytest.raises(ValueError, match='guidance'):
        m.sample_p_zs_given_zt(torch.tensor([0.3, 0.3]), torch.tensor([0.4, 0.4]), g, guidance=guide)


def test_unguided_calls_are_what_they_were(monkeypatch):
    """`guidance=None`: the step makes one `hip.sample_update` call and none into the new entry points."""
    calls = []
    for name in ('sample_update', 'sample_update_guided', 'guided_coefficients', 'clash_score'):
        getattr(hip, name)
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: calls.append(_n))

    class Denoiser(torch.nn.Module):
        def forward(self, g, t, batch_idxs=None):
            n = g.num_nodes('lig')
            return torch.zeros(n, 10), torch.zeros(n, 3)

    m = _model()
    m.dynamics = Denoiser()
    m.sample_p_zs_given_zt(torch.tensor([0.3, 0.3]), torch.tensor([0.4, 0.4]), _encoded(m), guidance=None)
    assert calls == ['sample_update']
