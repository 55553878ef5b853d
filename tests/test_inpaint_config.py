"""Inpainting (sampling around fixed atoms), the parts that need no GPU: the host mirror of the step coefficients against the
oracle's schedule arithmetic, the argument validation of the public entry points, and that the plain reverse step makes the
calls it made before the feature existed."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import hip, synth
from keypoint_diffusion_amd.ligand_diffuser import InpaintContext, KeypointDiffusion
from oracle import diffusion as odiff

from . import util

CUT = util.CUTOFFS_ALL_ATOM


def _model(T=10, precision=1e-4, norm=1.0):
    m = KeypointDiffusion(10, 10, None, n_timesteps=T, architecture='egnn', rec_encoder_type='fixed',
                          graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=dict(util.EGNN_C2, n_layers=1),
                          precision=precision, lig_feat_norm_constant=norm)
    return m.eval()


def oracle_coefficients(T, precision):
    """[T,6] = {alpha_t|s, var, sigma_step, alpha_s, sigma_s, sigma_t|s} for (s, t) = (i / T, (i + 1) / T), from oracle.diffusion."""
    table = odiff.gamma_table(T, precision)
    s = torch.arange(T, dtype=torch.float32) / T
    t = (torch.arange(T, dtype=torch.float32) + 1) / T
    g_s, g_t = odiff.gamma_at(table, s, T), odiff.gamma_at(table, t, T)
    s2, s_ts, a_ts = odiff.sigma_and_alpha_t_given_s(g_t, g_s)
    ref = torch.stack([a_ts, s2 / a_ts / odiff.sigma(g_t), s_ts * odiff.sigma(g_s) / odiff.sigma(g_t),
                       odiff.alpha(g_s), odiff.sigma(g_s), s_ts], dim=1)
    return s, t, ref.float()


@pytest.mark.parametrize('T', [10, 1000])
@pytest.mark.parametrize('precision', [1e-4, 1e-5])
def test_host_inpaint_coefficients_all_timesteps(T, precision):
    m = _model(T, precision)
    s, t, ref = oracle_coefficients(T, precision)
    got = m.inpaint_coefficients(s, t)
    assert got.shape == (T, 6) and got.dtype == torch.float32 and got.is_contiguous()
    assert float(((got - ref).abs() / ref.abs().clamp_min(1e-6)).max()) < 1e-4
    assert torch.equal(got[:, :3], m.step_coefficients(s, t))
    if precision == 1e-4:                                        # the figures the frame-bookkeeping bound quotes
        assert abs(float(got[0, 4]) - 0.01) < 1e-5 and abs(float(got[0, 3]) - 0.99995) < 1e-6


def _encoded(m, n_rec=(30, 22), n_lig=(5, 7)):
    return m.encode_receptors(G.batch(synth.synth_complexes(list(n_rec), list(n_lig), 20, CUT, seed=4)))


def test_validation_errors_name_the_argument():
    m = _model()
    g = _encoded(m)
    n = g.num_nodes('lig')
    ok = torch.zeros(n, dtype=torch.bool)
    with pytest.raises(ValueError, match='fixed'):
        m.inpaint_from_encoded_receptors(g, torch.zeros(n + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match='fixed'):
        m.inpaint_from_encoded_receptors(g, torch.zeros(n, 1, dtype=torch.bool))
    with pytest.raises(ValueError, match='fixed'):
        m.inpaint_from_encoded_receptors(g, torch.zeros(n, dtype=torch.float32))
    with pytest.raises(ValueError, match='fixed'):
        m.inpaint_from_encoded_receptors(g, torch.zeros(n, dtype=torch.int64))
    for r in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='resamplings'):
            m.inpaint_from_encoded_receptors(g, ok, resamplings=r)
    g.nodes['lig'].data['h_0'] = torch.zeros(n, 9)
    with pytest.raises(ValueError, match='atom_nf'):
        m.inpaint_from_encoded_receptors(g, ok)
    # a host graph: refused, never computed on the CPU
    with pytest.raises(hip.KpdError, match='GPU'):
        m.inpaint_from_encoded_receptors(_encoded(m), ok)
    with pytest.raises(hip.KpdError, match='GPU'):
        m.inpaint_from_encoded_receptors(_encoded(m), ok.to(torch.uint8), resamplings=2, overwrite_fixed=False)


def test_validation_of_known_atoms_per_pocket():
    m = _model()
    pocket = synth.synth_complexes([30], [1], 20, CUT, seed=9)[0]
    pocket.remove_nodes(pocket.nodes('lig'), ntype='lig')
    pos, feat = torch.zeros(4, 3), torch.zeros(4, 10)
    with pytest.raises(ValueError, match='known_feat'):
        m.inpaint_given_pocket(pocket, pos, torch.zeros(4, 9), torch.tensor([6]))
    with pytest.raises(ValueError, match='known_feat'):
        m.inpaint_given_pocket(pocket, pos, torch.zeros(3, 10), torch.tensor([6]))
    with pytest.raises(ValueError, match='known_pos'):
        m.inpaint_given_pocket(pocket, torch.zeros(4, 2), feat, torch.tensor([6]))
    with pytest.raises(ValueError, match='n_lig_atoms'):
        m.inpaint_given_pocket(pocket, pos, feat, torch.tensor([6, 3]))          # 3 < 4 known atoms
    with pytest.raises(ValueError, match='resamplings'):
        m.inpaint_given_pocket(pocket, pos, feat, torch.tensor([6]), resamplings=0)
    with pytest.raises(ValueError, match='known'):
        m._sample([pocket], [[6]], known=[(pos, feat), (pos, feat)])
    with pytest.raises(ValueError, match='atom_nf'):
        m._sample([pocket], [[6]], known=[(pos, torch.zeros(4, 11))])
    with pytest.raises(hip.KpdError, match='GPU'):                               # valid arguments, host pocket
        m.inpaint_given_pocket(pocket, pos, feat, torch.tensor([6]))


def test_context_checks_its_tensors():
    with pytest.raises(ValueError, match='fixed'):
        InpaintContext(torch.zeros(5), torch.zeros(5, 3), torch.zeros(5, 10), torch.zeros(1, 3))
    with pytest.raises(ValueError, match='inpaint'):
        InpaintContext(torch.zeros(5, dtype=torch.bool), torch.zeros(4, 3), torch.zeros(5, 10), torch.zeros(1, 3))
    c = InpaintContext(torch.tensor([True, False]), torch.zeros(2, 3), torch.zeros(2, 10), torch.zeros(1, 3))
    assert c.fixed.dtype == torch.uint8 and c.fixed.tolist() == [1, 0]


class _Recorder:
    def __init__(self, monkeypatch):
        self.calls = []
        for name in ('sample_update', 'step_coefficients', 'sample_update_inpaint', 'inpaint_coefficients', 'sample_renoise',
                     'complex_noise'):
            getattr(hip, name)                                   # AttributeError without the feature
            monkeypatch.setattr(hip, name, self._record(name))

    def _record(self, name):
        def f(*args, **kw):
            self.calls.append((name, args, kw))
            if name.endswith('coefficients'):
                return torch.zeros(args[1].shape[0], 3 if name == 'step_coefficients' else 6)
        return f


class _Denoiser(torch.nn.Module):
    def forward(self, g, t, batch_idxs=None):
        n = g.num_nodes('lig')
        return torch.full((n, 10), 0.25), torch.full((n, 3), -0.5)


def test_plain_step_makes_the_calls_it_made_before(monkeypatch):
    """`inpaint=None`: one `hip.sample_update` with the [B,3] coefficients, no call into any of the new entry points.  (On host
    tensors the coefficients come from the torch mirror, so `hip.step_coefficients` is not called either -- as before.)"""
    m = _model()
    m.dynamics = _Denoiser()
    g = _encoded(m)
    rec = _Recorder(monkeypatch)
    s, t = torch.tensor([0.3, 0.3]), torch.tensor([0.4, 0.4])
    nx, nh = torch.randn(12, 3), torch.randn(12, 10)
    before = {k: g.nodes['lig'].data[k] for k in ('x_0', 'h_0')}
    out = m.sample_p_zs_given_zt(s, t, g, None, noise=(nx, nh))
    assert out is g and [c[0] for c in rec.calls] == ['sample_update']
    _, args, kw = rec.calls[0]
    assert not kw and len(args) == 10 and args[0] is g.prepared() and args[1] == 10
    assert args[2] is before['x_0'] and args[3] is before['h_0'] and args[4] is g.nodes['kp'].data['x_0']
    assert float(args[5][0, 0]) == -0.5 and float(args[6][0, 0]) == 0.25 and args[7] is nx and args[8] is nh
    assert torch.equal(args[9], m.step_coefficients(s, t)) and args[9].shape == (2, 3)
    # default noise: two global draws, positions first
    rec.calls.clear()
    torch.manual_seed(3)
    m.sample_p_zs_given_zt(s, t, g)
    torch.manual_seed(3)
    want = (torch.randn(12, 3), torch.randn(12, 10))
    assert [c[0] for c in rec.calls] == ['sample_update']
    assert torch.equal(rec.calls[0][1][7], want[0]) and torch.equal(rec.calls[0][1][8], want[1])


def test_inpaint_step_call_and_draw_order(monkeypatch):
    m = _model()
    m.dynamics = _Denoiser()
    g = _encoded(m)
    rec = _Recorder(monkeypatch)
    s, t = torch.tensor([0.3, 0.3]), torch.tensor([0.4, 0.4])
    ctx = InpaintContext(torch.arange(12) % 2 == 0, torch.randn(12, 3), torch.randn(12, 10), torch.zeros(2, 3))
    torch.manual_seed(5)
    m.sample_p_zs_given_zt(s, t, g, inpaint=ctx)
    m.renoise_zt_given_zs(s, t, g)
    torch.manual_seed(5)
    want = [torch.randn(12, w) for w in (3, 10, 3, 10, 3, 10)]     # step x, step h, known x, known h, re-noise x, re-noise h
    assert [c[0] for c in rec.calls] == ['sample_update_inpaint', 'sample_renoise']
    a = rec.calls[0][1]
    assert len(a) == 16 and torch.equal(a[9], m.inpaint_coefficients(s, t)) and a[9].shape == (2, 6)
    assert a[10] is ctx.fixed and a[11] is ctx.x and a[12] is ctx.h and a[13] is ctx.kp_com0
    for got, w in zip((a[7], a[8], a[14], a[15]), want[:4]):
        assert torch.equal(got, w)
    r = rec.calls[1][1]
    assert len(r) == 8 and torch.equal(r[5], want[4]) and torch.equal(r[6], want[5]) and r[7].shape == (2, 6)
    # a 4-tuple is used as given; a 2-tuple is completed with the known-part draws
    rec.calls.clear()
    m.sample_p_zs_given_zt(s, t, g, inpaint=ctx, noise=tuple(want[:4]))
    assert all(x is y for x, y in zip((rec.calls[0][1][7], rec.calls[0][1][8], rec.calls[0][1][14], rec.calls[0][1][15]), want[:4]))
    with pytest.raises(ValueError, match='noise'):
        m.sample_p_zs_given_zt(s, t, g, inpaint=ctx, noise=tuple(want[:3]))


def test_per_complex_tag_layout(monkeypatch):
    """Repetition u of step s: tags 6u, 6u + 1 (step), 6u + 2, 6u + 3 (known part), 6u + 4, 6u + 5 (re-noise), counter step s."""
    m = _model().use_complex_noise(7)
    m.dynamics = _Denoiser()
    g = _encoded(m)
    rec = _Recorder(monkeypatch)
    monkeypatch.setattr(hip, 'complex_noise', lambda pb, width, ids, seed, step, tag: rec.calls.append(('noise', width, seed, step, tag))
                        or torch.zeros(12, width))
    s, t = torch.tensor([0.3, 0.3]), torch.tensor([0.4, 0.4])
    ctx = InpaintContext(torch.zeros(12, dtype=torch.bool), torch.zeros(12, 3), torch.zeros(12, 10), torch.zeros(2, 3))
    ids = torch.tensor([4, 5])
    m.sample_p_zs_given_zt(s, t, g, complex_ids=ids, step=3, inpaint=ctx, repetition=2)
    m.renoise_zt_given_zs(s, t, g, complex_ids=ids, step=3, repetition=2)
    assert [c[1:] for c in rec.calls if c[0] == 'noise'] == [(3, 7, 3, 12), (10, 7, 3, 13), (3, 7, 3, 14), (10, 7, 3, 15),
                                                             (3, 7, 3, 16), (10, 7, 3, 17)]


def test_ordered_segment_sums():
    """The set-up means of the loop: a fixed summation order, so a segment's sum has the same bits whatever else is in the batch
    (and from call to call, which index_add_ on a GPU does not give); empty segments are 0; the value is the fp64 sum to fp32
    rounding of a 300-term sum."""
    from keypoint_diffusion_amd import graph as G
    gen = torch.Generator().manual_seed(4)
    counts = [1, 0, 5, 300, 64, 65, 0]
    x = 100.0 + 5.0 * torch.randn(sum(counts), 3, generator=gen)
    got = G.segment_sum_ordered(x, torch.tensor(counts))
    assert got.shape == (7, 3) and got.dtype == torch.float32
    for b, part in enumerate(x.split(counts)):
        want = part.double().sum(0)
        assert float((got[b].double() - want).abs().max()) <= 300 * 2.0 ** -24 * float(part.abs().sum(0).max())
        alone = G.segment_sum_ordered(part, torch.tensor([part.shape[0]]))
        assert torch.equal(alone[0], got[b]), b
    assert torch.equal(got[1], torch.zeros(3)) and torch.equal(got[0], x[0])
    assert G.segment_sum_ordered(torch.zeros(0, 3), torch.zeros(0, dtype=torch.long)).shape == (0, 3)
    m = _model()
    g = _encoded(m)
    for nt in ('kp', 'lig', 'rec'):
        a, b = G.readout_nodes(g, feat='x_0', op='mean', ntype=nt, ordered=True), G.readout_nodes(g, feat='x_0', op='mean', ntype=nt)
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-5)
