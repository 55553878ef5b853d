"""Addressing of the fused EGNN edge kernels (k_egnn_edge<4>, k_egnn_edge_kpt): a wave's row endpoints are scalar loads, both
branches' gathers are scalar row base + lane offset, and the run tests of the segmented sum are scalar.  None of that changes a
float, so the checks are oracle parity at the suite's tolerance and bitwise repeatability at the shapes where addressing can go wrong:
tiles with fewer rows than a wave owns (clamped rows), edge-type boundaries and runs that continue across tiles, destination nodes
without in-edges of a type, the tail split into feature-only / coordinate-only work items, and the layer-0 class-table gather."""
import pytest
import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import synth
from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
from oracle import egnn as oegnn

from . import util

pytestmark = pytest.mark.gpu
CUT = util.CUTOFFS_ALL_ATOM
TOL = 1e-4          # the suite's tolerance against the oracle (BASELINE.json: "within 1e-4 rel fp32")
T_STEPS = 20
TINY2 = ([7], [2])                          # every tile has 1 .. 15 rows: waves 1 - 3 of a tile own no valid row
TINY3 = ([7], [3])
RAGGED = ([5, 40, 130], [2, 9, 30])         # edge-type boundaries inside the tile range, runs across tiles, nodes without in-edges of a type
SPLIT = ([120, 90], [12, 30])               # a launch whose tiles all fall into the split last round (asserted below)


@pytest.fixture(scope='module')
def kd(cuda):
    m = KeypointDiffusion(10, 10, None, n_timesteps=T_STEPS, architecture='egnn', rec_encoder_type='fixed',
                          graph_config=dict(n_keypoints=20, graph_cutoffs=CUT), dynamics_config=util.EGNN_C2, precision=1e-5)
    synth.fill_state_dict_(m, 17)
    m.eval()
    m.oracle_sd = {k[len('dynamics.'):]: v.clone() for k, v in m.state_dict().items() if k.startswith('dynamics.')}
    return m.to(cuda)


def _batch(shape, seed=4321):
    return util.fixed_encode(util.make_batch(*shape, seed=seed))


def _times(B):
    return (torch.arange(B, dtype=torch.float32) + 1) / (B + 1)


def _forward(kd, gd):
    with torch.no_grad():
        h, x = kd.dynamics(gd, _times(gd.batch_size).to(gd.device), None)
    return h.clone(), x.clone()


def _parity_and_repeat(kd, cuda, shape):
    g = _batch(shape)
    ref = oegnn.egnn_dynamics_forward(kd.oracle_sd, dict(util.EGNN_C2, graph_cutoffs=CUT), util.to_obatch(g), _times(g.batch_size))
    gd = g.to(cuda)
    h1, x1 = _forward(kd, gd)
    h2, x2 = _forward(kd, gd)
    eh, ex = util.rel_err(h1, ref[0]), util.rel_err(x1, ref[1])
    print(f'{shape}: rel err vs oracle eps_h {eh:.3e} eps_x {ex:.3e}')
    assert eh < TOL and ex < TOL, (eh, ex)
    assert torch.equal(h1, h2) and torch.equal(x1, x2)
    return gd, (h1, x1)


@pytest.mark.parametrize('shape', [TINY2, TINY3], ids=['lig2', 'lig3'])
def test_tiles_smaller_than_a_waves_rows(cuda, kd, shape):
    _parity_and_repeat(kd, cuda, shape)
    c = kd.dynamics.engine().last_counts()
    assert 1 <= c['E_ll'] < 16 and 1 <= c['E_kl'] < 64 and c['E_kk'] < 64, c      # one partial tile per edge type


def test_ragged_batch(cuda, kd):
    _parity_and_repeat(kd, cuda, RAGGED)


def test_tail_split_work_items(cuda, kd):
    """The tile count as the engine computes it (64-edge tiles per edge type) and the split rule of the launcher: the remainder of an
    XCD's share over its workgroup slots (two per CU, an eighth of them per XCD) is non-zero and at most half the slots, so its tiles
    run as one feature-only and one coordinate-only work item each."""
    _parity_and_repeat(kd, cuda, SPLIT)
    c = kd.dynamics.engine().last_counts()
    tiles = sum((c[k] + 63) // 64 for k in ('E_ll', 'E_kl', 'E_lk', 'E_kk'))
    assert tiles == c['tiles'], (tiles, c)
    slots = 2 * torch.cuda.get_device_properties(cuda).multi_processor_count // 8
    rem = ((tiles + 7) // 8) % slots
    assert 0 < rem <= slots // 2, (tiles, slots, rem)


def test_table_and_prune_switches_are_bit_identical(cuda, kd):
    gd, (h, x) = _parity_and_repeat(kd, cuda, RAGGED)
    eng = kd.dynamics.engine()
    assert float(eng.debug('kp_table_ok', 1, device=cuda)[0]) == 1.0       # layer 0 gathered from the class table
    for off, on in (('kp_table=0', 'kp_table=1'), ('prune=0', 'prune=1')):
        eng.debug(off)
        try:
            h0, x0 = _forward(kd, gd)
        finally:
            eng.debug(on)
        assert torch.equal(h, h0) and torch.equal(x, x0), off
    h1, x1 = _forward(kd, gd)
    assert torch.equal(h, h1) and torch.equal(x, x1)


def test_step_graph_replays_equal_eager(cuda, kd):
    """One captured step graph, replayed twice, against the eager reverse steps on a twin batch."""
    g1 = _batch(RAGGED).to(cuda)
    g2 = _batch(RAGGED).to(cuda)
    gen = torch.Generator().manual_seed(5)
    nx = torch.randn(g1.num_nodes('lig'), 3, generator=gen).to(cuda)
    nh = torch.randn(g1.num_nodes('lig'), 10, generator=gen).to(cuda)
    ones = torch.ones(g1.batch_size, device=cuda)
    with torch.no_grad():
        sg = kd.capture_step(g1, noise=(nx, nh))
        for s in (19, 18):
            kd.sample_p_zs_given_zt(ones * (s / T_STEPS), ones * ((s + 1) / T_STEPS), g2, noise=(nx, nh))
            sg.step(s / T_STEPS, (s + 1) / T_STEPS)
            for nt, k in (('lig', 'x_0'), ('lig', 'h_0'), ('kp', 'x_0')):
                assert torch.equal(g1.nodes[nt].data[k], g2.nodes[nt].data[k]), (s, nt, k)
