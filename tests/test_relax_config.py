"""The relaxation rule of include/kpd.h as restated in tests/relax_ref.py, checked on the CPU against things that are true
whatever the implementation: the gradient is the derivative of the energy, the non-bonded term is continuous at the soft core and
at the cutoff, hand-made geometries relax to their known minima, the energy never rises.  Also the fixture condition of the GPU
trajectory test (every decision margin of the chosen seeds is >= 1e-9) and the Python surface's argument checks."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import molecule_ref as MR
from . import relax_ref as R
from .molecule_cases import ALLOWED, ELEMENTS, Z, one_hot
from .relax_cases import LIG_VDW, MINIMA, TRAJ_SEEDS, grow, make_pocket, measure, ring6, traj_case, vdw_rows

NONE = np.zeros((0, 3), dtype=np.float32), np.zeros((0, 2), dtype=np.float32)


def prepared(sym, pos):
    """Topology and per-atom vdW rows of a ligand, bonds from the restated bond rule."""
    m = MR.perceive(pos, one_hot(sym), Z, ALLOWED)
    z_atoms = [Z[c] for c in m['elem']]
    return R.topology(pos, z_atoms, m['bonds']), LIG_VDW[m['elem']]


def params(**kw):
    p = dict(R.DEFAULTS)
    p.update(kw)
    return p


@pytest.mark.parametrize('seed,n,m', [(1, 12, 0), (2, 17, 30), (3, 25, 60), (4, 1, 10), (5, 2, 0)])
def test_gradient_is_the_derivative_of_the_energy(seed, n, m):
    rng = np.random.default_rng(seed)
    sym, pos = grow(rng, n)
    topo, lv = prepared(sym, pos)
    psym, ppos = make_pocket(rng, m, pos) if m else ([], NONE[0])
    pv = vdw_rows(psym)
    P = params()
    x = pos.astype(np.float64) + 0.05 * rng.standard_normal(pos.shape)       # off the sampled geometry: every term has a force
    got = R.energy(x, topo, lv, ppos, pv, P)
    h = 1e-6
    for _ in range(12):
        i, c = int(rng.integers(n)), int(rng.integers(3))
        xp, xm = x.copy(), x.copy()
        xp[i, c] += h
        xm[i, c] -= h
        num = (R.energy(xp, topo, lv, ppos, pv, P)['E'] - R.energy(xm, topo, lv, ppos, pv, P)['E']) / (2 * h)
        # central differences: truncation h^2 f''' / 6 and rounding eps * abs_E / h, both far below this
        assert abs(num - got['g'][i, c]) <= 1e-5 * max(1.0, got['abs_g'][i]), (i, c, num, got['g'][i, c])
    rev = R.energy(x, topo, lv, ppos, pv, P, reverse=True)
    assert abs(rev['E'] - got['E']) <= 1e-11 * got['abs_E'] + 1e-300
    assert np.all(np.abs(rev['parts'] - got['parts']) <= 1e-11 * got['abs_E'] + 1e-300)


def test_soft_core_and_cutoff_are_continuous():
    P = params()
    x, D = np.float64(3.7), np.float64(0.09)
    for edge in (P['s'] * x, P['r_c']):
        d = edge * (1.0 + np.array([-1e-9, 1e-9]))
        e, k = R._lj(d * d, np.array([x, x]), np.array([D, D]), P)
        slope = max(abs(k[0] * d[0]), abs(k[1] * d[1]), 1.0)
        assert abs(e[1] - e[0]) <= 4e-9 * edge * slope, (edge, e)
    e, k = R._lj(np.array([P['r_c'] ** 2, 1e-14, 0.0]), np.array([x] * 3), np.array([D] * 3), P)
    assert e[0] == 0.0 and k[0] == 0.0                      # nothing at or beyond the cutoff
    assert np.isfinite(e[1:]).all() and k[1] == 0.0 and k[2] == 0.0 and e[1] > 0      # coincident: energy, no force
    d = np.array([P['s'] * x * 0.5])
    e1, k1 = R._lj(d * d, np.array([x]), np.array([D]), P)
    e2, k2 = R._lj((d + 1e-6) ** 2, np.array([x]), np.array([D]), P)
    assert abs((e2 - e1) / 1e-6 - k1 * d) <= 1e-4 * abs(k1 * d)      # inside the core the energy is a straight line in d


@pytest.mark.parametrize('case', MINIMA, ids=[c[0] for c in MINIMA])
def test_known_minima(case):
    name, sym, pos, bonds, angles = case
    topo, lv = prepared(sym, pos)
    assert len(topo['bonds']) == len(bonds), name
    r = R.minimize(pos, topo, lv, *NONE, params(w_intra=0.0, gtol=1e-7))
    L, A = measure(r['x'], bonds, angles)
    for k, v in bonds.items():
        assert abs(L[k] - v) < 1e-5, (name, k, L[k])        # |force| = k_b |d - r0| <= gtol, plus the fp32 rounding of a kept angle
    for k, v in angles.items():
        # E = 1/2 k_a (cos t - cos t0)^2: near 180 degrees the force is cubic in the deviation, (2 r gtol / k_a)^(1/3) ~ 0.07 degrees
        assert abs(A[k] - v) < (0.2 if v == 180.0 else 1e-3), (name, k, A[k])
    assert r['E'] <= 1e-9 and r['iters'] < 100 and not r['status'] & (R.NO_MOLECULE | R.BAD_INPUT), (name, r['E'], r['status'])


def test_lone_atom_settles_at_the_pair_minimum():
    pos = np.array([[0.3, -0.2, 0.5]], dtype=np.float32)
    dirn = np.array([1.0, 2.0, -2.0]) / 3.0
    ppos = (pos[0].astype(np.float64) + 2.0 * dirn).astype(np.float32).reshape(1, 3)
    topo = R.topology(pos, [6], np.zeros((0, 2), dtype=np.int64))
    lv, pv = vdw_rows(['C']), vdw_rows(['O'])
    r = R.minimize(pos, topo, lv, ppos, pv, params(gtol=1e-8))
    xij = np.sqrt(np.float64(lv[0, 0])) * np.sqrt(np.float64(pv[0, 0]))
    v = r['x64'][0] - ppos[0].astype(np.float64)           # the minimiser's own point: the rows written are its fp32 rounding
    d = np.linalg.norm(v)
    assert abs(d - xij) < 1e-6, (d, xij)                    # e'' = 72 D / x^2 ~ 0.4: |d - x| <= gtol / e''
    d0 = pos[0].astype(np.float64) - ppos[0].astype(np.float64)
    assert np.linalg.norm(np.cross(v / d, d0 / np.linalg.norm(d0))) < 1e-9        # along the line joining them
    assert v @ d0 > 0 and r['iters'] < 100


def test_noisy_six_ring_ends_planar_with_aromatic_rest_values():
    sym, pos = ring6(np.random.default_rng(6))
    topo, lv = prepared(sym, pos)
    assert len(topo['bonds']) == 6 and np.all(topo['r0'] == 1.42) and np.all(topo['cls'] == 2) and len(topo['A']) == 6
    r = R.minimize(pos, topo, lv, *NONE, params(w_intra=0.0, gtol=1e-7))
    bonds = {(int(i), int(j)): 1.42 for i, j in topo['bonds']}
    angles = {(int(a), int(c), int(b)): 120.0 for a, c, b in zip(topo['A'], topo['C'], topo['B'])}
    L, A = measure(r['x'], bonds, angles)
    assert max(abs(L[k] - 1.42) for k in L) < 1e-6 and max(abs(A[k] - 120.0) for k in A) < 1e-4
    assert np.all(r['x'][:, 2] == 0.0) and r['iters'] < 100


@pytest.mark.parametrize('seed', [21, 22, 23])
def test_energy_never_rises(seed):
    rng = np.random.default_rng(seed)
    sym, pos = grow(rng, int(rng.integers(8, 20)))
    topo, lv = prepared(sym, pos)
    psym, ppos = make_pocket(rng, 50, pos)
    r = R.minimize(pos, topo, lv, ppos, vdw_rows(psym), params(max_iters=80))
    h = np.array(r['history'])
    assert len(h) > 5 and np.all(h[1:] <= h[:-1]) and r['E'] < r['E_before']
    assert r['gmax'] <= R.DEFAULTS['gtol'] or r['status'] & (R.ITER_CAP | R.LINE_SEARCH)
    rev = R.minimize(pos, topo, lv, ppos, vdw_rows(psym), params(max_iters=3), reverse=True)
    fwd = R.minimize(pos, topo, lv, ppos, vdw_rows(psym), params(max_iters=3))
    assert np.abs(rev['x64'] - fwd['x64']).max() < 1e-9     # the order of the sums is no part of the rule


@pytest.mark.parametrize('seed', TRAJ_SEEDS)
def test_trajectory_seeds_have_no_coin_toss_decisions(seed):
    """The fixture condition of test_relax_gpu.py::test_trajectory: over the first five iterations every decision of the
    minimiser, and every rest-value choice, is at least 1e-9 away from its threshold."""
    sym, pos, psym, ppos = traj_case(seed)
    topo, lv = prepared(sym, pos)
    assert min(topo['margins']) >= 1e-9
    for K in (1, 2, 5):
        for reverse in (False, True):
            r = R.minimize(pos, topo, lv, ppos, vdw_rows(psym), params(max_iters=K), reverse=reverse)
            assert r['iters'] == K and R.min_margin(r['margins']) >= 1e-9, (seed, K, sorted(r['margins'], key=lambda t: t[1])[:3])


def test_exports_and_argument_checks():
    assert 'kpd_relax' in hip.EXPORTS and 'kpd_relax_defaults' in hip.EXPORTS
    p = hip.relax_params(max_iters=7, gtol=1e-4)
    assert (p.k_b, p.k_a, p.r_c, p.s, p.w_intra, p.gtol, p.max_step, p.max_iters) == (700.0, 200.0, 10.0, 0.6, 1.0, 1e-4, 0.2, 7)
    d = hip.relax_params()
    assert {k: getattr(d, k) for k in R.DEFAULTS} == R.DEFAULTS
    with pytest.raises(hip.KpdError):
        hip.relax_params(k_bond=1.0)
    with pytest.raises(hip.KpdError):
        hip.relax_params(s=1.5)
    with pytest.raises(hip.KpdError):
        molecule.vdw_table(['C', 'Xx'])
    assert molecule.vdw_table(['C', 'Xx'], {'Xx': (3.0, 0.1)}) == [list(molecule.VDW_PARAMS['C']), [3.0, 0.1]]
    with pytest.raises(hip.KpdError):
        molecule.vdw_table(['C'], {'C': (-1.0, 0.1)})
    # host tensors: there is no CPU implementation
    e = torch.zeros(3, dtype=torch.int32)
    mols = molecule.Molecules(torch.tensor([0, 3], dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32), e[:1], e, e, e,
                              torch.zeros(9, 2, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), torch.tensor([0, 0], dtype=torch.int32),
                              torch.zeros(3, 3), ['C', 'N', 'O'])
    with pytest.raises(hip.KpdError):
        mols.relax([torch.zeros(4, 3)], [['C'] * 4])
    with pytest.raises(ValueError):
        mols.relax([torch.zeros(4, 3)], [['C'] * 4, ['C']])
    with pytest.raises(hip.KpdError):
        molecule.relax_samples([dict(positions=[torch.zeros(3, 3)], features=[torch.zeros(3, 3)])],
                               [dict(positions=torch.zeros(4, 3), elements=['C'] * 4)], ['C', 'N', 'O'])
