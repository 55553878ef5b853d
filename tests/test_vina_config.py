"""The scoring function of include/kpd.h as restated in tests/vina_ref.py, checked against values worked out by hand, against
central differences and against its invariances; and the host-side surface (radii table, parameters).  No GPU is needed."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import vina_ref as R
from .molecule_cases import ALLOWED, ELEMENTS, Z, one_hot
from .molecule_ref import perceive
from .vina_cases import (A, D, GRAD_SEEDS, H, ROTOR_GRAPHS, TYPED, biphenyl, ethylbenzene, gly_ser_pro, grad_case, radii_of, z_of)

KINKS = np.array([-0.7, 0.0, 0.5, 1.5])
W = np.array([R.DEFAULTS[k] for k in R.WEIGHTS])


def pair(r, ti, tj, Ri=1.9, Rj=1.9, n_rot=0, params=None):
    """Unweighted terms of one ligand atom at the origin and one pocket atom at (r, 0, 0)."""
    e = R.evaluate(np.zeros((1, 3), np.float32), [ti], [Ri], np.array([[r, 0, 0]], np.float32), [tj], [Rj], n_rot, params)
    return e['terms'] / W, e


def test_two_atom_values_by_hand():
    t, e = pair(3.8, H, H)                                # d = 0 up to the fp32 rounding of 3.8 and 1.9
    assert abs(e['d'][0, 0]) < 1e-6
    assert np.allclose(t, [1.0, np.exp(-2.25), 0.0, 1.0, 0.0], rtol=0, atol=1e-5)
    t, e = pair(3.3, H, H)                                # d = -0.5
    assert abs(t[2] - 0.25) < 1e-6 and t[3] == 1.0 and t[4] == 0.0
    assert abs(t[0] - np.exp(-1.0)) < 1e-6 and abs(t[1] - np.exp(-3.0625)) < 1e-6
    # O(A) .. N(D): radii 1.7 and 1.8
    for r, want in ((3.15, 0.5), (2.8, 1.0), (2.5, 1.0), (3.5, 0.0), (3.6, 0.0)):
        for ti, tj, Ri, Rj in ((A, D, 1.7, 1.8), (D, A, 1.8, 1.7), (D | A, D | A, 1.7, 1.8)):
            t, _ = pair(r, ti, tj, Ri, Rj)
            assert abs(t[4] - want) < 1e-6 and t[3] == 0.0, (r, ti, tj, t)
    for ti, tj in ((D, D), (A, A), (H, D), (0, A), (H | D, H | D)):
        assert pair(2.8, ti, tj, 1.7, 1.8)[0][4] == 0.0
    # hydrophobic ramp, and only between two H atoms
    assert abs(pair(4.8, H, H)[0][3] - 0.5) < 1e-6 and pair(5.4, H, H)[0][3] == 0.0 and pair(3.8, H, D)[0][3] == 0.0
    # the rotor normalisation and the weights
    _, e0 = pair(3.3, H, H)
    _, e3 = pair(3.3, H, H, n_rot=3)
    assert e3['inter'] == e0['inter'] and abs(e3['score'] - e0['inter'] / (1 + 3 * 0.05846)) < 1e-15
    assert abs(e0['inter'] - (W * pair(3.3, H, H)[0]).sum()) < 1e-15
    # an atom that takes no part
    assert not pair(3.3, -1, H)[1]['terms'].any() and not pair(3.3, H, -1)[1]['terms'].any() and not pair(3.3, H, H, Rj=0.0)[1]['terms'].any()


def test_cutoff_is_decided_on_d2():
    below = np.nextafter(np.float32(8.0), np.float32(0.0))
    t8, e8 = pair(8.0, H, H)
    tb, eb = pair(below, H, H)
    assert e8['d2'][0, 0] == 64.0 and not e8['on'].any() and not t8.any()
    assert eb['on'].all()
    d = float(below) - np.float64(np.float32(1.9)) * 2
    assert abs(tb[0] - np.exp(-(d / 0.5) ** 2)) < 1e-15 and abs(tb[1] - np.exp(-((d - 3) / 2) ** 2)) < 1e-12 and tb[1] > 0.5
    # another cutoff moves the edge
    assert not pair(6.0, H, H, params=dict(r_c=6.0))[1]['on'].any() and pair(6.0, H, H, params=dict(r_c=6.5))[1]['on'].all()


@pytest.mark.parametrize('case', TYPED, ids=[c[0] for c in TYPED])
def test_ligand_typing(case):
    name, sym, pos, want = case
    m = perceive(pos, one_hot(sym), Z, ALLOWED)
    got = R.ligand_types(z_of(sym), m['bonds'], m['order'], radii_of(sym))
    assert got.tolist() == want, (name, got)
    # overrides are honoured where they are >= 0; a radius of 0 or Z = 1 leaves an atom out whatever its flags
    over = np.full(len(sym), -1)
    over[0] = 7
    got2 = R.ligand_types(z_of(sym), m['bonds'], m['order'], radii_of(sym), over)
    assert got2[0] == 7 and got2[1:].tolist() == want[1:]
    rad = radii_of(sym).copy()
    rad[0] = 0.0
    assert R.ligand_types(z_of(sym), m['bonds'], m['order'], rad, over)[0] == -1


def test_pocket_typing_of_gly_ser_pro():
    names, sym, pos, bonds, want = gly_ser_pro()
    adj, order = R.pocket_bonds(pos, z_of(sym))
    assert {(int(i), int(j)) for i, j in zip(*np.nonzero(np.triu(adj)))} == bonds
    for a, b in bonds:
        carbonyl = {names[a].split()[1], names[b].split()[1]} == {'C', 'O'}
        assert order[a, b] == (2 if carbonyl else 1), (names[a], names[b], order[a, b])
    types, status = R.pocket_types(pos, z_of(sym))
    assert status == 0 and {n: int(t) for n, t in zip(names, types)} == want
    # a zinc ion nearby is a donor and has no neighbours; a hydrogen takes no part and is no neighbour
    far = pos.max(axis=0) + np.float32(4.0)
    h = pos[names.index('PRO CG')] + np.array([0.0, 0.0, 1.09], dtype=np.float32)
    t2, _ = R.pocket_types(np.concatenate([pos, [far, h]]), np.concatenate([z_of(sym), [30, 1]]))
    assert t2[-2] == D and t2[-1] == -1 and t2[:-2].tolist() == types.tolist()
    # a non-finite atom: status bit 1, no neighbours, type -1; CA loses its N neighbour and becomes hydrophobic
    bad = pos.copy()
    bad[names.index('GLY N'), 1] = np.nan
    t3, st3 = R.pocket_types(bad, z_of(sym))
    assert st3 == 2 and t3[names.index('GLY N')] == -1 and t3[names.index('GLY CA')] == H


@pytest.mark.parametrize('case', ROTOR_GRAPHS, ids=[c[0] for c in ROTOR_GRAPHS])
def test_rotor_counts(case):
    name, z, bonds, orders, want = case
    assert R.rotors(z, bonds, orders) == want, name


def test_rotor_counts_of_perceived_geometries():
    rng = np.random.default_rng(4)
    for make, n_bonds, want in ((biphenyl, 13, 1), (ethylbenzene, 8, 1)):
        sym, pos = make(rng)
        m = perceive(pos, one_hot(sym), Z, ALLOWED)
        assert len(m['order']) == n_bonds and R.rotors(z_of(sym), m['bonds'], m['order']) == want


def scored(seed, pos=None, ppos=None, psym=None, **kw):
    sym, p, ps, pp = grad_case(seed)
    ps = ps if psym is None else psym
    m = perceive(p, one_hot(sym), Z, ALLOWED)
    return R.score_ligand(p if pos is None else pos, z_of(sym), m['bonds'], m['order'], radii_of(sym), pp if ppos is None else ppos,
                          z_of(ps), radii_of(ps), **kw)


@pytest.mark.parametrize('seed', GRAD_SEEDS)
def test_gradient_against_central_differences(seed):
    sym, pos, psym, ppos = grad_case(seed)
    e = scored(seed)
    near = e['d2'] < 81.0
    margin = min(np.abs(e['d'][near][:, None] - KINKS).min(), np.abs(np.sqrt(e['d2']) - 8.0).min())
    assert margin >= 1e-3, (seed, margin)                 # the seeds were chosen for this on the CPU; none is skipped
    assert e['on'].sum() > 100 and np.abs(e['terms']).min() > 0 and e['n_rot'] >= 1
    h, x = 1e-5, pos.astype(np.float64)
    num = np.zeros_like(x)
    for a in range(x.shape[0]):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[a, c] += h
            xm[a, c] -= h
            num[a, c] = (scored(seed, pos=xp, ptypes=e['ptypes'])['score'] - scored(seed, pos=xm, ptypes=e['ptypes'])['score']) / (2 * h)
    # h^2 / 6 times third derivatives of order 1e2 per unit of gradient contribution
    worst = (np.abs(num - e['grad']) / e['abs_grad'].clip(1e-300)).max()
    print(f'seed {seed}: worst |numeric - analytic| / sum|contributions| = {worst:.2e}')
    assert worst <= 1e-6
    # atom scores add up to inter
    assert abs(e['atom_score'].sum() - e['inter']) <= 1e-12 * e['abs_terms']


def test_invariances_of_the_restatement():
    seed = GRAD_SEEDS[0]
    sym, pos, psym, ppos = grad_case(seed)
    e = scored(seed)
    tol = 1e-12 * e['abs_terms']
    # a rigid motion of ligand and pocket together (in float64: the types are those of the unmoved pocket)
    rng = np.random.default_rng(0)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    shift = np.array([3.0, -2.0, 5.0])
    moved = R.evaluate(pos.astype(np.float64) @ q.T + shift, e['types'], radii_of(sym), ppos.astype(np.float64) @ q.T + shift, e['ptypes'],
                       radii_of(psym), e['n_rot'])
    assert np.abs(moved['terms'] - e['terms']).max() <= tol and abs(moved['score'] - e['score']) <= tol
    assert np.abs(moved['grad'] - e['grad'] @ q.T).max() <= 1e-12 * e['abs_grad'].max()
    # a permutation of the pocket atoms
    perm = rng.permutation(len(psym))
    p2 = scored(seed, ppos=ppos[perm], psym=[psym[k] for k in perm])
    assert np.array_equal(p2['ptypes'], e['ptypes'][perm]) and np.abs(p2['terms'] - e['terms']).max() <= tol
    assert np.abs(p2['grad'] - e['grad']).max() <= 1e-12 * e['abs_grad'].max()
    # one more pocket atom far away
    far = np.concatenate([ppos, ppos.max(axis=0, keepdims=True) + np.float32(30.0)])
    p3 = scored(seed, ppos=far, psym=list(psym) + ['C'])
    assert np.abs(p3['terms'] - e['terms']).max() <= tol and np.array_equal(p3['grad'], e['grad'])


def test_python_surface():
    assert molecule.XS_RADII['C'] == 1.9 and molecule.XS_RADII['Zn'] == 1.2 and 'B' not in molecule.XS_RADII
    assert molecule.xs_radius_table(['C', 'N', 'Zn']) == [1.9, 1.8, 1.2]
    assert molecule.xs_radius_table(['C', 'Xx'], {'Xx': 2.5, 'C': 1.0}) == [1.0, 2.5]
    with pytest.raises(hip.KpdError):
        molecule.xs_radius_table(['C', 'Xx'])
    with pytest.raises(hip.KpdError):
        molecule.xs_radius_table(['C'], {'C': float('nan')})
    p = hip.vina_params()
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS       # the restatement and the library agree on the defaults
    assert hip.vina_params(r_c=6.5, w_rot=0.0).r_c == 6.5
    for bad in (dict(r_cut=8.0), dict(r_c=-1.0), dict(r_c=0.0), dict(w_rot=-0.1), dict(w_hbond=float('inf'))):
        with pytest.raises(hip.KpdError):
            hip.vina_params(**bad)
    assert hip.VINA_REPORT == ('score', 'inter', 'gauss1', 'gauss2', 'repulsion', 'hydrophobic', 'hbond', 'n_rot')
    assert (hip.VINA_NO_MOLECULE, hip.VINA_BAD_INPUT, hip.VINA_ATOM_OUT) == (R.NO_MOLECULE, R.BAD_INPUT, R.ATOM_OUT)
    # tensors on the host are refused: there is no CPU implementation
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    host = molecule.Molecules(i32(0, 2), i32(1, 1, 2, 0).reshape(1, 4), i32(0), i32(0, 0), i32(1, 1), i32(0, 0), i32(0, 1).reshape(1, 2),
                              i32(1), i32(0, 1), torch.tensor([[0.0, 0, 0], [1.5, 0, 0]]), ELEMENTS)
    with pytest.raises(hip.KpdError):
        host.vina_score([torch.zeros(3, 3)], [['C', 'N', 'O']])
    with pytest.raises(hip.KpdError):
        hip.vina_pocket_types(torch.zeros(3, 3), i32(6, 7, 8), i32(0, 3))
