"""The float64 restatement of kpd_vina_minimize (tests/vina_min_ref.py) against hand-written torsion trees, central differences
and the invariants of the chart.  No GPU: these are the checks that make the restatement a yardstick for test_vina_min_gpu.py,
and the place where the seeds of its gradient and trajectory tests are qualified."""
import numpy as np
import pytest

from . import molecule_ref as MR
from . import vina_min_ref as R
from . import vina_ref as V
from .molecule_cases import ALLOWED, Z, one_hot
from .vina_cases import radii_of, z_of
from .vina_min_cases import GRAD_SEEDS, TRAJ_SEEDS, TREES, case, hexane, mixed_batch, traj_case, tree_molecule

KINKS = np.array([-0.7, 0.0, 0.5, 1.5])
# the deviation between the restatement and its reversed-sum twin over TRAJ_SEEDS and K = 1, 2, 5 (test_vina_min_gpu.py allows the
# kernel 100 x this, with a floor of 1e-9 A)
TRAJ_MEASURED_DEV = 1.5e-14


def perceived(sym, pos):
    m = MR.perceive(pos, one_hot(sym), Z, ALLOWED)
    assert m['status'] == 0
    return z_of(sym), m['bonds'], m['order'], m['frag']


def setup(sym, pos, psym, ppos, max_rotors=64):
    """Everything `R.minimize` needs for one ligand in one pocket."""
    z, bonds, orders, frag = perceived(sym, pos)
    types = V.ligand_types(z, bonds, orders, radii_of(sym))
    return dict(t=R.tree(z, bonds, orders, frag, max_rotors, types), types=types, radius=radii_of(sym), ppos=ppos,
                ptypes=V.pocket_types(ppos, z_of(psym))[0], pradius=radii_of(psym))


def run(s, pos, params=None, reverse=False):
    return R.minimize(pos, s['t'], s['types'], s['radius'], s['ppos'], s['ptypes'], s['pradius'], params, reverse)


def energy(s, x):
    return R.evaluate(x, s['t'], s['types'], s['radius'], s['ppos'], s['ptypes'], s['pradius'])


@pytest.mark.parametrize('entry', TREES, ids=[e[0] for e in TREES])
def test_trees_and_pair_lists_by_hand(entry):
    name, bonds, frag, rotors, moved, depth, piece, pairs = entry
    n = len(frag)
    t = R.tree([6] * n, bonds, [1] * len(bonds), frag)
    assert t['rotors'] == rotors and t['n_rot'] == len(rotors) == t['T'] and t['F'] == max(frag) + 1
    assert [set(np.nonzero(m)[0].tolist()) for m in t['M']] == moved and t['depth'].tolist() == depth
    assert t['order'] == sorted(range(len(rotors)), key=lambda k: -depth[k])
    assert t['piece'].tolist() == piece and R.pair_list(t) == pairs
    if name in ('a rotor whose far side holds the lowest atom',):
        return
    sym, pos = tree_molecule(name)                           # the bond rule finds the same graph in the coordinates
    z, b, o, f = perceived(sym, pos)
    assert b.tolist() == [list(p) for p in bonds] and f.tolist() == frag          # (a ring bond may come out as a length-class double)
    assert R.tree(z, b, o, f)['rotors'] == rotors
    frozen = R.tree(z, b, o, f, max_rotors=0)
    assert frozen['T'] == 0 and frozen['n_rot'] == len(rotors) and len(set(frozen['piece'].tolist())) == max(frag) + 1
    if name == 'hexane':                                     # the first rotor alone: the pieces {0, 1} and {2 .. 5}
        one = R.tree(z, b, o, f, max_rotors=1)
        assert one['rotors'] == [(1, 2)] and one['piece'].tolist() == [0, 0, 2, 2, 2, 2] and R.pair_list(one) == [(0, 4), (0, 5), (1, 5)]
    # an atom that takes no part has no pair
    off = R.tree(z, b, o, f, types=[-1] + [0] * (n - 1))
    assert all(0 not in p for p in R.pair_list(off))


def pair_margin(s, x):
    """The least distance of a pair, ligand x pocket or inside the ligand, from a kink of d or from the cutoff."""
    out = []
    for q, Q, on in ((s['ppos'].astype(np.float64), s['pradius'], None), (x, s['radius'], s['t']['pairs'])):
        r = np.linalg.norm(x[:, None, :] - q[None, :, :], axis=2)
        d = (r - s['radius'].astype(np.float64)[:, None]) - Q.astype(np.float64)[None, :]
        near = (r < 9.0) if on is None else (on & (r < 9.0))
        out += [np.abs(d[near][:, None] - KINKS).min(), np.abs(r[near] - 8.0).min()]
    return min(out)


@pytest.mark.parametrize('seed', GRAD_SEEDS)
def test_pose_gradient_against_central_differences(seed):
    sym, pos, psym, ppos = case(seed)
    s = setup(sym, pos, psym, ppos)
    t, x = s['t'], pos.astype(np.float64)
    assert pair_margin(s, x) >= 1e-3                         # the seeds were chosen for this on the CPU; none is skipped
    assert t['T'] >= 2 and len(R.pair_list(t)) >= 5 and t['depth'].max() >= 2
    e = energy(s, x)
    assert e['intra'] != 0.0 and e['inter'] != 0.0
    gd = R.project(x, e['g'], t)
    c = R.centres(x, t)
    D, h = len(gd), 1e-5
    assert D == 6 * t['F'] + t['T']
    worst = 0.0
    for d in range(D):
        step = np.zeros(D)
        step[d] = h
        num = (energy(s, R.move(x, step, t))['E'] - energy(s, R.move(x, -step, t))['E']) / (2 * h)
        if d < 6 * t['F']:                                   # the scale: the atoms' absolute gradient contributions times their levers
            idx = t['frag'] == d // 6
            lever = np.ones(idx.sum()) if d % 6 < 3 else np.linalg.norm(x[idx] - c[d // 6], axis=1)
        else:
            k = d - 6 * t['F']
            idx = t['M'][k]
            lever = np.linalg.norm(x[idx] - x[t['rotors'][k][1]], axis=1)
        scale = (e['abs_g'][idx] * lever).sum()
        worst = max(worst, abs(num - gd[d]) / max(scale, 1e-300))
    print(f'seed {seed}: D = {D}, worst |numeric - analytic| / sum|contributions| = {worst:.2e}')
    assert worst <= 1e-6                                     # h^2 / 6 times third derivatives of order 1e2 per unit of contribution
    # the first-order velocity is the derivative of move
    p = np.random.default_rng(seed).standard_normal(D)
    num = (R.move(x, h * p, t) - R.move(x, -h * p, t)) / (2 * h)
    assert np.abs(num - R.velocity(x, p, t)).max() <= 1e-6 * np.abs(p).max() * 30.0


def intra_piece_distances(x, piece):
    d = np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2)
    return d[piece[:, None] == piece[None, :]]


def test_move_is_the_exact_tree_kinematics():
    rng = np.random.default_rng(9)
    for sym, pos in (hexane(), tree_molecule('ethylbenzene'), tree_molecule('two ethanols + Cl'), case(GRAD_SEEDS[0])[:2]):
        z, bonds, orders, frag = perceived(sym, pos)
        t = R.tree(z, bonds, orders, frag)
        x = pos.astype(np.float64)
        D = 6 * t['F'] + t['T']
        delta = rng.standard_normal(D) * 0.4
        y = R.move(x, delta, t)
        assert np.abs(intra_piece_distances(y, t['piece']) - intra_piece_distances(x, t['piece'])).max() <= 1e-12
        bl = lambda v: np.linalg.norm(v[bonds[:, 0]] - v[bonds[:, 1]], axis=1)
        assert np.abs(bl(y) - bl(x)).max() <= 1e-12           # the rotor bonds join pieces: their lengths hold too
        assert np.abs(R.move(x, np.zeros(D), t) - x).max() <= 1e-14           # x_b + (x - x_b), c + (x - c): a rounding or two
        for k in range(t['T']):                              # a lone torsion moves its set and nothing else
            lone = np.zeros(D)
            lone[6 * t['F'] + k] = 0.7
            y1 = R.move(x, lone, t)
            far = np.abs(y1 - x).max(axis=1)
            assert (far[~t['M'][k]] <= 1e-14).all() and (far[t['M'][k]] > 1e-3).sum() >= t['M'][k].sum() - 1      # b_k lies on the axis
        # the deepest-first composition against a sequential rebuild: turn the shallowest rotor first and take every later axis
        # from the geometry already turned
        only_t = np.zeros(D)
        only_t[6 * t['F']:] = delta[6 * t['F']:]
        seq = x.copy()
        for k in reversed(t['order']):
            a, b = t['rotors'][k]
            u = (seq[b] - seq[a]) / np.linalg.norm(seq[b] - seq[a])
            th = delta[6 * t['F'] + k]
            for i in np.nonzero(t['M'][k])[0]:
                r = seq[i] - seq[b]
                seq[i] = seq[b] + r * np.cos(th) + np.cross(u, r) * np.sin(th) + u * (u @ r) * (1 - np.cos(th))
        assert np.abs(R.move(x, only_t, t) - seq).max() <= 1e-12


def test_minimisation_lowers_the_energy_and_keeps_the_pieces():
    ligs, pockets, pocket_of = mixed_batch()
    for b in (1, 2, 3, 6):
        sym, pos = ligs[b]
        psym, ppos = pockets[pocket_of[b]]
        s = setup(sym, pos, psym, ppos)
        out = run(s, pos, dict(max_iters=25))
        rep = out['report']
        assert rep['E_after'] <= rep['E_before'] and rep['iterations'] >= 1 and rep['evaluations'] >= rep['iterations'] + 2
        assert rep['rmsd'] > 0 and not out['status'] & 3
        y, x = out['x64'], pos.astype(np.float64)
        assert np.abs(intra_piece_distances(y, s['t']['piece']) - intra_piece_distances(x, s['t']['piece'])).max() <= 1e-11
        again = energy(s, out['pos_out'].astype(np.float64))
        assert again['E'] == rep['E_after'] and again['inter'] == rep['inter_after']
        rigid = setup(sym, pos, psym, ppos, max_rotors=0)
        out0 = run(rigid, pos, dict(max_iters=25))
        frag = rigid['t']['frag']
        assert np.abs(intra_piece_distances(out0['x64'], frag) - intra_piece_distances(x, frag)).max() <= 1e-11
        assert out0['report']['E_after'] <= out0['report']['E_before']
        assert bool(out0['status'] & R.FROZEN) == (s['t']['n_rot'] > 0) and out0['report']['n_active'] == 0


@pytest.mark.parametrize('seed', TRAJ_SEEDS)
def test_trajectory_seeds_take_no_coin_toss(seed):
    sym, pos, psym, ppos = traj_case(seed)
    s = setup(sym, pos, psym, ppos)
    assert s['t']['T'] >= 1
    for K in (1, 2, 5):
        ref, rev = run(s, pos, dict(max_iters=K)), run(s, pos, dict(max_iters=K), reverse=True)
        assert ref['report']['iterations'] == K
        assert R.min_margin(ref['margins'], ('converged', 'descent', 'armijo', 'pair', 'noise', 'round')) >= 1e-9, (seed, K)
        assert R.min_margin(ref['margins'], ('ulp',)) >= 1e-9
        for key in ('iterations', 'evaluations'):
            assert ref['report'][key] == rev['report'][key]
        assert ref['status'] == rev['status'] and np.array_equal(ref['pos_out'], rev['pos_out'])
        dev = np.abs(ref['x64'] - rev['x64']).max()
        print(f'seed {seed} K {K}: forward against reversed sums {dev:.2e} A, '
              f'|dE| {abs(ref["report"]["E_after"] - rev["report"]["E_after"]):.2e}')
        assert dev <= TRAJ_MEASURED_DEV
