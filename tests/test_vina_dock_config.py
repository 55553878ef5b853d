"""The float64 restatement of kpd_vina_dock (tests/vina_dock_ref.py) against the published Philox vectors, the invariants of a
mutation, the restatement of kpd_vina_minimize it is built on, and its own reversed-sum twin.  No GPU: these are the checks that
make the restatement a yardstick for test_vina_dock_gpu.py, and the place where its trajectory seeds are qualified."""
import math

import numpy as np
import pytest

from . import vina_dock_ref as D
from . import vina_min_ref as R
from . import vina_ref as V
from .test_vina_min_config import intra_piece_distances, perceived, run, setup
from .vina_cases import radii_of, z_of
from .vina_dock_cases import DOCK_PARAMS, DOCK_SEEDS, DOCK_SHAPE, dock_case, own_box
from .vina_min_cases import TRAJ_SEEDS, traj_case

# the deviation of the chains' refined points between the restatement and its reversed-sum twin over DOCK_SEEDS, measured here:
# 1.1e-14 .. 2.9e-14 A (profiles/vina_dock.md).  test_vina_dock_gpu.py allows the kernel 100 x this, with a floor of 1e-9 A.
DOCK_MEASURED_DEV = 3e-14
INTEGER_COLUMNS = ('best_step', 'accepted', 'box_rejected', 'evaluations', 'found')


def test_philox_known_answers():
    """Two of the known-answer vectors published with Random123 (Salmon et al., SC'11) for philox4x32-10."""
    assert D.philox((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert D.philox((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_uniforms_lie_inside_the_unit_interval_and_ball_vectors_inside_the_unit_ball():
    assert 0.0 < (0 + 0.5) * 2.0 ** -32 and (0xFFFFFFFF + 0.5) * 2.0 ** -32 < 1.0           # the two extreme words, exact in fp64
    us = [u for q in range(4) for s in range(8) for u in D.uniforms(q, s, 1, 3, 0x123456789abcdef)]
    assert all(0.0 < u < 1.0 for u in us) and len(set(us)) == len(us) and 0.3 < np.mean(us) < 0.7
    assert D.uniforms(0, 1, 2, 3, 5) != D.uniforms(0, 1, 2, 3, 5 << 32) and D.uniforms(0, 1, 2, 3, 5) != D.uniforms(0, 1, 2, 4, 5)
    tiny, top = 0.5 * 2.0 ** -32, (0xFFFFFFFF + 0.5) * 2.0 ** -32
    for u1 in (tiny, 0.5, top):
        for u2 in (tiny, 0.25, top):
            for u3 in (tiny, 0.5, top):
                v = D.ball(u1, u2, u3)
                assert np.isfinite(v).all() and np.linalg.norm(v) <= 1.0
    norms = [np.linalg.norm(D.ball(*us[k:k + 3])) for k in range(0, len(us) - 3, 3)]
    assert max(norms) <= 1.0 and min(norms) < 0.8 < max(norms)


def dihedral(p, a, b, c, d):
    b0, b1, b2 = p[a] - p[b], p[c] - p[b], p[d] - p[c]
    b1 = b1 / np.linalg.norm(b1)
    v, w = b0 - (b0 @ b1) * b1, b2 - (b2 @ b1) * b1
    return np.degrees(np.arctan2(np.cross(b1, v) @ w, v @ w))


def rotor_quads(t, bonds):
    """One dihedral (p, a, b, q) about every active rotor (a, b)."""
    nb = {}
    for i, j in np.asarray(bonds).tolist():
        nb.setdefault(i, []).append(j)
        nb.setdefault(j, []).append(i)
    return [(next(p for p in nb[a] if p != b), a, b, next(q for q in nb[b] if q != a)) for a, b in t['rotors']]


def test_mutations_move_one_entity():
    sym, pos, psym, ppos = dock_case(DOCK_SEEDS[0][0])
    z, bonds, orders, frag = perceived(sym, pos)
    t = R.tree(z, bonds, orders, frag)
    x = pos.astype(np.float64)
    F, T = t['F'], t['T']
    quads = rotor_quads(t, bonds)
    seen = set()
    for s in range(1, 60):
        delta, e = D.mutation_delta(x, t, s, 0, 5, 77, 2.0)
        kind = 'translation' if e < F else 'rotation' if e < 2 * F else 'rotor'
        seen.add(kind)
        y = R.move(x, delta, t)
        assert np.abs(intra_piece_distances(y, t['piece']) - intra_piece_distances(x, t['piece'])).max() <= 1e-12
        turn = np.array([(dihedral(y, *q) - dihedral(x, *q) + 180.0) % 360.0 - 180.0 for q in quads])
        if kind == 'rotor':                                   # exactly one dihedral changes, by the angle drawn
            k = e - 2 * F
            assert np.count_nonzero(delta) == 1 and abs(delta[6 * F + k]) <= math.pi
            want = (math.degrees(delta[6 * F + k]) + 180.0) % 360.0 - 180.0
            assert abs((turn[k] - want + 180.0) % 360.0 - 180.0) <= 1e-9 and np.abs(np.delete(turn, k)).max(initial=0.0) <= 1e-9
        else:
            assert np.abs(turn).max() <= 1e-9
            f = e if e < F else e - F
            shift = R.centres(y, t)[f] - R.centres(x, t)[f]
            if kind == 'rotation':                            # about the fragment's centre, by at most amplitude / r_f
                assert np.abs(shift).max() <= 1e-12 and np.count_nonzero(delta[:6 * F].reshape(F, 6)[:, :3]) == 0
                assert np.linalg.norm(delta[6 * f + 3:6 * f + 6]) * D.gyration(x, t, f) <= 2.0 + 1e-12
            else:
                assert np.abs(shift - delta[6 * f:6 * f + 3]).max() <= 1e-12 and np.linalg.norm(shift) <= 2.0 + 1e-12
    assert seen == {'translation', 'rotation', 'rotor'}
    d = D.start_delta(x, t, np.array([1.0, 2.0, 3.0]), np.array([2.0, 4.0, 6.0]), 1, 5, 77)      # a random start: every slot drawn
    c = R.centres(R.move(x, d, t), t)[0]
    assert np.count_nonzero(d) == 6 * F + T and (c > [1.0, 2.0, 3.0]).all() and (c < [2.0, 4.0, 6.0]).all()
    assert np.abs(d[6 * F:]).max() <= math.pi and np.linalg.norm(d[3:6]) <= math.pi


@pytest.mark.parametrize('seed', TRAJ_SEEDS[:2])
def test_minimise_is_the_loop_of_the_minimiser(seed):
    """From an fp32 start the restated loop and vina_min_ref.minimize reach the same float64 point bit for bit, so the anchor of
    include/kpd.h (n_chains = 1, n_steps = 0, step_iters = 0 is kpd_vina_minimize) holds in the restatement."""
    sym, pos, psym, ppos = traj_case(seed)
    s = setup(sym, pos, psym, ppos)
    P = dict(D.DEFAULTS, max_iters=5)
    ev = lambda y: R.evaluate(y, s['t'], s['types'], s['radius'], s['ppos'], s['ptypes'], s['pradius'], P)
    want = run(s, pos, dict(max_iters=5))
    x, e, n = D.minimise(pos.astype(np.float64), 5, ev, s['t'], P, False, [])
    assert np.array_equal(x, want['x64']) and n + 1 == want['report']['evaluations']
    z, bonds, orders, frag = perceived(sym, pos)
    lo, hi = own_box(pos)
    out = D.dock_ligand(pos, z, bonds, orders, frag, s['radius'], ppos, s['ptypes'], s['pradius'], lo, hi, n_chains=1, n_steps=0, n_modes=1,
                        params=dict(step_iters=0, max_iters=5))
    assert out['n_found'] == 1 and np.array_equal(out['chains'][0]['pos'], want['pos_out'])
    rep = out['report'][0]
    for key, col in (('score', 'score_after'), ('E', 'E_after'), ('inter', 'inter_after'), ('intra', 'intra_after'), ('gnorm', 'gnorm_after')):
        assert rep[key] == want['report'][col], key
    assert abs(rep['rmsd_input'] - want['report']['rmsd']) <= 1e-12 * want['report']['rmsd']


def dock(cs, ss, reverse=False, **shape):
    sym, pos, psym, ppos = dock_case(cs)
    z, bonds, orders, frag = perceived(sym, pos)
    lo, hi = own_box(pos)
    kw = dict(DOCK_SHAPE, **shape)
    return D.dock_ligand(pos, z, bonds, orders, frag, radii_of(sym), ppos, V.pocket_types(ppos, z_of(psym))[0], radii_of(psym), lo, hi,
                         lig_id=cs, seed=ss, params=DOCK_PARAMS, reverse=reverse, **kw)


@pytest.mark.parametrize('cs,ss', DOCK_SEEDS)
def test_trajectory_seeds_take_no_coin_toss(cs, ss):
    ref, rev = dock(cs, ss), dock(cs, ss, reverse=True)
    assert 9 <= len(ref['types']) <= 14 and ref['tree']['T'] >= 1
    worst = min(ref['margins'], key=lambda kv: kv[1])
    assert worst[1] >= 1e-9, (cs, ss, worst)
    assert ref['kept'] == rev['kept'] and ref['status'] == rev['status'] and ref['n_found'] == rev['n_found'] >= 1
    dev = 0.0
    for a, b in zip(ref['chains'], rev['chains']):
        assert [a['report'][k] for k in INTEGER_COLUMNS] == [b['report'][k] for k in INTEGER_COLUMNS]
        assert np.array_equal(a['pos'], b['pos'])
        dev = max(dev, np.abs(a['x64'] - b['x64']).max())
    print(f'case {cs} seed {ss}: forward against reversed sums {dev:.2e} A, least margin {worst[1]:.2e} ({worst[0]}), chains '
          f'{[[c["report"][k] for k in INTEGER_COLUMNS] for c in ref["chains"]]}')
    assert dev <= DOCK_MEASURED_DEV


def test_the_trajectory_seeds_cover_the_decisions():
    """Between them the cases reject at the box, in a step and at a random start, accept and refuse steps, find a best after step 0
    and rank chain 1 first."""
    runs = [dock(cs, ss) for cs, ss in DOCK_SEEDS]
    chains = [c['report'] for r in runs for c in r['chains']]
    assert any(c['box_rejected'] for c in chains) and any(c['accepted'] < 3 - c['box_rejected'] for c in chains)
    assert any(c['best_step'] > 0 for c in chains) and any(c['best_step'] == 0 for c in chains)
    assert any(r['kept'][0] == 1 for r in runs) and any(r['kept'][0] == 0 for r in runs)
    assert any(not c['found'] and c['box_rejected'] == 1 for c in chains) and any(r['status'] & D.FEW_MODES for r in runs)
    one = dock(*DOCK_SEEDS[0], n_chains=1, n_modes=1)         # chain 0 does not depend on n_chains
    assert one['chains'][0]['report'] == runs[0]['chains'][0]['report'] and np.array_equal(one['chains'][0]['pos'], runs[0]['chains'][0]['pos'])
    other = dock(DOCK_SEEDS[0][0], DOCK_SEEDS[0][1] + 1)      # another seed, another search
    assert not np.array_equal(other['chains'][1]['pos'], runs[0]['chains'][1]['pos'])
