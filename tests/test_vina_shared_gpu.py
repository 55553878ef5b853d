"""kpd_vina_score and kpd_vina_minimize take one perceived ligand in its pocket through one set of helpers (csrc/vina_core.h):
pocket staging, bond graph, typing, graph walk, pocket pair sums.  On the same graphs both must leave out the same ligands with the same
status bits 0 and 1, count the same rotors and compute the same pocket sum bit for bit; the one intended difference is a bond
listed as (j, i).  The minimiser's set-up is also run beyond one word of the bit matrix, which the score's tests reach and the
minimiser's (at most 25 atoms) do not.  Every raw call runs with canaries (score_gpu, minimize_gpu)."""
import numpy as np
import pytest

from . import vina_min_ref as R
from .molecule_cases import Z, one_hot
from .relax_cases import grow, make_pocket
from .test_pocket_ligand_frontend_gpu import edited
from .test_vina_gpu import EVAL_TOL, Inputs, bits, pocket_types_gpu, same_ligand, score_gpu
from .test_vina_min_gpu import COLS, minimize_gpu, ref_of

pytestmark = pytest.mark.gpu

# a grown ligand of 40 atoms (two words per row of the bit matrix) in a pocket of 40: chosen on the CPU so that the restatement
# finds 3 fragments, 11 rotors and two rotors, (5, 32) and (31, 33), whose atoms lie in different words; asserted in the test
WIDE_SEED = 7017


def test_same_graph_both_kernels(cuda):
    rng = np.random.default_rng(3)                               # the batch of test_pocket_ligand_frontend_gpu.py
    ligs = [(one_hot(s), p) for s, p in (grow(rng, n) for n in (9, 12, 7, 15, 11, 6))]
    anchor = np.concatenate([p for _, p in ligs])
    pockets = [make_pocket(rng, 20, anchor, reach=4.0), make_pocket(rng, 90, anchor, reach=4.0)]
    inp = Inputs(cuda, ligs, pockets, [0, 1, 0, 1, 1, -1])
    ty, _ = pocket_types_gpu(inp)
    ptr, bptr, B, F = [int(a) for a in inp.ptr], [int(a) for a in inp.got['bond_ptr']], inp.B, len(Z)
    bonds = inp.t['bonds']

    def both(x):
        return score_gpu(x, ty, max_atoms=16), minimize_gpu(x, ty, max_atoms=16, max_iters=0)

    good_s, good_m = both(inp)
    assert not (good_s['status'] & 3).any() and not (good_m['status'] & 3).any()
    assert good_s['report'][:, 7].tolist() == good_m['report'][:, COLS['n_rot']].tolist() and good_s['report'][:, 7].max() >= 2
    # the same code on the same inputs in the same order: the pocket sum is the same number, not a close one
    assert bits(good_m['report'][:, COLS['inter_before']]) == bits(good_s['report'][:, 1]), (good_m['report'][:, 4], good_s['report'][:, 1])
    assert good_s['report'][:5, 1].all()

    beyond = bonds[bptr[2]].clone()
    beyond[1] = ptr[3]                                           # ligand 2: a bond to the first atom of ligand 3
    before = bonds[bptr[4] + 1].clone()
    before[0] = ptr[4] - 1                                       # ligand 4: a bond from the last atom of ligand 3
    cases = [                                                    # (edits of the perceived tensors, the ligands they leave out)
        (dict(order={bptr[3] + 2: 4}), [3]),                     # a bond order of 4
        (dict(bonds={bptr[1] + 1: bonds[bptr[1]].clone()}), [1]),                            # a bond repeated
        (dict(elem={ptr[0]: -1, ptr[4] + 2: F}), [0, 4]),        # a class below 0, and F
        (dict(bonds={bptr[2]: beyond, bptr[4] + 1: before}), [2, 4]),                        # a bond index beyond the ligand, either side
    ]
    for edits, out in cases:
        s, m = both(edited(inp, **edits))
        want = [1 if b in out else 0 for b in range(B)]
        assert (s['status'] & 3).tolist() == (m['status'] & 3).tolist() == want, (edits, s['status'], m['status'])
        for b in range(B):
            if b in out:
                assert not s['report'][b].any() and not m['report'][b].any(), (edits, b)
            else:
                same_ligand(good_s, inp, b, s, inp, b)
                assert bits(good_m['report'][b]) == bits(m['report'][b]) and good_m['status'][b] == m['status'][b], (edits, b)

    # the one intended difference: a bond listed as (j, i) is a bond to the score and no molecule to the minimiser
    k = bptr[3] + 1
    s, m = both(edited(inp, bonds={k: bonds[k].flip(0)}))
    for b in range(B):
        same_ligand(good_s, inp, b, s, inp, b)
    assert (m['status'] & 3).tolist() == [0, 0, 0, R.NO_MOLECULE, 0, 0] and not m['report'][3].any()


def test_minimiser_set_up_beyond_one_word(cuda):
    rng = np.random.default_rng(WIDE_SEED)
    sym, pos = grow(rng, 40)
    inp = Inputs(cuda, [(one_hot(sym), pos)], [make_pocket(rng, 40, pos, reach=5.0, keep_out=1.5)], [0])
    ty, pst = pocket_types_gpu(inp)
    assert not pst.any() and not inp.got['status'].any()
    ref = ref_of(inp, 0, ty, dict(max_iters=0))
    t, want, f = ref['tree'], ref['report'], ref['first']
    crossing = [(a, b) for a, b in t['rotors'] if a >> 5 != b >> 5]
    assert t['F'] <= 8 and t['n_rot'] >= 2 and crossing, (t['F'], t['n_rot'], t['rotors'])      # a changed grow() must not hollow this out
    out = minimize_gpu(inp, ty, max_atoms=40, max_iters=0)
    rep = out['report'][0]
    assert (rep[COLS['n_rot']], rep[COLS['n_active']], rep[COLS['n_frag']]) == (want['n_rot'], want['n_active'], want['n_frag'])
    assert (want['n_rot'], want['n_active'], want['n_frag']) == (t['n_rot'], t['T'], t['F'])
    assert out['status'][0] == ref['status'] and bits(out['pos']) == bits(inp.pos)
    tol = EVAL_TOL * f['abs_terms']
    for key in ('E', 'inter', 'intra'):
        dev = abs(rep[COLS[key + '_before']] - f[key])
        print(f'{key}: deviation / sum|terms| = {dev / f["abs_terms"]:.2e} (allowed {EVAL_TOL:.0e})')
        assert dev <= tol, (key, dev, tol)
    assert rep[COLS['intra_before']] != 0 and rep[COLS['inter_before']] != 0
