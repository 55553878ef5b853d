"""Minimisation of ligands under the Vina-form score on the GPU (kpd_vina_minimize, Molecules.vina_minimize, minimize_samples)
against the float64 restatement of include/kpd.h (tests/vina_min_ref.py).  Every raw call runs with canary bytes behind each
output buffer and byte-compares its inputs afterwards; the bond graphs come from kpd_mol_perceive, as a caller's would.
Ligands of 1 .. 25 atoms, pockets of 40 .. 120 atoms, batches of at most 8, max_iters <= 60.  Nothing is timed."""
import ctypes

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import vina_min_ref as R
from . import vina_ref as V
from .molecule_cases import ELEMENTS, Z, one_hot
from .relax_cases import grow, make_pocket
from .test_molecule_gpu import Guarded
from .test_vina_gpu import EVAL_TOL, Inputs, bits, pocket_types_gpu, rows, score_gpu, to
from .test_vina_min_config import TRAJ_MEASURED_DEV
from .vina_cases import LIG_RADIUS, RADII
from .vina_min_cases import TRAJ_SEEDS, mixed_batch, traj_case

pytestmark = pytest.mark.gpu

# Trajectories: the restatement against itself with every sum reversed deviates, over TRAJ_SEEDS and K = 1, 2, 5 iterations, by at
# most TRAJ_MEASURED_DEV = 1.5e-14 A in the positions (measured on the CPU and asserted below and in test_vina_min_config.py;
# profiles/vina_min.md).  The GPU is allowed 100 x that, which is below the floor of 1e-9 A; so the floor is the tolerance.
TRAJ_FACTOR, TRAJ_FLOOR = 100.0, 1e-9
COLS = {k: c for c, k in enumerate(R.REPORT)}
LEFT_OUT = R.NO_MOLECULE | R.BAD_INPUT | R.FRAGMENTS


def minimize_gpu(inp, ptypes, max_atoms=32, max_pocket=None, max_rotors=64, pos=None, order=None, frag=None, pocket_of=None, px=None,
                 pptr=None, type_in=None, bonds=None, **params):
    """kpd_vina_minimize through the C ABI with canaries; returns a dict of numpy arrays: pos [N,3] float32, report [B,16], status [B]."""
    dev, t = inp.dev, inp.t
    N, B = t['pos'].shape[0], inp.B
    pos_d = t['pos'] if pos is None else to(dev, pos, torch.float32)
    order_d = t['order'] if order is None else to(dev, order, torch.int32)
    frag_d = t['frag'] if frag is None else to(dev, frag, torch.int32)
    bonds_d = t['bonds'] if bonds is None else to(dev, bonds, torch.int32)
    px_d, prad_d = to(dev, inp.px if px is None else px, torch.float32), to(dev, inp.prad, torch.float32)
    pty_d, pptr_d = to(dev, ptypes, torch.int32), to(dev, inp.pptr if pptr is None else pptr, torch.int32)
    pof_d = to(dev, inp.pocket_of if pocket_of is None else pocket_of, torch.int32)
    zt, lr = torch.tensor(Z, dtype=torch.int32, device=dev), to(dev, LIG_RADIUS, torch.float32)
    tin_d = None if type_in is None else to(dev, type_in, torch.int32)
    ins = [pos_d, order_d, frag_d, px_d, prad_d, pty_d, pptr_d, pof_d, zt, lr, t['ptr'], t['elem'], bonds_d, t['bond_ptr'], t['status']]
    ins += [] if tin_d is None else [tin_d]
    keep = [x.clone() for x in ins]
    g = Guarded(dev)
    out, rep, st = g.new(3 * N, torch.float32), g.new(16 * B, torch.float64), g.new(B)
    p = hip.vina_min_params(**params)
    hip.check(hip.lib().kpd_vina_minimize(pos_d.data_ptr(), t['ptr'].data_ptr(), N, B, max_atoms, t['elem'].data_ptr(), len(Z), zt.data_ptr(),
                                          lr.data_ptr(), frag_d.data_ptr(), bonds_d.data_ptr(), order_d.data_ptr(),
                                          t['bond_ptr'].data_ptr(), t['cap'], t['status'].data_ptr(),
                                          None if tin_d is None else tin_d.data_ptr(), px_d.data_ptr(), prad_d.data_ptr(),
                                          pty_d.data_ptr(), pptr_d.data_ptr(), px_d.shape[0], pptr_d.numel() - 1,
                                          inp.max_pocket if max_pocket is None else max_pocket, pof_d.data_ptr(), max_rotors,
                                          ctypes.byref(p), out.data_ptr(), rep.data_ptr(), st.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    for a, b in zip(keep, ins):
        assert a.reshape(-1).view(torch.uint8).equal(b.reshape(-1).view(torch.uint8)), 'an input buffer was written'
    return dict(pos=out[:3 * N].cpu().numpy().reshape(N, 3), report=rep[:16 * B].cpu().numpy().reshape(B, 16),
                status=st[:B].cpu().numpy().astype(np.int64))


def ref_of(inp, b, ptypes, params=None, max_rotors=64, type_in=None, reverse=False):
    """The restatement's result for ligand b of the batch."""
    a0, a1 = int(inp.ptr[b]), int(inp.ptr[b + 1])
    z, bonds, orders = inp.graph(b)
    q = int(inp.pocket_of[b])
    q0, q1 = (int(inp.pptr[q]), int(inp.pptr[q + 1])) if q >= 0 else (0, 0)
    return R.minimize_ligand(inp.pos[a0:a1], z, bonds, orders, inp.got['frag'][a0:a1], LIG_RADIUS[inp.got['elem'][a0:a1]], inp.px[q0:q1],
                             ptypes[q0:q1], inp.prad[q0:q1], params=params, type_in=type_in, max_rotors=max_rotors, reverse=reverse)


def same_ligand(x, inp, b, y, inp2, k):
    """Ligand b of run x equals ligand k of run y bit for bit."""
    assert bits(x['report'][b]) == bits(y['report'][k]) and x['status'][b] == y['status'][k], (b, x['report'][b], y['report'][k])
    assert bits(x['pos'][rows(inp, b)]) == bits(y['pos'][rows(inp2, k)]), b


@pytest.fixture(scope='module')
def batch(cuda):
    """The mixed batch (ring only, one rotor, three rotors, three bodies, a lone atom, biphenyl, grown ligands of 14 and 25 atoms) in
    pockets of 40, 80 and 120 atoms, with the types of the pockets and the restatement's trees."""
    ligs, pockets, pocket_of = mixed_batch()
    inp = Inputs(cuda, [(one_hot(s), p) for s, p in ligs], pockets, pocket_of)
    ty, pst = pocket_types_gpu(inp)
    assert not pst.any() and not inp.got['status'].any()
    return dict(inp=inp, ptypes=ty)


@pytest.fixture(scope='module')
def full(batch):
    return minimize_gpu(batch['inp'], batch['ptypes'], max_iters=60)


def test_one_evaluation(batch):
    inp, ty = batch['inp'], batch['ptypes']
    out = minimize_gpu(inp, ty, max_iters=0)
    assert bits(out['pos']) == bits(inp.pos)
    score = score_gpu(inp, ty, max_atoms=32, outputs=False)
    worst = 0.0
    for b in range(inp.B):
        ref = ref_of(inp, b, ty, dict(max_iters=0))
        rep, want, f = out['report'][b], ref['report'], ref['first']
        tol = EVAL_TOL * f['abs_terms']
        for key in ('E', 'inter', 'intra'):
            dev = abs(rep[COLS[key + '_before']] - f[key])
            worst = max(worst, dev / max(f['abs_terms'], 1e-300))
            assert dev <= tol, (b, key, dev, tol)
            assert rep[COLS[key + '_after']] == rep[COLS[key + '_before']]
        assert abs(rep[COLS['score_before']] - want['score_before']) <= tol and rep[COLS['score_after']] == rep[COLS['score_before']]
        # kpd_vina_score on the same inputs
        assert abs(rep[COLS['inter_before']] - score['report'][b, 1]) <= tol and abs(rep[COLS['score_before']] - score['report'][b, 0]) <= tol
        lever = 1.0 + np.abs(inp.pos[rows(inp, b)].astype(np.float64) - inp.pos[rows(inp, b)].astype(np.float64).mean(axis=0)).sum(axis=1).max()
        assert abs(rep[COLS['gnorm_before']] - want['gnorm_before']) <= EVAL_TOL * f['abs_g'].sum() * lever
        assert (rep[COLS['n_rot']], rep[COLS['n_active']], rep[COLS['n_frag']]) == (want['n_rot'], want['n_active'], want['n_frag']), b
        assert rep[COLS['rmsd']] == 0.0 and rep[COLS['iterations']] == 0 and rep[COLS['evaluations']] == 1
        assert out['status'][b] == ref['status'], (b, out['status'][b], ref['status'])
    print(f'one evaluation: worst deviation / sum|terms| = {worst:.2e} (allowed {EVAL_TOL:.0e})')
    assert out['report'][:, COLS['n_rot']].tolist() == [0, 1, 3, 0, 0, 1] + out['report'][6:, COLS['n_rot']].tolist()
    assert out['report'][:6, COLS['n_frag']].tolist() == [1, 1, 1, 3, 1, 1] and (out['report'][6:, COLS['n_rot']] >= 2).all()
    assert (out['report'][:, COLS['intra_before']] != 0).sum() >= 5


@pytest.mark.parametrize('K', [1, 2, 5])
def test_trajectory(cuda, K):
    cases = [traj_case(s) for s in TRAJ_SEEDS]
    inp = Inputs(cuda, [(one_hot(c[0]), c[1]) for c in cases], [(c[2], c[3]) for c in cases], list(range(len(cases))))
    ty, _ = pocket_types_gpu(inp)
    out = minimize_gpu(inp, ty, max_atoms=16, max_iters=K)
    tol = max(TRAJ_FACTOR * TRAJ_MEASURED_DEV, TRAJ_FLOOR)
    for b in range(inp.B):
        ref = ref_of(inp, b, ty, dict(max_iters=K))
        rev = ref_of(inp, b, ty, dict(max_iters=K), reverse=True)
        assert np.abs(ref['x64'] - rev['x64']).max() <= TRAJ_MEASURED_DEV            # the measurement behind the constant
        assert (ref['report']['iterations'], ref['report']['evaluations'], ref['status']) == \
            (rev['report']['iterations'], rev['report']['evaluations'], rev['status'])
        mine, rep = out['pos'][rows(inp, b)], out['report'][b]
        # pos_out is the fp32 rounding of the kernel's fp64 point, which must lie within tol of the restatement's
        half_ulp = 0.5 * np.spacing(np.abs(mine)).astype(np.float64)
        dev = np.abs(mine.astype(np.float64) - ref['x64']) - half_ulp
        want = ref['report']
        print(f'seed {TRAJ_SEEDS[b]} K {K}: positions beyond rounding {max(dev.max(), 0.0):.2e} A, '
              f'|dE| {abs(rep[COLS["E_after"]] - want["E_after"]):.2e} of {want["E_after"]:.6g}')
        assert dev.max() <= tol, (b, dev.max())
        tol_e = max(TRAJ_FACTOR * 4e-16 * max(1.0, abs(want['E_after'])), EVAL_TOL * ref['last']['abs_terms'])
        assert abs(rep[COLS['E_after']] - want['E_after']) <= tol_e and abs(rep[COLS['E_before']] - want['E_before']) <= tol_e
        assert (rep[COLS['iterations']], rep[COLS['evaluations']], out['status'][b]) == (want['iterations'], want['evaluations'], ref['status'])
        assert rep[COLS['iterations']] == K and rep[COLS['E_after']] < rep[COLS['E_before']]


def piece_pairs(piece):
    return piece[:, None] == piece[None, :]


def test_full_runs(batch, full):
    inp, ty = batch['inp'], batch['ptypes']
    score = score_gpu(inp, ty, max_atoms=32, pos=full['pos'], outputs=False)
    moved = 0
    for b in range(inp.B):
        rep, st = full['report'][b], full['status'][b]
        z, bonds, orders = inp.graph(b)
        a = rows(inp, b)
        types = V.ligand_types(z, bonds, orders, LIG_RADIUS[inp.got['elem'][a]])
        t = R.tree(z, bonds, orders, inp.got['frag'][a], 64, types)
        x, y = inp.pos[a].astype(np.float64), full['pos'][a].astype(np.float64)
        assert not st & LEFT_OUT and rep[COLS['E_after']] <= rep[COLS['E_before']] and rep[COLS['iterations']] <= 60, (b, st, rep)
        assert rep[COLS['evaluations']] >= rep[COLS['iterations']] + (2 if rep[COLS['iterations']] else 1)
        # rigid by construction: the input rows are the exact start, so a distance inside a piece, or along a bond, moves by the
        # fp32 rounding of the two ends written at most (half an ulp of each coordinate, through the triangle inequality), plus
        # 1e-12 for at most 60 composed fp64 moves of a few ulps of 10 A (1e-15) each
        half = np.sqrt((np.spacing(np.abs(full['pos'][a])).astype(np.float64) ** 2).sum(axis=1)) * 0.5
        bound = half[:, None] + half[None, :] + 1e-12
        dx, dy = np.linalg.norm(x[:, None] - x[None, :], axis=2), np.linalg.norm(y[:, None] - y[None, :], axis=2)
        same = piece_pairs(t['piece'])
        for i, j in bonds:
            same[i, j] = same[j, i] = True
        assert (np.abs(dy - dx)[same] <= bound[same]).all(), (b, (np.abs(dy - dx) - bound)[same].max())
        # the numbers of the report describe the rows written
        e = R.evaluate(y, t, types, LIG_RADIUS[inp.got['elem'][a]], *pocket_of_ligand(inp, b, ty))
        tol = EVAL_TOL * e['abs_terms']
        assert abs(rep[COLS['E_after']] - e['E']) <= tol and abs(rep[COLS['inter_after']] - e['inter']) <= tol, (b, rep, e['E'])
        assert abs(rep[COLS['intra_after']] - e['intra']) <= tol
        assert abs(rep[COLS['inter_after']] - score['report'][b, 1]) <= tol and abs(rep[COLS['score_after']] - score['report'][b, 0]) <= tol
        d = y - x
        rmsd = np.sqrt((d * d).sum() / len(x))
        assert abs(rep[COLS['rmsd']] - rmsd) <= 1e-12 * max(rmsd, 1e-30) + 1e-300
        assert rep[COLS['gnorm_after']] <= 1e-3 or st & (R.LINE_SEARCH | R.ITER_CAP), (b, rep[COLS['gnorm_after']], st)
        moved += rep[COLS['iterations']] > 0
    assert moved >= inp.B - 1 and (full['report'][:, COLS['rmsd']] > 1e-3).sum() >= inp.B - 1


def pocket_of_ligand(inp, b, ptypes):
    q = int(inp.pocket_of[b])
    q0, q1 = (int(inp.pptr[q]), int(inp.pptr[q + 1])) if q >= 0 else (0, 0)
    return inp.px[q0:q1], ptypes[q0:q1], inp.prad[q0:q1]


def test_bitwise_invariance(batch, full):
    inp, ty = batch['inp'], batch['ptypes']
    again = minimize_gpu(inp, ty, max_iters=60)                                              # the repeat
    for k in full:
        assert bits(full[k]) == bits(again[k]), k
    for kw in (dict(max_atoms=256), dict(max_pocket=0), dict(max_atoms=25, max_pocket=50)):  # the bounds are no part of the result
        o = minimize_gpu(inp, ty, max_iters=60, **kw)
        for k in full:
            assert bits(full[k]) == bits(o[k]), (kw, k)
    top = int(full['report'][:, COLS['n_rot']].max())
    o = minimize_gpu(inp, ty, max_iters=60, max_rotors=top)                                  # max_rotors = T against 64
    for k in full:
        assert bits(full[k]) == bits(o[k]), k
    order = list(range(inp.B))[::-1]                                                         # the reversed batch
    rev = Inputs(inp.dev, [inp.ligs[b] for b in order], inp.pockets, [inp.pocket_of[b] for b in order])
    o = minimize_gpu(rev, ty, max_iters=60)
    for k, b in enumerate(order):
        same_ligand(full, inp, b, o, rev, k)
    for b in range(inp.B):                                                                   # each ligand alone, LDS sized for it
        one = Inputs(inp.dev, [inp.ligs[b]], inp.pockets, [inp.pocket_of[b]])
        same_ligand(full, inp, b, minimize_gpu(one, ty, max_iters=60, max_atoms=len(inp.ligs[b][1]),
                                               max_rotors=int(full['report'][b, COLS['n_rot']])), one, 0)


def dihedral(p, a, b, c, d):
    b0, b1, b2 = p[a] - p[b], p[c] - p[b], p[d] - p[c]
    b1 = b1 / np.linalg.norm(b1)
    v, w = b0 - (b0 @ b1) * b1, b2 - (b2 @ b1) * b1
    return np.degrees(np.arctan2(np.cross(b1, v) @ w, v @ w))


def test_frozen_rotors_and_type_override(batch, full):
    inp, ty = batch['inp'], batch['ptypes']
    hexane = 2
    a = rows(inp, hexane)
    x = inp.pos[a].astype(np.float64)
    quads = [(0, 1, 2, 3), (1, 2, 3, 4), (2, 3, 4, 5)]                                       # the dihedrals about the rotors (1,2), (2,3), (3,4)
    for mr in (0, 1):
        o = minimize_gpu(inp, ty, max_iters=60, max_rotors=mr)
        rep = o['report'][hexane]
        assert o['status'][hexane] & R.FROZEN and rep[COLS['n_active']] == mr and rep[COLS['n_rot']] == 3
        assert rep[COLS['iterations']] > 0 and rep[COLS['rmsd']] > 1e-3 and rep[COLS['E_after']] < rep[COLS['E_before']]
        y = o['pos'][a].astype(np.float64)
        for k, q in enumerate(quads):
            turn = abs((dihedral(y, *q) - dihedral(x, *q) + 180.0) % 360.0 - 180.0)
            if k >= mr:
                assert turn <= 1e-3, (mr, k, turn)           # fp32 rows: 1e-6 A over levers of 1 A is 1e-4 degrees
        for b in range(inp.B):                               # a ligand without frozen rotors keeps its bits
            if full['report'][b, COLS['n_rot']] <= mr:
                same_ligand(full, inp, b, o, inp, b)
            ref = ref_of(inp, b, ty, dict(max_iters=0), max_rotors=mr)
            assert (o['report'][b, COLS['n_active']], bool(o['status'][b] & R.FROZEN)) == (ref['report']['n_active'], bool(ref['status'] & R.FROZEN))
    free = dihedral(full['pos'][a].astype(np.float64), *quads[2]) - dihedral(x, *quads[2])
    assert abs((free + 180.0) % 360.0 - 180.0) > 1e-2        # the same torsion does turn when it is active
    # lig_type_in >= 0 replaces the perceived flags, -1 keeps them
    tin = np.full(inp.pos.shape[0], -1)
    tin[rows(inp, 1)] = 7
    o = minimize_gpu(inp, ty, max_iters=0, type_in=tin)
    first = minimize_gpu(inp, ty, max_iters=0)
    ref = ref_of(inp, 1, ty, dict(max_iters=0), type_in=tin[rows(inp, 1)])
    assert abs(o['report'][1, COLS['E_before']] - ref['report']['E_before']) <= EVAL_TOL * ref['first']['abs_terms']
    assert o['report'][1, COLS['E_before']] != first['report'][1, COLS['E_before']]
    for b in range(inp.B):
        if b != 1:
            same_ligand(first, inp, b, o, inp, b)


def test_bad_inputs(cuda):
    rng = np.random.default_rng(3)
    ligs = [(one_hot(s), p) for s, p in (grow(rng, n) for n in (9, 12, 7, 15, 11, 6))]
    nine = np.array([[4.0 * k, 0.0, 0.0] for k in range(9)], dtype=np.float32)               # nine atoms that bond to nothing
    ligs.append((one_hot(['C'] * 9), nine))
    anchor = np.concatenate([p for _, p in ligs[:6]])
    pockets = [make_pocket(rng, 40, anchor, reach=4.0), make_pocket(rng, 90, anchor, reach=4.0)]
    inp = Inputs(cuda, ligs, pockets, [0, 1, 0, 1, 1, -1, 0])
    ty, _ = pocket_types_gpu(inp)
    good = minimize_gpu(inp, ty, max_atoms=16, max_iters=10)
    assert good['status'][6] == R.FRAGMENTS and not (good['status'][:6] & LEFT_OUT).any() and good['report'][:5, COLS['iterations']].all()

    def check(o, changed, pos=None, base=None):
        """The ligands of `changed` carry a left-out bit, a zero report and their input rows; every other one has the bits of the
        well-formed run `base` (the run `good` unless another pocket_of makes another baseline)."""
        src, base = inp.pos if pos is None else pos, good if base is None else base
        for b in range(inp.B):
            if b not in changed:
                same_ligand(base, inp, b, o, inp, b)
            else:
                assert o['status'][b] & LEFT_OUT and not o['report'][b].any(), (b, o['status'][b])
                assert bits(o['pos'][rows(inp, b)]) == bits(src[rows(inp, b)]), b

    check(good, [6])                                                                         # nine fragments: bit 5, rows copied
    pos = inp.pos.copy()
    pos[int(inp.ptr[1]) + 3, 1] = np.nan                                                     # ligand 1: a NaN coordinate
    o = minimize_gpu(inp, ty, max_atoms=16, max_iters=10, pos=pos)
    assert o['status'][1] == R.BAD_INPUT
    check(o, [1, 6], pos)
    o = minimize_gpu(inp, ty, max_atoms=16, max_iters=10, pocket_of=[0, 1, 2, 1, 1, -2, 0])  # pocket_of = P, and below -1
    assert (o['status'] & 3).tolist() == [0, 0, 2, 0, 0, 2, 0]
    check(o, [2, 5, 6])
    pptr = np.array([0, int(inp.pptr[2]), int(inp.pptr[1])])                                 # a descending pocket_ptr: pocket 1 is malformed
    apart = [-1, 1, -1, 1, 1, -1, -1]                                                        # nobody else reads the rows pocket 1 lost
    base = minimize_gpu(inp, ty, max_atoms=16, max_iters=10, pocket_of=apart)                # the same pocket_of, well-formed pocket_ptr
    assert base['status'][6] == R.FRAGMENTS and not (base['status'][:6] & LEFT_OUT).any()
    o = minimize_gpu(inp, ty, max_atoms=16, max_iters=10, pptr=pptr, pocket_of=apart)
    assert (o['status'] & 3).tolist() == [0, 2, 0, 2, 2, 0, 0] and o['status'][[1, 3, 4]].tolist() == [R.BAD_INPUT] * 3
    check(o, [1, 3, 4, 6], base=base)
    order = inp.got['order'].astype(np.int32).copy()
    order[int(inp.got['bond_ptr'][3]) + 2] = 4                                               # ligand 3: a bond order of 4
    o = minimize_gpu(inp, ty, max_atoms=16, max_iters=10, order=order)
    assert o['status'][3] == R.NO_MOLECULE
    check(o, [3, 6])
    bonds = inp.t['bonds'].cpu().numpy().copy()
    k = int(inp.got['bond_ptr'][3]) + 1
    bonds[k] = bonds[k][::-1]                                                                # ligand 3: a bond listed as (j, i)
    o = minimize_gpu(inp, ty, max_atoms=16, max_iters=10, bonds=bonds)
    assert o['status'][3] == R.NO_MOLECULE
    check(o, [3, 6])
    for bad in (-1, 15, 1):                                                                  # ligand 3: frag below 0, beyond n, a bond between two labels
        frag = inp.got['frag'].astype(np.int32).copy()
        frag[int(inp.ptr[3]) + 4] = bad
        o = minimize_gpu(inp, ty, max_atoms=16, max_iters=10, frag=frag)
        assert o['status'][3] == R.NO_MOLECULE, (bad, o['status'][3])
        check(o, [3, 6])
    o = minimize_gpu(inp, ty, max_atoms=8, max_iters=10)                                     # more atoms than max_atoms: left out
    assert (o['status'] & 1).tolist() == [1, 1, 0, 1, 1, 0, 1]
    check(o, [0, 1, 3, 4, 6])


def test_python_surface(cuda):
    rng = np.random.default_rng(5)
    ligs = [grow(rng, n) for n in (8, 11, 5, 9, 14, 7)]
    pos = [torch.from_numpy(p).to(cuda) for _, p in ligs]
    feat = [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in ligs]
    anchor = np.concatenate([p for _, p in ligs])
    pockets = [make_pocket(rng, 40, anchor, reach=4.0), make_pocket(rng, 60, anchor, reach=4.0)]
    ppos, psym = [torch.from_numpy(p).to(cuda) for _, p in pockets], [s for s, _ in pockets]
    mols = molecule.build_molecules(pos, feat, ELEMENTS)
    pof = [0, 0, 0, 1, 1, 1]
    m = mols.vina_minimize(ppos, psym, pocket_of=pof, radii=RADII, max_iters=30)
    assert m.report.shape == (6, 16) and m.status.shape == (6,) and not bool((m.status & LEFT_OUT).any())
    assert [tuple(p.shape) for p in m.pos] == [tuple(p.shape) for p in pos]
    assert bool((m.report[:, 3] <= m.report[:, 2]).all()) and bool((m.report[:, 11] > 0).all())
    t = m.table()
    assert list(t) == ['lig_idx', 'score_before', 'score_after', 'rmsd', 'n_rot', 'iterations'] and t['lig_idx'] == list(range(6))
    assert t['score_after'] == m.report[:, 1].tolist() and t['n_rot'] == [int(v) for v in m.report[:, 13].tolist()]
    # the molecules at the new pose: the same graph, and kpd_vina_score there gives the reported score
    before, after = mols.sdf(), m.molecules.sdf()
    for b, (x, y) in enumerate(zip(before, after)):
        lx, ly, n = x.split('\n'), y.split('\n'), ligs[b][1].shape[0]
        assert len(lx) == len(ly) and lx[:4] == ly[:4] and lx[4 + n:] == ly[4 + n:]
        want = m.pos[b].cpu().numpy()
        for a in range(n):
            assert ly[4 + a][:30] == '%10.4f%10.4f%10.4f' % tuple(float(v) for v in want[a]) and ly[4 + a][30:] == lx[4 + a][30:]
    v = m.molecules.vina_score(ppos, psym, pocket_of=pof, radii=RADII, pocket_types=m.pocket_types)
    raw = mols.vina_score(ppos, psym, pocket_of=pof, radii=RADII)
    assert torch.equal(raw.pocket_types, m.pocket_types)
    for got, want in ((v.report, m.report[:, 1]), (raw.report, m.report[:, 0])):           # within EVAL_TOL of the sum of the |terms|
        assert bool(((got[:, 0] - want).abs() <= EVAL_TOL * got[:, 2:7].abs().sum(dim=1)).all())
    rigid = mols.vina_minimize(ppos, psym, pocket_of=pof, radii=RADII, max_iters=30, max_rotors=0)
    assert bool((rigid.report[:, 14] == 0).all()) and bool(((rigid.status & R.FROZEN) != 0).equal(rigid.report[:, 13] > 0))
    with pytest.raises(hip.KpdError):
        mols.vina_minimize(ppos, psym, pocket_of=pof, radii=RADII, max_rotors=65)
    with pytest.raises(hip.KpdError):
        mols.vina_minimize(ppos, psym, pocket_of=pof, radii=RADII, gtoll=1.0)
    with pytest.raises(hip.KpdError):                                                        # a host tensor
        mols.vina_minimize([p.cpu() for p in ppos], psym, pocket_of=pof, radii=RADII)
    # minimize_samples: two pockets x three ligands as `_sample` returns them (host tensors, copied to `device`)
    samples = [dict(positions=[p.cpu() for p in pos[3 * q:3 * q + 3]], features=[f.cpu() for f in feat[3 * q:3 * q + 3]]) for q in range(2)]
    pk = [dict(positions=torch.from_numpy(p), elements=s) for s, p in pockets]
    ms = molecule.minimize_samples(samples, pk, ELEMENTS, device=cuda, radii=RADII, max_iters=30)
    assert torch.equal(ms.report, m.report) and torch.equal(ms.molecules.pos, m.molecules.pos)
    relaxed, mr = molecule.minimize_samples(samples, pk, ELEMENTS, device=cuda, relax=True, radii=RADII, relax_params=dict(max_iters=20),
                                            max_iters=30)
    direct = relaxed.molecules.vina_minimize(ppos, psym, pocket_of=pof, radii=RADII, max_iters=30)
    assert torch.equal(mr.report, direct.report) and bool((relaxed.report[:, 4] > 0).all()) and not torch.equal(mr.report, m.report)
    # an empty batch: empty tensors from Molecules.vina_minimize and from the library call
    z32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=cuda)
    none = molecule.Molecules(z32(1), z32(0, 4), z32(0), z32(0), z32(0), z32(0), z32(0, 2), z32(0), z32(1), torch.zeros(0, 3, device=cuda),
                              ELEMENTS, sizes=[])
    e = none.vina_minimize(ppos[:1], psym[:1], radii=RADII)
    assert len(none) == 0 and e.report.shape == (0, 16) and e.status.shape == (0,) and len(e.pos) == 0 and e.molecules.pos.shape == (0, 3)
    assert e.table() == dict(lig_idx=[], score_before=[], score_after=[], rmsd=[], n_rot=[], iterations=[])
    assert torch.equal(e.pocket_types, m.pocket_types[:len(psym[0])])
    empty = dict(elem=z32(0), frag=z32(0), bonds=z32(0, 2), order=z32(0), bond_ptr=z32(1), status=z32(0))
    p0, r0, s0 = hip.vina_minimize(torch.zeros(0, 3, device=cuda), z32(1), Z, torch.tensor(LIG_RADIUS, device=cuda), empty, m.molecules.pos[:0],
                                   torch.zeros(0, device=cuda), z32(0), z32(1), z32(0))
    assert p0.shape == (0, 3) and r0.shape == (0, 16) and s0.shape == (0,)
