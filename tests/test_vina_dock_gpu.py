"""The Monte-Carlo search under the Vina-form score on the GPU (kpd_vina_dock, Molecules.vina_dock, dock_samples) against the
float64 restatement of include/kpd.h (tests/vina_dock_ref.py) and against kpd_vina_minimize.  Every raw call runs with canary bytes
behind each output buffer and byte-compares its inputs afterwards.  Ligands of 1 .. 25 atoms, pockets of 40 .. 120 atoms, at most
9 ligands x 4 chains x 6 steps.  Nothing is timed."""
import ctypes

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import vina_dock_ref as D
from . import vina_min_ref as R
from . import vina_ref as V
from .molecule_cases import ELEMENTS, Z, one_hot
from .relax_cases import grow, make_pocket
from .test_molecule_gpu import Guarded
from .test_vina_dock_config import DOCK_MEASURED_DEV, INTEGER_COLUMNS
from .test_vina_gpu import EVAL_TOL, Inputs, bits, pocket_types_gpu, rows, to
from .test_vina_min_gpu import COLS as MIN_COLS, minimize_gpu, piece_pairs, pocket_of_ligand
from .vina_cases import LIG_RADIUS, RADII
from .vina_dock_cases import DOCK_PARAMS, DOCK_SEEDS, DOCK_SHAPE, dock_case, own_box
from .vina_min_cases import hexane, mixed_batch

pytestmark = pytest.mark.gpu

# the rule of profiles/vina_min.md: the kernel may deviate from the restatement by 100 x what the restatement deviates from its own
# reversed-sum twin (DOCK_MEASURED_DEV = 3e-14 A, measured and asserted in test_vina_dock_config.py), with a floor of 1e-9 A
TRAJ_FACTOR, TRAJ_FLOOR = 100.0, 1e-9
COLS = {k: c for c, k in enumerate(D.REPORT)}
CCOLS = {k: c for c, k in enumerate(D.CHAIN_REPORT)}
LEFT_OUT = D.NO_MOLECULE | D.BAD_INPUT | D.FRAGMENTS | D.BAD_BOX
FULL = dict(n_chains=4, n_steps=6, n_modes=4, step_iters=10, max_iters=30)


def dock_gpu(inp, ptypes, lo, hi, n_chains, n_steps, n_modes, seed=0, lig_id=None, max_atoms=32, max_pocket=None, max_rotors=64,
             pos=None, pocket_of=None, struct=None, **params):
    """kpd_vina_dock through the C ABI with canaries; returns a dict of numpy arrays: pos [n_modes,N,3] float32, n_found [B], report
    [B,n_modes,8], chain_pos [n_chains,N,3], chain_report [B,n_chains,10], status [B]."""
    dev, t = inp.dev, inp.t
    N, B = t['pos'].shape[0], inp.B
    pos_d = t['pos'] if pos is None else to(dev, pos, torch.float32)
    px_d, prad_d = to(dev, inp.px, torch.float32), to(dev, inp.prad, torch.float32)
    pty_d, pptr_d = to(dev, ptypes, torch.int32), to(dev, inp.pptr, torch.int32)
    pof_d = to(dev, inp.pocket_of if pocket_of is None else pocket_of, torch.int32)
    lo_d, hi_d = to(dev, np.asarray(lo, dtype=np.float32).reshape(B, 3), torch.float32), to(dev, np.asarray(hi, dtype=np.float32).reshape(B, 3), torch.float32)
    id_d = None if lig_id is None else to(dev, np.asarray(lig_id), torch.int32)
    zt, lr = torch.tensor(Z, dtype=torch.int32, device=dev), to(dev, LIG_RADIUS, torch.float32)
    ins = [pos_d, px_d, prad_d, pty_d, pptr_d, pof_d, lo_d, hi_d, zt, lr, t['ptr'], t['elem'], t['frag'], t['bonds'], t['order'], t['bond_ptr'],
           t['status']] + ([] if id_d is None else [id_d])
    keep = [x.clone() for x in ins]
    g = Guarded(dev)
    nm, nc = max(n_modes, 1), max(n_chains, 1)
    out, nf, rep = g.new(3 * N * nm, torch.float32), g.new(B), g.new(8 * B * nm, torch.float64)
    cpos, crep, st = g.new(3 * N * nc, torch.float32), g.new(10 * B * nc, torch.float64), g.new(B)
    p = hip.vina_dock_params(**params) if struct is None else struct
    hip.check(hip.lib().kpd_vina_dock(pos_d.data_ptr(), t['ptr'].data_ptr(), N, B, max_atoms, t['elem'].data_ptr(), len(Z), zt.data_ptr(),
                                      lr.data_ptr(), t['frag'].data_ptr(), t['bonds'].data_ptr(), t['order'].data_ptr(),
                                      t['bond_ptr'].data_ptr(), t['cap'], t['status'].data_ptr(), None, px_d.data_ptr(), prad_d.data_ptr(),
                                      pty_d.data_ptr(), pptr_d.data_ptr(), px_d.shape[0], pptr_d.numel() - 1,
                                      inp.max_pocket if max_pocket is None else max_pocket, pof_d.data_ptr(), max_rotors, lo_d.data_ptr(),
                                      hi_d.data_ptr(), None if id_d is None else id_d.data_ptr(), seed, n_chains, n_steps, n_modes,
                                      ctypes.byref(p), out.data_ptr(), nf.data_ptr(), rep.data_ptr(), cpos.data_ptr(), crep.data_ptr(),
                                      st.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    for a, b in zip(keep, ins):
        assert a.reshape(-1).view(torch.uint8).equal(b.reshape(-1).view(torch.uint8)), 'an input buffer was written'
    return dict(pos=out[:3 * N * nm].cpu().numpy().reshape(nm, N, 3), n_found=nf[:B].cpu().numpy().astype(np.int64),
                report=rep[:8 * B * nm].cpu().numpy().reshape(B, nm, 8), chain_pos=cpos[:3 * N * nc].cpu().numpy().reshape(nc, N, 3),
                chain_report=crep[:10 * B * nc].cpu().numpy().reshape(B, nc, 10), status=st[:B].cpu().numpy().astype(np.int64))


def boxes(inp):
    """Every ligand's own input bounding box widened by BOX_ADD."""
    both = [own_box(inp.pos[rows(inp, b)]) for b in range(inp.B)]
    return np.stack([lo for lo, _ in both]), np.stack([hi for _, hi in both])


def same_ligand(x, inp, b, y, inp2, k, chains=None):
    """Ligand b of run x equals ligand k of run y bit for bit (`chains`: only these chains, and nothing of the modes)."""
    if chains is None:
        assert bits(x['report'][b]) == bits(y['report'][k]) and x['status'][b] == y['status'][k] and x['n_found'][b] == y['n_found'][k], \
            (b, x['report'][b], y['report'][k], x['status'][b], y['status'][k])
        assert bits(x['pos'][:, rows(inp, b)]) == bits(y['pos'][:, rows(inp2, k)]), b
    cs = range(x['chain_pos'].shape[0]) if chains is None else chains
    for c in cs:
        assert bits(x['chain_report'][b, c]) == bits(y['chain_report'][k, c]), (b, c, x['chain_report'][b, c], y['chain_report'][k, c])
        assert bits(x['chain_pos'][c, rows(inp, b)]) == bits(y['chain_pos'][c, rows(inp2, k)]), (b, c)


@pytest.fixture(scope='module')
def plain(cuda):
    """The mixed batch of test_vina_min_gpu.py as it is."""
    ligs, pockets, pocket_of = mixed_batch()
    inp = Inputs(cuda, [(one_hot(s), p) for s, p in ligs], pockets, pocket_of)
    ty, pst = pocket_types_gpu(inp)
    assert not pst.any() and not inp.got['status'].any()
    return dict(inp=inp, ptypes=ty)


@pytest.fixture(scope='module')
def batch(cuda):
    """The mixed batch (ring only, one rotor, three rotors, three bodies, a lone atom, biphenyl, grown ligands of 14 and 25 atoms)
    and a second hexane without a pocket (pocket_of = -1), in pockets of 40, 80 and 120 atoms."""
    ligs, pockets, pocket_of = mixed_batch()
    ligs, pocket_of = ligs + [hexane()], pocket_of + [-1]
    inp = Inputs(cuda, [(one_hot(s), p) for s, p in ligs], pockets, pocket_of)
    ty, pst = pocket_types_gpu(inp)
    assert not pst.any() and not inp.got['status'].any()
    lo, hi = boxes(inp)
    return dict(inp=inp, ptypes=ty, lo=lo, hi=hi)


@pytest.fixture(scope='module')
def full(batch):
    return dock_gpu(batch['inp'], batch['ptypes'], batch['lo'], batch['hi'], seed=2024, **FULL)


def test_anchor_is_the_minimiser(plain):
    """n_chains = 1, n_steps = 0, step_iters = 0: mode 0 is kpd_vina_minimize's result to the bit."""
    inp, ty = plain['inp'], plain['ptypes']
    lo, hi = boxes(inp)
    want = minimize_gpu(inp, ty, max_iters=60)
    got = dock_gpu(inp, ty, lo, hi, 1, 0, 1, step_iters=0, max_iters=60)
    assert bits(got['pos'][0]) == bits(want['pos']) and bits(got['chain_pos'][0]) == bits(want['pos'])
    assert (got['n_found'] == 1).all() and not (got['status'] & (D.FEW_MODES | D.START_OUTSIDE | LEFT_OUT)).any()
    shared = D.NO_MOLECULE | D.BAD_INPUT | D.ATOM_OUT | D.FROZEN | D.FRAGMENTS
    assert ((got['status'] & shared) == (want['status'] & shared)).all()
    for col, src in (('score', 'score_after'), ('E', 'E_after'), ('inter', 'inter_after'), ('intra', 'intra_after'), ('rmsd_input', 'rmsd'),
                     ('gnorm', 'gnorm_after')):
        assert bits(got['report'][:, 0, COLS[col]]) == bits(want['report'][:, MIN_COLS[src]]), col
    assert (got['report'][:, 0, COLS['rmsd_best']] == 0).all() and (got['report'][:, 0, COLS['chain']] == 0).all()
    assert (want['report'][:, MIN_COLS['iterations']] > 0).sum() >= inp.B - 1


def test_trajectories_against_the_restatement(cuda):
    cases = [dock_case(cs) for cs, _ in DOCK_SEEDS]
    inp = Inputs(cuda, [(one_hot(c[0]), c[1]) for c in cases], [(c[2], c[3]) for c in cases], list(range(len(cases))))
    ty, _ = pocket_types_gpu(inp)
    lo, hi = boxes(inp)
    ids = [cs for cs, _ in DOCK_SEEDS]
    tol = max(TRAJ_FACTOR * DOCK_MEASURED_DEV, TRAJ_FLOOR)
    for b, (cs, ss) in enumerate(DOCK_SEEDS):
        out = dock_gpu(inp, ty, lo, hi, seed=ss, lig_id=ids, max_atoms=16, **DOCK_SHAPE, **DOCK_PARAMS)
        a = rows(inp, b)
        z, bonds, orders = inp.graph(b)
        q0, q1 = int(inp.pptr[b]), int(inp.pptr[b + 1])
        ref = D.dock_ligand(inp.pos[a], z, bonds, orders, inp.got['frag'][a], LIG_RADIUS[inp.got['elem'][a]], inp.px[q0:q1], ty[q0:q1],
                            inp.prad[q0:q1], lo[b], hi[b], lig_id=cs, seed=ss, params=DOCK_PARAMS, **DOCK_SHAPE)
        ev = lambda y: R.evaluate(y, ref['tree'], ref['types'], LIG_RADIUS[inp.got['elem'][a]], inp.px[q0:q1], ty[q0:q1], inp.prad[q0:q1])
        for c, ch in enumerate(ref['chains']):
            mine, rep, want = out['chain_pos'][c, a], out['chain_report'][b, c], ch['report']
            # chain_pos is the fp32 rounding of the kernel's fp64 point, which must lie within tol of the restatement's
            half_ulp = 0.5 * np.spacing(np.abs(mine)).astype(np.float64)
            dev = np.abs(mine.astype(np.float64) - ch['x64']) - half_ulp
            tol_e = max(TRAJ_FACTOR * 4e-16 * max(1.0, abs(want['E'])), EVAL_TOL * ev(ch['pos'].astype(np.float64))['abs_terms'])
            print(f'case {cs} seed {ss} chain {c}: positions beyond rounding {max(dev.max(), 0.0):.2e} A, |dE| {abs(rep[0] - want["E"]):.2e} '
                  f'of {want["E"]:.6g}, integer columns {[int(rep[CCOLS[k]]) for k in INTEGER_COLUMNS]}')
            assert [rep[CCOLS[k]] for k in INTEGER_COLUMNS] == [want[k] for k in INTEGER_COLUMNS], (cs, c)
            assert dev.max() <= tol, (cs, c, dev.max())
            for key in ('E', 'inter', 'intra', 'score'):
                assert abs(rep[CCOLS[key]] - want[key]) <= tol_e, (cs, c, key)
        assert out['n_found'][b] == ref['n_found'] and out['status'][b] == ref['status']
        assert out['report'][b, :ref['n_found'], COLS['chain']].tolist() == ref['kept'] and not out['report'][b, ref['n_found']:].any()
        for m, row in enumerate(ref['report']):
            assert abs(out['report'][b, m, COLS['rmsd_best']] - row['rmsd_best']) <= 1e-5       # fp32 rows an ulp apart at 40 A
            assert abs(out['report'][b, m, COLS['rmsd_input']] - row['rmsd_input']) <= 1e-5


def test_full_small_runs(batch, full):
    inp, ty, lo, hi = batch['inp'], batch['ptypes'], batch['lo'], batch['hi']
    nm = FULL['n_modes']
    first = minimize_gpu(inp, ty, max_iters=0)
    at_mode = [minimize_gpu(inp, ty, max_iters=0, pos=full['pos'][m]) for m in range(nm)]
    assert not (full['status'] & (LEFT_OUT | D.START_OUTSIDE)).any() and (full['n_found'] >= 1).all()
    assert (full['n_found'] >= 2).sum() >= 5 and (full['chain_report'][:, :, CCOLS['accepted']] > 0).any()
    assert (full['chain_report'][:, :, CCOLS['best_step']] > 0).any()
    taken = 0
    for b in range(inp.B):
        a = rows(inp, b)
        z, bonds, orders = inp.graph(b)
        radius = LIG_RADIUS[inp.got['elem'][a]]
        types = V.ligand_types(z, bonds, orders, radius)
        t = R.tree(z, bonds, orders, inp.got['frag'][a], 64, types)
        x = inp.pos[a].astype(np.float64)
        k = int(full['n_found'][b])
        assert bool(full['status'][b] & D.FEW_MODES) == (k < nm) and bits(full['pos'][k:, a]) == bits(np.broadcast_to(inp.pos[a], (nm - k,) + inp.pos[a].shape))
        assert not full['report'][b, k:].any()
        same = piece_pairs(t['piece'])
        for i, j in bonds:
            same[i, j] = same[j, i] = True
        dx = np.linalg.norm(x[:, None] - x[None, :], axis=2)
        for m in range(k):
            rep, y32 = full['report'][b, m], full['pos'][m, a]
            y = y32.astype(np.float64)
            # rigid by construction, as in test_vina_min_gpu.py: the fp32 rounding of the two ends, plus 1e-11 for at most 110
            # composed fp64 moves (7 minimisations of 10 iterations, 30 of the refinement, 7 mutations) of a few ulps of 40 A each
            half = np.sqrt((np.spacing(np.abs(y32)).astype(np.float64) ** 2).sum(axis=1)) * 0.5
            bound = half[:, None] + half[None, :] + 1e-11
            dy = np.linalg.norm(y[:, None] - y[None, :], axis=2)
            assert (np.abs(dy - dx)[same] <= bound[same]).all(), (b, m, (np.abs(dy - dx) - bound)[same].max())
            # the report describes the rows written: kpd_vina_minimize's one evaluation there, and the restatement's
            e = R.evaluate(y, t, types, radius, *pocket_of_ligand(inp, b, ty))
            tol = EVAL_TOL * e['abs_terms']
            other = at_mode[m]['report'][b]
            for key in ('E', 'inter', 'intra', 'score'):
                assert abs(rep[COLS[key]] - other[MIN_COLS[key + '_before']]) <= tol, (b, m, key)
            assert abs(rep[COLS['E']] - e['E']) <= tol and abs(rep[COLS['gnorm']] - other[MIN_COLS['gnorm_before']]) <= 1e-9 * max(1.0, rep[COLS['gnorm']])
            c = int(rep[COLS['chain']])
            assert bits(full['chain_pos'][c, a]) == bits(y32) and full['chain_report'][b, c, CCOLS['found']] == 1
            assert bits(full['chain_report'][b, c, [0, 1, 2, 8, 9]]) == bits(rep[[COLS['E'], COLS['inter'], COLS['intra'], COLS['gnorm'], COLS['score']]])
            d = y - x
            assert abs(rep[COLS['rmsd_input']] - np.sqrt((d * d).sum() / len(x))) <= 1e-12 * max(rep[COLS['rmsd_input']], 1e-30) + 1e-300
            if m:                                             # ascending in E, min_rmsd or more from every better mode
                assert rep[COLS['E']] >= full['report'][b, m - 1, COLS['E']]
                for o in range(m):
                    assert D.rmsd(y32, full['pos'][o, a]) >= 1.0 - 1e-12, (b, m, o)
                assert abs(rep[COLS['rmsd_best']] - D.rmsd(y32, full['pos'][0, a])) <= 1e-12
            if c >= 1:                                        # a random start and its steps stay in the box (half an fp32 ulp of slack)
                ctr = y.sum(axis=0) / len(y)
                assert (ctr >= lo[b] - 4e-6).all() and (ctr <= hi[b] + 4e-6).all(), (b, m, c, ctr, lo[b], hi[b])
                taken += 1
        assert full['report'][b, 0, COLS['E']] <= first['report'][b, MIN_COLS['E_before']], b
        cr = full['chain_report'][b]
        steps = cr[:, CCOLS['accepted']] + cr[:, CCOLS['box_rejected']]
        assert (steps <= FULL['n_steps']).all() and (cr[:, CCOLS['best_step']] <= FULL['n_steps']).all() and (cr[:, CCOLS['evaluations']] >= 3).all()
    assert taken >= 3


def test_bitwise_invariance(batch, full):
    inp, ty, lo, hi = batch['inp'], batch['ptypes'], batch['lo'], batch['hi']
    run = lambda i=inp, l=lo, h=hi, **kw: dock_gpu(i, ty, l, h, **dict(dict(FULL, seed=2024), **kw))
    again = run()                                                                            # the repeat
    for k in full:
        assert bits(full[k]) == bits(again[k]), k
    ids = run(lig_id=list(range(inp.B)))                                                     # lig_id = NULL is the ligand's index
    for k in full:
        assert bits(full[k]) == bits(ids[k]), k
    for kw in (dict(max_atoms=256), dict(max_pocket=0), dict(max_atoms=25, max_pocket=50)):  # the bounds are no part of the result
        o = run(**kw)
        for k in full:
            assert bits(full[k]) == bits(o[k]), (kw, k)
    first = minimize_gpu(inp, ty, max_iters=0)
    top = int(first['report'][:, MIN_COLS['n_rot']].max())
    o = run(max_rotors=top)                                                                  # max_rotors = T against 64
    for k in full:
        assert bits(full[k]) == bits(o[k]), k
    order = list(range(inp.B))[::-1]                                                         # the reversed batch, lig_id carried
    rev = Inputs(inp.dev, [inp.ligs[b] for b in order], inp.pockets, [inp.pocket_of[b] for b in order])
    o = run(rev, lo[order], hi[order], lig_id=order)
    for k, b in enumerate(order):
        same_ligand(full, inp, b, o, rev, k)
    for b in (1, 3, 4, 7, 8):                                                                # a ligand alone, LDS sized for it
        one = Inputs(inp.dev, [inp.ligs[b]], inp.pockets, [inp.pocket_of[b]])
        same_ligand(full, inp, b, run(one, lo[b:b + 1], hi[b:b + 1], lig_id=[b], max_atoms=len(inp.ligs[b][1]),
                                      max_rotors=int(first['report'][b, MIN_COLS['n_rot']])), one, 0)
    two = run(n_chains=2, n_modes=2)                                                         # chains 0 and 1 do not depend on n_chains
    for b in range(inp.B):
        same_ligand(full, inp, b, two, inp, b, chains=(0, 1))
    other = run(seed=2025)                                                                   # another seed: chain 0's start is the same
    assert bits(other['chain_pos'][1:]) != bits(full['chain_pos'][1:])
    high = run(seed=2024 + (1 << 32))                                                        # the high half of the seed is part of the key
    assert bits(high['chain_pos'][1:]) != bits(full['chain_pos'][1:])


def test_bad_inputs(batch, full):
    inp, ty, lo, hi = batch['inp'], batch['ptypes'], batch['lo'], batch['hi']
    run = lambda l=lo, h=hi, **kw: dock_gpu(inp, ty, l, h, **dict(dict(FULL, seed=2024), **kw))

    def check(o, changed, bit, src=None):
        src = inp.pos if src is None else src
        for b in range(inp.B):
            if b not in changed:
                same_ligand(full, inp, b, o, inp, b)
            else:
                assert o['status'][b] == bit and o['n_found'][b] == 0 and not o['report'][b].any() and not o['chain_report'][b].any(), (b, o['status'][b])
                a = rows(inp, b)
                for block in (o['pos'], o['chain_pos']):
                    assert bits(block[:, a]) == bits(np.broadcast_to(src[a], (block.shape[0],) + src[a].shape)), b

    bad_lo, bad_hi = lo.copy(), hi.copy()
    bad_lo[1, 2] = bad_hi[1, 2] + 1.0                                                        # lo > hi
    bad_hi[3, 0] = np.nan
    bad_lo[6, 1] = -np.inf
    check(run(bad_lo, bad_hi), [1, 3, 6], D.BAD_BOX)
    flat_lo, flat_hi = lo.copy(), hi.copy()                                                  # lo = hi is a box; a far one only sets bit 8
    flat_lo[2], flat_hi[2] = 100.0, 100.0
    o = run(flat_lo, flat_hi)
    assert o['status'][2] & D.START_OUTSIDE and not o['status'][2] & LEFT_OUT and o['n_found'][2] >= 1
    cr = o['chain_report'][2]                                # chain 0 keeps its start and loses every step; a random start ends at once
    assert cr[0, CCOLS['box_rejected']] == FULL['n_steps'] and cr[0, CCOLS['found']] == 1 and not cr[:, CCOLS['accepted']].any()
    assert (cr[1:, CCOLS['box_rejected']] == 1).all() and not cr[1:, CCOLS['found']].any() and o['n_found'][2] == 1
    pos = inp.pos.copy()
    pos[int(inp.ptr[5]) + 2, 0] = np.nan                                                     # a NaN coordinate: bit 1
    check(run(pos=pos), [5], D.BAD_INPUT, pos)
    check(run(max_atoms=14), [7], D.NO_MOLECULE)                                             # more atoms than max_atoms: bit 0
    for kw in (dict(n_chains=0), dict(n_chains=65, n_modes=4), dict(n_modes=0), dict(n_modes=5), dict(n_steps=-1), dict(max_rotors=65)):
        with pytest.raises(hip.KpdError):
            run(**kw)
    for name, value in (('temperature', 0.0), ('amplitude', -1.0), ('min_rmsd', 0.0), ('temperature', float('nan')), ('step_iters', -1)):
        p = hip.vina_dock_params()
        setattr(p, name, value)
        with pytest.raises(hip.KpdError):
            run(struct=p)
        with pytest.raises(hip.KpdError):
            hip.vina_dock_params(**{name: value})


def test_python_surface(cuda):
    rng = np.random.default_rng(5)
    ligs = [grow(rng, n) for n in (8, 11, 5, 9, 14, 7)]
    pos = [torch.from_numpy(p).to(cuda) for _, p in ligs]
    feat = [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in ligs]
    anchor = np.concatenate([p for _, p in ligs])
    pockets = [make_pocket(rng, 40, anchor, reach=4.0), make_pocket(rng, 60, anchor, reach=4.0)]
    ppos, psym = [torch.from_numpy(p).to(cuda) for _, p in pockets], [s for s, _ in pockets]
    mols = molecule.build_molecules(pos, feat, ELEMENTS)
    pof = [0, 0, 0, 1, 1, -1]
    kw = dict(pocket_of=pof, radii=RADII, n_chains=3, n_steps=2, seed=7, step_iters=5, max_iters=10)
    d = mols.vina_dock(ppos, psym, **kw)
    assert d.report.shape == (6, 3, 8) and d.chain_report.shape == (6, 3, 10) and d.n_found.shape == (6,) and d.n_modes == 3
    assert not bool((d.status & LEFT_OUT).any()) and bool((d.n_found >= 1).all())
    own = [own_box(p) for _, p in ligs]                                                      # no box: the ligand's own, widened by 4
    assert bits(d.box[0].cpu().numpy()) == bits(np.stack([l for l, _ in own])) and bits(d.box[1].cpu().numpy()) == bits(np.stack([h for _, h in own]))
    refs = [ligs[1][1], ligs[4][1]]                                                          # autobox_ligand: per pocket, widened by autobox_add
    ab = mols.vina_dock(ppos, psym, autobox_ligand=[torch.from_numpy(r) for r in refs], autobox_add=3.0, **kw)
    want = [own_box(refs[q], 3.0) if q >= 0 else own_box(ligs[b][1], 3.0) for b, q in enumerate(pof)]
    assert bits(ab.box[0].cpu().numpy()) == bits(np.stack([l for l, _ in want])) and bits(ab.box[1].cpu().numpy()) == bits(np.stack([h for _, h in want]))
    per_pocket = (np.array([[-9.0, -9.0, -9.0], [-8.0, -8.0, -8.0]], dtype=np.float32), np.array([[9.0, 9.0, 9.0], [8.0, 8.0, 8.0]], dtype=np.float32))
    bp = mols.vina_dock(ppos, psym, box=per_pocket, **kw)
    assert bp.box[0][:5, 0].tolist() == [-9.0, -9.0, -9.0, -8.0, -8.0] and bits(bp.box[0][5].cpu().numpy()) == bits(own[5][0])
    per_ligand = (d.box[0].clone(), d.box[1].clone())
    bl = mols.vina_dock(ppos, psym, box=per_ligand, **kw)
    assert torch.equal(bl.report, d.report) and torch.equal(bl.molecules.pos, d.molecules.pos)
    # the SDF: per ligand its found modes in rank order; the table: one row per found mode
    found = d.n_found.tolist()
    text = d.sdf()
    assert [s.count('$$$$') for s in text] == found
    for b in range(6):
        assert text[b].startswith(d.mode(0).sdf()[b]) and (found[b] < 2 or text[b].endswith(d.mode(found[b] - 1).sdf()[b]))
    t = d.table()
    assert list(t) == ['lig_idx', 'mode', 'score', 'rmsd_input', 'chain'] and len(t['mode']) == sum(found)
    assert t['lig_idx'] == [b for b in range(6) for _ in range(found[b])] and t['score'][0] == d.report[0, 0, 0].item()
    # mode 0 is a drop-in pose: kpd_vina_score there gives the reported score
    v = d.molecules.vina_score(ppos, psym, pocket_of=pof, radii=RADII, pocket_types=d.pocket_types)
    assert bool(((v.report[:, 0] - d.report[:, 0, 0]).abs() <= EVAL_TOL * v.report[:, 2:7].abs().sum(dim=1) + 1e-300).all())
    assert [tuple(p.shape) for p in torch.split(d.mode(2).pos, [len(p) for _, p in ligs])] == [tuple(p.shape) for p in pos]
    with pytest.raises(IndexError):
        d.mode(3)
    with pytest.raises(hip.KpdError):
        mols.vina_dock(ppos, psym, pocket_of=pof, radii=RADII, n_chains=65)
    with pytest.raises(hip.KpdError):
        mols.vina_dock(ppos, psym, pocket_of=pof, radii=RADII, temperatur=1.0)
    with pytest.raises(hip.KpdError):                                                        # a host tensor
        mols.vina_dock([p.cpu() for p in ppos], psym, pocket_of=pof, radii=RADII)
    # dock_samples: two pockets x three ligands as `_sample` returns them
    samples = [dict(positions=[p.cpu() for p in pos[3 * q:3 * q + 3]], features=[f.cpu() for f in feat[3 * q:3 * q + 3]]) for q in range(2)]
    pk = [dict(positions=torch.from_numpy(p), elements=s) for s, p in pockets]
    skw = dict(kw, pocket_of=None)
    del skw['pocket_of']
    ds = molecule.dock_samples(samples, pk, ELEMENTS, device=cuda, ref_ligands=refs, autobox_add=3.0, **skw)
    direct = mols.vina_dock(ppos, psym, autobox_ligand=refs, autobox_add=3.0, **dict(kw, pocket_of=[0, 0, 0, 1, 1, 1]))
    assert torch.equal(ds.report, direct.report) and torch.equal(ds.molecules.pos, direct.molecules.pos)
    # an empty batch
    z32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=cuda)
    none = molecule.Molecules(z32(1), z32(0, 4), z32(0), z32(0), z32(0), z32(0), z32(0, 2), z32(0), z32(1), torch.zeros(0, 3, device=cuda),
                              ELEMENTS, sizes=[])
    e = none.vina_dock(ppos[:1], psym[:1], radii=RADII, n_chains=2)
    assert e.report.shape == (0, 2, 8) and e.n_found.shape == (0,) and e.status.shape == (0,) and e.molecules.pos.shape == (0, 3)
    assert e.sdf() == [] and e.table() == dict(lig_idx=[], mode=[], score=[], rmsd_input=[], chain=[])
