"""Relaxation of ligands inside rigid pockets on the GPU (kpd_relax, keypoint_diffusion_amd.molecule.Molecules.relax) against the
float64 restatement of include/kpd.h (tests/relax_ref.py).  Every raw call runs with canary bytes behind each output buffer; the
bond graphs come from kpd_mol_perceive, as a caller's would.  max_iters <= 60 throughout."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import relax_ref as R
from .molecule_cases import ALLOWED, ELEMENTS, TWO_ETHANOLS_CL, Z, one_hot
from .relax_cases import LIG_VDW, MINIMA, TRAJ_SEEDS, grow, make_pocket, measure, ring6, traj_case, vdw_rows
from .test_molecule_gpu import Guarded, cloud, concat, perceive_gpu

pytestmark = pytest.mark.gpu

# One evaluation: two fp64 sums of <= 1e5 terms in different orders, with or without FMA contraction, differ by at most about
# 1e-11 of the sum of the absolute terms; the kernel is allowed 1e-10 of it (plus, for the bonded terms, 16 roundings of their
# inputs: relax_ref.tolerances says why; without that a two-atom ligand at its minimum, E = 8e-13, can be met by nobody).
EVAL_TOL = 1e-10
# Trajectories: the restatement against itself with every sum reversed deviates, over the seeds below and K = 1, 2, 5 iterations,
# by at most 1.5e-14 A in the positions and 4e-16 max(1, |E|) in the energy (measured on the CPU, profiles/relax.md).  The GPU is
# allowed 100 x that, which is below the floor of 1e-9 A; so the floor is the tolerance.
TRAJ_MEASURED_DEV, TRAJ_FACTOR, TRAJ_FLOOR = 1.5e-14, 100.0, 1e-9


class Inputs:
    """A batch on the device: perceived ligands, pockets, pocket_of; and the per-ligand pieces the restatement needs."""

    def __init__(self, dev, ligs, pockets, pocket_of):
        pos, feat, ptr = concat(ligs)
        self.got, self.t = perceive_gpu(dev, pos, feat, ptr)
        self.dev, self.pos, self.ptr, self.B = dev, pos, ptr, len(ligs)
        self.pockets = pockets                                  # [(symbols, pos float32)]
        sizes = [len(p) for _, p in pockets]
        self.pptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.px = np.concatenate([p.reshape(-1, 3) for _, p in pockets] + [np.zeros((0, 3), np.float32)]).astype(np.float32)
        self.pv = np.concatenate([vdw_rows(s) for s, _ in pockets] + [np.zeros((0, 2), np.float32)]).astype(np.float32)
        self.pocket_of = np.asarray(pocket_of, dtype=np.int64)
        self.max_pocket = max(sizes, default=0)

    def ligand(self, b, pos=None):
        """(pos, topology, per-atom vdW, pocket pos, pocket vdW) of ligand b for the restatement."""
        a0, a1 = int(self.ptr[b]), int(self.ptr[b + 1])
        p0, p1 = int(self.got['bond_ptr'][b]), int(self.got['bond_ptr'][b + 1])
        elem = self.got['elem'][a0:a1]
        x = self.pos[a0:a1] if pos is None else pos[a0:a1]
        topo = R.topology(self.pos[a0:a1], [Z[c] for c in elem], self.got['bonds'][p0:p1] - a0)
        q = int(self.pocket_of[b])
        ppos, pv = (self.pockets[q][1], vdw_rows(self.pockets[q][0])) if q >= 0 else (np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32))
        return x, topo, LIG_VDW[elem], ppos, pv


def relax_gpu(inp, max_atoms=256, max_pocket=None, pos=None, bonds=None, pocket_of=None, px=None, **params):
    """kpd_relax through the C ABI with canaries; returns (pos_out [N,3] float32, report [B,12], status [B]) as numpy."""
    dev, t = inp.dev, inp.t
    N, B = t['pos'].shape[0], inp.B
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    pos_d = t['pos'] if pos is None else to(pos, torch.float32)
    bonds_d = t['bonds'] if bonds is None else to(bonds, torch.int32)
    px_d, pv_d = to(inp.px if px is None else px, torch.float32), to(inp.pv, torch.float32)
    pptr_d = to(inp.pptr, torch.int32)
    pof_d = to(inp.pocket_of if pocket_of is None else pocket_of, torch.int32)
    zt, lv = torch.tensor(Z, dtype=torch.int32, device=dev), to(LIG_VDW, torch.float32)
    keep = [x.clone() for x in (px_d, pv_d, pptr_d, pof_d, pos_d)]
    g = Guarded(dev)
    out, rep, st = g.new(3 * N, torch.float32), g.new(12 * B, torch.float64), g.new(B)
    p = hip.relax_params(**params)
    import ctypes
    hip.check(hip.lib().kpd_relax(pos_d.data_ptr(), t['ptr'].data_ptr(), N, B, max_atoms, t['elem'].data_ptr(), len(Z), zt.data_ptr(),
                                  lv.data_ptr(), bonds_d.data_ptr(), t['bond_ptr'].data_ptr(), t['cap'], t['status'].data_ptr(),
                                  px_d.data_ptr(), pv_d.data_ptr(), pptr_d.data_ptr(), px_d.shape[0], len(inp.pptr) - 1,
                                  inp.max_pocket if max_pocket is None else max_pocket, pof_d.data_ptr(), ctypes.byref(p),
                                  out.data_ptr(), rep.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    for a, b in zip(keep, (px_d, pv_d, pptr_d, pof_d, pos_d)):
        assert a.reshape(-1).view(torch.uint8).equal(b.reshape(-1).view(torch.uint8)), 'an input buffer was written'
    return out[:3 * N].cpu().numpy().reshape(N, 3), rep[:12 * B].cpu().numpy().reshape(B, 12), st[:B].cpu().numpy().astype(np.int64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope='module')
def batch(cuda):
    """About 70 ligands of 1 .. 40 atoms (a single atom, one without bonds, two fragments, strained clouds), one of 256 and one of
    257 atoms; pockets of 0, 37, 300 and 700 atoms (700 is more than fits in LDS beside a 256-atom ligand) and pocket_of = -1."""
    rng = np.random.default_rng(7)
    ligs = [(one_hot(s), p) for s, p in (grow(rng, n) for n in [1, 2, 40] + [int(rng.integers(3, 40)) for _ in range(58)])]
    ligs.append((one_hot(['C', 'O', 'N']), np.array([[0, 0, 0], [4.1, 0, 0], [0, 4.3, 0.5]], dtype=np.float32)))      # no bonds
    ligs.append((one_hot(TWO_ETHANOLS_CL[0]), TWO_ETHANOLS_CL[1]))                                                      # fragments
    ligs += [cloud(rng, int(rng.integers(5, 30)), s) for s in (1.0, 1.6, 2.2, 1.6)]                                       # strained
    i256, i257 = len(ligs), len(ligs) + 1
    big = grow(rng, 256)
    ligs.append((one_hot(big[0]), big[1]))
    ligs.append(cloud(rng, 257, 1.6))
    anchor = np.concatenate([p for _, p in ligs[:20]])
    pockets = [([], np.zeros((0, 3), np.float32))] + [make_pocket(rng, m, anchor[:40], reach=5.0, keep_out=0.8) for m in (37, 300, 700)]
    pocket_of = [(-1, 0, 1, 2, 3)[b % 5] for b in range(len(ligs))]
    pocket_of[i256], pocket_of[i257] = 3, 2
    inp = Inputs(cuda, ligs, pockets, pocket_of)
    first = []
    for b in range(inp.B):
        if b == i257:
            first.append(None)
            continue
        x, topo, lv, ppos, pv = inp.ligand(b)
        first.append(R.energy(x.astype(np.float64), topo, lv, ppos, pv, R.DEFAULTS))
    return dict(inp=inp, first=first, i256=i256, i257=i257)


def test_one_evaluation(batch):
    inp, first = batch['inp'], batch['first']
    out, rep, st = relax_gpu(inp, max_iters=0)
    assert bits(out).tobytes() == bits(inp.pos).tobytes()
    assert st[batch['i257']] == 1 and not rep[batch['i257']].any()
    worst = 0.0
    for b, f in enumerate(first):
        if f is None:
            continue
        tol_e, tol_g = R.tolerances(f, EVAL_TOL)
        dev = (abs(rep[b, 0] - f['E']), abs(rep[b, 10] - f['parts'][3]), abs(rep[b, 11] - f['gmax']))
        worst = max(worst, dev[0] / max(f['abs_E'], 1e-300), dev[1] / max(f['abs_E'], 1e-300))
        assert dev[0] <= tol_e and dev[1] <= tol_e and dev[2] <= tol_g, (b, dev, tol_e, tol_g)
        assert rep[b, 1] == rep[b, 0] and rep[b, 2] == 0.0 and rep[b, 3] == rep[b, 11] and rep[b, 4] == 0 and rep[b, 5] == 1
        assert rep[b, 9] == rep[b, 10] and st[b] == (4 if rep[b, 11] > 1e-3 else 0), (b, st[b])
    print(f'one evaluation: worst |dE| / sum|terms| = {worst:.2e} (allowed {EVAL_TOL:.0e})')
    assert st[0] == 0 and rep[0, 0] == 0.0                   # a single atom without a pocket: nothing to do


@pytest.mark.parametrize('K', [1, 2, 5])
def test_trajectory(cuda, K):
    cases = [traj_case(s) for s in TRAJ_SEEDS]
    inp = Inputs(cuda, [(one_hot(c[0]), c[1]) for c in cases], [(c[2], c[3]) for c in cases], list(range(len(cases))))
    out, rep, st = relax_gpu(inp, max_atoms=16, max_iters=K)
    tol = max(TRAJ_FACTOR * TRAJ_MEASURED_DEV, TRAJ_FLOOR)
    for b in range(inp.B):
        x, topo, lv, ppos, pv = inp.ligand(b)
        ref = R.minimize(x, topo, lv, ppos, pv, dict(max_iters=K))
        rev = R.minimize(x, topo, lv, ppos, pv, dict(max_iters=K), reverse=True)
        assert np.abs(ref['x64'] - rev['x64']).max() <= TRAJ_MEASURED_DEV            # the measurement behind the constant
        a0, a1 = int(inp.ptr[b]), int(inp.ptr[b + 1])
        mine = out[a0:a1].astype(np.float64)
        # pos_out is the fp32 rounding of the kernel's fp64 point, which must lie within tol of the restatement's
        half_ulp = 0.5 * np.spacing(np.abs(out[a0:a1])).astype(np.float64)
        dev = np.abs(mine - ref['x64']) - half_ulp
        print(f'seed {TRAJ_SEEDS[b]} K {K}: positions beyond rounding {max(dev.max(), 0.0):.2e} A, '
              f'|dE| {abs(rep[b, 1] - ref["E"]):.2e} of {ref["E"]:.6g}')
        assert dev.max() <= tol, (b, dev.max())
        tol_e = max(TRAJ_FACTOR * 4e-16 * max(1.0, abs(ref['E'])), R.tolerances(ref['last'], EVAL_TOL)[0])
        assert abs(rep[b, 1] - ref['E']) <= tol_e and abs(rep[b, 0] - ref['E_before']) <= tol_e
        assert (rep[b, 4], rep[b, 5], st[b]) == (ref['iters'], ref['evals'], ref['status'])


@pytest.fixture(scope='module')
def full(batch):
    return relax_gpu(batch['inp'], max_iters=60)


def test_full_runs(batch, full):
    inp = batch['inp']
    out, rep, st = full
    moved = 0
    for b in range(inp.B):
        a0, a1 = int(inp.ptr[b]), int(inp.ptr[b + 1])
        if b == batch['i257']:
            assert st[b] == 1 and not rep[b].any() and bits(out[a0:a1]).tobytes() == bits(inp.pos[a0:a1]).tobytes()
            continue
        assert not st[b] & 3 and rep[b, 1] <= rep[b, 0] and rep[b, 4] <= 60 and rep[b, 5] >= rep[b, 4] + 1, (b, st[b], rep[b])
        x, topo, lv, ppos, pv = inp.ligand(b, out)
        e = R.energy(x.astype(np.float64), topo, lv, ppos, pv, R.DEFAULTS)
        tol, tol_g = R.tolerances(e, EVAL_TOL)
        assert abs(rep[b, 1] - e['E']) <= tol and np.all(np.abs(rep[b, 6:10] - e['parts']) <= tol), (b, rep[b], e['E'], e['parts'])
        assert abs(rep[b, 3] - e['gmax']) <= tol_g, (b, rep[b, 3], e['gmax'], tol_g)
        assert e['gmax'] <= 1e-3 or st[b] & 12, (b, e['gmax'], st[b])
        d = out[a0:a1].astype(np.float64) - inp.pos[a0:a1].astype(np.float64)
        rmsd = np.sqrt((d * d).sum() / (a1 - a0))
        assert abs(rep[b, 2] - rmsd) <= 1e-12 * max(rmsd, 1e-30) + 1e-300, (b, rep[b, 2], rmsd)        # the same fp32 rows, in fp64
        moved += rep[b, 4] > 0
    assert moved >= inp.B - 8


def test_known_minima_on_the_device(cuda):
    ring = ring6(np.random.default_rng(6))
    cases = [(c[1], c[2]) for c in MINIMA] + [ring]
    inp = Inputs(cuda, [(one_hot(s), p) for s, p in cases], [], [-1] * len(cases))
    out, rep, st = relax_gpu(inp, max_atoms=8, max_iters=60, w_intra=0.0, gtol=1e-5)
    assert not (st & 3).any() and (rep[:, 4] < 60).all(), (st, rep[:, 4])
    for b, c in enumerate(MINIMA):
        L, A = measure(out[int(inp.ptr[b]):int(inp.ptr[b + 1])], c[3], c[4])
        for k, v in c[3].items():
            assert abs(L[k] - v) < 1e-5, (c[0], k, L[k])     # k_b |d - r0| <= gtol, and fp32 rows
        for k, v in c[4].items():
            # near 180 degrees the force is cubic in the deviation: (2 r gtol / k_a)^(1/3) = 0.3 degrees
            assert abs(A[k] - v) < (0.5 if v == 180.0 else 1e-3), (c[0], k, A[k])
    p = out[int(inp.ptr[len(MINIMA)]):]
    d = np.linalg.norm(p - np.roll(p, -1, axis=0), axis=1)
    assert np.abs(d - 1.42).max() < 1e-5 and np.all(p[:, 2] == 0.0), d
    # a lone atom 2 A from one pocket atom settles at d = x_ij on the line joining them
    pos = np.array([[0.3, -0.2, 0.5]], dtype=np.float32)
    dirn = np.array([1.0, 2.0, -2.0]) / 3.0
    ppos = (pos[0].astype(np.float64) + 2.0 * dirn).astype(np.float32).reshape(1, 3)
    lone = Inputs(cuda, [(one_hot(['C']), pos)], [(['O'], ppos)], [0])
    out, rep, st = relax_gpu(lone, max_atoms=1, max_iters=60, gtol=1e-6)
    v, d0 = out[0].astype(np.float64) - ppos[0], pos[0].astype(np.float64) - ppos[0]
    xij = np.sqrt(np.float64(LIG_VDW[0, 0])) * np.sqrt(np.float64(vdw_rows(['O'])[0, 0]))
    assert abs(np.linalg.norm(v) - xij) < 1e-5 and rep[0, 4] < 60        # e'' = 72 D / x^2 ~ 0.4: |d - x| <= gtol / e''
    assert np.linalg.norm(np.cross(v / np.linalg.norm(v), d0 / np.linalg.norm(d0))) < 1e-6 and v @ d0 > 0


def test_batch_invariance(batch, full):
    inp = batch['inp']
    out, rep, st = full
    again = relax_gpu(inp, max_iters=60)
    for a, b in zip(full, again):
        assert bits(a).tobytes() == bits(b).tobytes()
    # staging is no part of the result: nothing staged, and LDS sized for 64 atoms (the 256-atom ligand is then left out)
    o2, r2, s2 = relax_gpu(inp, max_atoms=64, max_pocket=0, max_iters=60)
    small = [b for b in range(inp.B) if inp.ptr[b + 1] - inp.ptr[b] <= 64]
    assert s2[batch['i256']] == 1 and np.array_equal(s2[small], st[small]) and bits(r2[small]).tobytes() == bits(rep[small]).tobytes()
    # the reversed batch, and ligands alone
    ligs = [(inp.t['pos'][int(inp.ptr[b]):int(inp.ptr[b + 1])].cpu().numpy(), b) for b in range(inp.B)]
    feat = one_hot([ELEMENTS[c] for c in inp.got['elem'][:int(inp.ptr[batch['i257']])]])
    order = [b for b in range(inp.B) if b != batch['i257']][::-1]
    rev = Inputs(inp.dev, [(feat[int(inp.ptr[b]):int(inp.ptr[b + 1])], ligs[b][0]) for b in order], inp.pockets, [inp.pocket_of[b] for b in order])
    o3, r3, s3 = relax_gpu(rev, max_iters=60)
    for k, b in enumerate(order):
        assert bits(r3[k]).tobytes() == bits(rep[b]).tobytes() and s3[k] == st[b], (b, r3[k], rep[b])
        assert bits(o3[int(rev.ptr[k]):int(rev.ptr[k + 1])]).tobytes() == bits(out[int(inp.ptr[b]):int(inp.ptr[b + 1])]).tobytes(), b
    for b in (2, 7, 33, batch['i256']):
        one = Inputs(inp.dev, [(feat[int(inp.ptr[b]):int(inp.ptr[b + 1])], ligs[b][0])], inp.pockets, [inp.pocket_of[b]])
        o1, r1, s1 = relax_gpu(one, max_atoms=int(inp.ptr[b + 1] - inp.ptr[b]), max_iters=60)
        assert bits(r1[0]).tobytes() == bits(rep[b]).tobytes() and s1[0] == st[b], b
        assert bits(o1).tobytes() == bits(out[int(inp.ptr[b]):int(inp.ptr[b + 1])]).tobytes(), b


def test_left_out_ligands(cuda):
    rng = np.random.default_rng(3)
    ligs = [(one_hot(s), p) for s, p in (grow(rng, n) for n in (9, 12, 7, 15, 11, 6))]
    anchor = np.concatenate([p for _, p in ligs])
    inp = Inputs(cuda, ligs, [make_pocket(rng, 20, anchor), make_pocket(rng, 90, anchor)], [0, 1, 0, 1, 5, -2])
    good, _, good_st = relax_gpu(inp, max_atoms=16, max_iters=10, pocket_of=[0, 1, 0, 1, 1, -1])
    pos = inp.pos.copy()
    pos[int(inp.ptr[1]) + 3, 1] = np.nan                         # ligand 1: a NaN coordinate
    px = inp.px.copy()
    bonds = inp.got['bonds'].astype(np.int32).copy()
    p2, p3 = int(inp.got['bond_ptr'][2]), int(inp.got['bond_ptr'][3])
    bonds[p2, 1] = int(inp.ptr[3]) + 1                          # ligand 2: a bond that leaves the ligand
    bonds[p3 + 1] = bonds[p3]                                   # ligand 3: a bond twice
    out, rep, st = relax_gpu(inp, max_atoms=16, max_iters=10, pos=pos, bonds=bonds)
    assert st.tolist()[1:] == [2, 1, 1, 2, 2] and not st[0] & 3, st       # ligands 4, 5: pocket_of = 5 and -2, out of range
    assert not rep[1:].any() and bits(out[int(inp.ptr[1]):]).tobytes() == bits(pos[int(inp.ptr[1]):]).tobytes()
    assert bits(out[:int(inp.ptr[1])]).tobytes() == bits(good[:int(inp.ptr[1])]).tobytes()
    px[int(inp.pptr[1]) + 50, 2] = np.inf                       # a non-finite pocket atom: every ligand of pocket 1
    out, rep, st = relax_gpu(inp, max_atoms=16, max_pocket=10, max_iters=10, px=px, pocket_of=[0, 1, 0, 1, 1, -1])
    assert (st & 3).tolist() == [0, 2, 0, 2, 2, 0], st
    # more atoms than max_atoms: left out, not truncated
    out, rep, st = relax_gpu(inp, max_atoms=8, max_iters=10, pocket_of=[0, 1, 0, 1, 1, -1])
    assert (st & 1).tolist() == [1, 1, 0, 1, 1, 0], st


def test_through_the_python_surface(cuda):
    rng = np.random.default_rng(5)
    ligs = [grow(rng, n) for n in (8, 11, 5, 9, 14, 7)]
    pos = [torch.from_numpy(p).to(cuda) for _, p in ligs]
    feat = [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in ligs]
    anchor = np.concatenate([p for _, p in ligs])
    pockets = [make_pocket(rng, 25, anchor), make_pocket(rng, 60, anchor)]
    mols = molecule.build_molecules(pos, feat, ELEMENTS)
    ppos = [torch.from_numpy(p).to(cuda) for _, p in pockets]
    r = mols.relax(ppos, [s for s, _ in pockets], pocket_of=[0, 0, 0, 1, 1, 1], max_iters=30)
    assert len(r.pos) == 6 and [tuple(p.shape) for p in r.pos] == [tuple(p.shape) for p in pos]
    assert r.report.shape == (6, 12) and r.status.shape == (6,) and not bool((r.status & 3).any())
    assert bool((r.report[:, 1] <= r.report[:, 0]).all()) and bool((r.report[:, 4] > 0).all())
    before, after = mols.sdf(), r.molecules.sdf()
    for b, (x, y) in enumerate(zip(before, after)):
        lx, ly = x.split('\n'), y.split('\n')
        n = ligs[b][1].shape[0]
        assert len(lx) == len(ly) and lx[:4] == ly[:4] and lx[4 + n:] == ly[4 + n:]          # header, counts, bonds, tail
        want = r.pos[b].cpu().numpy()
        for a in range(n):
            assert ly[4 + a][30:] == lx[4 + a][30:]
            assert ly[4 + a][:30] == '%10.4f%10.4f%10.4f' % tuple(float(v) for v in want[a])
    assert r.molecules.metrics() == mols.metrics() and torch.equal(r.molecules.keys(), mols.keys())
    t = r.table()
    assert list(t) == ['lig_idx', 'rmsd', 'energy_before', 'energy_after', 'pocket_energy'] and t['lig_idx'] == list(range(6))
    assert t['rmsd'] == r.report[:, 2].tolist() and t['energy_after'] == r.report[:, 1].tolist()
    # one pocket: pocket_of defaults to it; several: it must be given; an unknown element needs vdw=
    one = mols.relax(ppos[:1], [pockets[0][0]], max_iters=30)
    assert torch.equal(one.report[:3], r.report[:3])
    with pytest.raises(ValueError):
        mols.relax(ppos, [s for s, _ in pockets])
    with pytest.raises(hip.KpdError):
        mols.relax(ppos[:1], [['Xx'] * 25])
    assert mols.relax(ppos[:1], [['Xx'] * 25], vdw={'Xx': (3.5, 0.1)}, max_iters=5).report.shape == (6, 12)
    # relax_samples: two pockets x three ligands, as `_sample` returns them (host tensors, copied to `device`)
    samples = [dict(positions=[p.cpu() for p in pos[3 * q:3 * q + 3]], features=[f.cpu() for f in feat[3 * q:3 * q + 3]]) for q in range(2)]
    pk = [dict(positions=torch.from_numpy(p), elements=s) for s, p in pockets]
    rs = molecule.relax_samples(samples, pk, ELEMENTS, device=cuda, max_iters=30)
    assert torch.equal(rs.report, r.report) and torch.equal(rs.molecules.pos, r.molecules.pos)
    # a ligand that is left out has no row in the table
    bad = [p.clone() for p in pos]
    bad[2][1, 0] = float('nan')
    rb = molecule.build_molecules(bad, feat, ELEMENTS).relax(ppos, [s for s, _ in pockets], pocket_of=[0, 0, 0, 1, 1, 1], max_iters=30)
    assert rb.table()['lig_idx'] == [0, 1, 3, 4, 5] and int(rb.status[2]) == 2
