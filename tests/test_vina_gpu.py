"""Scores of ligands in rigid pockets on the GPU (kpd_vina_pocket_types, kpd_vina_score, keypoint_diffusion_amd.molecule) against
the float64 restatement of include/kpd.h (tests/vina_ref.py).  Every raw call runs with canary bytes behind each output buffer
and byte-compares its inputs afterwards; the bond graphs come from kpd_mol_perceive, as a caller's would.  Nothing is timed."""
import ctypes

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import vina_ref as R
from .molecule_cases import ELEMENTS, TWO_ETHANOLS_CL, Z, one_hot
from .relax_cases import grow, make_pocket
from .test_molecule_gpu import Guarded, cloud, concat, perceive_gpu
from .vina_cases import LIG_RADIUS, RADII, biphenyl, chlorobenzene, ethylbenzene, radii_of, z_of

pytestmark = pytest.mark.gpu

# Two fp64 sums of <= 1e5 terms in different orders, plus 1-ulp differences of exp, differ by at most about 1e-11 of the sum of
# the absolute terms; the kernel is allowed 1e-10 of it (EVAL_TOL of test_relax_gpu.py).
EVAL_TOL = 1e-10
ZARR = np.array(Z, dtype=np.int64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


class Inputs:
    """A batch on the device: perceived ligands, pockets, pocket_of; and the per-ligand pieces the restatement needs."""

    def __init__(self, dev, ligs, pockets, pocket_of):
        pos, feat, ptr = concat(ligs)
        self.got, self.t = perceive_gpu(dev, pos, feat, ptr)
        self.dev, self.ligs, self.pos, self.ptr, self.B = dev, ligs, pos, ptr, len(ligs)
        self.pockets = pockets                                  # [(symbols, pos float32)]
        sizes = [len(p) for _, p in pockets]
        self.pptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.px = np.concatenate([p.reshape(-1, 3) for _, p in pockets] + [np.zeros((0, 3), np.float32)]).astype(np.float32)
        self.pz = np.concatenate([z_of(s) for s, _ in pockets] + [np.zeros(0, np.int64)])
        self.prad = np.concatenate([radii_of(s) for s, _ in pockets] + [np.zeros(0, np.float32)]).astype(np.float32)
        self.pocket_of = np.asarray(pocket_of, dtype=np.int64)
        self.max_pocket = max(sizes, default=0)

    def graph(self, b):
        """(atomic numbers, local bonds, orders) of ligand b as kpd_mol_perceive left them."""
        a0, a1 = int(self.ptr[b]), int(self.ptr[b + 1])
        p0, p1 = int(self.got['bond_ptr'][b]), int(self.got['bond_ptr'][b + 1])
        return ZARR[self.got['elem'][a0:a1]], self.got['bonds'][p0:p1] - a0, self.got['order'][p0:p1]

    def ref(self, b, ptypes, lig_radius=LIG_RADIUS, params=None):
        """The restatement's result for ligand b; ptypes: the types of all pocket atoms."""
        a0, a1 = int(self.ptr[b]), int(self.ptr[b + 1])
        z, bonds, orders = self.graph(b)
        q = int(self.pocket_of[b])
        q0, q1 = (int(self.pptr[q]), int(self.pptr[q + 1])) if q >= 0 else (0, 0)
        return R.score_ligand(self.pos[a0:a1], z, bonds, orders, lig_radius[self.got['elem'][a0:a1]], self.px[q0:q1], self.pz[q0:q1],
                              self.prad[q0:q1], params=params, ptypes=ptypes[q0:q1])


def to(dev, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)


def pocket_types_gpu(inp, px=None, pptr=None):
    """kpd_vina_pocket_types through the C ABI with canaries; returns (types [M], status [P]) as numpy."""
    dev = inp.dev
    px_d, pz_d = to(dev, inp.px if px is None else px, torch.float32), to(dev, inp.pz, torch.int32)
    pptr_d = to(dev, inp.pptr if pptr is None else pptr, torch.int32)
    keep = [x.clone() for x in (px_d, pz_d, pptr_d)]
    M, P = px_d.shape[0], pptr_d.numel() - 1
    g = Guarded(dev)
    ty, st = g.new(M), g.new(P)
    hip.check(hip.lib().kpd_vina_pocket_types(px_d.data_ptr(), pz_d.data_ptr(), pptr_d.data_ptr(), M, P, ty.data_ptr(), st.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    for a, b in zip(keep, (px_d, pz_d, pptr_d)):
        assert a.reshape(-1).view(torch.uint8).equal(b.reshape(-1).view(torch.uint8)), 'an input buffer was written'
    return ty[:M].cpu().numpy().astype(np.int64), st[:P].cpu().numpy().astype(np.int64)


def score_gpu(inp, ptypes, max_atoms=256, max_pocket=None, pos=None, order=None, pocket_of=None, px=None, pptr=None, lig_radius=None,
              type_in=None, outputs=True, **params):
    """kpd_vina_score through the C ABI with canaries; returns a dict of numpy arrays: report [B,8], status [B] and, with `outputs`,
    grad [N,3], atom [N], type [N]."""
    dev, t = inp.dev, inp.t
    N, B = t['pos'].shape[0], inp.B
    pos_d = t['pos'] if pos is None else to(dev, pos, torch.float32)
    order_d = t['order'] if order is None else to(dev, order, torch.int32)
    px_d, prad_d = to(dev, inp.px if px is None else px, torch.float32), to(dev, inp.prad, torch.float32)
    pty_d, pptr_d = to(dev, ptypes, torch.int32), to(dev, inp.pptr if pptr is None else pptr, torch.int32)
    pof_d = to(dev, inp.pocket_of if pocket_of is None else pocket_of, torch.int32)
    zt, lr = torch.tensor(Z, dtype=torch.int32, device=dev), to(dev, LIG_RADIUS if lig_radius is None else lig_radius, torch.float32)
    tin_d = None if type_in is None else to(dev, type_in, torch.int32)
    ins = [pos_d, order_d, px_d, prad_d, pty_d, pptr_d, pof_d, zt, lr, t['ptr'], t['elem'], t['bonds'], t['bond_ptr'], t['status']]
    ins += [] if tin_d is None else [tin_d]
    keep = [x.clone() for x in ins]
    g = Guarded(dev)
    rep, st = g.new(8 * B, torch.float64), g.new(B)
    grad, atom, ty = (g.new(3 * N, torch.float64), g.new(N, torch.float64), g.new(N)) if outputs else (None, None, None)
    ptr = lambda x: None if x is None else x.data_ptr()
    p = hip.vina_params(**params)
    hip.check(hip.lib().kpd_vina_score(pos_d.data_ptr(), t['ptr'].data_ptr(), N, B, max_atoms, t['elem'].data_ptr(), len(Z), zt.data_ptr(),
                                       lr.data_ptr(), t['bonds'].data_ptr(), order_d.data_ptr(), t['bond_ptr'].data_ptr(), t['cap'],
                                       t['status'].data_ptr(), ptr(tin_d), px_d.data_ptr(), prad_d.data_ptr(), pty_d.data_ptr(),
                                       pptr_d.data_ptr(), px_d.shape[0], pptr_d.numel() - 1,
                                       inp.max_pocket if max_pocket is None else max_pocket, pof_d.data_ptr(), ctypes.byref(p),
                                       rep.data_ptr(), ptr(grad), ptr(atom), ptr(ty), st.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    for a, b in zip(keep, ins):
        assert a.reshape(-1).view(torch.uint8).equal(b.reshape(-1).view(torch.uint8)), 'an input buffer was written'
    out = dict(report=rep[:8 * B].cpu().numpy().reshape(B, 8), status=st[:B].cpu().numpy().astype(np.int64))
    if outputs:
        out.update(grad=grad[:3 * N].cpu().numpy().reshape(N, 3), atom=atom[:N].cpu().numpy(), type=ty[:N].cpu().numpy().astype(np.int64))
    return out


def rows(inp, b):
    return slice(int(inp.ptr[b]), int(inp.ptr[b + 1]))


def same_ligand(x, inp, b, y, inp2, k):
    """Ligand b of run x equals ligand k of run y bit for bit."""
    assert bits(x['report'][b]) == bits(y['report'][k]) and x['status'][b] == y['status'][k], (b, x['report'][b], y['report'][k])
    for key in ('grad', 'atom', 'type'):
        if key in x and key in y:
            assert bits(x[key][rows(inp, b)]) == bits(y[key][rows(inp2, k)]), (b, key)


@pytest.fixture(scope='module')
def batch(cuda):
    """About 70 ligands of 1 .. 40 atoms (a single atom, one without bonds, two fragments, rings, strained clouds), one of 256 and
    one of 257 atoms; pockets of 0, 37, 300 and 700 atoms; pocket_of cycling through -1 and all four."""
    rng = np.random.default_rng(7)
    ligs = [(one_hot(s), p) for s, p in (grow(rng, n) for n in [1, 2, 40] + [int(rng.integers(3, 40)) for _ in range(55)])]
    ligs += [(one_hot(s), p) for s, p in (biphenyl(rng), ethylbenzene(rng), chlorobenzene(rng))]                         # rings
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
    ptypes = np.concatenate([R.pocket_types(p, z_of(s))[0] for s, p in pockets])
    ref = [None if b == i257 else inp.ref(b, ptypes) for b in range(inp.B)]
    return dict(inp=inp, ptypes=ptypes, ref=ref, i256=i256, i257=i257)


@pytest.fixture(scope='module')
def full(batch):
    inp = batch['inp']
    ty, st = pocket_types_gpu(inp)
    return dict(ptypes=ty, pstatus=st, out=score_gpu(inp, ty))


def test_types_and_rotors_are_equal_in_every_integer(batch, full):
    inp, out = batch['inp'], full['out']
    assert np.array_equal(full['ptypes'], batch['ptypes']) and not full['pstatus'].any()
    assert len(set(batch['ptypes'].tolist())) >= 4                 # the pockets are dense enough to show several types
    n_ring = 0
    for b, e in enumerate(batch['ref']):
        if e is None:
            assert out['status'][b] == 1 and not out['report'][b].any() and (out['type'][rows(inp, b)] == -1).all()
            assert not out['grad'][rows(inp, b)].any() and not out['atom'][rows(inp, b)].any()
            continue
        assert np.array_equal(out['type'][rows(inp, b)], e['types']), b
        assert out['report'][b, 7] == e['n_rot'], (b, out['report'][b, 7], e['n_rot'])
        assert out['status'][b] == (4 if ((e['types'] < 0).any() or (e['ptypes'] < 0).any()) else 0), (b, out['status'][b])
    assert out['report'][batch['i256'], 7] > 50 and sum(e['n_rot'] for e in batch['ref'] if e) > 200


def test_terms_and_gradient(batch, full):
    inp, out = batch['inp'], full['out']
    worst = [0.0, 0.0, 0.0]
    for b, e in enumerate(batch['ref']):
        if e is None:
            continue
        tol, tol_g, tol_a = R.tolerances(e, EVAL_TOL)
        rep = out['report'][b]
        dev = np.abs(np.concatenate([[rep[0] - e['score'], rep[1] - e['inter']], rep[2:7] - e['terms']]))
        dg, da = np.abs(out['grad'][rows(inp, b)] - e['grad']), np.abs(out['atom'][rows(inp, b)] - e['atom_score'])
        if e['abs_terms'] > 0:
            worst = [max(worst[0], dev.max() / e['abs_terms']), max(worst[1], (dg / e['abs_grad'].clip(1e-300)).max()),
                     max(worst[2], (da / e['abs_atom'].clip(1e-300)).max())]
        assert (dev <= tol).all(), (b, dev, tol)
        assert (dg <= tol_g).all() and (da <= tol_a).all(), (b, dg.max(), da.max())
        if inp.pocket_of[b] < 0 or inp.pockets[int(inp.pocket_of[b])][1].shape[0] == 0:
            assert not rep[:7].any() and not out['grad'][rows(inp, b)].any()      # no pocket: all terms 0, N_rot still reported
    print(f'worst deviation / sum|terms|: report {worst[0]:.2e}, grad {worst[1]:.2e}, atom_score {worst[2]:.2e} (allowed {EVAL_TOL:.0e})')
    in_pocket = [b for b, e in enumerate(batch['ref']) if e and inp.pocket_of[b] > 0]                # pocket 0 is empty
    assert len(in_pocket) >= 40 and all(out['report'][b, 0] != 0 for b in in_pocket)
    assert np.abs([e['terms'] for e in batch['ref'] if e]).sum(axis=0).min() > 0                     # all five terms at work


def test_bitwise_identity(batch, full):
    inp, out, ty = batch['inp'], full['out'], full['ptypes']
    again = score_gpu(inp, ty)                                                               # the repeat
    for k in out:
        assert bits(out[k]) == bits(again[k]), k
    lean = score_gpu(inp, ty, outputs=False)                                                 # grad / atom_score / lig_type NULL
    assert bits(lean['report']) == bits(out['report']) and np.array_equal(lean['status'], out['status'])
    for mp in (0, 300, 700):                                                                 # staging is no part of the result
        o = score_gpu(inp, ty, max_pocket=mp)
        for k in out:
            assert bits(out[k]) == bits(o[k]), (mp, k)
    small = [b for b in range(inp.B) if b not in (batch['i256'], batch['i257'])]
    sub = Inputs(inp.dev, [inp.ligs[b] for b in small], inp.pockets, [inp.pocket_of[b] for b in small])
    for nm in (40, 256):                                                                     # LDS sized for 40 atoms or for 256
        o = score_gpu(sub, ty, max_atoms=nm)
        for k, b in enumerate(small):
            same_ligand(out, inp, b, o, sub, k)
    order = [b for b in range(inp.B)][::-1]                                                  # the reversed batch
    rev = Inputs(inp.dev, [inp.ligs[b] for b in order], inp.pockets, [inp.pocket_of[b] for b in order])
    o = score_gpu(rev, ty)
    for k, b in enumerate(order):
        same_ligand(out, inp, b, o, rev, k)
    for b in (2, 7, 33, 58, batch['i256']):                                                  # a ligand alone
        one = Inputs(inp.dev, [inp.ligs[b]], inp.pockets, [inp.pocket_of[b]])
        same_ligand(out, inp, b, score_gpu(one, ty, max_atoms=len(inp.ligs[b][1])), one, 0)
    o = score_gpu(sub, ty, max_atoms=16)                                                     # more atoms than max_atoms: left out
    for k, b in enumerate(small):
        if len(inp.ligs[b][1]) > 16:
            assert o['status'][k] == 1 and not o['report'][k].any()
        else:
            same_ligand(out, inp, b, o, sub, k)


def test_bad_inputs(cuda):
    rng = np.random.default_rng(3)
    ligs = [(one_hot(s), p) for s, p in (grow(rng, n) for n in (9, 12, 7, 15, 11, 6))]
    anchor = np.concatenate([p for _, p in ligs])
    inp = Inputs(cuda, ligs, [make_pocket(rng, 20, anchor, reach=4.0), make_pocket(rng, 90, anchor, reach=4.0)], [0, 1, 0, 1, 1, -1])
    ty, pst = pocket_types_gpu(inp)
    good = score_gpu(inp, ty, max_atoms=16)
    assert not (good['status'] & 3).any() and not pst.any() and good['report'][:5, 0].all()

    def others_keep_their_bits(o, changed):
        for b in range(inp.B):
            if b not in changed:
                same_ligand(good, inp, b, o, inp, b)
            elif o['status'][b] & 3:
                assert not o['report'][b].any() and not o['grad'][rows(inp, b)].any() and not o['atom'][rows(inp, b)].any()
                assert (o['type'][rows(inp, b)] == -1).all()

    pos = inp.pos.copy()
    pos[int(inp.ptr[1]) + 3, 1] = np.nan                         # ligand 1: a NaN coordinate
    o = score_gpu(inp, ty, max_atoms=16, pos=pos)
    assert o['status'][1] == 2
    others_keep_their_bits(o, [1])
    px = inp.px.copy()
    px[int(inp.pptr[1]) + 50, 2] = np.nan                        # a NaN pocket atom: every ligand of pocket 1, and the pocket's status
    ty_bad, pst_bad = pocket_types_gpu(inp, px=px)
    want, want_st = R.pocket_types(px[int(inp.pptr[1]):], inp.pz[int(inp.pptr[1]):])
    assert pst_bad.tolist() == [0, 2] and want_st == 2 and ty_bad[int(inp.pptr[1]) + 50] == -1
    assert np.array_equal(ty_bad[int(inp.pptr[1]):], want) and np.array_equal(ty_bad[:int(inp.pptr[1])], ty[:int(inp.pptr[1])])
    o = score_gpu(inp, ty_bad, max_atoms=16, max_pocket=10, px=px)
    assert (o['status'] & 3).tolist() == [0, 2, 0, 2, 2, 0]
    others_keep_their_bits(o, [1, 3, 4])
    o = score_gpu(inp, ty, max_atoms=16, pocket_of=[0, 1, 2, 1, 1, -2])      # pocket_of = P, and below -1
    assert (o['status'] & 3).tolist() == [0, 0, 2, 0, 0, 2]
    others_keep_their_bits(o, [2, 5])
    pptr = np.array([0, int(inp.pptr[2]), int(inp.pptr[1])])    # a descending pocket_ptr: pocket 1 is malformed
    o = score_gpu(inp, ty, max_atoms=16, pptr=pptr, pocket_of=[-1, 1, -1, 1, 1, -1])
    assert (o['status'] & 3).tolist() == [0, 2, 0, 2, 2, 0]
    ty_m, pst_m = pocket_types_gpu(inp, pptr=pptr)
    assert pst_m.tolist() == [0, 1]
    order = inp.got['order'].astype(np.int32).copy()
    order[int(inp.got['bond_ptr'][3]) + 2] = 4                   # ligand 3: a bond order of 4
    o = score_gpu(inp, ty, max_atoms=16, order=order)
    assert o['status'][3] == 1
    others_keep_their_bits(o, [3])
    # a class with radius 0: its atoms take no part (bit 2); the restatement with those atoms deleted gives the same sums
    cls = int(inp.got['elem'][rows(inp, 1)][4])
    rad = LIG_RADIUS.copy()
    rad[cls] = 0.0
    o = score_gpu(inp, ty, max_atoms=16, lig_radius=rad)
    for b in range(inp.B - 1):
        e_full = inp.ref(b, ty, lig_radius=rad)
        gone = inp.got['elem'][rows(inp, b)] == cls
        assert np.array_equal(o['type'][rows(inp, b)], e_full['types']) and ((o['type'][rows(inp, b)] == -1) == gone).all()
        assert bool(o['status'][b] & 4) == bool(gone.any()) and not o['status'][b] & 3
        z, bonds, orders = inp.graph(b)
        q0, q1 = int(inp.pptr[inp.pocket_of[b]]), int(inp.pptr[inp.pocket_of[b] + 1])
        e = R.evaluate(inp.pos[rows(inp, b)][~gone], e_full['types'][~gone], rad[inp.got['elem'][rows(inp, b)]][~gone], inp.px[q0:q1],
                       ty[q0:q1], inp.prad[q0:q1], R.rotors(z, bonds, orders))
        tol, tol_g, _ = R.tolerances(e, EVAL_TOL)
        assert abs(o['report'][b, 0] - e['score']) <= tol and (np.abs(o['report'][b, 2:7] - e['terms']) <= tol).all()
        assert (np.abs(o['grad'][rows(inp, b)][~gone] - e['grad']) <= tol_g).all() and not o['grad'][rows(inp, b)][gone].any()
        assert not o['atom'][rows(inp, b)][gone].any()
    assert o['status'][1] & 4
    # overrides: lig_type_in >= 0 replaces the perceived flags, -1 keeps them
    tin = np.full(inp.pos.shape[0], -1)
    tin[rows(inp, 0)] = 7
    o = score_gpu(inp, ty, max_atoms=16, type_in=tin)
    assert (o['type'][rows(inp, 0)] == 7).all()
    others_keep_their_bits(o, [0])
    e = R.evaluate(inp.pos[rows(inp, 0)], np.full(9, 7), LIG_RADIUS[inp.got['elem'][rows(inp, 0)]], inp.px[:int(inp.pptr[1])],
                   ty[:int(inp.pptr[1])], inp.prad[:int(inp.pptr[1])], R.rotors(*inp.graph(0)))
    assert (np.abs(o['report'][0, 2:7] - e['terms']) <= R.tolerances(e, EVAL_TOL)[0]).all()
    # parameters reach the kernel
    o = score_gpu(inp, ty, max_atoms=16, r_c=6.0, w_rot=0.0, w_hbond=-1.0)
    e = inp.ref(2, ty, params=dict(r_c=6.0, w_rot=0.0, w_hbond=-1.0))
    assert abs(o['report'][2, 0] - e['score']) <= R.tolerances(e, EVAL_TOL)[0] and o['report'][2, 0] == o['report'][2, 1]


def test_end_to_end(batch, full, cuda):
    inp, out = batch['inp'], full['out']
    pos = [torch.from_numpy(np.ascontiguousarray(p)).to(cuda) for _, p in inp.ligs]
    feat = [torch.from_numpy(np.ascontiguousarray(f)).to(cuda) for f, _ in inp.ligs]
    ppos = [torch.from_numpy(p).to(cuda) for _, p in inp.pockets]
    psym = [list(s) for s, _ in inp.pockets]
    mols = molecule.build_molecules(pos, feat, ELEMENTS)
    with pytest.raises(hip.KpdError):
        mols.vina_score(ppos, psym, pocket_of=inp.pocket_of)          # ELEMENTS has boron, XS_RADII has not
    v = mols.vina_score(ppos, psym, pocket_of=inp.pocket_of, radii=RADII, grad=True)
    assert bits(v.report.cpu().numpy()) == bits(out['report']) and np.array_equal(v.status.cpu().numpy(), out['status'])
    assert np.array_equal(v.lig_types.cpu().numpy(), out['type']) and np.array_equal(v.pocket_types.cpu().numpy(), full['ptypes'])
    assert bits(torch.cat(v.grad).cpu().numpy()) == bits(out['grad']) and bits(torch.cat(v.atom_score).cpu().numpy()) == bits(out['atom'])
    assert [tuple(g.shape) for g in v.grad] == [(len(p), 3) for _, p in inp.ligs]
    score = v.score.cpu().numpy()
    assert np.isnan(score[batch['i257']]) and np.isnan(score).sum() == 1
    t = v.table()
    assert list(t) == ['lig_idx', 'score', 'inter', 'gauss1', 'gauss2', 'repulsion', 'hydrophobic', 'hbond', 'n_rot', 'efficiency']
    assert t['lig_idx'] == [b for b in range(inp.B) if b != batch['i257']]
    assert t['score'] == out['report'][t['lig_idx'], 0].tolist() and t['n_rot'] == [int(e['n_rot']) for e in batch['ref'] if e]
    b = t['lig_idx'][5]
    assert t['efficiency'][5] == out['report'][b, 0] / (out['type'][rows(inp, b)] >= 0).sum()
    lean = mols.vina_score(ppos, psym, pocket_of=inp.pocket_of, radii=RADII)
    assert lean.grad is None and lean.atom_score is None and torch.equal(lean.report, v.report)
    # the caller's pocket types replace the perceived ones: without flags, no hydrophobic and no hbond term
    mine = [[0] * len(s) for s in psym]
    w = mols.vina_score(ppos, psym, pocket_of=inp.pocket_of, radii=RADII, pocket_types=mine)
    assert not bool(w.pocket_types.any()) and not bool(w.report[:, 5:7].any()) and torch.equal(w.report[:, 2:5], v.report[:, 2:5])
    again = mols.vina_score(ppos, psym, pocket_of=inp.pocket_of, radii=RADII, pocket_types=v.pocket_types)
    assert torch.equal(again.report, v.report)


def test_score_samples(cuda):
    rng = np.random.default_rng(5)
    ligs = [grow(rng, n) for n in (8, 11, 5, 9, 14, 7)]
    anchor = np.concatenate([p for _, p in ligs])
    pockets = [make_pocket(rng, 25, anchor, reach=4.0), make_pocket(rng, 60, anchor, reach=4.0)]
    samples = [dict(positions=[torch.from_numpy(p) for _, p in ligs[3 * q:3 * q + 3]],
                    features=[torch.from_numpy(one_hot(s)) for s, _ in ligs[3 * q:3 * q + 3]]) for q in range(2)]
    pk = [dict(positions=torch.from_numpy(p), elements=s) for s, p in pockets]
    raw = molecule.score_samples(samples, pk, ELEMENTS, device=cuda, radii=RADII)
    raw2, after, relaxed = molecule.score_samples(samples, pk, ELEMENTS, device=cuda, relax=True, max_iters=20, radii=RADII)
    assert torch.equal(raw.report, raw2.report) and raw.report.shape == (6, 8) and not bool((raw.status & 3).any())
    assert bool((relaxed.report[:, 4] > 0).all()) and not torch.equal(after.report[:, 0], raw.report[:, 0])
    ppos = [torch.from_numpy(p).to(cuda) for _, p in pockets]
    direct = relaxed.molecules.vina_score(ppos, [s for s, _ in pockets], pocket_of=[0, 0, 0, 1, 1, 1], radii=RADII)
    assert torch.equal(direct.report, after.report) and torch.equal(direct.lig_types, after.lig_types)
    assert torch.equal(after.pocket_types, raw.pocket_types) and torch.equal(after.report[:, 7], raw.report[:, 7])
