#!/usr/bin/env python
"""Generate the pocket-extraction fixtures tests/golden/pocket_XX.npz from the reference's own functions.

Run in the build container only (needs /root/reference, which never travels to the GPU box):
    python tests/golden/make_pocket_golden.py
`data_processing.pdbbind_processing.get_pocket_atoms` and `get_interface_points` are plain torch + scipy.  The
packages the module imports but these two functions never call (prody, rdkit, dgl, torch_cluster) are replaced by
EMPTY placeholder modules, as in make_golden.py, and the prody selection by a three-method stand-in (getCoords,
getElements, getResindices).  Nothing of the reference is copied: the fixtures hold synthetic inputs and the
reference's outputs.

Per complex (one file each, so that every file stays well under 1 MB):
  inputs    rec_pos fp32 [n,3], rec_el uint8 [n] (index into `elements`, len(elements) = "other"), rec_res int32 [n],
            lig_pos fp32 [m,3], params = (box_padding, pocket_cutoff, dist_thr, excl_thr)
  reference byres_mask (over the non-"other" atoms), pocket_pos, pocket_feat        <- get_pocket_atoms
            ip_box    interface points of get_pocket_atoms (float64 dist_mat, box candidate set)
            ip_pocket get_interface_points(lig, pocket_pos) (fp32 torch.cdist, pocket candidate set)
  margins   float64 distance of the closest decision to its threshold: (dist_thr, pocket_cutoff, excl box set,
            excl pocket set); a draw is REJECTED and redrawn unless all four are >= 1e-4 and a float64 replay of the
            selection equals the reference's output bitwise.  n_rejected = draws rejected before this one was kept.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
ELEMENTS = ['C', 'N', 'O', 'S', 'H']            # receptor element list of the fixtures; anything else is "other"
MARGIN = 1e-4
N_CASES = 8
# (box_padding, pocket_cutoff, dist_thr, excl_thr).  The kernels take one parameter set per batch, so the cases come in two
# groups that can each run as one batch: the shipped values (the box contains every cutoff sphere), and a box that clips both
# the cutoff spheres and the interface-distance spheres (box and pocket candidate sets differ).
PARAMS = [(8, 8, 5, 2), (4, 6, 5, 2)] * 4
N_RES = [300, 420, 560, 700, 840, 980, 1100, 1130]     # ~12 atoms per residue: 3.6 k .. 13.6 k atoms


def _placeholders():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod('prody', AtomGroup=object, Selection=object)
    rdkit = mod('rdkit')
    rdkit.Chem = mod('rdkit.Chem', SDMolSupplier=None, AllChem=mod('rdkit.Chem.AllChem'))
    rdkit.Chem.rdchem = mod('rdkit.Chem.rdchem', Mol=object)
    mod('dgl', DGLHeteroGraph=object, DGLGraph=object)
    mod('torch_cluster', radius=None, radius_graph=None)


class Selection:
    """The three prody.Selection methods get_pocket_atoms calls."""

    def __init__(self, pos, el, res):
        self._pos, self._el, self._res = pos, el, res

    def getCoords(self):
        return self._pos.astype(np.float64)

    def getElements(self):
        names = ELEMENTS + ['SE']
        return np.array([names[i] for i in self._el])

    def getResindices(self):
        return self._res.astype(np.int64)


def draw(seed, n_res):
    """A synthetic whole receptor (globule of residues with hydrogens and a few "other" atoms, a cavity around the
    ligand) and a ligand (a 1.5 A random walk), offset by 40 A so that the coordinates are not centred."""
    rng = np.random.default_rng(seed)
    per = rng.integers(6, 19, n_res)
    R = (3 * per.sum() / 0.095 / (4 * np.pi)) ** (1 / 3)
    c = rng.normal(size=(n_res, 3))
    c = c / np.linalg.norm(c, axis=1, keepdims=True) * R * rng.random((n_res, 1)) ** (1 / 3)
    m = int(rng.integers(8, 37))
    start = rng.normal(size=3)
    start = start / np.linalg.norm(start) * R * 0.4
    steps = rng.normal(size=(m, 3))
    steps = 1.5 * steps / np.linalg.norm(steps, axis=1, keepdims=True)
    lig = start + np.cumsum(steps, axis=0)
    pos = np.repeat(c, per, axis=0) + rng.normal(size=(per.sum(), 3)) * 1.7
    res = np.repeat(np.arange(n_res), per)
    d = np.linalg.norm(pos[:, None] - lig[None], axis=2).min(1)
    clash = np.unique(res[d < 2.2])
    keep = ~np.isin(res, clash)
    pos, res = pos[keep], res[keep]
    res = np.unique(res, return_inverse=True)[1]            # contiguous again, as prody's getResindices
    el = rng.choice(len(ELEMENTS) + 1, size=pos.shape[0], p=[0.32, 0.08, 0.1, 0.01, 0.47, 0.02])
    off = np.array([40.0, -40.0, 40.0])
    return (pos + off).astype(np.float32), el.astype(np.uint8), res.astype(np.int32), (lig + off).astype(np.float32)


def greedy64(points32, excl):
    """float64 replay of the greedy rule (pdbbind_processing.py:312-321) + the smallest |d - excl| it met."""
    p = points32.astype(np.float64)
    sel, margin = [0], np.inf
    for i in range(1, p.shape[0]):
        d = np.sqrt(((p[sel] - p[i]) ** 2).sum(1)).min()
        margin = min(margin, abs(d - excl))
        if d >= excl:
            sel.append(i)
    return np.asarray(sel), margin


def candidates64(lig, rec, thr):
    """(ligand, receptor) pairs closer than thr in torch.where order, midpoints in fp32, and the distance margin."""
    d = np.sqrt(((lig.astype(np.float64)[:, None] - rec.astype(np.float64)[None]) ** 2).sum(2))
    li, ri = np.nonzero(d < thr)
    mid = (lig[li] + rec[ri]) / np.float32(2)
    return mid.astype(np.float32), (np.abs(d - thr).min() if d.size else np.inf)


def one_case(seed, n_res, params, ref):
    pad, cut, thr, excl = params
    pos, el, res, lig = draw(seed, n_res)
    element_map = {e: i for i, e in enumerate(ELEMENTS)}
    element_map['other'] = len(ELEMENTS)
    ligt = torch.from_numpy(lig.copy())
    try:
        ppos, pfeat, mask, ip_box = ref.get_pocket_atoms(Selection(pos, el, res), ligt.clone(), pad, cut, element_map, thr, excl)
        ip_pocket = ref.get_interface_points(ligt.clone(), ppos, distance_threshold=thr, exclusion_threshold=excl)
    except ref.InterfacePointException:
        return None, 'no interface point'
    # ---- float64 replay + margins -------------------------------------------------------
    other = el == len(ELEMENTS)
    p, r = pos[~other], res[~other]
    lo, hi = lig.min(0) - np.float32(pad), lig.max(0) + np.float32(pad)
    box = (p >= lo).all(1) & (p <= hi).all(1)
    d = np.sqrt(((p[box].astype(np.float64)[:, None] - lig.astype(np.float64)[None]) ** 2).sum(2))
    dmin = d.min(1)
    m_cut = np.abs(dmin - cut).min()
    my_mask = np.isin(r, r[box][dmin < cut])
    _, m_thr = candidates64(lig, pos, thr)
    cand_box, _ = candidates64(lig, p[box], thr)
    cand_pocket, _ = candidates64(lig, p[my_mask], thr)
    if not cand_box.shape[0] or not cand_pocket.shape[0]:
        return None, 'no candidate'
    sel_b, m_eb = greedy64(cand_box, excl)
    sel_p, m_ep = greedy64(cand_pocket, excl)
    margins = np.array([m_thr, m_cut, m_eb, m_ep])
    if margins.min() < MARGIN:
        return None, f'margin {margins.min():.2e}'
    same = (np.array_equal(my_mask, mask.numpy()) and np.array_equal(p[my_mask], ppos.numpy())
            and np.array_equal(cand_box[sel_b], ip_box.numpy()) and np.array_equal(cand_pocket[sel_p], ip_pocket.numpy()))
    if not same:
        return None, 'float64 replay differs from the reference'
    feat = pfeat.numpy()
    assert np.array_equal(feat, np.eye(len(ELEMENTS) + 1)[el[~other]][my_mask][:, :-1])
    out = dict(rec_pos=pos, rec_el=el, rec_res=res, lig_pos=lig, params=np.asarray(params, np.float64),
               elements=np.asarray(ELEMENTS), byres_mask=mask.numpy(), pocket_pos=ppos.numpy(), pocket_feat=feat.astype(bool),
               ip_box=ip_box.numpy(), ip_pocket=ip_pocket.numpy(), margins=margins, seed=seed,
               counts=np.asarray([box.sum(), my_mask.sum(), cand_box.shape[0], cand_pocket.shape[0]]))
    return out, 'ok'


def main():
    _placeholders()
    sys.path.insert(0, REF)
    from data_processing import pdbbind_processing as ref
    seed, total_rej = 1000, 0
    for k in range(N_CASES):
        rejected = 0
        while True:
            out, why = one_case(seed, N_RES[k], PARAMS[k], ref)
            seed += 1
            if out is not None:
                break
            rejected += 1
            print(f'case {k}: seed {seed - 1} rejected ({why})')
            assert rejected <= 8, 'more than half of the draws rejected: something else is wrong'
        total_rej += rejected
        out['n_rejected'] = rejected
        path = os.path.join(HERE, f'pocket_{k:02d}.npz')
        np.savez_compressed(path, **out)
        print(f'pocket_{k:02d}.npz: {out["rec_pos"].shape[0]} atoms, {out["lig_pos"].shape[0]} ligand atoms, box/pocket/cand_box/cand_pocket '
              f'{out["counts"].tolist()}, points {out["ip_box"].shape[0]}/{out["ip_pocket"].shape[0]}, margins '
              f'{np.array2string(out["margins"], precision=1, formatter={"float_kind": lambda v: "%.1e" % v})}, {os.path.getsize(path) / 1024:.0f} KiB, {rejected} rejected')
    print(f'{total_rej} draws rejected in all')


if __name__ == '__main__':
    main()
