"""kpd_mol_keys, kpd_mol_sanitize and kpd_mol_add_hs take "one perceived ligand and its bond graph in the scope S" through one
front end (csrc/molgraph_core.h): on the same batch, clean and under edits of what perception left, the three must leave out the same
ligands (bit 0 of their status words), touch nothing of them, and agree on which atoms count.  The batch is written down in the
layout of kpd_mol_perceive: all-carbon chains of 5 .. 12 atoms and of 63, 64, 65, 256 (the edges of the lane passes) and 257 atoms,
the two ethanols and a chloride of molecule_cases, and a hub with six spokes.  kpd_mol_add_hs is fed what kpd_mol_sanitize wrote
for the same edited batch.  The expected vectors are written out; sanitize_ref and hydrogens_ref must give them too (molset_ref
reads the graph without validating it, so it has no say on an edit).  Every raw call runs with canaries.
kpd_mol_smiles and kpd_pose_rmsd take the same front end, bond loop included (pose_rmsd with its labels 1 .. 15 for the orders), and
get the same batch and edits in a test of their own below."""
import numpy as np
import pytest

from . import hydrogens_cases as HC
from . import hydrogens_ref as HR
from . import pose_rmsd_ref as PR
from . import sanitize_cases as SC
from . import sanitize_ref as SR
from . import smiles_ref as SMR
from . import test_pose_rmsd_gpu as TR
from . import test_smiles_gpu as TS
from .molecule_cases import ELEMENTS, TWO_ETHANOLS_CL
from .test_hydrogens_gpu import add_hs_gpu
from .test_molset_gpu import keys_gpu, to_device
from .test_sanitize_gpu import sanitize_gpu

pytestmark = pytest.mark.gpu
F = len(HC.Z_H)                                     # the three calls get the same class table: the ten elements and H
CHAINS = list(range(5, 13)) + [63, 64, 65, 256, 257]
TOO_LARGE, ETHANOLS, HUB, B = 12, 13, 14, 15


def base_batch():
    """pos [N,3], ptr [B+1] and mol (elem, frag, bonds, order, bond_ptr, status) as numpy; rows ascend in (i, j), every i < j."""
    ligs = []                                       # (positions, classes, fragment labels, local bonds)
    for n in CHAINS:
        ligs.append((HC.carbon_chain(n)[1], [0] * n, [0] * n, [(a, a + 1) for a in range(n - 1)]))
    sym, p, bonds = TWO_ETHANOLS_CL
    ligs.append((p, [ELEMENTS.index(s) for s in sym], [0, 0, 0, 1, 1, 1, 2], sorted(bonds)))
    hub = np.concatenate([np.zeros((1, 3)), 1.5 * np.eye(3), -1.5 * np.eye(3), [[3.0, 0.0, 0.0]]])
    ligs.append((hub, [0] * 8, [0] * 8, [(0, k) for k in range(1, 7)] + [(1, 7)]))      # atom 7 hangs on spoke 1
    ptr = np.concatenate([[0], np.cumsum([len(l[0]) for l in ligs])]).astype(np.int64)
    mol = dict(elem=np.concatenate([l[1] for l in ligs]).astype(np.int64), frag=np.concatenate([l[2] for l in ligs]).astype(np.int64),
               bonds=np.concatenate([np.array(l[3]).reshape(-1, 2) + a0 for l, a0 in zip(ligs, ptr)]).astype(np.int64),
               bond_ptr=np.concatenate([[0], np.cumsum([len(l[3]) for l in ligs])]).astype(np.int64), status=np.zeros(B, dtype=np.int64))
    mol['order'] = np.ones(len(mol['bonds']), dtype=np.int64)
    return np.concatenate([l[0] for l in ligs]).astype(np.float32), ptr, mol


def cases(ptr, mol):
    """(name, edits: array -> {index: value}, bit 0 of the status of every ligand)."""
    N, cap, bp = int(ptr[B]), len(mol['order']), mol['bond_ptr']

    def want(*left_out):
        return [int(b in left_out or b == TOO_LARGE) for b in range(B)]
    return [
        ('clean', {}, want()),
        ('a lig_ptr entry beyond the atoms', dict(ptr={3: N + 5}), want(2, 3)),
        ('a lig_ptr entry below 0', dict(ptr={6: -1}), want(5, 6)),
        ('bond_ptr[B] beyond cap_bonds', dict(bond_ptr={B: cap + 1}), want(HUB)),
        ('mol_status bits 1, 2, 4, 8', dict(status={0: 1, 1: 2, 2: 4, 3: 8}), want(0, 1, 3)),       # bit 4 alone leaves the ligand in
        ('a class of -1 and of F', dict(elem={ptr[4]: -1, ptr[5] + 2: F}), want(4, 5)),
        ('a fragment label of -1 and of n', dict(frag={ptr[6] + 1: -1, ptr[7]: ptr[8] - ptr[7]}), want(6, 7)),
        ('a bond that leaves its ligand', dict(bonds={bp[1]: (ptr[1], ptr[2])}), want(1)),
        ('an order of 0 and of 4', dict(order={bp[2] + 1: 0, bp[11] + 70: 4}), want(2, 11)),
        ('a bond repeated as (j, i)', dict(bonds={bp[3] + 1: mol['bonds'][bp[3]][::-1]}), want(3)),
        ('a hub with seven spokes', dict(bonds={bp[HUB] + 6: (ptr[HUB], ptr[HUB] + 7)}), want(HUB)),
    ]


def edited(ptr, mol, edits):
    arrays = dict(mol, ptr=ptr)
    for name, changes in edits.items():
        arrays[name] = np.array(arrays[name])
        for i, v in changes.items():
            arrays[name][int(i)] = v
    return arrays.pop('ptr'), arrays


def run_three(dev, pos, ptr, mol, largest):
    keys = keys_gpu(dev, to_device(dict(mol, ptr=ptr), dev), z=HC.Z_H, largest_only=largest)
    san = sanitize_gpu(dev, pos, ptr, mol, largest, z=HC.Z_H, allowed=HC.ALLOWED_H, mass=HC.MASS_H_TABLE)
    hyd, _, _ = add_hs_gpu(dev, pos, ptr, mol, san, largest)
    return keys, san, hyd


@pytest.mark.parametrize('largest', [False, True])
def test_the_three_leave_out_the_same_ligands(cuda, largest):
    pos, ptr0, mol0 = base_batch()
    for name, edits, want in cases(ptr0, mol0):
        ptr, mol = edited(ptr0, mol0, edits)
        keys, san, hyd = run_three(cuda, pos, ptr, mol, largest)
        got = [(o['status'] & 1).tolist() for o in (keys, san, hyd)]
        assert got[0] == got[1] == got[2] == want, (name, got)
        san_ref = SR.sanitize_batch(pos, ptr, mol, HC.Z_H, HC.ALLOWED_H, HC.MASS_H_TABLE, SC.MASS_H, largest)
        hyd_ref = HR.add_hs_batch(pos, ptr, mol, san_ref, HC.Z_H, HC.ALLOWED_H, HC.H_CLASS, largest)
        assert (san_ref['status'] & 1).tolist() == (hyd_ref['status'] & 1).tolist() == want, name      # the restatements say the same
        for b in np.nonzero(want)[0]:
            rows = slice(int(ptr0[b]), int(ptr0[b + 1]))            # the rows the ligand has in the clean batch
            assert keys['key'][b] == 0 and not keys['fp'][b].any() and not keys['atom_inv'][rows].any(), (name, b)
            assert (san['valence_k'][rows] == -1).all() and not san['atom_h'][rows].any() and san['valid'][b] == 0, (name, b)
            assert hyd['n_h'][b] == 0, (name, b)
            a0, a1, o0, o1 = int(ptr[b]), int(ptr[b + 1]), int(hyd['out_ptr'][b]), int(hyd['out_ptr'][b + 1])
            if 0 <= a0 <= a1 <= len(pos):                           # a well-formed segment is copied through
                assert o1 - o0 == a1 - a0 and np.array_equal(hyd['pos'][o0:o1].view(np.int32), pos[a0:a1].view(np.int32)), (name, b)
                assert np.array_equal(hyd['elem'][o0:o1], mol['elem'][a0:a1]) and np.array_equal(hyd['source'][o0:o1], np.arange(a0, a1)), (name, b)
            else:
                assert o1 == o0, (name, b)


@pytest.mark.parametrize('largest', [False, True])
def test_the_three_agree_on_the_scope_at_a_tie(cuda, largest):
    pos, ptr, mol = base_batch()
    keys, san, hyd = run_three(cuda, pos, ptr, mol, largest)
    a0, a1 = int(ptr[ETHANOLS]), int(ptr[ETHANOLS + 1])
    in_keys = np.nonzero(keys['atom_inv'][a0:a1])[0].tolist()
    assert in_keys == np.nonzero(san['valence_k'][a0:a1] >= 0)[0].tolist() == ([0, 1, 2] if largest else list(range(7)))
    o0, o1 = int(hyd['out_ptr'][ETHANOLS]), int(hyd['out_ptr'][ETHANOLS + 1])
    added = hyd['source'][o0:o1] == -1
    parents = set((hyd['parent'][o0:o1][added] - o0).tolist())
    # 3 + 2 + 1 hydrogens per ethanol, one on the chloride
    assert hyd['n_h'][ETHANOLS] == added.sum() == (6 if largest else 13) and parents == set(in_keys)
    for b in range(B):                              # and on every other ligand of the batch
        r = slice(int(ptr[b]), int(ptr[b + 1]))
        assert np.array_equal(keys['atom_inv'][r] != 0, san['valence_k'][r] >= 0), b


# ---- the two other users of the front end: kpd_mol_smiles and kpd_pose_rmsd ------------------------------------------------------------
SYMBOLS_H = ELEMENTS + ['H']                        # the names of the classes of HC.Z_H
_RESTATED = {}


def remembered(fn):
    """fn with its results kept by the text of its arguments.  An edit touches one or two ligands: the restatement of every other
    ligand of the batch (the 256-atom chain is a quarter of a second in Python) is computed once, not in each of the eleven cases."""
    def call(*args):
        key = fn.__name__ + repr(args)
        if key not in _RESTATED:
            _RESTATED[key] = fn(*args)
        return _RESTATED[key]
    return call


@pytest.mark.parametrize('largest', [False, True])
def test_smiles_and_pose_rmsd_leave_out_the_same_ligands(cuda, largest, monkeypatch):
    """kpd_mol_smiles gets the edited perception arrays with the sanitiser's outputs of the clean batch (an edit of `order` goes to
    order_k), so only its own front end can refuse a ligand; kpd_pose_rmsd gets the edited `order` as bond_label, K = 1, skip_h off
    and the clean positions as reference and pose.  Bit 0 of both status vectors is the written-out vector of the three calls above;
    a bond label of 4 is in kpd_pose_rmsd's range, so there ligand 11 stays in."""
    monkeypatch.setattr(SMR, 'smiles_ligand', remembered(SMR.smiles_ligand))
    monkeypatch.setattr(PR, 'ligand_graph', remembered(PR.ligand_graph))
    pos, ptr0, mol0 = base_batch()
    N = len(pos)
    san0 = sanitize_gpu(cuda, pos, ptr0, mol0, largest, z=HC.Z_H, allowed=HC.ALLOWED_H, mass=HC.MASS_H_TABLE)
    assert (san0['status'] & 1).tolist() == [int(b == TOO_LARGE) for b in range(B)]
    for name, edits, want in cases(ptr0, mol0):
        want_rmsd = [int(b in (2, TOO_LARGE)) for b in range(B)] if name == 'an order of 0 and of 4' else want
        edits = dict(edits, order_k=edits['order']) if 'order' in edits else edits
        ptr, mol = edited(ptr0, dict(mol0, order_k=san0['order_k']), edits)
        san = dict(san0, order_k=mol.pop('order_k'))
        # the restatements first: they must give the written-out vectors
        smi_ref = SMR.smiles_batch(ptr, mol, san, HC.Z_H, SYMBOLS_H, largest)
        rms_ref = PR.pose_rmsd_batch(ptr, mol, HC.Z_H, pos[None], pos, largest_only=largest, skip_h=False, bond_label=mol['order'])
        assert [st & 1 for st in smi_ref[2]] == want and (rms_ref['status'] & 1).tolist() == want_rmsd, name
        texts, at, st, _ = smi = TS.smiles_gpu(cuda, ptr, mol, san, largest, elements=SYMBOLS_H, z=HC.Z_H)
        rms = TR.rmsd_gpu(cuda, ptr, mol, pos[None], pos, largest=largest, skip_h=False, bond_label=mol['order'], z=HC.Z_H)
        assert [x & 1 for x in st] == want and (rms['status'] & 1).tolist() == want_rmsd, (name, st, rms['status'])
        TS.assert_same(smi, smi_ref, name)          # a ligand that stays in: its bytes, and every output of kpd_pose_rmsd
        TR.assert_same(rms, rms_ref, name)
        for b in range(B):
            rows = slice(int(ptr0[b]), int(ptr0[b + 1]))            # the rows the ligand has in the clean batch
            if want[b]:
                assert at[b + 1] == at[b] and texts[b] == b'', (name, b)
            else:
                assert texts[b] and texts[b] == smi_ref[0][b], (name, b)
            if want_rmsd[b]:
                assert rms['rmsd'][b, 0] == 0 and rms['plain'][b, 0] == 0 and rms['nodes'][b, 0] == 0, (name, b)
                assert (rms['map'][0, rows] == -1).all(), (name, b)
            else:
                assert rms['nodes'][b, 0] >= 1 and (rms['map'][0, rows] >= 0).any(), (name, b)       # -1 only outside S
        assert rms['map'].shape == (1, N)
