"""Canonical SMILES of sanitised ligands on the GPU (kpd_mol_smiles, Sanitized.smiles) against the restatement of the rule in
include/kpd.h (tests/smiles_ref.py), byte for byte: every string, every text_ptr, every status.  The restatement is fed what the
GPU perceived and sanitised, or the hand-written labelled graph the kernel is fed, so only the string writing is under test.
Every raw call runs with canary bytes behind each output buffer and around the scratch."""
import random

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule, utils
from . import sanitize_cases as C
from . import smiles_cases as SC
from . import smiles_ref as S
from .molecule_cases import ELEMENTS, TWO_ETHANOLS_CL, Z, one_hot
from .molecule_cases import TEXTBOOK as SMALL
from .test_molecule_gpu import CANARY, Guarded, concat, perceive_gpu
from .test_sanitize_gpu import mol_of, sanitize_gpu
from .util import guarded, intact

pytestmark = pytest.mark.gpu
ELEMENTS_ALL = ELEMENTS + ['H', 'Si']               # the classes of the hand-written graphs
Z_ALL = Z + [1, 14]


def smiles_gpu(dev, ptr, mol, san, largest=False, aromatic=True, capacity=None, elements=ELEMENTS, z=Z):
    """kpd_mol_smiles through the C ABI.  mol / san: integer numpy arrays in the layout of kpd_mol_perceive / kpd_mol_sanitize.
    Returns (the bytes of every ligand, b'' where nothing was written for it; text_ptr; status; the whole text buffer)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)
    N, B, cap_bonds = len(mol['elem']), len(ptr) - 1, len(san['order_k'])
    ins = [t(np.asarray(ptr)), t(mol['elem']), t(np.asarray(z)), hip._packed_symbols(elements, dev), t(mol['frag']),
           t(np.asarray(mol['bonds']).reshape(-1)), t(san['order_k']), t(san['bond_flags']), t(mol['bond_ptr']), t(mol['status']),
           t(san['status']), t(san['atom_h']), t(san['atom_flags'])]
    before = [x.clone() for x in ins]
    cap = 36 * N + 16 if capacity is None else capacity
    g = Guarded(dev)
    text, tptr, status = g.new(cap, torch.uint8), g.new(B + 1, torch.int64), g.new(B)
    L = hip.lib()
    nb = int(L.kpd_smiles_scratch_bytes(N, B))
    scratch, p_scr = guarded(nb, torch.uint8, dev, CANARY)
    p = [x.data_ptr() for x in ins]
    hip.check(L.kpd_mol_smiles(p[0], N, B, p[1], len(z), p[2], p[3], p[4], p[5], p[6], p[7], p[8], cap_bonds, p[9], p[10], p[11], p[12],
                               int(largest), int(aromatic), text.data_ptr(), cap, tptr.data_ptr(), status.data_ptr(), p_scr,
                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    assert intact(scratch, nb, CANARY), f'kpd_mol_smiles wrote outside its {nb} bytes of scratch'
    for x, y in zip(ins, before):                   # inputs are never written
        assert torch.equal(x, y)
    at, st = tptr[:B + 1].cpu().tolist(), status[:B].cpu().tolist()
    raw = bytes(text[:cap].cpu().numpy())
    return [raw[at[b]:at[b + 1]] if not st[b] else b'' for b in range(B)], at, st, raw


def assert_same(got, ref, what=''):
    texts, at, st, _ = got
    ref_texts, ref_at, ref_st = ref
    assert st == ref_st, (what, [b for b in range(len(st)) if st[b] != ref_st[b]][:8])
    assert at == ref_at, (what, 'text_ptr')
    for b, (x, y) in enumerate(zip(texts, ref_texts)):
        assert x == (y if not ref_st[b] else b''), (what, b, x, y)


def arrays(graphs, elements=ELEMENTS_ALL, cap_bonds=None):
    """Labelled graphs -> (ptr, mol, san) as kpd_mol_perceive and kpd_mol_sanitize would have left them: frag = the connected
    components in order of first atom, order_k = the label (1 under an aromatic bond), the aromatic bits, status 0."""
    ptr, elem, frag, bonds, order_k, bflags, h_all, aflags, bond_ptr = [0], [], [], [], [], [], [], [], [0]
    for Zs, h, ar, sym, bb, labels in graphs:
        a0, n = ptr[-1], len(Zs)
        comp = list(range(n))
        for _ in range(n):
            for i, j in bb:
                comp[i] = comp[j] = min(comp[i], comp[j])
        names = {c: k for k, c in enumerate(sorted(set(comp)))}
        elem += [elements.index(s) for s in sym]
        frag += [names[c] for c in comp]
        h_all += list(h)
        aflags += [2 * a for a in ar]
        bonds += [(a0 + i, a0 + j) for i, j in bb]
        order_k += [1 if l == 4 else l for l in labels]
        bflags += [4 if l == 4 else 0 for l in labels]
        ptr.append(a0 + n)
        bond_ptr.append(len(bonds))
    cap = len(bonds) if cap_bonds is None else cap_bonds
    pad = cap - len(bonds)
    i64 = lambda x: np.asarray(x, dtype=np.int64)
    B = len(graphs)
    mol = dict(elem=i64(elem), frag=i64(frag), bonds=i64(bonds + [(0, 0)] * pad).reshape(-1, 2), bond_ptr=i64(bond_ptr), status=np.zeros(B, dtype=np.int64))
    san = dict(order_k=i64(order_k + [0] * pad), bond_flags=i64(bflags + [0] * pad), atom_h=i64(h_all), atom_flags=i64(aflags),
               status=np.zeros(B, dtype=np.int64))
    return i64(ptr), mol, san


def run_graphs(dev, graphs, **kw):
    ptr, mol, san = arrays(graphs, cap_bonds=kw.pop('cap_bonds', None))
    got = smiles_gpu(dev, ptr, mol, san, elements=ELEMENTS_ALL, z=Z_ALL, **kw)
    ref = S.smiles_batch(ptr, mol, san, Z_ALL, ELEMENTS_ALL, kw.get('largest', False), kw.get('aromatic', True), kw.get('capacity'))
    return got, ref


# ---- 7. byte equality through perceive -> sanitise -> smiles ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def perceived(cuda):
    ligs = ([(sym, p) for _, sym, p, _ in C.TEXTBOOK] + [(sym, p) for _, sym, p in C.TEMPLATES] + [(sym, p) for sym, p, _ in C.generated(48)] +
            [(sym, p) for _, sym, p, _ in SMALL] + [TWO_ETHANOLS_CL[:2]])
    pos, feat, ptr = concat(ligs)
    out, _ = perceive_gpu(cuda, pos, feat, ptr)
    return ligs, pos, ptr, mol_of(out)


@pytest.mark.parametrize('largest', [False, True])
def test_bytes_equal_the_restatement(cuda, perceived, largest):
    ligs, pos, ptr, mol = perceived
    san = sanitize_gpu(cuda, pos, ptr, mol, largest)
    for aromatic in (True, False):
        got = smiles_gpu(cuda, ptr, mol, san, largest, aromatic)
        assert_same(got, S.smiles_batch(ptr, mol, san, Z, ELEMENTS, largest, aromatic), f'largest={largest} aromatic={aromatic}')
        assert not any(got[2]) and all(got[0])
        if aromatic:
            assert got[0][0] == b'c1ccccc1' and got[0][-1] == (b'OCC' if largest else b'Cl.OCC.OCC')
        else:
            assert got[0][0] == b'C=1C=CC=CC1' and not any(ch in text for text in got[0] for ch in b'cnos')


# ---- 8. labelled graphs fed directly ------------------------------------------------------------------------------------------------
def test_hand_written_graphs_and_their_renumberings(cuda):
    """Every input of the CPU numbering test (TEXTBOOK and TEMPLATES in both modes, generated(48), the 700 random graphs, the
    graphs written by hand) and the two closure-number graphs, each with 8 seeded renumberings, through the kernel in one call.
    The kernel's bytes of every original equal the restatement's, and the bytes of every renumbered copy equal its original's
    (the restatement is run on the originals only: the 6 600 copies would add four seconds of Python to this test;
    that it gives a copy the bytes of its original is what tests/test_smiles_config.py asserts)."""
    from .test_smiles_config import RENUMBERINGS, labelled
    base = []
    for aromatic in (True, False):
        base += [labelled(sym, p, aromatic) for _, sym, p, _ in C.TEXTBOOK] + [labelled(sym, p, aromatic) for _, sym, p in C.TEMPLATES]
    base += [labelled(sym, p) for sym, p, _ in C.generated(48)] + SC.random_set() + [c[1] for c in SC.BY_HAND]
    n_hand = len(SC.BY_HAND)
    base += [SC.TEN_CLOSURES, SC.EXHAUSTED]
    rng = random.Random(8)
    graphs = list(base) + [SC.permuted(g0, rng) for g0 in base for _ in range(RENUMBERINGS)]
    ptr, mol, san = arrays(graphs)
    texts, at, st, _ = smiles_gpu(cuda, ptr, mol, san, elements=ELEMENTS_ALL, z=Z_ALL)
    first = arrays(base)
    ref_texts, ref_at, ref_st = S.smiles_batch(*first, Z_ALL, ELEMENTS_ALL)
    assert st[:len(base)] == ref_st and at[:len(base) + 1] == ref_at and texts[:len(base)] == ref_texts
    for k in range(len(base)):
        copies = slice(len(base) + k * RENUMBERINGS, len(base) + (k + 1) * RENUMBERINGS)
        assert texts[copies] == [texts[k]] * RENUMBERINGS and st[copies] == [st[k]] * RENUMBERINGS, k       # the numbering does not show
    hand = texts[len(base) - 2 - n_hand:len(base) - 2]
    assert hand == [c[3].encode() for c in SC.BY_HAND]
    assert b'%10' in texts[len(base) - 2] and st[len(base) - 2] == 0 and st[len(base) - 1] == S.CLOSURES_EXHAUSTED and texts[len(base) - 1] == b''
    assert at[-1] == sum(len(x) for x in texts)
    kek, ref = run_graphs(cuda, [c[1] for c in SC.BY_HAND], aromatic=False)
    assert_same(kek, ref, 'the Kekule mode ignores the aromatic bits')


# ---- 9. edges ----------------------------------------------------------------------------------------------------------------------
def dumbbell(n):
    """A chain of n carbons whose first and last six are closed to rings."""
    bonds = [(k, k + 1) for k in range(n - 1)] + [(0, 5), (n - 6, n - 1)]
    deg = np.bincount(np.array(bonds).flatten(), minlength=n)
    return [6] * n, [4 - int(d) for d in deg], [0] * n, ['C'] * n, bonds, [1] * len(bonds)


def test_sizes_at_the_edges(cuda):
    one = SC.graph(['N'], {})
    chain257 = ([6] * 257, [2] * 257, [0] * 257, ['C'] * 257, [(k, k + 1) for k in range(256)], [1] * 256)
    empty = ([], [], [], [], [], [])
    graphs = [one, dumbbell(256), chain257, empty, SC.BY_HAND[2][1], SC.BY_HAND[6][1]]
    ptr, mol, san = arrays(graphs)
    mol['status'][4] = 8                            # left out by perception
    got = smiles_gpu(cuda, ptr, mol, san, elements=ELEMENTS_ALL, z=Z_ALL)
    assert_same(got, S.smiles_batch(ptr, mol, san, Z_ALL, ELEMENTS_ALL), 'edges')
    texts, at, st, _ = got
    assert texts[0] == b'N' and st == [0, 0, 1, 1, 1, 0] and texts[2:5] == [b'', b'', b''] and texts[5] == b'c1ccccc1'
    assert texts[1].count(b'C') == 256 and texts[1].count(b'1') == 4 and texts[1].count(b'(') == texts[1].count(b')')    # number 1 twice
    assert set(texts[1]) <= set(b'C1()') and at[-1] == sum(len(x) for x in texts)
    # B = 1 and B = 0
    got, ref = run_graphs(cuda, [SC.BY_HAND[13][1]])
    assert_same(got, ref, 'B = 1')
    assert got[0] == [b'O=c1cccc[nH]1']
    got, ref = run_graphs(cuda, [])
    assert got[:3] == ([], [0], []) and ref[1] == [0]


def test_capacity_one_byte_short(cuda):
    graphs = [c[1] for c in SC.BY_HAND[:8]]
    full, ref = run_graphs(cuda, graphs)
    total = full[1][-1]
    got, ref = run_graphs(cuda, graphs, capacity=total - 1)
    assert_same(got, ref, 'one byte short')
    texts, at, st, raw = got
    assert at == full[1] and st == [0] * 7 + [S.CAPACITY] and texts[:7] == full[0][:7]
    assert raw[at[7]:] == bytes([CANARY]) * (total - 1 - at[7])         # nothing of the ligand that does not fit is written
    got, _ = run_graphs(cuda, graphs, capacity=0)
    assert got[2] == [S.CAPACITY] * 8 and got[1] == full[1]


# ---- 10. invariance -----------------------------------------------------------------------------------------------------------------
def test_alone_in_a_batch_with_spare_bond_rows_and_again(cuda):
    from .test_smiles_config import labelled
    target = labelled(*C.generated(3)[2][:2])
    others = SC.random_set(63)
    alone, _ = run_graphs(cuda, [target])
    want = alone[0][0]
    assert want and alone[2] == [0]
    for at in (0, 31, 63):
        graphs = others[:at] + [target] + others[at:]
        n_atoms = sum(len(g[0]) for g in graphs)
        tight, ref = run_graphs(cuda, graphs)
        assert_same(tight, ref, f'target at {at}')
        wide, _ = run_graphs(cuda, graphs, cap_bonds=3 * n_atoms)
        again, _ = run_graphs(cuda, graphs)
        assert tight[0][at] == want and wide[:3] == tight[:3] and again[:3] == tight[:3]


# ---- 11. the Python surface ---------------------------------------------------------------------------------------------------------
def build(dev, ligs):
    return molecule.build_molecules([torch.from_numpy(np.asarray(p, dtype=np.float32)).to(dev) for _, p in ligs],
                                    [torch.from_numpy(one_hot(sym)).to(dev) for sym, _ in ligs], ELEMENTS)


def test_surface(cuda, tmp_path):
    by_name = {c[0]: (c[1], c[2]) for c in C.TEXTBOOK}
    names = ['benzene 1.397', 'benzene 1.38', 'pyridine', 'phenol', 'cyclopentadienyl']
    ligs = [by_name[k] for k in names] + [TWO_ETHANOLS_CL[:2]]
    mols = build(cuda, ligs)
    san = mols.sanitize(largest_frag=True)
    assert san.smiles() == ['c1ccccc1', 'c1ccccc1', 'c1ccccn1', 'Oc1ccccc1', 'C1C=CC=C1', 'OCC']
    assert san.smiles(kekule=True)[:2] == ['C=1C=CC=CC1'] * 2 and san.valid.tolist()[4] is False        # invalid, but it has a string
    whole = mols.sanitize()
    assert whole.smiles()[5] == 'Cl.OCC.OCC' and whole.smiles(largest_frag=True) == san.smiles() and whole.unique(largest_frag=True) == san.unique()
    assert whole.metrics(by='smiles')['uniqueness'] == san.metrics(by='smiles')['uniqueness']        # largest-fragment strings either way
    with pytest.raises(hip.KpdError):
        san.smiles(largest_frag=False)
    assert san.unique() == [0, 2, 3, 4, 5] and san.unique(kekule=True) == [0, 2, 3, 4, 5]
    keyed, by_string = san.metrics(), san.metrics(by='smiles')
    assert by_string['uniqueness'] == 3 / 4 and {k: v for k, v in by_string.items() if k != 'uniqueness'} == {k: v for k, v in keyed.items() if k != 'uniqueness'}
    assert san.metrics(by='smiles', train_smiles=['c1ccccc1'])['novelty'] == 2 / 3
    pos = [torch.from_numpy(np.asarray(p, dtype=np.float32)) for _, p in ligs]
    feat = [torch.from_numpy(one_hot(sym)) for sym, _ in ligs]
    samples = [dict(positions=pos[:2], features=feat[:2]), dict(positions=pos[2:], features=feat[2:])]
    out = molecule.analyze_samples(samples, ELEMENTS, device=cuda, smiles=True)
    assert out.pop('smiles') == [['c1ccccc1', 'c1ccccc1'], ['c1ccccn1', 'Oc1ccccc1', 'C1C=CC=C1', 'OCC']]
    plain = molecule.analyze_samples(samples, ELEMENTS, device=cuda, sanitize=True)                # the defaults are unchanged
    assert sorted(out) == sorted(plain) and 'smiles' not in plain
    assert all(torch.equal(out[k], plain[k]) if isinstance(plain[k], torch.Tensor) else out[k] == plain[k] for k in plain)
    assert molecule.analyze_samples(samples, ELEMENTS, device=cuda) == mols.metrics()
    dev_pos, dev_feat = [p.to(cuda) for p in pos], [f.to(cuda) for f in feat]
    assert utils.sampled_ligands_smiles(dev_pos, dev_feat, ELEMENTS) == san.smiles()
    assert utils.sampled_ligands_smiles(dev_pos, dev_feat, ELEMENTS, largest_frag=False)[5] == 'Cl.OCC.OCC'
    utils.write_smiles_file(tmp_path / 'out.smi', dev_pos + [torch.zeros(0, 3, device=cuda)], dev_feat + [torch.zeros(0, len(ELEMENTS), device=cuda)],
                            ELEMENTS)
    assert (tmp_path / 'out.smi').read_text() == 'c1ccccc1\nc1ccccc1\nc1ccccn1\nOc1ccccc1\nC1C=CC=C1\nOCC\n\n'
    # a small capacity is met by the second call
    m = san.molecules
    mol = dict(elem=m.elem, frag=m.frag, bonds=m.bonds, bond_ptr=m.bond_ptr, status=m.status)
    text, ptr, status = hip.mol_smiles(m.lig_ptr, Z, ELEMENTS, mol, san._out, largest_only=True, capacity=5)
    assert text.decode() == ''.join(san.smiles()) and status == [0] * 6 and ptr[-1] == len(text)


def test_a_hydrogenated_batch_writes_its_hydrogens(cuda):
    nx = pytest.importorskip('networkx')
    from .test_smiles_config import reads_back
    by_name = {c[0]: (c[1], c[2]) for c in C.TEXTBOOK}
    hyd = build(cuda, [by_name['pyrrole'], SMALL[0][1:3]]).sanitize().add_hs()
    san = hyd.molecules.sanitize()
    strings = san.smiles()
    assert strings[0].count('[H]') == 5 and strings[1].count('[H]') == 6 and 'n' in strings[0] and '[nH]' not in strings[0]
    m = san.molecules
    ptr, bp = m.lig_ptr.tolist(), m.bond_ptr.tolist()
    for b, text in enumerate(strings):
        a0, a1 = ptr[b], ptr[b + 1]
        elem = m.elem[a0:a1].tolist()
        ar = san.aromatic_atoms[a0:a1].int().tolist()
        bonds = [(i - a0, j - a0) for i, j in m.bonds[bp[b]:bp[b + 1]].tolist()]
        labels = [4 if f else o for o, f in zip(m.order[bp[b]:bp[b + 1]].tolist(), san.aromatic_bonds[bp[b]:bp[b + 1]].tolist())]
        g = ([SC.NUMBERS[m.lig_elements[e]] for e in elem], san.h[a0:a1].tolist(), ar, [m.lig_elements[e] for e in elem], bonds, labels)
        assert reads_back(nx, text, g), text
