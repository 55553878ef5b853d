"""Substructure search without a GPU: the SMARTS compiler (keypoint_diffusion_amd.smarts) against tables written by hand, the
restatement of include/kpd.h's rule (tests/match_ref.py) against its own brute force over every injective map, chemistry counted by
hand, and invariance under renumbering.  Nothing here is compared with RDKit."""
import random

import numpy as np
import pytest

from keypoint_diffusion_amd import smarts
from . import match_cases as MC
from . import match_ref as R
from . import sanitize_cases as SC
from .molecule_cases import TEXTBOOK as MOL_TEXTBOOK

C, N, O = 1 << 6, 1 << 7, 1 << 8
ANY16 = 0xffff


def alt(z=smarts.ALL_Z, cls=15, D=ANY16, H=ANY16, X=ANY16, v=ANY16, x=ANY16, need=(), forbid=()):
    return (z, cls, D, H, X, v, x, tuple(need), tuple(forbid))


def alts_of(row, t):
    return {(a['z'], a['cls'], a['D'], a['H'], a['X'], a['v'], a['x'], tuple(a['need']), tuple(a['forbid'])) for a in row['alts'][t]}


def rows_of(*patterns):
    p = smarts.compile(list(patterns))
    return p, R.decode(p.host.tolist())


def one_atom(pattern):
    p, rows = rows_of(pattern)
    assert p.rows == [len(rows) - 1] and rows[-1]['na'] == 1
    return alts_of(rows[-1], 0)


# ---- 1. the compiler ----------------------------------------------------------------------------------------------------------------
ALI, ARO = 1 | 12, 2 | 12           # class words: aliphatic / aromatic, in a ring or not
PRIMITIVES = [
    ('C', {alt(z=C, cls=ALI)}), ('c', {alt(z=C, cls=ARO)}), ('*', {alt()}), ('a', {alt(cls=ARO)}), ('A', {alt(cls=ALI)}),
    ('Cl', {alt(z=1 << 17, cls=ALI)}), ('Br', {alt(z=1 << 35, cls=ALI)}), ('Si', {alt(z=1 << 14, cls=ALI)}), ('As', {alt(z=1 << 33, cls=ALI)}),
    ('[#6]', {alt(z=C)}), ('[C]', {alt(z=C, cls=ALI)}), ('[n]', {alt(z=N, cls=ARO)}), ('[Cl]', {alt(z=1 << 17, cls=ALI)}),
    ('[*]', {alt()}), ('[a]', {alt(cls=ARO)}), ('[A]', {alt(cls=ALI)}), ('[H]', {alt(z=1 << 1)}), ('[#1]', {alt(z=1 << 1)}),
    ('[D2]', {alt(D=1 << 2)}), ('[D]', {alt(D=1 << 1)}), ('[H2]', {alt(H=1 << 2)}), ('[CH]', {alt(z=C, cls=ALI, H=1 << 1)}),
    ('[X4]', {alt(X=1 << 4)}), ('[v3]', {alt(v=1 << 3)}), ('[x2]', {alt(x=1 << 2)}), ('[x]', {alt(x=0xfffe)}), ('[D20]', {alt(D=1 << 15)}),
    ('[R]', {alt(cls=3 | 8)}), ('[R0]', {alt(cls=3 | 4)}), ('[+0]', {alt()}), ('[C@@]', {alt(z=C, cls=ALI)}),
    # precedence: ";" loosest, "," in between, "&" (and nothing) tightest
    ('[C,N;H1]', {alt(z=C, cls=ALI, H=2), alt(z=N, cls=ALI, H=2)}),
    ('[C,N&H1]', {alt(z=C, cls=ALI), alt(z=N, cls=ALI, H=2)}),
    # not (6 and aliphatic) = not 6, or aromatic; the product of two of them keeps "neither element" and "aromatic"
    ('[!C]', {alt(z=smarts.ALL_Z & ~C), alt(cls=ARO)}),
    ('[!C&!N]', {alt(z=smarts.ALL_Z & ~C & ~N), alt(cls=ARO)}),
    ('[!#6]', {alt(z=smarts.ALL_Z & ~C)}), ('[!R]', {alt(cls=3 | 4)}), ('[!D1]', {alt(D=ANY16 & ~2)}), ('[!a]', {alt(cls=ALI)}),
    ('[O,S;X2;!H0]', {alt(z=O, cls=ALI, X=4, H=0xfffe), alt(z=1 << 16, cls=ALI, X=4, H=0xfffe)}),
]


@pytest.mark.parametrize('pattern,expected', PRIMITIVES, ids=[p for p, _ in PRIMITIVES])
def test_primitives_and_precedence(pattern, expected):
    assert one_atom(pattern) == expected


def test_a_charge_is_never_true_and_is_noted():
    p, rows = rows_of('[N+]', '[O-]', '[N+0]')
    assert all(a['z'] == 0 for a in rows[0]['alts'][0]) and all(a['z'] == 0 for a in rows[1]['alts'][0])
    assert alts_of(rows[2], 0) == {alt(z=N, cls=ALI)}
    assert len(p.notes) == 2 and 'charge' in p.notes[0] and "'[N+]'" in p.notes[0]
    assert any('chirality' in n for n in smarts.compile(['[C@H]']).notes)


BONDS = [('CC', 0x99), ('C-C', 0x11), ('C=C', 0x22), ('C#C', 0x44), ('C:C', 0x88), ('C~C', 0xff), ('C@C', 0xf0), ('C!@C', 0x0f),
         ('C!-C', 0xee), ('C-,=C', 0x33), ('C-!@C', 0x01), ('C=&@C', 0x20), ('C-,:;@C', 0x90), ('C!:C', 0x77)]


@pytest.mark.parametrize('pattern,mask', BONDS, ids=[p for p, _ in BONDS])
def test_bond_masks(pattern, mask):
    _, rows = rows_of(pattern)
    assert rows[0]['parent'] == [-1, 0] and rows[0]['pmask'] == [0, mask] and rows[0]['closures'] == []


def test_branches_and_ring_closures():
    _, rows = rows_of('C(N)(=O)O', 'C1CC1', 'C1CC=1', 'C=1CC1', 'C%12CC%12', 'C12CC1C2', 'CC(C(N)O)S')
    assert rows[0]['parent'] == [-1, 0, 0, 0] and rows[0]['pmask'] == [0, 0x99, 0x22, 0x99]
    assert rows[1]['parent'] == [-1, 0, 1] and rows[1]['closures'] == [(0, 2, 0x99)]
    assert rows[2]['closures'] == [(0, 2, 0x22)] and rows[3]['closures'] == [(0, 2, 0x22)] and rows[4]['closures'] == [(0, 2, 0x99)]
    assert rows[5]['parent'] == [-1, 0, 1, 2] and rows[5]['closures'] == [(0, 2, 0x99), (0, 3, 0x99)]
    assert rows[6]['parent'] == [-1, 0, 1, 2, 2, 1]
    _, rows = rows_of('C(CC1)1', 'C(CC=1)1')            # a closure that ends behind a closed branch: the earlier atom comes first
    assert rows[0]['parent'] == [-1, 0, 1] and rows[0]['closures'] == [(0, 2, 0x99)] and rows[1]['closures'] == [(0, 2, 0x22)]


def test_patterns_on_a_device_are_a_view():
    p = smarts.compile(['C', '[$(CO)]'])
    q = p.to('cpu')
    assert q is not p and p.table is p.host and q.host is p.host and q.rows == p.rows == [0, 2]
    assert p.row_index('cpu').tolist() == [0, 2] and p.row_index('cpu') is q.row_index('cpu')
    assert p.user_index('cpu').tolist() == [0, -1, 1, -1]


@pytest.mark.parametrize('pattern,column', MC.UNSUPPORTED, ids=[p for p, _ in MC.UNSUPPORTED])
def test_unsupported_constructs_name_the_column(pattern, column):
    with pytest.raises(ValueError) as e:
        smarts.compile([pattern])
    assert repr(pattern) in str(e.value) and f'column {column}:' in str(e.value)


def test_lifting_puts_inner_rows_first_and_shares_them():
    p, rows = rows_of('[NX3;!$(NC=O)]', '[$(NC=O)]C', '[$([NX3][$(C=O)])]', 'O')
    # rows: 0 "NC=O", 1 the first pattern, 2 the second (it shares row 0), 3 "C=O", 4 "[NX3][$(C=O)]", 5 the third, 6 "O"
    assert p.n == 4 and p.rows == [1, 2, 5, 6] and p.n_rows == 7 and len(p.names) == 4
    assert alts_of(rows[1], 0) == {alt(z=N, cls=ALI, X=8, forbid=[0])} and alts_of(rows[2], 0) == {alt(need=[0])}
    assert rows[0]['na'] == 3 and rows[3]['na'] == 2
    assert {a[7] for a in alts_of(rows[4], 1)} == {(3,)} and alts_of(rows[5], 0) == {alt(need=[4])}
    for k, row in enumerate(rows):                      # a pattern references lower rows only
        assert all(r < k for t in range(row['na']) for a in row['alts'][t] for r in a['need'] + a['forbid'])


def test_limits():
    assert len(one_atom('[C,N,O,F,P,S,Cl,Br]')) == 8
    with pytest.raises(ValueError, match='9 alternatives'):
        smarts.compile(['[C,N,O,F,P,S,Cl,Br,I]'])
    assert rows_of('C' * 16)[1][0]['na'] == 16
    with pytest.raises(ValueError, match='column 16: more than 16 atoms'):
        smarts.compile(['C' * 17])
    eight = ['C', 'N', 'O', 'CC', 'C=O', 'c1ccccc1', '[OX2H]', 'CN']
    assert smarts.compile(eight * 64).n_rows == 512
    with pytest.raises(ValueError, match='more than 512 rows'):
        smarts.compile(eight * 64 + ['C'])
    with pytest.raises(ValueError, match=r'more than 2 "\$'):
        smarts.compile(['[$(CC);$(CN);$(CO)]'])


# ---- 2. the restatement against brute force -----------------------------------------------------------------------------------------
def test_the_search_equals_the_brute_force_on_random_queries_and_graphs():
    graphs, table = MC.random_graphs(), MC.random_table()
    rows = R.decode(table)
    ptr, mol, san = MC.batch(graphs)
    with_hit = pairs = 0
    for b in range(len(graphs)):
        g = R.graph_of(ptr, mol, san, MC.ZC, b)
        assert g is not None
        every = R.brute_force(rows, ptr, mol, san, MC.ZC, b)
        res_all, capped = R.match_ligand(rows, g, R.ALL)
        res_one, capped_one = R.match_ligand(rows, g, R.ANCHORS)
        assert not capped and not capped_one
        for p, embeds in enumerate(every):
            what = f'graph {b}, row {p}'
            assert set(res_all[p]['embeddings']) == embeds and len(res_all[p]['embeddings']) == len(embeds), what
            assert res_all[p]['n_embed'] == len(embeds), what
            assert res_all[p]['anchors'] == sorted({f[0] for f in embeds}) == res_one[p]['anchors'], what
            assert res_all[p]['cover'] == {a for f in embeds for a in f}, what
            assert (res_one[p]['first'] in embeds) if embeds else res_one[p]['first'] is None, what
            assert res_one[p]['first'] == res_all[p]['first'], what
            pairs += 1
            with_hit += bool(embeds)
    assert pairs == len(graphs) * len(rows) and 4 * with_hit >= pairs and 4 * (pairs - with_hit) >= pairs, (with_hit, pairs)


# ---- 3. chemistry by hand -----------------------------------------------------------------------------------------------------------
def run(graphs, patterns, mode=R.ANCHORS, **kw):
    p = patterns if isinstance(patterns, smarts.Patterns) else smarts.compile(patterns)
    ptr, mol, san = MC.batch(graphs)
    out = R.match_batch(ptr, mol, san, MC.ZC, p.host.tolist(), mode, **kw)
    return p, out


def everything():
    """Every named molecule: those of tests/sanitize_cases.py (molecules and ring templates) as the restated sanitiser labels them,
    those tests/smiles_cases.py writes by hand, and the small functional-group molecules of tests/match_cases.py."""
    out = MC.pipeline_named()
    out.update(MC.smiles_named())
    out.update(MC.NAMED)
    return out


def check_hits(molecules, cases):
    names = sorted({m for _, m, _ in cases})
    texts = list(dict.fromkeys(s for s, _, _ in cases))
    p, out = run([molecules[m] for m in names], texts)
    assert not out['status'].any()
    for s, m, hits in cases:
        assert out['hits'][names.index(m), p.rows[texts.index(s)]] == hits, (s, m)


def test_anchors_counted_by_hand():
    check_hits(MC.NAMED, MC.HITS)


def test_anchors_counted_by_hand_on_what_the_sanitiser_makes_of_the_named_molecules():
    pipeline = MC.pipeline_named()
    assert len(pipeline) == len(SC.TEXTBOOK) + len(SC.TEMPLATES)
    check_hits(pipeline, MC.PIPELINE_HITS)
    check_hits(pipeline, [(s, 'template ' + m, hits) for s, m, hits in MC.PIPELINE_HITS if 'template ' + m in pipeline])
    names = list(MC.PIPELINE_RINGS)
    _, out = run([pipeline[m] for m in names], ['c1ccccc1'], R.ALL)
    assert out['n_embed'][:, 0].tolist() == [MC.PIPELINE_RINGS[m] for m in names]


def test_benzene_in_benzene_and_in_rings_that_are_not_aromatic():
    pipeline = MC.pipeline_named()
    graphs = [MC.BENZENE, pipeline['benzene 1.397'], pipeline['cyclohexane'], MC.NAMED['cyclohexane'], MC.NAMED['Kekule ring, not planar']]
    p, out = run(graphs, ['c1ccccc1'], R.ALL)
    assert out['hits'][:, 0].tolist() == [6, 6, 0, 0, 0] and out['n_embed'][:, 0].tolist() == [12, 12, 0, 0, 0]
    assert out['first_map'][0, 0, :6].tolist() == [0, 1, 2, 3, 4, 5] and (out['first_map'][0, 0, 6:] == -1).all()
    assert (out['cover'][:12, 0] == 1).all() and not out['cover'][12:].any() and (out['first_map'][2:] == -1).all()


def test_explicit_hydrogens_from_add_hs_give_the_same_answers_as_the_implicit_parent():
    """The explicit-hydrogen molecule is what the restated kpd_mol_add_hs and a second kpd_mol_sanitize leave (the chain
    `Sanitized.add_hs().molecules.sanitize()` runs): every heavy atom answers every query as it does in the parent."""
    texts = ['[OX2H]', '[NX3;H2]', '[CH3]', '[CH2]', '[H]', '[#6;H1]', '[D1]', '[D2]', '[X4]', '[X3]', '[v4]', '[v3]', '[nH]', '[cH]', '[OH]', '[NH2]',
             '[H0]', '[H1]', '[H2]', '[H3]']
    ligs = [(name, sym, pos) for name, sym, pos, _ in SC.TEXTBOOK] + [(name, sym, pos) for name, sym, pos, _ in MOL_TEXTBOOK]
    assert len(ligs) >= 25
    n_hydrogens = 0
    for name, sym, pos in ligs:
        if any(s not in MC.ELEMENTS for s in sym):
            continue
        parent, explicit, source = MC.with_hydrogens(sym, pos)
        n, total = len(parent['sym']), sum(parent['atom_h'])
        assert source[:n] == list(range(n)) and len(explicit['sym']) == n + total and not any(explicit['atom_h']), name
        n_hydrogens += total
        p, out = run([parent, explicit], texts)
        for k, s in enumerate(texts):
            heavy_a = {a for a in range(n) if out['anchor'][a, 0] >> p.rows[k] & 1}
            heavy_b = {a for a in range(n) if out['anchor'][n + a, 0] >> p.rows[k] & 1}
            assert heavy_a == heavy_b, (name, s)
        assert out['hits'][0, p.rows[4]] == 0 and out['hits'][1, p.rows[4]] == total, name
    assert n_hydrogens > 100


def test_amide_nitrogen_through_a_recursive_query():
    p, out = run([MC.NAMED['acetamide'], MC.NAMED['ethylamine']], ['[$([NX3]C=O)]', '[NX3;!$([NX3]C=O)]'])
    assert p.n_rows == 3 and p.rows == [1, 2]
    assert out['first_map'][0, 1, 0] == 3 and out['hits'][:, 1].tolist() == [1, 0] and out['hits'][:, 2].tolist() == [0, 1]
    assert out['first_map'][1, 2, 0] == 4 + 2


def test_every_functional_group_hits_its_example_and_not_its_decoys():
    assert 18 <= len(smarts.FUNCTIONAL_GROUPS) <= 24 and set(MC.GROUP_EXAMPLES) == set(smarts.FUNCTIONAL_GROUPS)
    names = sorted(MC.NAMED)
    p, out = run([MC.NAMED[m] for m in names], smarts.compile(smarts.FUNCTIONAL_GROUPS))
    assert p.names == list(smarts.FUNCTIONAL_GROUPS)
    for k, group in enumerate(p.names):
        example, decoys = MC.GROUP_EXAMPLES[group]
        assert len(decoys) == 3 and out['hits'][names.index(example), p.rows[k]] > 0, (group, example)
        for d in decoys:
            assert out['hits'][names.index(d), p.rows[k]] == 0, (group, d)


def test_the_functional_groups_of_the_existing_named_molecules():
    """Exactly the groups written down for every named molecule and ring template of tests/sanitize_cases.py (as the restated
    sanitiser labels them) and every molecule of tests/smiles_cases.py: no other group hits."""
    molecules = MC.pipeline_named()
    molecules.update(MC.smiles_named())
    assert set(molecules) == set(MC.GROUPS_OF) and len(molecules) >= 45
    names = sorted(molecules)
    p, out = run([molecules[m] for m in names], smarts.compile(smarts.FUNCTIONAL_GROUPS))
    for b, m in enumerate(names):
        assert {p.names[k] for k, r in enumerate(p.rows) if out['hits'][b, r] > 0} == MC.GROUPS_OF[m], m


def test_max_nodes_cuts_a_search_and_the_bounds_are_lower_bounds():
    p, full = run([MC.BENZENE], ['c1ccccc1'], R.ALL)
    _, cut = run([MC.BENZENE], ['c1ccccc1'], R.ALL, max_nodes=7)            # an anchor's first embedding takes 5 nodes
    assert full['status'][0] == 0 and cut['status'][0] == R.MAX_NODES
    assert cut['hits'][0, 0] == 6 and 0 < cut['n_embed'][0, 0] < full['n_embed'][0, 0] == 12
    _, one = run([MC.BENZENE], ['c1ccccc1'], R.ANCHORS, max_nodes=1)
    assert one['status'][0] == R.MAX_NODES and one['hits'][0, 0] == 0


# ---- 4. invariance under renumbering ------------------------------------------------------------------------------------------------
def test_renumbering_moves_nothing_but_the_atom_numbers():
    groups = smarts.compile(smarts.FUNCTIONAL_GROUPS)
    tg = np.zeros(groups.n_rows, dtype=np.int64) - 1
    value = np.zeros(groups.n_rows)
    rng = random.Random(5)
    for k, r in enumerate(groups.rows):
        tg[r], value[r] = k % 2, rng.uniform(-1.0, 1.0)
    for name, g in everything().items():
        ptr, mol, san = MC.batch([g])
        ref = R.match_batch(ptr, mol, san, MC.ZC, groups.host.tolist(), R.ALL, type_group=tg, value=value, G=2)
        for k in range(8):
            h, p = MC.renumbered(g, rng, keep_order=k == 0)
            ptr, mol, san = MC.batch([h])
            got = R.match_batch(ptr, mol, san, MC.ZC, groups.host.tolist(), R.ALL, type_group=tg, value=value, G=2)
            what = f'{name}, renumbering {k}'
            assert (got['hits'] == ref['hits']).all() and (got['n_embed'] == ref['n_embed']).all() and (got['untyped'] == ref['untyped']).all(), what
            for a in range(len(p)):
                assert (got['anchor'][p[a]] == ref['anchor'][a]).all() and (got['cover'][p[a]] == ref['cover'][a]).all(), what
                assert (got['atom_type'][:, p[a]] == ref['atom_type'][:, a]).all(), what
            if k == 0:
                assert got['type_sum'].tobytes() == ref['type_sum'].tobytes(), what
            else:                                        # the order of the additions moved
                assert np.allclose(got['type_sum'], ref['type_sum'], rtol=1e-12, atol=1e-300), what
