"""Structure files without a GPU: the Python restatement of kpd_pdb_parse on the hand-written records, the number rule, the residue
rule, the generators of the tile-edge cases, and the API's refusal of host tensors."""
import os
import random
import re

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, structure

from . import structure_cases as SC
from . import structure_ref as R


def parse(data, ptr=None):
    return R.parse_pdb(data, [0, len(data)] if ptr is None else ptr, SC.REC_EL, SC.RESNAMES)


def test_the_formatter_writes_the_columns_of_the_format():
    for line, args in zip(SC.LITERAL, SC.LITERAL_ARGS):
        assert SC.rec(*args) == line
    line = SC.LITERAL[1]
    assert (line[12:16], line[16], line[17:20], line[21], line[22:26], line[26]) == ('CA  ', ' ', ' CA', 'A', ' 301', 'A')
    assert (line[30:38], line[38:46], line[46:54], line[54:60], line[60:66], line[76:78]) == ('  -0.001', ' 123.456', '-100.250', '  0.50', '  7.25', 'CA')


def test_hand_records():
    out = parse(SC.hand_main())
    want = [w for _, w in SC.HAND_MAIN if w is not None]
    assert out['atom_ptr'] == [0, len(want)] and out['n_lines'] == len(SC.HAND_MAIN)
    assert out['status'] == [R.BAD_RECORD]
    for i, w in enumerate(want):
        if 'sym' in w:
            assert out['sym'][i] == R.pack(w['sym'].encode()), (i, w)
            assert out['elem'][i] == w.get('elem', SC.REC_EL.index(w['sym']) if w['sym'] in SC.REC_EL else len(SC.REC_EL)), (i, w)
        if 'pos' in w:
            assert out['pos'][i].tobytes() == np.array(w['pos'], dtype=np.float32).tobytes(), (i, w)       # the sign of -0.0 too
        if w.get('nan'):
            assert np.isnan(out['pos'][i]).all(), (i, w)
        if 'occ' in w:
            assert out['occ_b'][i, 0] == np.float32(w['occ'])
        if w.get('occ_nan'):
            assert np.isnan(out['occ_b'][i]).all()
        for k in ('res_idx', 'flags', 'resseq', 'tags'):
            if k in w:
                assert out[k][i] == w[k], (i, k, w, out[k][i])
    assert out['n_res'] == [out['res_idx'][-1] + 1]
    lines = SC.hand_main().split(b'\n')
    offs = np.cumsum([0] + [len(l) + 1 for l in lines])
    kept = [k for k, (_, w) in enumerate(SC.HAND_MAIN) if w is not None]
    assert out['line_off'].tolist() == [offs[k] for k in kept]
    assert out['name'][1] == R.pack(b' CA ') and out['resname'][1] == R.pack(b'ALA') and out['res_class'][1] == 0
    ca = [i for i, (_, w) in enumerate((x for x in SC.HAND_MAIN if x[1] is not None)) if 'Ca' == w.get('sym')]
    assert len(ca) == 1 and not out['flags'][ca[0]] & R.CALPHA and out['res_class'][ca[0]] == 20      # calcium 'CA  ' is no C-alpha


def test_models_line_ends_and_residue_runs():
    m = parse(SC.two_models())
    assert m['atom_ptr'] == [0, 2] and m['status'] == [R.MODELS] and m['pos'][:, 0].tolist() == [1.0, 2.0]
    c = parse(SC.crlf_no_final_newline())
    assert c['atom_ptr'] == [0, 2] and c['status'] == [0] and c['n_lines'] == 3
    assert c['pos'].tolist() == [[1.25, 2.5, 3.75], [4.0, 5.0, 6.0]] and c['sym'].tolist() == [ord('N'), ord('C')]
    assert not np.isnan(c['occ_b']).any()               # the '\r' is not part of column 79
    s = parse(SC.split_residue())
    assert s['res_idx'].tolist() == [0, 0, 1, 2] and s['n_res'] == [3]
    e = parse(b'')
    assert e['atom_ptr'] == [0, 0] and e['status'] == [R.EMPTY] and e['n_lines'] == 0
    # a file boundary ends a line: the second file's first record is whole although no '\n' precedes it
    a, b = SC.crlf_no_final_newline(), SC.split_residue()
    both = R.parse_pdb(a + b, [0, len(a), len(a) + len(b)], SC.REC_EL, SC.RESNAMES)
    assert both['atom_ptr'] == [0, 2, 6] and both['res_idx'].tolist() == [0, 0, 0, 0, 1, 2] and both['n_lines'] == 3 + 4
    assert R.parse_pdb(a, [0, len(a) + 1], SC.REC_EL)['status'] == [R.BAD_SEGMENT]


def test_number_rule_one_division_gives_pythons_float():
    """mantissa / 10^k in one fp64 division is float(text) for every field the formats can hold (both operands are exact in
    fp64 up to 15 digits, and IEEE division rounds the exact quotient once)."""
    g = random.Random(20240)
    n = 0
    for fmt, scale in (('%8.3f', 9999.0), ('%10.4f', 99999.0), ('%6.2f', 999.0)):
        for _ in range(30000):
            t = fmt % g.uniform(-scale / 10, scale)
            digits = t.strip().lstrip('+-').replace('.', '')
            k = len(t.strip().split('.')[1])
            v = int(digits) / 10 ** k
            assert (-v if '-' in t else v) == float(t), t
            assert R.real(t.encode()) == np.float32(float(t))
            n += 1
    for _ in range(20000):                                  # 15-digit fields, the point anywhere
        d = ''.join(g.choice('0123456789') for _ in range(15))
        k = g.randrange(16)
        t = (d[:15 - k] + '.' + d[15 - k:]) if k else d
        assert int(d) / 10 ** k == float(t), t
        assert R.real(t.encode()) == np.float32(float(t))
        n += 1
    assert n >= 100000


@pytest.mark.parametrize('field, value', [(b'  1.', 1.0), (b'.5  ', 0.5), (b' -0.000 ', -0.0), (b'+12.5', 12.5), (b'007', 7.0),
                                          (b'', None), (b'    ', None), (b'.', None), (b'-', None), (b'1.2.3', None), (b'1 2', None),
                                          (b'- 1', None), (b'1e3', None), (b'nan', None), (b'inf', None), (b'\t1.0', None), (b'1.0\x80', None),
                                          (b'1_0', None), (b'1234567890123456', None), (b'0000001234567890.12345', 1234567890.12345)])
def test_real_fields(field, value):
    got = R.real(field)
    if value is None:
        assert got is None
    else:
        assert got is not None and np.float32(value).tobytes() == got.tobytes()


def test_integer_fields():
    assert [R.integer(f) for f in (b'  -5', b' 12 ', b'+3', b'0012')] == [-5, 12, 3, 12]
    assert [R.integer(f) for f in (b'A000', b'1_0', b'    ', b'1 2', b'-', b'1.0', b'\t1', b'1234567890')] == [None] * 8


def test_tile_edge_generators():
    T = hip.STRUCT_TILE
    src = open(os.path.join(os.path.dirname(hip.__file__), '..', 'include', 'kpd.h')).read()
    assert int(re.search(r'#define KPD_STRUCT_TILE (\d+)', src).group(1)) == T
    for n in (0, 1, 79, 80, 81, T - 1, T, T + 1):
        f = SC.file_of_length(n, seed=n)
        assert len(f) == n
        assert parse(f)['n_lines'] == -(-n // 80)
    f = SC.simple_file(5, 1, line_len=T // 4)
    assert len(f) == 5 * T // 4 and [i for i, c in enumerate(f) if c == 10] == [k * T // 4 - 1 for k in range(1, 6)]
    text, ptr = SC.concat([SC.file_of_length(T - 1, 1), b'', SC.file_of_length(2, 2), SC.file_of_length(T + 1, 3)])
    assert ptr == [0, T - 1, T - 1, T + 1, 2 * T + 2] and len(text) == ptr[-1]
    h = SC.hostile_bytes(4096, 7)
    assert len(h) == 4096 and h == SC.hostile_bytes(4096, 7) and b'\nATOM  ' in h and max(h) >= 0x80
    out = parse(h)                                          # the restatement takes any bytes
    assert out['atom_ptr'][1] == out['pos'].shape[0]


def test_text_written_from_arrays_reads_back():
    g = np.random.default_rng(3)
    pos = g.uniform(-200, 200, (50, 3)).astype(np.float32)
    el = g.integers(0, 11, 50)
    res = np.repeat(np.arange(10), 5)
    out = parse(SC.pdb_from_arrays(pos, el, res))
    want = np.array([[np.float32(float('%8.3f' % v)) for v in p] for p in pos], dtype=np.float32)
    assert out['pos'].tobytes() == want.tobytes()
    assert out['elem'].tolist() == el.tolist() and out['res_idx'].tolist() == res.tolist() and out['status'] == [0]
    assert (out['flags'] == R.STD).all() and out['res_class'].tolist() == (res % 20).tolist()


def test_the_api_refuses_host_tensors():
    text = torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(hip.KpdError):
        hip.pdb_parse(text, torch.tensor([0, 10]), SC.REC_EL)
    with pytest.raises(hip.KpdError):
        structure.read_pdb([SC.hand_main()], SC.REC_EL, device='cpu')


# ---- SDF ---------------------------------------------------------------------------------------------------------------------------------
from .molecule_cases import ALLOWED, ELEMENTS, Z  # noqa: E402


def records_of(out):
    """[(status, atoms, [(i, j, order)] local to the record)] of what parse_sdf returned."""
    got = []
    for m in range(out['mol_ptr'][-1]):
        a0, a1, p0, p1 = out['lig_ptr'][m], out['lig_ptr'][m + 1], out['bond_ptr'][m], out['bond_ptr'][m + 1]
        got.append((out['status'][m], a1 - a0, [(int(i) - a0, int(j) - a0, int(o)) for (i, j), o in zip(out['bonds'][p0:p1], out['order'][p0:p1])]))
    return got


@pytest.mark.parametrize('name', sorted(SC.HAND_SDF))
def test_hand_sdf_blocks(name):
    f, want = SC.HAND_SDF[name]
    assert records_of(R.parse_sdf(f, [0, len(f)], ELEMENTS, Z, ALLOWED)) == want


def test_sdf_details_of_the_restatement():
    f, _ = SC.HAND_SDF['shuffled bonds, explicit hydrogens']
    out = R.parse_sdf(f, [0, len(f)], ELEMENTS, Z, ALLOWED)
    assert out['pos'].tolist() == [[0.0, 0.0, 0.0], [np.float32(1.52), 0.0, 0.0], [2.0, np.float32(1.35), 0.0]]
    assert out['elem'].tolist() == [0, 0, 2] and out['valence'].tolist() == [1, 2, 1] and out['frag'].tolist() == [0, 0, 0]
    assert out['summary'].tolist() == [[2, 1, 3, 0]] and f[out['title_off'][0, 0]:out['title_off'][0, 1]] == b'ethanol'
    keep = R.parse_sdf(f, [0, len(f)], ELEMENTS, Z, ALLOWED, remove_h=False)       # H and D are "other" for these classes
    assert keep['status'] == [R.MOL_BAD_ATOM] and keep['lig_ptr'] == [0, 7] and keep['elem'].tolist() == [0, 0, 2, 10, 10, 10, 10]
    assert keep['bonds'].tolist() == [[0, 1], [0, 3], [0, 4], [0, 6], [1, 2], [2, 5]] and keep['summary'].tolist() == [[6, 1, 7, 4]]
    f, _ = SC.HAND_SDF['two records and a bare block']
    out = R.parse_sdf(f, [0, len(f)], ELEMENTS, Z, ALLOWED)
    assert out['mol_ptr'] == [0, 3] and out['lig_ptr'] == [0, 2, 2, 3] and out['summary'].tolist() == [[1, 1, 2, 0], [0, 0, 0, 0], [0, 1, 1, 1]]
    assert [f[a:b] for a, b in out['title_off']] == [b'first', b'only hydrogens', b'bare']
    big = SC.big_molecule(256, 1)
    assert R.parse_sdf(big, [0, len(big)], ELEMENTS, Z, ALLOWED)['status'] == [0]
    for f in (SC.big_molecule(257, 1), SC.big_molecule(20, 1, degree7=True)):
        assert R.parse_sdf(f, [0, len(f)], ELEMENTS, Z, ALLOWED)['status'] == [R.MOL_LEFT_OUT | R.SD_LIMITS]


def test_the_sdf_api_refuses_host_tensors():
    from keypoint_diffusion_amd import molecule
    with pytest.raises(hip.KpdError):
        hip.sdf_parse(torch.zeros(10, dtype=torch.uint8), torch.tensor([0, 10]), ELEMENTS, Z, ALLOWED)
    with pytest.raises(hip.KpdError):
        structure.read_sdf([SC.HAND_SDF['CRLF'][0]], ELEMENTS, device='cpu')
    with pytest.raises(hip.KpdError):
        molecule.Molecules.from_sdf([SC.HAND_SDF['CRLF'][0]], ELEMENTS, device='cpu')
