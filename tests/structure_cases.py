"""Deterministic PDB text for the structure-file tests: text written from arrays, hand-written records, files that sit on the
edges of the line scan's tiles, and hostile bytes."""
import random

import numpy as np

from . import structure_ref as R

REC_EL = ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B']       # the receptor elements of tests/test_pocket_gpu.py
RESNAMES = R.STD_AA


def rec(kind, serial, name, alt, resn, chain, resseq, icode, x, y, z, occ='  1.00', b=' 20.00', el='', cut=None):
    """One record from strings, every field right-justified into its columns (name left-justified); `cut` keeps that many columns."""
    line = f'{kind:<6}{serial:>5} {name:<4}{alt}{resn:>3} {chain}{resseq:>4}{icode}   {x:>8}{y:>8}{z:>8}{occ:>6}{b:>6}          {el:>2}'
    return line if cut is None else line[:cut]


# two records written out in full, column by column, that rec() has to reproduce (tests/test_structure_config.py)
LITERAL = [
    'ATOM      1  N   ALA A   1      11.104   6.134  -6.504  1.00 20.00           N',
    'HETATM 1234 CA    CA A 301A     -0.001 123.456-100.250  0.50  7.25          CA',
]
LITERAL_ARGS = [
    ('ATOM', '1', ' N', ' ', 'ALA', 'A', '1', ' ', '11.104', '6.134', '-6.504', '1.00', '20.00', 'N'),
    ('HETATM', '1234', 'CA', ' ', 'CA', 'A', '301', 'A', '-0.001', '123.456', '-100.250', '0.50', '7.25', 'CA'),
]

# (line, what the record must read as) -- None for lines that are no record.  Values are written by hand, not computed.
A = 'ATOM'
H = 'HETATM'
HAND_MAIN = [
    ('REMARK   2 RESOLUTION.    1.80 ANGSTROMS.', None),
    (rec(A, '1', ' N', ' ', 'ALA', 'A', '1', ' ', '11.104', '6.134', '-6.504', el='N'),
     dict(sym='N', pos=(11.104, 6.134, -6.504), res_idx=0, flags=R.STD, resseq=1)),
    (rec(A, '2', ' CA', ' ', 'ALA', 'A', '1', ' ', '12.560', '6.000', '-6.100', el='C'),
     dict(sym='C', res_idx=0, flags=R.STD | R.CALPHA)),
    (rec(A, '3', 'HD11', ' ', 'LEU', 'A', '2', ' ', '1.000', '2.000', '3.000'),
     dict(sym='H', res_idx=1, flags=R.STD | R.HYDROGEN | R.GUESSED)),
    ('ANISOU    3 HD11 LEU A   2     2406   1892   1614    198    519   -328       H', None),
    (rec(A, '4', ' CA', 'A', 'SER', 'A', '3', ' ', '4.000', '5.000', '6.000', '0.60', el='C'),
     dict(sym='C', res_idx=2, flags=R.STD | R.CALPHA, occ=0.6)),
    (rec(A, '5', ' CA', 'B', 'SER', 'A', '3', ' ', '4.100', '5.100', '6.100', '0.40', el='C'),
     dict(sym='C', res_idx=2, flags=R.STD | R.CALPHA | R.ALTLOC, occ=0.4)),
    (rec(A, '6', ' CA', ' ', 'SER', 'A', '3', 'A', '7.000', '8.000', '9.000', el='C'),
     dict(res_idx=3, tags=ord('A') | ord('A') << 8 | 32 << 16)),
    (rec(A, '7', ' N', ' ', 'GLY', 'B', '-5', ' ', '-0.000', '0.000', '-12.345', el='N'),
     dict(res_idx=4, resseq=-5, pos=(-0.0, 0.0, -12.345))),
    ('TER       8      GLY B  -5', None),
    (rec(H, '9', 'CA', ' ', 'CA', 'A', '301', ' ', '1.000', '1.000', '1.000'),
     dict(sym='Ca', res_idx=5, flags=R.HETATM | R.GUESSED)),
    (rec(H, '10', 'CL', ' ', 'CL', 'A', '302', ' ', '2.000', '1.000', '1.000', el='CL'), dict(sym='Cl', elem=6, res_idx=6, flags=R.HETATM)),
    (rec(H, '11', 'FE', ' ', 'HEM', 'A', '303', ' ', '3.000', '1.000', '1.000', el='FE'), dict(sym='Fe', elem=10, flags=R.HETATM)),
    (rec(H, '12', 'SE', ' ', 'MSE', 'A', '304', ' ', '4.000', '1.000', '1.000'), dict(sym='Se', flags=R.HETATM | R.GUESSED)),
    (rec(H, '13', ' O', ' ', 'HOH', 'A', '401', ' ', '5.000', '1.000', '1.000', el='O'), dict(sym='O', flags=R.HETATM | R.WATER)),
    (rec(H, '14', ' H1', ' ', 'HOH', 'A', '401', ' ', '5.500', '1.000', '1.000'),
     dict(sym='H', flags=R.HETATM | R.WATER | R.HYDROGEN | R.GUESSED)),
    (rec(A, '*****', ' C', ' ', 'VAL', 'A', '5', ' ', '6.000', '1.000', '1.000', el='C'), dict(sym='C', flags=R.STD, pos=(6.0, 1.0, 1.0))),
    (rec(A, '16', ' C', ' ', 'VAL', 'A', '5', ' ', '', '1.000', '1.000', el='C'), dict(flags=R.STD | R.BAD, nan=True)),
    (rec(A, '17', ' C', ' ', 'VAL', 'A', '5', ' ', '1.00e+01', '1.000', '1.000', el='C'), dict(flags=R.STD | R.BAD, nan=True)),
    (rec(A, '18', ' C', ' ', 'VAL', 'A', '5', ' ', '1.000', '\t  1.000', '1.000', el='C'), dict(flags=R.STD | R.BAD, nan=True)),
    (rec(A, '19', ' C', ' ', 'VAL', 'A', '5', ' ', '1.000', '1.000', '1.0\x800', el='C'), dict(flags=R.STD | R.BAD, nan=True)),
    (rec(A, '20', ' O', ' ', 'VAL', 'A', '5', ' ', '1.000', '2.000', '3.000', el='O', cut=54),
     dict(sym='O', flags=R.STD | R.GUESSED, pos=(1.0, 2.0, 3.0), occ_nan=True)),
    (rec(A, '21', ' O', ' ', 'VAL', 'A', '5', ' ', '1.000', '2.000', '3.000', '0.75', el='O', cut=66),
     dict(sym='O', flags=R.STD | R.GUESSED, occ=0.75)),
    (rec(A, '22', ' O', ' ', 'VAL', 'A', '5', ' ', '1.000', '2.000', '3.000', el='O', cut=76), dict(sym='O', flags=R.STD | R.GUESSED)),
    (rec(A, '23', ' O', ' ', 'VAL', 'A', '5', ' ', '1.000', '2.000', '3.000', el='O', cut=53), dict(flags=R.STD | R.GUESSED | R.BAD, nan=True)),
    (rec(A, '24', ' O', ' ', 'VAL', 'A', 'A000', ' ', '1.000', '2.000', '3.000', el='O'), dict(flags=R.STD | R.BAD, nan=True, resseq=0)),
    (rec(H, '25', '1HB', ' ', 'LIG', 'A', '500', ' ', '1.000', '2.000', '3.000'), dict(sym='H', flags=R.HETATM | R.HYDROGEN | R.GUESSED)),
    (rec(H, '26', ' D1', ' ', 'LIG', 'A', '500', ' ', '1.000', '2.000', '3.000', el='D'), dict(sym='D', flags=R.HETATM | R.HYDROGEN)),
    (rec(H, '27', 'CL1', ' ', 'LIG', 'A', '500', ' ', '1.000', '2.000', '3.000', el='cl'), dict(sym='Cl', elem=6, flags=R.HETATM)),
    ('END', None),
]


def hand_main() -> bytes:
    return ('\n'.join(line for line, _ in HAND_MAIN) + '\n').encode('latin-1')


def two_models() -> bytes:
    """Two MODELs: only the first is kept; status bit 3."""
    m = lambda x: rec(A, '1', ' CA', ' ', 'GLY', 'A', '1', ' ', x, '0.000', '0.000', el='C')
    return '\n'.join(['MODEL        1', m('1.000'), m('2.000'), 'ENDMDL', 'MODEL        2', m('3.000'), 'ENDMDL', 'END', '']).encode()


def crlf_no_final_newline() -> bytes:
    """CRLF line ends, and a last record that the end of the file ends."""
    a = rec(A, '1', ' N', ' ', 'GLY', 'A', '1', ' ', '1.250', '2.500', '3.750', el='N')
    b = rec(A, '2', ' C', ' ', 'GLY', 'A', '1', ' ', '4.000', '5.000', '6.000', el='C')
    return (a + '\r\n' + 'REMARK\r\n' + b).encode()


def split_residue() -> bytes:
    """Residue A 1 in two runs around A 2: three residue starts by the run-length rule (prody's getResindices would give two)."""
    r = lambda n, s: rec(A, n, ' C', ' ', 'GLY', 'A', s, ' ', '1.000', '1.000', '1.000', el='C')
    return '\n'.join([r('1', '1'), r('2', '1'), r('3', '2'), r('4', '1'), '']).encode()


def pdb_from_arrays(pos, el_idx, res_idx, elements=REC_EL, other='Zn', hetatm_from=None) -> bytes:
    """A PDB file from arrays: coordinates as %8.3f, element symbols in upper case in columns 77-78 (`other` for the index past the
    list), residues named by their index over the standard amino acids, numbered from 1, chain A."""
    lines = []
    for i, (p, e, r) in enumerate(zip(np.asarray(pos, dtype=np.float64), el_idx, res_idx)):
        sym = elements[e] if e < len(elements) else other
        kind = H if hetatm_from is not None and i >= hetatm_from else A
        lines.append(rec(kind, str((i + 1) % 100000), ' ' + sym.upper() if len(sym) == 1 else sym.upper(), ' ', RESNAMES[int(r) % 20], 'A',
                         str(int(r) + 1), ' ', '%.3f' % p[0], '%.3f' % p[1], '%.3f' % p[2], el=sym.upper()))
    return ('\n'.join(lines) + '\nEND\n').encode()


def simple_file(n_atoms: int, seed: int, line_len: int = 80) -> bytes:
    """n_atoms records of exactly line_len bytes each, '\\n' included (records are padded or cut behind column 66)."""
    g = random.Random(seed)
    out = []
    for i in range(n_atoms):
        line = rec(A, str(i + 1), ' C', ' ', RESNAMES[(i // 3) % 20], 'A', str(i // 3 + 1), ' ', '%.3f' % g.uniform(-99, 99),
                   '%.3f' % g.uniform(-99, 99), '%.3f' % g.uniform(-99, 99), el='C')
        out.append(line.ljust(line_len - 1)[:line_len - 1])
    return ('\n'.join(out) + '\n').encode() if out else b''


def file_of_length(n_bytes: int, seed: int) -> bytes:
    """A file of exactly n_bytes bytes (n_bytes >= 0): 80-byte records, then one shorter last line without a newline."""
    body = simple_file(n_bytes // 80, seed)
    tail = n_bytes - len(body)
    last = rec(A, '9', ' O', ' ', 'GLY', 'B', '7', ' ', '1.000', '2.000', '3.000', el='O').ljust(79)[:tail]
    return body + last.encode()


def concat(files):
    """(text, file_ptr) of a list of files."""
    ptr = [0]
    for f in files:
        ptr.append(ptr[-1] + len(f))
    return b''.join(files), ptr


def hostile_bytes(n: int, seed: int) -> bytes:
    """Seeded random bytes, with newlines and record names sprinkled in so that the record parser runs on garbage too."""
    g = random.Random(seed)
    b = bytearray(g.randbytes(n))
    for _ in range(n // 50):
        b[g.randrange(n)] = 10
    for _ in range(n // 100):
        p = g.randrange(n - 8)
        b[p:p + 7] = b'\n' + g.choice([b'ATOM  ', b'HETATM', b'ENDMDL'])
    return bytes(b)


def truncations(data: bytes, count: int, seed: int):
    g = random.Random(seed)
    return [data[:g.randrange(len(data) + 1)] for _ in range(count)]


# ---- SDF / MOL V2000 text ------------------------------------------------------------------------------------------------------------
def mol_block(title, atoms, bonds, props=(), items=(), version='V2000', end=True, sep=True, counts=None):
    """A MOL block from (x, y, z, symbol[, charge field]) atoms and (i, j, type) bonds (1-based); x, y, z: numbers (written as
    %10.4f) or strings (written as they are); props: property lines in front of 'M  END'; items: data-item lines behind it."""
    fx = lambda v: v if isinstance(v, str) else '%10.4f' % v
    na, nb = counts if counts is not None else (len(atoms), len(bonds))
    lines = [title, '  hand      3D', '', '%3d%3d  0  0  0  0  0  0  0  0999 %s' % (na, nb, version)]
    for a in atoms:
        chg = a[4] if len(a) > 4 else 0
        lines.append('%s%s%s %-3s 0%3d  0  0  0  0  0  0  0  0  0  0' % (fx(a[0]), fx(a[1]), fx(a[2]), a[3], chg))
    lines += ['%3d%3d%3d  0' % b if not isinstance(b, str) else b for b in bonds]
    lines += list(props) + (['M  END'] if end else []) + list(items) + (['$$$$'] if sep else [])
    return ('\n'.join(lines) + '\n').encode('latin-1')


ETHANOL_H = [(0.0, 0.0, 0.0, 'C'), (1.52, 0.0, 0.0, 'C'), (2.0, 1.35, 0.0, 'O'), (-0.4, 1.0, 0.0, 'H'), (-0.4, -0.5, 0.9, 'H'),
             (2.95, 1.3, 0.0, 'H'), (-0.4, -0.5, -0.9, 'D')]
ETHANOL_H_BONDS = [(6, 3, 1), (3, 2, 1), (1, 4, 1), (2, 1, 1), (5, 1, 1), (1, 7, 1)]          # in no order, i > j among them
BENZENE = [(1.4 * np.cos(k * np.pi / 3), 1.4 * np.sin(k * np.pi / 3), 0.0, 'C') for k in range(6)]

# name -> (file, hand-checked: records, and per record (status, atoms kept with hydrogens removed, bonds [(i, j, order)] 0-based))
SD = R
HAND_SDF = {
    'shuffled bonds, explicit hydrogens': (mol_block('ethanol', ETHANOL_H, ETHANOL_H_BONDS),
                                           [(0, 3, [(0, 1, 1), (1, 2, 1)])]),
    'aromatic type 4': (mol_block('benzene', BENZENE, [(k + 1, (k + 1) % 6 + 1, 4) for k in range(6)]),
                        [(SD.SD_AROMATIC, 6, [(0, 1, 1), (0, 5, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 5, 1)])]),
    'M  CHG and a charge field': (mol_block('acetate', [(0.0, 0.0, 0.0, 'C'), (1.5, 0.0, 0.0, 'C'), (2.1, 1.1, 0.0, 'O'), (2.1, -1.1, 0.0, 'O', 5)],
                                            [(1, 2, 1), (2, 3, 2), (2, 4, 1)], props=['M  CHG  1   4  -1']),
                                  [(SD.SD_CHARGES, 4, [(0, 1, 1), (1, 2, 2), (1, 3, 1)])]),
    'data items': (mol_block('with items', [(0.0, 0.0, 0.0, 'C'), (1.2, 0.0, 0.0, 'O')], [(1, 2, 2)],
                             items=['> <score>', '-7.5', '', '> <note>', 'M  END is no end here', '']),
                   [(0, 2, [(0, 1, 2)])]),
    'V3000': (mol_block('v3', [], [], version='V3000', props=['M  V30 BEGIN CTAB', 'M  V30 END CTAB'], counts=(0, 0)),
              [(SD.MOL_LEFT_OUT | SD.SD_V3000, 0, [])]),
    'truncated': (mol_block('cut', ETHANOL_H, ETHANOL_H_BONDS, sep=False)[:300], [(SD.MOL_LEFT_OUT | SD.SD_TRUNCATED, 0, [])]),
    'no M  END': (mol_block('no end', [(0.0, 0.0, 0.0, 'C')], [], end=False), [(SD.MOL_LEFT_OUT | SD.SD_TRUNCATED, 0, [])]),
    'bond to atom 0': (mol_block('b0', [(0.0, 0.0, 0.0, 'C'), (1.5, 0.0, 0.0, 'C')], [(0, 1, 1)]), [(SD.MOL_LEFT_OUT | SD.SD_UNPARSABLE, 0, [])]),
    'bond to atom n + 1': (mol_block('bn', [(0.0, 0.0, 0.0, 'C'), (1.5, 0.0, 0.0, 'C')], [(1, 3, 1)]), [(SD.MOL_LEFT_OUT | SD.SD_UNPARSABLE, 0, [])]),
    'duplicate bond': (mol_block('dup', [(0.0, 0.0, 0.0, 'C'), (1.5, 0.0, 0.0, 'C')], [(1, 2, 1), (2, 1, 2)]), [(SD.MOL_LEFT_OUT | SD.SD_LIMITS, 0, [])]),
    'self bond': (mol_block('self', [(0.0, 0.0, 0.0, 'C'), (1.5, 0.0, 0.0, 'C')], [(1, 2, 1), (2, 2, 1)]), [(SD.MOL_LEFT_OUT | SD.SD_LIMITS, 0, [])]),
    'bond type 6': (mol_block('query', [(0.0, 0.0, 0.0, 'C'), (1.5, 0.0, 0.0, 'C')], [(1, 2, 6)]), [(SD.MOL_LEFT_OUT | SD.SD_UNPARSABLE, 0, [])]),
    'coordinate with an exponent': (mol_block('exp', [('1.0000e+00', 0.0, 0.0, 'C')], []), [(SD.MOL_LEFT_OUT | SD.SD_UNPARSABLE, 0, [])]),
    'unsupported element': (mol_block('iron', [(0.0, 0.0, 0.0, 'FE'), (2.0, 0.0, 0.0, 'O')], [(1, 2, 1)]), [(SD.MOL_BAD_ATOM, 2, [(0, 1, 1)])]),
    'two records and a bare block': (mol_block('first', [(0.0, 0.0, 0.0, 'C'), (1.5, 0.0, 0.0, 'N')], [(1, 2, 3)]) +
                                     mol_block('only hydrogens', [(0.0, 0.0, 0.0, 'H'), (0.7, 0.0, 0.0, 'H')], [(1, 2, 1)]) +
                                     mol_block('bare', [(0.0, 0.0, 0.0, 'S')], [], sep=False) + b'\n\n',
                                     [(0, 2, [(0, 1, 3)]), (SD.MOL_EMPTY, 0, []), (0, 1, [])]),
    'CRLF': (mol_block('crlf', [(0.0, 0.0, 0.0, 'C'), (1.2, 0.0, 0.0, 'O')], [(1, 2, 2)]).replace(b'\n', b'\r\n'), [(0, 2, [(0, 1, 2)])]),
    'nothing': (b'', []),
    'blank lines only': (b'\n\r\n\n', []),
    'separator first': (b'$$$$\n', [(SD.MOL_LEFT_OUT | SD.SD_TRUNCATED, 0, [])]),
}


def big_molecule(n_atoms, seed, degree7=False):
    """A chain of n_atoms carbons with random extra bonds (a tree otherwise), as a block; degree7: atom 1 gets seven bonds."""
    g = random.Random(seed)
    atoms = [(g.uniform(-50, 50), g.uniform(-50, 50), g.uniform(-50, 50), 'C') for _ in range(n_atoms)]
    bonds = [(k + 1, k + 2, 1 + k % 3) for k in range(n_atoms - 1)]
    if degree7:
        bonds += [(1, k, 1) for k in range(3, 9)]
    g.shuffle(bonds)
    return mol_block('big %d' % n_atoms, atoms, bonds)
