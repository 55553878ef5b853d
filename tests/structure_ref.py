"""Plain-Python restatement of kpd_pdb_parse (include/kpd.h is the definition): slicing, `int` and `float`, one file and one line
at a time.  It is what the kernel is compared with, bit for bit; it is not prody or BioPython."""
import re

import numpy as np

STD_AA = ('ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL').split()
WATERS = 'HOH DOD WAT H2O OH2 TIP SOL'.split()
TWO_LETTER = ('Li Be Ne Na Mg Al Si Cl Ar Ca Sc Ti Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Zr Mo Ru Rh Pd Ag Cd In Sn '
              'Sb Te Xe Cs Ba Pt Au Pb').split()
HETATM, HYDROGEN, WATER, ALTLOC, STD, CALPHA, GUESSED, BAD = 1, 2, 4, 8, 16, 32, 64, 128
EMPTY, CAPACITY, BAD_RECORD, MODELS, BAD_SEGMENT, LINES = 1, 2, 4, 8, 16, 32

_REAL = re.compile(rb' *[+-]?([0-9]*)(\.?)([0-9]*) *\Z')
_INT = re.compile(rb' *[+-]?[0-9]{1,9} *\Z')


def real(field: bytes):
    """The fp32 value of a real field, or None: blanks, sign, digits with at most one '.', blanks; <= 15 digits."""
    m = _REAL.match(field)
    if not m or not (m.group(1) or m.group(3)):
        return None
    digits = m.group(1) + m.group(3)
    if len(digits.lstrip(b'0')) > 15 or len(m.group(3)) > 15:
        return None
    return np.float32(float(field.decode('ascii')))


def integer(field: bytes):
    return int(field.decode('ascii')) if _INT.match(field) else None


def split_lines(data: bytes, lo: int, hi: int):
    """(offset, content) of the lines of data[lo:hi]: a line ends with '\\n' or with the file; one '\\r' is dropped; 80 columns."""
    out, p = [], lo
    while p < hi:
        q = data.find(b'\n', p, hi)
        end = hi if q < 0 else q + 1
        c = data[p:end - 1] if q >= 0 else data[p:end]
        if c.endswith(b'\r'):
            c = c[:-1]
        out.append((p, c[:80]))
        p = end
    return out


def pack(b: bytes) -> int:
    return int.from_bytes(b.ljust(4, b'\0'), 'little')


def _is_letter(c: int) -> bool:
    return 65 <= c <= 90 or 97 <= c <= 122


def title(c0: int, c1: int = 32) -> bytes:
    """The non-blank bytes in order, a letter in first place upper and in second place lower case."""
    b = bytes(c for c in (c0, c1) if c != 32)
    if not b:
        return b''
    first = b[:1].upper() if _is_letter(b[0]) else b[:1]
    rest = (b[1:].lower() if _is_letter(b[1]) else b[1:]) if len(b) > 1 else b''
    return first + rest


def record(kind: bytes, off: int, c: bytes, elements, resnames):
    """One kept record: content c (at most 80 bytes) -> its outputs, residue key included."""
    col = c.ljust(80)                                   # columns beyond the content read as blanks
    name, alt, resn, chain, rs, icode = col[12:16], col[16:17], col[17:20], col[21:22], col[22:26], col[26:27]
    xyz = [real(col[30 + 8 * k:38 + 8 * k]) for k in range(3)]
    resseq = integer(rs)
    bad = len(c) < 54 or resseq is None or any(v is None for v in xyz)
    nan = np.float32('nan')
    pos = [nan] * 3 if bad else xyz
    occ_b = [v if v is not None else nan for v in (real(col[54:60]), real(col[60:66]))]
    std = resn.decode('latin-1') in STD_AA
    flags = 0
    if col[76:78] != b'  ':
        sym = title(col[76], col[77])
    else:
        a, b = col[12], col[13]
        if a == 32 or 48 <= a <= 57:
            sym = title(b)
        elif _is_letter(a) and std:
            sym = title(a)
        elif _is_letter(a) and _is_letter(b) and title(a, b).decode('ascii') in TWO_LETTER:
            sym = title(a, b)
        else:
            sym = title(a)
        flags |= GUESSED
    s = sym.decode('latin-1')
    r = resn.decode('latin-1')
    flags |= HETATM if kind == b'HETATM' else 0
    flags |= HYDROGEN if s in ('H', 'D') else 0
    flags |= WATER if r in WATERS else 0
    flags |= ALTLOC if alt not in (b' ', b'A') else 0
    flags |= STD if std else 0
    flags |= CALPHA if std and name == b' CA ' else 0
    flags |= BAD if bad else 0
    return dict(pos=pos, occ_b=occ_b, sym=pack(sym), elem=elements.index(s) if s in elements else len(elements), name=pack(name),
                resname=pack(resn), res_class=resnames.index(r) if r in resnames else len(resnames), resseq=resseq or 0,
                tags=chain[0] | icode[0] << 8 | alt[0] << 16, line_off=off, flags=flags, key=(resn, chain, rs, icode))


FIELDS = (('pos', np.float32), ('occ_b', np.float32), ('sym', np.int32), ('elem', np.int32), ('name', np.int32), ('resname', np.int32),
          ('res_class', np.int32), ('resseq', np.int32), ('tags', np.int32), ('line_off', np.int64), ('res_idx', np.int32), ('flags', np.int32))


def parse_pdb(data: bytes, file_ptr, elements, resnames=()):
    """Everything kpd_pdb_parse returns when its capacities suffice: the per-atom arrays of all files, atom_ptr, n_res, status,
    n_lines."""
    elements, resnames = list(elements), list(resnames)
    rows, atom_ptr, n_res, status, n_lines = [], [0], [], [], 0
    for lo, hi in zip(file_ptr[:-1], file_ptr[1:]):
        if lo < 0 or hi < lo or hi > len(data):
            atom_ptr.append(atom_ptr[-1])
            n_res.append(0)
            status.append(BAD_SEGMENT)
            continue
        lines = split_lines(data, lo, hi)
        n_lines += len(lines)
        st, res, prev, ended, count = 0, -1, None, False, 0
        for off, c in lines:
            kind = c[:6]
            if kind == b'ENDMDL':
                ended = True
            if kind not in (b'ATOM  ', b'HETATM'):
                continue
            if ended:
                st |= MODELS
                continue
            r = record(kind, off, c, elements, resnames)
            if r['key'] != prev:
                res += 1
            prev = r.pop('key')
            r['res_idx'] = res
            st |= BAD_RECORD if r['flags'] & BAD else 0
            rows.append(r)
            count += 1
        atom_ptr.append(atom_ptr[-1] + count)
        n_res.append(res + 1)
        status.append(st | (0 if count else EMPTY))
    out = {}
    for name, dt in FIELDS:
        shape = (0, 3) if name == 'pos' else (0, 2) if name == 'occ_b' else (0,)
        vals = [r[name] for r in rows]
        if dt == np.int32:
            vals = [v - (1 << 32) if v >= 1 << 31 else v for v in vals]
        out[name] = np.array(vals, dtype=dt) if rows else np.zeros(shape, dtype=dt)
    out.update(atom_ptr=atom_ptr, n_res=n_res, status=status, n_lines=n_lines)
    return out


# ---- kpd_sdf_parse ------------------------------------------------------------------------------------------------------------------
MOL_EMPTY, MOL_CAPACITY, MOL_BAD_ATOM, MOL_LEFT_OUT = 1, 2, 4, 8
SD_AROMATIC, SD_CHARGES, SD_V3000, SD_UNPARSABLE, SD_TRUNCATED, SD_LIMITS = 16, 32, 64, 128, 256, 512
KNOWN_Z = (1, 5, 6, 7, 8, 9, 14, 15, 16, 17, 33, 35, 53)          # the element table of kpd_mol_perceive


def sdf_records(lines):
    """The records of a file's lines [(offset, end, content)]: closed by a '$$$$' line; a last run unless it is all without content."""
    recs, cur = [], []
    for ln in lines:
        if ln[2][:4] == b'$$$$':
            recs.append(cur)
            cur = []
        else:
            cur.append(ln)
    if any(c for _, _, c in cur):
        recs.append(cur)
    return recs


def sdf_record(rec, elements, z, allowed, remove_h):
    """One record -> (status, atoms [(pos, sym, elem)], bonds {(i, j): order}); a record that is left out has neither."""
    F = len(elements)
    left_out = lambda why: (why | MOL_LEFT_OUT, [], {})
    if len(rec) < 4:
        return left_out(SD_TRUNCATED)
    c = rec[3][2].ljust(80)
    if len(rec[3][2]) >= 39 and c[34:39] == b'V3000':
        return left_out(SD_V3000)
    na, nb = integer(c[0:3]), integer(c[3:6])
    if len(rec[3][2]) < 39 or c[34:39] != b'V2000' or na is None or nb is None or na < 0 or nb < 0:
        return left_out(SD_UNPARSABLE)
    if 4 + na + nb > len(rec):
        return left_out(SD_TRUNCATED)
    rest = [l[2] for l in rec[4 + na + nb:]]
    ends = [k for k, l in enumerate(rest) if l[:6] == b'M  END']
    if not ends:
        return left_out(SD_TRUNCATED)
    st = SD_CHARGES if any(l[:6] in (b'M  CHG', b'M  ISO') for l in rest[:ends[0]]) else 0
    atoms, keep, bad = [], [], False
    for _, _, l in rec[4:4 + na]:
        l = l.ljust(80)
        xyz = [real(l[10 * d:10 * d + 10]) for d in range(3)]
        tok = l[31:34].lstrip(b' ').split(b' ')[0]
        sym = bytes([tok[0]]).upper() + tok[1:].lower() if tok else b''
        if (integer(l[34:36]) or 0) != 0 or (integer(l[36:39]) or 0) != 0:
            st |= SD_CHARGES
        if any(v is None for v in xyz) or not sym:
            bad = True
            continue
        s = sym.decode('latin-1')
        keep.append(not (remove_h and s in ('H', 'D')))
        atoms.append((xyz, pack(sym), elements.index(s) if s in elements else F))
    if bad:
        return left_out(st | SD_UNPARSABLE)
    new = np.cumsum([0] + [int(k) for k in keep])
    kept = [a for a, k in zip(atoms, keep) if k]
    if len(kept) > 256:
        return left_out(st | SD_LIMITS)
    if any(e == F or z[e] not in KNOWN_Z for _, _, e in kept):
        st |= MOL_BAD_ATOM
    bonds, why = {}, 0
    for _, _, l in rec[4 + na:4 + na + nb]:
        l = l.ljust(80)
        i, j, t = integer(l[0:3]), integer(l[3:6]), integer(l[6:9])
        if None in (i, j, t) or not (1 <= i <= na and 1 <= j <= na and 1 <= t <= 4):
            why |= SD_UNPARSABLE
            continue
        if i == j:
            why |= SD_LIMITS
            continue
        if t == 4:
            st |= SD_AROMATIC
            t = 1
        if not (keep[i - 1] and keep[j - 1]):
            continue
        key = (min(new[i - 1], new[j - 1]), max(new[i - 1], new[j - 1]))
        if key in bonds:
            why |= SD_LIMITS
            continue
        bonds[key] = t
    deg = [0] * len(kept)
    for i, j in bonds:
        deg[i] += 1
        deg[j] += 1
    if len(bonds) > 3 * len(kept) or any(d > 6 for d in deg):
        why |= SD_LIMITS
    if why:
        return left_out((st | why) & ~(MOL_BAD_ATOM | SD_AROMATIC))
    return st | (0 if kept else MOL_EMPTY), kept, bonds


def parse_sdf(data: bytes, file_ptr, elements, z, allowed, remove_h=True):
    """Everything kpd_sdf_parse returns when its capacities suffice."""
    elements = list(elements)
    mol_ptr, file_status, n_lines = [0], [], 0
    lig_ptr, bond_ptr, status, summary, titles = [0], [0], [], [], []
    pos, sym, elem, valence, frag, bond_ij, order = [], [], [], [], [], [], []
    for lo, hi in zip(file_ptr[:-1], file_ptr[1:]):
        if lo < 0 or hi < lo or hi > len(data):
            mol_ptr.append(mol_ptr[-1])
            file_status.append(BAD_SEGMENT)
            continue
        lines, p = [], lo
        while p < hi:                                      # as split_lines, with the end of the content
            q = data.find(b'\n', p, hi)
            end = hi if q < 0 else q + 1
            c = data[p:end - 1] if q >= 0 else data[p:end]
            if c.endswith(b'\r'):
                c = c[:-1]
            lines.append((p, p + len(c), c[:80]))
            p = end
        n_lines += len(lines)
        recs = sdf_records(lines)
        mol_ptr.append(mol_ptr[-1] + len(recs))
        file_status.append(0)
        for rec in recs:
            st, atoms, bonds = sdf_record(rec, elements, z, allowed, remove_h)
            a0, n = lig_ptr[-1], len(atoms)
            titles.append([rec[0][0], rec[0][1]] if rec else [0, 0])
            status.append(st)
            lig_ptr.append(a0 + n)
            bond_ptr.append(bond_ptr[-1] + len(bonds))
            val, lab = [0] * n, list(range(n))
            for (i, j), t in sorted(bonds.items()):
                bond_ij.append([a0 + i, a0 + j])
                order.append(t)
                val[i] += t
                val[j] += t
            changed = True
            while changed:                                  # components: every atom takes the lowest atom it can reach
                changed = False
                for i, j in bonds:
                    l = min(lab[i], lab[j])
                    if lab[i] != l or lab[j] != l:
                        lab[i] = lab[j] = l
                        changed = True
            roots = sorted(set(lab))
            sizes = [lab.count(r) for r in roots]
            invalid = sum(1 for (_, _, e), v in zip(atoms, val) if v == 0 or e == len(elements) or z[e] not in KNOWN_Z or v > allowed[e])
            summary.append([len(bonds), len(roots), max(sizes, default=0), invalid] if n else [0, 0, 0, 0])
            for (xyz, s, e), v, l in zip(atoms, val, lab):
                pos.append(xyz)
                sym.append(s)
                elem.append(e)
                valence.append(v)
                frag.append(roots.index(l))
    i32 = lambda v, shape=(0,): np.array(v, dtype=np.int32) if len(v) else np.zeros(shape, dtype=np.int32)
    return dict(mol_ptr=mol_ptr, file_status=file_status, n_lines=n_lines, lig_ptr=lig_ptr, bond_ptr=bond_ptr, status=status,
                summary=i32(summary, (0, 4)), title_off=np.array(titles, dtype=np.int64).reshape(-1, 2),
                pos=np.array(pos, dtype=np.float32).reshape(-1, 3), sym=i32(sym), elem=i32(elem), valence=i32(valence), frag=i32(frag),
                bonds=i32(bond_ij, (0, 2)), order=i32(order))
