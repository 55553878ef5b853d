"""Structure files on the device: PDB and SDF text -> the arrays and `Molecules` the rest of the library takes.

Upstream's entry points all begin with a parse (byop.py reads receptor.pdb, process_crossdocked.py / process_bindingmoad.py read
~10^5 complexes) and leave it to prody and BioPython: per-file, per-atom Python work.  Here the files are read on the host as
bytes, concatenated once, copied with one H2D copy and parsed by `kpd_pdb_parse` / `kpd_sdf_parse` (csrc/structure_io.hip) for the whole batch;
include/kpd.h states every column, rounding and flag.  Nothing is filtered by the kernel: `Receptors.mask` turns its flags into
the probe / emit masks of `pocket.extract_pockets`.

No CPU implementation: device='cpu' raises `hip.KpdError`.  Not supported: mmCIF, PDBQT, gzip, hybrid-36, prody's selection
grammar, BioPython's highest-occupancy altloc choice, CONECT records, V3000 blocks, formal charges, isotopes, stereo flags.
"""
import os
from typing import List, Optional, Sequence, Union

import torch

from . import hip

# constants.py:9-10 (aa_encoding, one-letter, alphabetical) as the residue names of columns 18-20: res_class is upstream's aa_to_idx
AA_RESNAMES = ['ALA', 'CYS', 'ASP', 'GLU', 'PHE', 'GLY', 'HIS', 'ILE', 'LYS', 'LEU', 'MET', 'ASN', 'PRO', 'GLN', 'ARG', 'SER', 'THR',
               'VAL', 'TRP', 'TYR']


def _file_bytes(f: Union[str, bytes, os.PathLike]) -> bytes:
    """bytes are a file's content, and so is a str that holds a newline; any other str (or PathLike) is a path."""
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    if isinstance(f, str) and '\n' in f:
        return f.encode('latin-1')
    with open(f, 'rb') as fh:
        return fh.read()


def _to_device(files, device):
    """The files' bytes, concatenated once and copied with one H2D copy: (host bytes, text, file_ptr)."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise hip.KpdError(f'structure files are parsed on the GPU (got device {dev}); there is no CPU parser')
    parts = [_file_bytes(f) for f in files]
    blob = b''.join(parts)
    ptr = [0]
    for p in parts:
        ptr.append(ptr[-1] + len(p))
    text = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev) if blob else torch.zeros(0, dtype=torch.uint8, device=dev)
    return blob, text, torch.tensor(ptr, dtype=torch.int64).to(dev), ptr


class Receptors:
    """What `read_pdb` parsed: per-atom device tensors over all files (pos [n,3], occ_b [n,2], sym, elem, name, resname, res_class,
    resseq, tags, line_off, res_idx, flags; include/kpd.h, kpd_pdb_parse) and per file `segments` (B + 1 atom offsets), `n_res`
    and `status` (host lists)."""

    def __init__(self, out: dict, elements: Sequence[str], resnames: Sequence[str], blob: bytes, file_ptr: List[int], files):
        for k in ('pos', 'occ_b', 'sym', 'elem', 'name', 'resname', 'res_class', 'resseq', 'tags', 'line_off', 'res_idx', 'flags'):
            setattr(self, k, out[k])
        self.segments, self.n_res, self.status = out['atom_ptr'], out['n_res'], out['status']
        self.elements, self.resnames = list(elements), list(resnames)
        self.files = list(files)
        self._blob, self._file_ptr = blob, file_ptr

    def __len__(self) -> int:
        return len(self.segments) - 1

    def flag(self, bit: int) -> torch.Tensor:
        return (self.flags & bit) != 0

    def mask(self, remove_hydrogen: bool = True, remove_water: bool = True, altloc: bool = True, hetatm: bool = True) -> torch.Tensor:
        """bool [n]: the atoms a selection keeps.  Bad records (NaN coordinates) are never kept.  remove_hydrogen / remove_water:
        prody's 'not hydrogen' / 'not water' by this library's lists (H or D; HOH DOD WAT H2O OH2 TIP SOL).  altloc: drop alternate
        locations other than blank and 'A' (prody's default).  hetatm=False drops HETATM records too."""
        drop = hip.PDB_BAD | (hip.PDB_HYDROGEN if remove_hydrogen else 0) | (hip.PDB_WATER if remove_water else 0) | \
            (hip.PDB_ALTLOC if altloc else 0) | (0 if hetatm else hip.PDB_HETATM)
        return (self.flags & drop) == 0

    def features(self):
        """(one-hot [n,F] bool over `elements`, other_atoms_mask [n] bool): upstream's onehot_encode_elements without its last column."""
        F = len(self.elements)
        return torch.nn.functional.one_hot(self.elem.long(), F + 1)[:, :F].bool(), self.elem == F

    def residue_features(self) -> torch.Tensor:
        """One-hot [n,R] bool over `resnames` (all False for other residues): the ca_only features of byop.py:169-175."""
        Rn = len(self.resnames)
        return torch.nn.functional.one_hot(self.res_class.long(), Rn + 1)[:, :Rn].bool()

    def lines(self, rows: torch.Tensor) -> List[bytes]:
        """Per file, the original record lines (each ended by '\\n') of the atoms `rows` (global atom numbers, or a bool mask over
        the atoms), in atom order: what byop.py:199-204 writes as pocket.pdb."""
        rows = torch.as_tensor(rows)
        if rows.dtype == torch.bool:
            rows = rows.nonzero().flatten()
        rows = rows.long().to(self.line_off.device)
        offs = self.line_off[rows].cpu().tolist()
        out = [bytearray() for _ in range(len(self))]
        b = 0
        for r, off in sorted(zip(rows.cpu().tolist(), offs)):
            while r >= self.segments[b + 1]:
                b += 1
            end = self._blob.find(b'\n', off, self._file_ptr[b + 1])
            line = self._blob[off:self._file_ptr[b + 1] if end < 0 else end]
            out[b] += line.rstrip(b'\r') + b'\n'
        return [bytes(o) for o in out]


def read_pdb(files, rec_elements: Sequence[str], resnames: Optional[Sequence[str]] = None, device='cuda') -> Receptors:
    """Parse a batch of PDB files on the GPU.  `files`: paths, or contents as bytes or as str holding a newline.  rec_elements:
    the receptor element symbols in Title case (`elem` indexes them; len(rec_elements) = "other"); resnames: the residue names
    `res_class` indexes (default: upstream's aa_to_idx order).  Raises KpdError for a file whose records do not fit the tables
    after the second call (cannot happen) or for device='cpu'."""
    files = list(files)
    resnames = AA_RESNAMES if resnames is None else list(resnames)
    blob, text, file_ptr, ptr = _to_device(files, device)
    out = hip.pdb_parse(text, file_ptr, rec_elements, resnames)
    if any(s & (hip.PDB_CAPACITY | hip.PDB_LINES | hip.PDB_BAD_SEGMENT) for s in out['status']):
        raise hip.KpdError(f'read_pdb: status {out["status"]} (internal sizing error)')
    return Receptors(out, rec_elements, resnames, blob, ptr, files)


def read_sdf(files, lig_elements: Sequence[str], remove_hydrogen: bool = True, allowed_bonds=None, device='cuda'):
    """Parse a batch of SDF / MOL V2000 files on the GPU (`kpd_sdf_parse`) into `molecule.Molecules` with the bonds the files
    state: one molecule per record, in file order.  `files` as for `read_pdb`; lig_elements: the F ligand element symbols;
    remove_hydrogen: drop H / D atoms and their bonds (upstream's RemoveAllHs, parse_ligand:58-67); allowed_bonds: the validity
    table of `build_molecules`.  `pos`, `lig_elements` and the sizes are set, so `.sdf()`, `.keys()`, `.sanitize()`, `.pose_rmsd()`,
    `.vina_score()` and `.relax()` work on file ligands.  Added to the molecules: `.mol_ptr` (B + 1 offsets: the records of every
    file), `.titles` (the title line of every record), `.file_status`.  A record that could not be read has no atoms and
    status bit 8 (hip.MOL_BAD_SEGMENT) beside the reason (hip.SDF_*); one with an unsupported element has hip.MOL_BAD_ATOM."""
    from . import molecule
    files = list(files)
    z, allowed = molecule._class_tables(lig_elements, allowed_bonds)
    blob, text, file_ptr, ptr = _to_device(files, device)
    m = hip.sdf_parse(text, file_ptr, lig_elements, z, allowed, remove_h=remove_hydrogen)
    if any(s & (hip.PDB_CAPACITY | hip.PDB_LINES | hip.PDB_BAD_SEGMENT) for s in m['file_status']) or m['n_atoms'] > m['pos'].shape[0]:
        raise hip.KpdError(f'read_sdf: file status {m["file_status"]} (internal sizing error)')
    mols = molecule.Molecules(m['lig_ptr'], m['summary'], m['status'], m['elem'], m['valence'], m['frag'], m['bonds'], m['order'], m['bond_ptr'],
                              m['pos'], lig_elements, sizes=m['sizes'])
    mols._allowed = allowed
    if allowed_bonds is not None and 'H' in allowed_bonds:
        mols._allowed_h = molecule._class_tables(['H'], allowed_bonds)[1][0]
    mols.mol_ptr, mols.file_status, mols.sym = m['mol_ptr'], m['file_status'], m['sym']
    mols.titles = [blob[a:b].decode('latin-1') for a, b in m['title_off'].cpu().tolist()]
    return mols


def load_complexes(rec_files, lig_files, rec_elements: Sequence[str], lig_elements: Sequence[str], form: str = 'crossdocked',
                   remove_hydrogen: bool = True, ca_only: bool = False, device='cuda', **extract_pockets_kwargs):
    """Files -> the processed-dataset dict: parse both sides on the GPU, build the masks and call `pocket.extract_pockets`.
    rec_files[i] (PDB) and lig_files[i] (SDF with one ligand) are complex i.  Returns (data, skipped) as `extract_pockets`;
    `data` is what `ProteinLigandDataset(processed_data_file=data)` takes.
      * form='crossdocked' (process_crossdocked.py:96-152): receptor atoms = not water (and not hydrogen with remove_hydrogen),
        altLoc blank or 'A'; probe = emit = kept & ~other, the ligand box, candidates='box'.
      * form='byop' (byop.py:119-197, process_bindingmoad.py:124-204): probe = every atom of a standard residue, hydrogens
        included; emit = heavy atoms of supported elements in standard residues (with ca_only: the C-alphas, features = residue
        one-hots); no box; candidates='pocket'.
    `skipped` gains, with upstream's exception in the reason: 'unparsable receptor' (parse_protein's Unparsable: no atom),
    'ligand has unsupported elements' (Unparsable, parse_ligand:77-78), 'more than one ligand in the file' (NotImplementedError,
    parse_ligand:60-61) and 'unparsable ligand' (the record could not be read; rdkit would return None)."""
    from . import pocket
    if form not in ('crossdocked', 'byop'):
        raise ValueError("form must be 'crossdocked' or 'byop'")
    rec_files, lig_files = list(rec_files), list(lig_files)
    if len(rec_files) != len(lig_files):
        raise ValueError('one ligand file per receptor file')
    rec = read_pdb(rec_files, rec_elements, device=device)
    ligs = read_sdf(lig_files, lig_elements, remove_hydrogen=remove_hydrogen, device=device)
    dev = rec.pos.device
    lig_status = ligs.status.cpu().tolist()
    reasons, good = {}, []
    for i in range(len(rec_files)):
        m0, m1 = ligs.mol_ptr[i], ligs.mol_ptr[i + 1]
        if rec.segments[i + 1] == rec.segments[i]:
            reasons[i] = 'unparsable receptor (Unparsable: no atom record)'
        elif m1 - m0 > 1:
            reasons[i] = 'more than one ligand in the file (NotImplementedError)'
        elif m1 == m0 or lig_status[m0] & (hip.MOL_BAD_SEGMENT | hip.MOL_EMPTY):
            reasons[i] = 'unparsable ligand (no readable record)'
        elif lig_status[m0] & hip.MOL_BAD_ATOM:
            reasons[i] = 'ligand has unsupported elements (Unparsable)'
        else:
            good.append(i)
    feat, other = rec.features()
    std = rec.flag(hip.PDB_STD_AA)
    if form == 'crossdocked':
        kept = rec.mask(remove_hydrogen=remove_hydrogen, remove_water=True, altloc=True)
        masks = dict(other_atoms_mask=other | ~kept, candidates='box')
        extract_pockets_kwargs.setdefault('lig_box_padding', 6)
    else:
        base = rec.mask(remove_hydrogen=False, remove_water=False, altloc=True) & std
        emit = base & rec.flag(hip.PDB_CALPHA) if ca_only else base & ~rec.flag(hip.PDB_HYDROGEN) & ~other
        masks = dict(probe_mask=base, emit_mask=emit, candidates='pocket')
        extract_pockets_kwargs['lig_box_padding'] = None
        if ca_only:
            feat = rec.residue_features()
    # the complexes that go on: rows of both sides, host arithmetic on B + 1 numbers
    lig_ptr = ligs.lig_ptr.cpu().tolist()
    rrow = torch.cat([torch.arange(rec.segments[i], rec.segments[i + 1]) for i in good] + [torch.zeros(0, dtype=torch.long)]).to(dev)
    lrow = torch.cat([torch.arange(lig_ptr[ligs.mol_ptr[i]], lig_ptr[ligs.mol_ptr[i] + 1]) for i in good] + [torch.zeros(0, dtype=torch.long)]).to(dev)
    seg = lambda counts: [0] + torch.tensor(counts, dtype=torch.long).cumsum(0).tolist() if counts else [0]
    rseg = seg([rec.segments[i + 1] - rec.segments[i] for i in good])
    lseg = seg([lig_ptr[ligs.mol_ptr[i] + 1] - lig_ptr[ligs.mol_ptr[i]] for i in good])
    F = len(lig_elements)
    lig_feat = torch.nn.functional.one_hot(ligs.elem[lrow].long().clamp(0, F), F + 1)[:, :F].bool()
    sub = {k: (v[rrow] if isinstance(v, torch.Tensor) else v) for k, v in masks.items()}
    data, skipped = pocket.extract_pockets(rec.pos[rrow], feat[rrow], rec.res_idx[rrow], rseg, ligs.pos[lrow], lig_feat, lseg,
                                           rec_files=[rec_files[i] for i in good], lig_files=[lig_files[i] for i in good], **sub,
                                           **extract_pockets_kwargs)
    skipped = sorted([(good[k], why) for k, why in skipped] + list(reasons.items()))
    return data, skipped
