"""Pocket extraction on the device: whole receptors + ligands -> pocket atoms and interface points.

The array-level part of upstream's dataset construction.  File parsing (PDB / SDF, element fixing, the
standard-amino-acid test) is `structure.read_pdb` / `read_sdf` / `load_complexes` (csrc/structure_io.hip); everything after
"coordinates, element features and residue index per atom" runs here, batched, in `kpd_pocket_select` and
`kpd_interface_points` (csrc/pocket.hip):

* `get_pocket_atoms`       data_processing/pdbbind_processing.py:85-149 (the CrossDocked form: box, cutoff, whole residues)
* `get_interface_points`   data_processing/pdbbind_processing.py:295-325
* `select_pocket_residues` process_bindingmoad.py:124-204 / byop.py:119-197 (the residue-wise form)
* `extract_pockets`        the loop of process_crossdocked.py:96-152 over a batch, returning the flat processed-dataset
                           dict `ProteinLigandDataset(processed_data_file=dict)` takes

No CPU implementation: CPU tensors raise `hip.KpdError`.  Threshold tests are taken on fp64 squared distances of the
fp32 coordinates (include/kpd.h); they agree with upstream's wherever upstream's own decision is stable.
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import hip

MAX_POCKET_ATOMS = 2048        # kpd_build_rec_graph's limit per pocket


class InterfacePointException(Exception):
    """pdbbind_processing.py:327-331: no (ligand, receptor) pair closer than the distance threshold."""

    def __init__(self, original_exception: Exception = None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.original_exception = original_exception


def _ptr(counts: Sequence[int], device) -> torch.Tensor:
    p = torch.zeros(len(counts) + 1, dtype=torch.int64)
    p[1:] = torch.as_tensor(list(counts), dtype=torch.int64).cumsum(0)
    if int(p[-1]) >= 2 ** 31:
        raise hip.KpdError('more than 2^31 - 1 atoms in one batch')
    return p.to(torch.int32).to(device)


def _single(rec_positions: torch.Tensor, lig_positions: torch.Tensor):
    dev = rec_positions.device
    if not lig_positions.is_cuda:
        raise hip.KpdError(f'ligand positions must live on the GPU (got {lig_positions.device}); pocket extraction has no CPU implementation')
    if lig_positions.shape[0] > hip.POCKET_MAX_LIG:
        raise hip.KpdError(f'{lig_positions.shape[0]} ligand atoms: at most {hip.POCKET_MAX_LIG} are supported')
    return _ptr([rec_positions.shape[0]], dev), _ptr([lig_positions.shape[0]], dev)


def _points(rec_x, rec_ptr, cand, lig_x, lig_ptr, dist_thr, excl_thr):
    """kpd_interface_points with the candidate capacity grown to what the first call reports (a second call only for
    complexes with more than 2048 candidates)."""
    out = hip.interface_points(rec_x, rec_ptr, cand, lig_x, lig_ptr, dist_thr, excl_thr)
    need = max(out['n_cand'], default=0)
    if need > 2048:
        out = hip.interface_points(rec_x, rec_ptr, cand, lig_x, lig_ptr, dist_thr, excl_thr, cap_cand=need)
    if any(s & (hip.POCKET_CAPACITY | hip.POCKET_BAD_SEGMENT) for s in out['status']):
        raise hip.KpdError(f'interface points: status {out["status"]} (more than 4096 points in one complex, or malformed segments)')
    return out


def get_interface_points(ligand_positions: torch.Tensor, rec_positions: torch.Tensor, dist_mat: torch.Tensor = None,
                         distance_threshold: float = 5, exclusion_threshold: float = 2) -> torch.Tensor:
    """pdbbind_processing.py:295-325 on the GPU.  `dist_mat` is accepted and ignored (distances are computed in the kernel).
    Raises InterfacePointException when no pair is closer than `distance_threshold` (upstream: IndexError at :314, wrapped at :147)."""
    rec_ptr, lig_ptr = _single(rec_positions, ligand_positions)
    cand = torch.ones(rec_positions.shape[0], dtype=torch.uint8, device=rec_positions.device)
    out = _points(rec_positions, rec_ptr, cand, ligand_positions, lig_ptr, distance_threshold, exclusion_threshold)
    if out['status'][0] & hip.POCKET_EMPTY:
        raise InterfacePointException(IndexError('no ligand-receptor pair closer than the distance threshold'))
    return out['points']


def get_pocket_atoms(rec_positions: torch.Tensor, rec_features: torch.Tensor, other_atoms_mask: torch.Tensor,
                     rec_res_idx: torch.Tensor, ligand_atom_positions: torch.Tensor, box_padding: float, pocket_cutoff: float,
                     interface_distance_threshold: float, interface_exclusion_threshold: float
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """pdbbind_processing.py:85-149 on the GPU, with the prody selection replaced by the three arrays upstream takes from it
    (coordinates, featurized elements + "other" mask, getResindices).  As upstream, "other"-element atoms are dropped before
    everything else (:108-111): they neither select a residue nor appear in the pocket nor pair into interface points, and
    the returned by-residue mask is indexed over the non-"other" atoms.  Returns (pocket_positions, pocket_features,
    byres_pocket_atom_mask, interface_points); raises InterfacePointException when there is no candidate pair."""
    rec_ptr, lig_ptr = _single(rec_positions, ligand_atom_positions)
    if not other_atoms_mask.is_cuda:
        raise hip.KpdError('other_atoms_mask must live on the GPU')
    keep = ~other_atoms_mask.bool()
    sel = hip.pocket_select(rec_positions, rec_ptr, rec_res_idx.to(torch.int32), keep, keep, ligand_atom_positions, lig_ptr,
                            rec_positions.shape[0], box_padding, pocket_cutoff)
    if sel['status'][0] & (hip.POCKET_BAD_RES | hip.POCKET_BAD_SEGMENT):
        raise hip.KpdError(f'get_pocket_atoms: residue indices outside [0, n_atoms) (status {sel["status"][0]})')
    out = _points(rec_positions, rec_ptr, sel['in_box'] & keep, ligand_atom_positions, lig_ptr, interface_distance_threshold,
                  interface_exclusion_threshold)
    if out['status'][0] & hip.POCKET_EMPTY:
        raise InterfacePointException(IndexError('no ligand-receptor pair closer than the distance threshold'))
    rows = sel['rows'].long()
    return rec_positions[rows], rec_features[rows], sel['pocket_mask'][keep], out['points']


def select_pocket_residues(rec_positions: torch.Tensor, rec_res_idx: torch.Tensor, lig_positions: torch.Tensor, pocket_cutoff: float,
                           probe_mask: Optional[torch.Tensor] = None, emit_mask: Optional[torch.Tensor] = None, ca_only: bool = False,
                           ca_mask: Optional[torch.Tensor] = None, interface_distance_threshold: float = 5,
                           interface_exclusion_threshold: float = 2):
    """The residue-wise selection of process_bindingmoad.py:124-204 / byop.py:119-197 for one structure: a residue is in the
    pocket if any of its `probe_mask` atoms (every atom of a standard residue, hydrogens included; default all atoms) is closer
    than `pocket_cutoff` to a ligand atom; no box.  Of the selected residues the `emit_mask` atoms are returned (heavy atoms
    of supported elements; default all atoms), or with `ca_only` the `ca_mask` atoms (one C-alpha per residue), in which
    case the interface points are the empty [0,3] tensor, as upstream (:193-197).
    Returns (rows, pocket_res_idx, interface_points): rows = indices of the pocket atoms into the input arrays (ascending),
    pocket_res_idx = per pocket atom, the rank of its residue among the selected residues in order of first appearance.
    byop.py:156 indexes the residues of atoms it filters afterwards with other_atoms_mask without filtering the index list; here
    pocket_res_idx is aligned with the emitted atoms (the only sensible reading; only equality of the labels is ever used).
    Raises ValueError when no residue is selected (:140-141) and InterfacePointException when there is no candidate pair."""
    rec_ptr, lig_ptr = _single(rec_positions, lig_positions)
    dev, n = rec_positions.device, rec_positions.shape[0]
    ones = torch.ones(n, dtype=torch.bool, device=dev)
    probe = ones if probe_mask is None else probe_mask.bool()
    if ca_only:
        if ca_mask is None:
            raise ValueError('ca_only=True needs ca_mask (the C-alpha atoms)')
        emit = ca_mask.bool()
    else:
        emit = ones if emit_mask is None else emit_mask.bool()
    sel = hip.pocket_select(rec_positions, rec_ptr, rec_res_idx.to(torch.int32), probe, emit, lig_positions, lig_ptr, n, None, pocket_cutoff)
    st = sel['status'][0]
    if st & (hip.POCKET_BAD_RES | hip.POCKET_BAD_SEGMENT):
        raise hip.KpdError(f'select_pocket_residues: residue indices outside [0, n_atoms) (status {st})')
    if st & hip.POCKET_EMPTY:
        raise ValueError('no valid pocket residues found.')
    if ca_only:
        points = torch.zeros(0, 3, device=dev)
    else:
        out = _points(rec_positions, rec_ptr, sel['pocket_mask'], lig_positions, lig_ptr, interface_distance_threshold,
                      interface_exclusion_threshold)
        if out['status'][0] & hip.POCKET_EMPTY:
            raise InterfacePointException(IndexError('no ligand-receptor pair closer than the distance threshold'))
        points = out['points']
    return sel['rows'].long(), sel['pocket_res'].long(), points


def extract_pockets(rec_pos: torch.Tensor, rec_feat: torch.Tensor, rec_res_idx: torch.Tensor, rec_segments: Sequence[int],
                    lig_pos: torch.Tensor, lig_feat: torch.Tensor, lig_segments: Sequence[int], lig_box_padding: Optional[float] = 6,
                    pocket_cutoff: float = 4, interface_distance_threshold: float = 5, interface_exclusion_threshold: float = 2,
                    other_atoms_mask: Optional[torch.Tensor] = None, probe_mask: Optional[torch.Tensor] = None,
                    emit_mask: Optional[torch.Tensor] = None, candidates: str = 'box', rec_files: Optional[List[str]] = None,
                    lig_files: Optional[List[str]] = None):
    """Pockets and interface points of B structures in one launch sequence, as the processed-dataset dict.

    The structures are flat arrays + segment tables (`rec_segments`, `lig_segments`: B + 1 offsets each): rec_pos [n,3],
    rec_feat [n,F] (element one-hots without the "other" column), rec_res_idx [n] (per structure, in [0, atoms of it)),
    lig_pos [m,3], lig_feat [m,Fl], all on the GPU.
      * CrossDocked form (default): probe = emit = ~other_atoms_mask, box of `lig_box_padding`, candidates='box'
        (interface points from the box atoms, pdbbind_processing.py:142-145).
      * BindingMOAD / byop form: lig_box_padding=None, probe_mask / emit_mask given, candidates='pocket'
        (interface points from the pocket atoms, process_bindingmoad.py:200).
    Returns (data, skipped).  `data` holds rec_pos, rec_feat (bool), rec_res_idx, interface_points ([n,3] fp32, concatenated),
    lig_pos, lig_feat (bool), rec_segments, lig_segments, ip_segments (+ rec_files / lig_files when given) of the complexes
    that were kept, in input order: what `ProteinLigandDataset(processed_data_file=data)` takes.  `skipped` lists
    (index, reason) of the others: no pocket atom or no interface point (upstream skips those too,
    process_crossdocked.py:120-130) or more than 2048 pocket atoms (kpd_build_rec_graph's limit per pocket).
    Sizes are read back once per entry point; there is no host loop over device work."""
    if candidates not in ('box', 'pocket'):
        raise ValueError("candidates must be 'box' or 'pocket'")
    if not (rec_pos.is_cuda and lig_pos.is_cuda):
        raise hip.KpdError('extract_pockets: the structure arrays must live on the GPU; pocket extraction has no CPU implementation')
    dev = rec_pos.device
    rseg = [int(v) for v in torch.as_tensor(rec_segments).tolist()]
    lseg = [int(v) for v in torch.as_tensor(lig_segments).tolist()]
    B = len(rseg) - 1
    if len(lseg) != B + 1 or rseg[0] != 0 or lseg[0] != 0 or rseg[-1] != rec_pos.shape[0] or lseg[-1] != lig_pos.shape[0]:
        raise ValueError('segment tables must be B + 1 offsets covering the arrays')
    rc = [b - a for a, b in zip(rseg[:-1], rseg[1:])]
    lc = [b - a for a, b in zip(lseg[:-1], lseg[1:])]
    if min(rc + lc, default=0) < 0:
        raise ValueError('segment tables must be ascending')
    if max(lc, default=0) > hip.POCKET_MAX_LIG:
        raise hip.KpdError(f'{max(lc)} ligand atoms in one complex: at most {hip.POCKET_MAX_LIG} are supported')
    rec_ptr, lig_ptr = _ptr(rc, dev), _ptr(lc, dev)
    ones = torch.ones(rec_pos.shape[0], dtype=torch.bool, device=dev)
    keep = ones if other_atoms_mask is None else ~other_atoms_mask.to(dev).bool()
    probe = keep if probe_mask is None else probe_mask.to(dev).bool()
    emit = keep if emit_mask is None else emit_mask.to(dev).bool() & keep
    res = rec_res_idx.to(dev).to(torch.int32)
    sel = hip.pocket_select(rec_pos, rec_ptr, res, probe, emit, lig_pos, lig_ptr, max(rc, default=0), lig_box_padding, pocket_cutoff)
    cand = (sel['in_box'] & probe) if candidates == 'box' else sel['pocket_mask']
    ips = _points(rec_pos, rec_ptr, cand, lig_pos, lig_ptr, interface_distance_threshold, interface_exclusion_threshold)
    pptr, iptr = sel['pocket_ptr'], ips['ip_ptr']
    kept, skipped = [], []
    for b in range(B):
        st = sel['status'][b]
        if st & (hip.POCKET_BAD_RES | hip.POCKET_BAD_SEGMENT):
            skipped.append((b, 'residue indices outside [0, n_atoms)'))
        elif pptr[b + 1] == pptr[b]:
            skipped.append((b, 'no pocket atom'))
        elif ips['status'][b] & hip.POCKET_EMPTY:
            skipped.append((b, 'no interface point'))
        elif pptr[b + 1] - pptr[b] > MAX_POCKET_ATOMS:
            skipped.append((b, f'{pptr[b + 1] - pptr[b]} pocket atoms: more than {MAX_POCKET_ATOMS}'))
        else:
            kept.append(b)

    def take(ptr):                      # rows of the kept complexes and their new segment table (host arithmetic on B + 1 numbers)
        idx = [torch.arange(ptr[b], ptr[b + 1]) for b in kept]
        seg = torch.zeros(len(kept) + 1, dtype=torch.long)
        if kept:
            seg[1:] = torch.tensor([ptr[b + 1] - ptr[b] for b in kept]).cumsum(0)
        return (torch.cat(idx) if idx else torch.zeros(0, dtype=torch.long)).to(dev), seg

    prow, rec_seg = take(pptr)
    irow, ip_seg = take(iptr)
    lrow, lig_seg = take(lseg)
    rows = sel['rows'].long()[prow]
    data = dict(rec_pos=rec_pos[rows].float(), rec_feat=rec_feat[rows].bool(), rec_res_idx=sel['pocket_res'].long()[prow],
                interface_points=ips['points'][irow], lig_pos=lig_pos[lrow].float(), lig_feat=lig_feat[lrow].bool(),
                rec_segments=rec_seg, lig_segments=lig_seg, ip_segments=ip_seg)
    if rec_files is not None:
        data['rec_files'] = [rec_files[b] for b in kept]
    if lig_files is not None:
        data['lig_files'] = [lig_files[b] for b in kept]
    return data, skipped
