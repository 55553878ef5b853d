"""Molecules from sampled ligands, computed on the GPU: bonds, valences, fragments, sample-quality metrics, SDF text.

The array-level part of what the reference does after the reverse loop: `make_mol_openbabel` (analysis/molecule_builder.py:38-60,
a per-ligand XYZ string round trip through openbabel), `check_atom_valency` and `compute_avg_frag_size`
(analysis/metrics.py:156-206, over rdkit molecules), the atom-type KL divergence (`LigandTypeDistribution.kl_divergence`,
:225-236) and the SDF writing of sample.py / test.py.  Here it is one batched call for all ligands (`kpd_mol_perceive`,
`kpd_sdf_emit`, csrc/molecule.hip), and the metrics are torch reductions over the device tensors it returns.

The numbers about the SET of samples are here too: `uniqueness` and `novelty` (analysis/metrics.py:135-147) and the Tanimoto
`diversity` of a pocket's samples (`MoleculeProperties.calculate_diversity`, :263-277).  Upstream compares canonical SMILES
and RDKit fingerprints; here a key that is equal for isomorphic bond graphs and a substructure bit vector are computed from
the bond graph on the device (`kpd_mol_keys`, `kpd_fp_diversity`, csrc/molset.hip; include/kpd.h is their definition), and
the set operations are torch calls.  A key describes the constitution only (no stereo) and, unless `with_orders=False`,
inherits the length-class bond orders.

openbabel's perception rules are not restated: include/kpd.h defines the rule used here, the lookup-table builder of the
EDM / DiffSBDD lineage (covalent radii for connectivity, length classes for the bond orders, valence caps).  The bond orders
are length classes, not a Kekule structure; connectivity, fragments and `metrics` do not depend on them.  What needs
sanitisation, a force field or a docking program (`validity`, QED / SA, UFF relaxation, docking) stays with the caller, who
can read the SDF blocks with rdkit.  There is no CPU implementation: tensors must live on the GPU and the HIP library must be
present.
"""
from typing import Dict, List, Optional, Sequence

import torch

from . import hip

# atomic numbers of the element symbols a dataset may name (lig_elements / rec_elements of the configs, upstream's allowed_bonds)
ATOMIC_NUMBERS: Dict[str, int] = {
    'H': 1, 'He': 2, 'Li': 3, 'Be': 4, 'B': 5, 'C': 6, 'N': 7, 'O': 8, 'F': 9, 'Ne': 10, 'Na': 11, 'Mg': 12, 'Al': 13, 'Si': 14,
    'P': 15, 'S': 16, 'Cl': 17, 'Ar': 18, 'K': 19, 'Ca': 20, 'Sc': 21, 'Ti': 22, 'V': 23, 'Cr': 24, 'Mn': 25, 'Fe': 26, 'Co': 27,
    'Ni': 28, 'Cu': 29, 'Zn': 30, 'Ga': 31, 'Ge': 32, 'As': 33, 'Se': 34, 'Br': 35, 'Kr': 36, 'Rb': 37, 'Sr': 38, 'Y': 39,
    'Zr': 40, 'Nb': 41, 'Mo': 42, 'Tc': 43, 'Ru': 44, 'Rh': 45, 'Pd': 46, 'Ag': 47, 'Cd': 48, 'In': 49, 'Sn': 50, 'Sb': 51,
    'Te': 52, 'I': 53, 'Xe': 54, 'Cs': 55, 'Ba': 56, 'W': 74, 'Pt': 78, 'Au': 79, 'Hg': 80, 'Pb': 82, 'Bi': 83,
}

# the largest number of bonds upstream allows per element (constants.py `allowed_bonds`, maxima of the lists); `check_atom_valency`
# counts an atom with more, or with none, as invalid.  Not the valence caps of the bond rule (include/kpd.h): S is 4 here, 6 there.
ALLOWED_BONDS: Dict[str, int] = {'H': 1, 'C': 4, 'N': 3, 'O': 2, 'F': 1, 'B': 3, 'Al': 3, 'Si': 4, 'P': 5, 'S': 4, 'Cl': 1, 'As': 3,
                                 'Br': 1, 'I': 1, 'Hg': 2, 'Bi': 5}

EPS = 1e-10         # LigandTypeDistribution.EPS


class Molecules:
    """The perceived molecules of a batch of ligands, as device tensors:
    elem [N] (element class of every atom), valence [N], frag [N] (rank of the atom's fragment inside its ligand), bonds [3N,2]
    (global atom rows, i < j, per ligand sorted; ligand b's are rows bond_ptr[b] : bond_ptr[b+1], the rows from bond_ptr[B] on are
    unused capacity), order [3N] (length classes 1 / 2 / 3), bond_ptr [B+1], summary [B,4] =
    {n_bonds, n_frags, largest_frag_atoms, n_invalid_atoms}, status [B] (bits: 1 empty, 2 bond capacity, 4 non-finite coordinate
    or unknown element, 8 left out: malformed or more than 256 atoms), lig_ptr [B+1].  Atoms of a ligand that was left out
    read -1 in elem / valence / frag."""

    def __init__(self, lig_ptr: torch.Tensor, summary: torch.Tensor, status: torch.Tensor, elem: Optional[torch.Tensor] = None,
                 valence: Optional[torch.Tensor] = None, frag: Optional[torch.Tensor] = None, bonds: Optional[torch.Tensor] = None,
                 order: Optional[torch.Tensor] = None, bond_ptr: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None,
                 lig_elements: Optional[Sequence[str]] = None):
        self.lig_ptr, self.summary, self.status = lig_ptr, summary, status
        self.elem, self.valence, self.frag, self.bonds, self.order, self.bond_ptr = elem, valence, frag, bonds, order, bond_ptr
        self.pos, self.lig_elements = pos, None if lig_elements is None else list(lig_elements)

    def __len__(self) -> int:
        return int(self.lig_ptr.numel()) - 1

    def sdf(self, largest_frag: bool = False, strict: bool = True) -> List[str]:
        """One MOL V2000 block (closed by `$$$$`) per ligand, written on the GPU; `largest_frag`: only the largest fragment,
        renumbered (upstream's `process_molecule(largest_frag=True)`).  A ligand that has no block (left out, a non-finite
        coordinate, a coordinate that does not fit `%10.4f`) raises; with `strict=False` its entry is the empty string."""
        if self.pos is None or self.lig_elements is None or self.bonds is None:
            raise hip.KpdError('these Molecules carry no coordinates: build them with build_molecules')
        if len(self) == 0:
            return []
        mol = dict(elem=self.elem, frag=self.frag, bonds=self.bonds, order=self.order, bond_ptr=self.bond_ptr, status=self.status)
        text, ptr, status = hip.sdf_emit(self.pos, self.lig_ptr, self.lig_elements, mol, largest_only=largest_frag)
        bad = [(b, s) for b, s in enumerate(status) if s]
        if bad and strict:
            raise hip.KpdError(f'sdf: no block for ligand {bad[0][0]} (status {bad[0][1]}: 1 non-finite coordinate, 2 coordinate wider '
                               f'than %10.4f, 4 no molecule, 8 text capacity); {len(bad)} of {len(status)} ligands affected')
        return ['' if status[b] else text[ptr[b]:ptr[b + 1]].decode('ascii') for b in range(len(status))]

    def metrics(self, type_counts: Optional[torch.Tensor] = None, connectivity_thresh: float = 0.5) -> Dict[str, float]:
        """Upstream's sample-quality numbers that need no SMILES (analysis/metrics.py), reduced in torch on the tensors' device:
        atom_validity = 1 - invalid atoms / atoms (`check_atom_valency`), avg_frag_frac = mean of largest fragment atoms / atoms
        (`compute_avg_frag_size`), connectivity = share of ligands with that ratio >= `connectivity_thresh`, and, when the
        training set's `type_counts` [F] are given, atom_type_kldiv (`LigandTypeDistribution.kl_divergence`, its EPS included,
        in float64).  Upstream computes `connectivity` over the molecules rdkit could sanitise; here it is over all ligands.
        Ligands that are empty or were left out do not count, as upstream skips a molecule it could not build; with no ligand
        left every number is upstream's 0.0."""
        n = (self.lig_ptr[1:] - self.lig_ptr[:-1]).double()
        use = (n > 0) & ((self.status & hip.MOL_BAD_SEGMENT) == 0)
        if not bool(use.any()):
            out = dict(atom_validity=0.0, avg_frag_frac=0.0, connectivity=0.0)
        else:
            n, s = n[use], self.summary[use].double()
            frac = s[:, 2] / n
            res = torch.stack([1 - s[:, 3].sum() / n.sum(), frac.mean(), (frac >= connectivity_thresh).double().mean()]).tolist()
            out = dict(atom_validity=res[0], avg_frag_frac=res[1], connectivity=res[2])
        if type_counts is not None:
            if self.elem is None:
                raise hip.KpdError('atom_type_kldiv needs the element classes (elem)')
            counts = torch.as_tensor(type_counts).to(self.elem.device).double().flatten()
            p = counts / counts.sum()
            e = self.elem[self.elem >= 0].long()
            if e.numel() and int(e.max()) >= p.numel():
                raise ValueError(f'type_counts has {p.numel()} entries, the samples use class {int(e.max())}')
            q = torch.bincount(e, minlength=p.numel()).double()
            q = q / q.sum()
            out['atom_type_kldiv'] = float(-torch.sum(p * torch.log(q / (p + EPS) + EPS)))
        return out

    def _keys(self, largest_frag: bool, with_orders: bool, radius: int = 2, nbits: int = 2048) -> Dict[str, torch.Tensor]:
        if self.lig_elements is None or self.bonds is None:
            raise hip.KpdError('these Molecules carry no bond graph: build them with build_molecules')
        if len(self) == 0:
            dev = self.lig_ptr.device
            return dict(key=torch.zeros(0, dtype=torch.int64, device=dev), fp=torch.zeros(0, int(nbits) // 32, dtype=torch.int32, device=dev),
                        status=torch.zeros(0, dtype=torch.int32, device=dev))
        mol = dict(elem=self.elem, frag=self.frag, bonds=self.bonds, order=self.order, bond_ptr=self.bond_ptr, status=self.status)
        z = [ATOMIC_NUMBERS.get(el, 0) for el in self.lig_elements]
        return hip.mol_keys(self.lig_ptr, z, mol, largest_only=largest_frag, with_orders=with_orders, radius=radius, nbits=nbits)

    def keys(self, largest_frag: bool = True, with_orders: bool = True) -> torch.Tensor:
        """One int64 per ligand that is equal for isomorphic bond graphs and different otherwise (the key of include/kpd.h,
        computed on the GPU): what upstream uses canonical SMILES for.  `largest_frag`: of the largest fragment, as upstream
        takes the SMILES of (`compute_connectivity`); `with_orders=False`: of the connectivity alone, independent of the
        length-class bond orders.  Constitution only: no stereo.  A ligand without a molecule (empty, left out) has key 0."""
        return self._keys(largest_frag, with_orders)['key']

    def fingerprints(self, radius: int = 2, nbits: int = 2048, largest_frag: bool = True, with_orders: bool = True) -> torch.Tensor:
        """Substructure bit vectors [B, nbits/32] int32 (the fingerprint of include/kpd.h): one bit per atom and per
        neighbourhood radius 0 .. `radius`; all zero for a ligand without a molecule."""
        return self._keys(largest_frag, with_orders, radius, nbits)['fp']

    def set_metrics(self, group_ptr: Optional[torch.Tensor] = None, train_keys: Optional[torch.Tensor] = None,
                    connectivity_thresh: float = 0.5, radius: int = 2, nbits: int = 2048, largest_frag: bool = True,
                    with_orders: bool = True) -> Dict[str, object]:
        """Upstream's numbers about the set of samples, from keys and fingerprints instead of SMILES and RDKit fingerprints:
        uniqueness = distinct keys / connected ligands (`compute_uniqueness`, analysis/metrics.py:135-140; "connected": has a
        molecule and largest fragment atoms / atoms >= `connectivity_thresh`, `compute_connectivity` without the sanitisation
        step before it, as in `metrics`), novelty = share of those distinct keys that are not in `train_keys`
        (`compute_novelty`; only when `train_keys`, e.g. from `training_keys`, is given), and with `group_ptr` [G+1] (int32
        offsets: consecutive ligands of a pocket form a group) diversity_per_group [G] (float64 device tensor: the mean
        Tanimoto distance over the pairs of a group's ligands that have a molecule, 0.0 for fewer than two,
        `MoleculeProperties.calculate_diversity`), diversity (its mean) and diversity_std (`np.std`, as upstream prints).
        An empty set gives upstream's 0.0."""
        r = self._keys(largest_frag, with_orders, radius, nbits)
        has = (r['status'] & hip.KEY_NO_MOLECULE) == 0
        n = (self.lig_ptr[1:] - self.lig_ptr[:-1]).double()
        connected = has & (self.summary[:, 2].double() / n >= connectivity_thresh)
        keys = r['key'][connected]
        distinct = torch.unique(keys)
        out: Dict[str, object] = dict(uniqueness=distinct.numel() / keys.numel() if keys.numel() else 0.0)
        if train_keys is not None:
            known = torch.isin(distinct, torch.as_tensor(train_keys, dtype=torch.int64).to(distinct.device))
            out['novelty'] = float((~known).double().mean()) if distinct.numel() else 0.0
        if group_ptr is not None:
            group_ptr = torch.as_tensor(group_ptr, dtype=torch.int32).to(self.lig_ptr.device).contiguous()
            if group_ptr.numel() < 2 or len(self) == 0:           # no groups, or no ligands in them
                per_group = torch.zeros(max(group_ptr.numel() - 1, 0), dtype=torch.float64, device=group_ptr.device)
            else:
                div_sum, n_pairs, status = hip.fp_diversity(r['fp'], has, group_ptr)
                if bool(status.any()):
                    raise hip.KpdError(f'set_metrics: group_ptr must be ascending offsets into the {len(self)} ligands')
                per_group = torch.where(n_pairs > 0, div_sum / n_pairs.clamp(min=1).double(), torch.zeros_like(div_sum))
            out['diversity_per_group'] = per_group
            out['diversity'] = float(per_group.mean()) if per_group.numel() else 0.0
            out['diversity_std'] = float(per_group.std(unbiased=False)) if per_group.numel() else 0.0
        return out


def _class_tables(lig_elements: Sequence[str], allowed_bonds: Optional[Dict[str, object]]):
    allowed_bonds = ALLOWED_BONDS if allowed_bonds is None else allowed_bonds
    z, allowed = [], []
    for el in lig_elements:
        z.append(ATOMIC_NUMBERS.get(el, 0))                 # 0: unknown to the bond rule, never bonded, always invalid
        a = allowed_bonds.get(el, 0)
        allowed.append(int(a) if isinstance(a, int) else int(max(a)))       # metrics.py:180-183
    return z, allowed


def build_molecules(lig_pos: List[torch.Tensor], lig_feat: List[torch.Tensor], lig_elements: Sequence[str],
                    allowed_bonds: Optional[Dict[str, object]] = None) -> Molecules:
    """Perceive the molecules of all sampled ligands in one batched call.  `lig_pos` / `lig_feat`: the lists every sampling entry
    point returns ([n_i,3] and [n_i,F] per ligand, still on the GPU), `lig_elements`: the F element symbols of the feature
    columns, `allowed_bonds`: element -> largest valence (or a list of valences) for the validity count, upstream's table by
    default."""
    if len(lig_pos) != len(lig_feat):
        raise ValueError('lig_pos and lig_feat must have one entry per ligand')
    z, allowed = _class_tables(lig_elements, allowed_bonds)
    if not lig_pos:
        e = torch.zeros(0, dtype=torch.int32)
        return Molecules(torch.zeros(1, dtype=torch.int32), e.reshape(0, 4), e, e, e, e, e.reshape(0, 2), e, torch.zeros(1, dtype=torch.int32),
                         None, lig_elements)
    sizes = [int(p.shape[0]) for p in lig_pos]
    pos = torch.cat([p.reshape(-1, 3) for p in lig_pos])
    feat = torch.cat(list(lig_feat))
    if not pos.is_cuda:
        raise hip.KpdError(f'ligands must live on the GPU (got {pos.device}); molecule building has no CPU implementation')
    ptr = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0).to(torch.int32).to(pos.device)
    if feat.dim() != 2 or feat.shape[1] != len(lig_elements):
        raise hip.KpdError(f'features {tuple(feat.shape)} do not match the {len(lig_elements)} element symbols')
    m = hip.mol_perceive(pos, feat, ptr, z, allowed)
    return Molecules(ptr, m['summary'], m['status'], m['elem'], m['valence'], m['frag'], m['bonds'], m['order'], m['bond_ptr'],
                     hip._dev_f32(pos, 'pos'), lig_elements)


def training_keys(lig_pos: List[torch.Tensor], lig_feat: List[torch.Tensor], lig_elements: Sequence[str], largest_frag: bool = True,
                  with_orders: bool = True) -> torch.Tensor:
    """The keys of the training ligands as a sorted int64 tensor without repeats, for `set_metrics(train_keys=...)`.
    `lig_pos` / `lig_feat`: the processed dataset's ligand coordinates and one-hot features (GPU tensors, as for
    `build_molecules`).  The ligands are perceived by the same rule as the samples, so novelty compares like with like; pass
    the `largest_frag` / `with_orders` the samples' keys will be computed with.  Ligands without a molecule are left out."""
    mols = build_molecules(lig_pos, lig_feat, lig_elements)
    r = mols._keys(largest_frag, with_orders)
    return torch.unique(r['key'][(r['status'] & hip.KEY_NO_MOLECULE) == 0])


def analyze_samples(samples: List[dict], lig_elements: Sequence[str], type_counts: Optional[torch.Tensor] = None,
                    allowed_bonds: Optional[Dict[str, object]] = None, connectivity_thresh: float = 0.5, device=None,
                    train_keys: Optional[torch.Tensor] = None, set_metrics: bool = False) -> Dict[str, float]:
    """The part of `ModelAnalyzer.sample_and_analyze` (analysis/metrics.py:60-100) that needs no rdkit: `samples` is the list
    of {'positions', 'features'} dicts `_sample` returns, one per pocket; the result is `Molecules.metrics` over all of them
    and, with `set_metrics=True`, `Molecules.set_metrics` as well (uniqueness, novelty against `train_keys` if given, and the
    diversity of every pocket's ligands).
    `_sample` hands its ligands back on the host: name the GPU to work on as `device` and they are copied there (one copy of
    the concatenated batch would do as well: `build_molecules` takes GPU tensors only and never computes on the host)."""
    lig_pos, lig_feat = [], []
    for rec in samples:
        lig_pos.extend(rec['positions'])
        lig_feat.extend(rec['features'])
    if device is not None:
        lig_pos, lig_feat = [p.to(device) for p in lig_pos], [f.to(device) for f in lig_feat]
    mols = build_molecules(lig_pos, lig_feat, lig_elements, allowed_bonds)
    out = mols.metrics(type_counts, connectivity_thresh)
    if set_metrics:
        group_ptr = torch.tensor([0] + [len(rec['positions']) for rec in samples], dtype=torch.int64).cumsum(0).to(torch.int32)
        out.update(mols.set_metrics(group_ptr, train_keys, connectivity_thresh))
    return out
