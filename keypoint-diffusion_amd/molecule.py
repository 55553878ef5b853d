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
are length classes, not a Kekule structure; connectivity, fragments and `metrics` do not depend on them.  `Molecules.sanitize`
(`kpd_mol_sanitize`, csrc/sanitize.hip) adds what upstream gets from Chem.SanitizeMol and MoleculeProperties: ring and aromaticity
perception, Kekule bond orders, implicit hydrogen counts, `validity` and molecular weight / donors / acceptors / rotatable bonds /
Lipinski count, by a rule include/kpd.h defines (NOT RDKit's, and not compared with it).  QED, SA and logP need RDKit's parameter
files and stay with the caller, who can read the SDF blocks with rdkit.  `Sanitized.add_hs` (`kpd_mol_add_hs`, csrc/hydrogens.hip)
turns the hydrogen counts into atoms with coordinates and bonds, where upstream calls Chem.AddHs(lig, addCoords=True): ideal sites by a
rule include/kpd.h defines, NOT RDKit's coordinates; the result is a `Molecules` every call below takes unchanged.  The scoring half of docking is here: `Molecules.vina_score` / `score_samples` evaluate the AutoDock Vina
FUNCTIONAL FORM (five pair terms over ligand x pocket heavy atoms, divided by 1 + w_rot N_rot) with its analytic gradient for the
whole batch in one launch (`kpd_vina_score`, csrc/vina.hip).  The typing is a rule of this library's own, defined in
include/kpd.h (no hydrogens, no aromaticity), and the weights and radii are recalled constants: the scores rank samples scored
here against each other and ARE NOT gnina's or Vina's numbers.  That call scores the poses it is given; `Molecules.vina_minimize`
/ `minimize_samples` minimise them under the function and `Molecules.vina_dock` / `dock_samples` search for poses under it
(`kpd_vina_minimize`, `kpd_vina_dock`): this library's own minimiser and search, defined in include/kpd.h, NOT gnina's.

Where upstream minimises every sample inside its pocket with RDKit's UFF (analysis/pocket_minimization.py), `Molecules.relax` /
`relax_samples` relax the whole batch in one kernel launch (`kpd_relax`, csrc/relax.hip) with a force field of this library's
own, defined in include/kpd.h: harmonic bonds and angles around the ideal values nearest to the sampled geometry, soft-core
Lennard-Jones inside the ligand and against the pocket, L-BFGS.  It is NOT UFF: heavy atoms only (unless the molecules of
`Sanitized.add_hs` are passed, `relax_samples(add_hs=True)`), no torsions or inversions,
no electrostatics, a rigid pocket.  Its energies rank samples relaxed here against each other; they are not comparable with
RDKit's, and whoever needs UFF itself still runs RDKit on the SDF blocks.

There is no CPU implementation: tensors must live on the GPU and the HIP library must be present.
"""
from typing import Dict, List, Optional, Sequence

import torch

from . import hip, smarts

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

# van der Waals parameters for `Molecules.relax`, element -> (x in Angstrom, D in kcal/mol), in the form of the UFF table of Rappe
# et al. 1992.  RECALLED, NOT CHECKED AGAINST THE PAPER: nothing may rely on these being UFF's values; pass `vdw=` to override.
VDW_PARAMS: Dict[str, tuple] = {
    'H': (2.886, 0.044), 'B': (4.083, 0.180), 'C': (3.851, 0.105), 'N': (3.660, 0.069), 'O': (3.500, 0.060), 'F': (3.364, 0.050),
    'Na': (2.983, 0.030), 'Mg': (3.021, 0.111), 'Si': (4.295, 0.402), 'P': (4.147, 0.305), 'S': (4.035, 0.274), 'Cl': (3.947, 0.227),
    'K': (3.812, 0.035), 'Ca': (3.399, 0.238), 'Mn': (2.961, 0.013), 'Fe': (2.912, 0.013), 'Co': (2.872, 0.014), 'Ni': (2.834, 0.015),
    'Cu': (3.495, 0.005), 'Zn': (2.763, 0.124), 'As': (4.230, 0.309), 'Se': (4.205, 0.291), 'Br': (4.189, 0.251), 'I': (4.500, 0.339),
}


def vdw_table(elements: Sequence[str], vdw: Optional[Dict[str, tuple]] = None) -> List[List[float]]:
    """[{x, D}] for the element symbols, from `vdw` first and VDW_PARAMS second; an element in neither raises."""
    rows = []
    for el in elements:
        row = (vdw or {}).get(el, VDW_PARAMS.get(el))
        if row is None:
            raise hip.KpdError(f'relax: no van der Waals parameters for element {el!r}; pass vdw={{{el!r}: (x, D)}}')
        x, d = float(row[0]), float(row[1])
        if not (0 < x < float('inf') and 0 <= d < float('inf')):
            raise hip.KpdError(f'relax: van der Waals parameters of {el!r} must be x > 0 and D >= 0 (got {row!r})')
        rows.append([x, d])
    return rows


# surface radii for `Molecules.vina_score`, element -> Angstrom, in the form of Vina's "xs" radii (1.2 for the metals the typing
# rule knows).  RECALLED, NOT CHECKED AGAINST TROTT & OLSON 2010 OR VINA'S SOURCE: nothing may rely on these being Vina's values;
# pass `radii=` to override.
XS_RADII: Dict[str, float] = {
    'C': 1.9, 'N': 1.8, 'O': 1.7, 'F': 1.5, 'Si': 2.2, 'P': 2.1, 'S': 2.0, 'Cl': 1.8, 'Br': 2.0, 'I': 2.2,
    'Mg': 1.2, 'Ca': 1.2, 'Mn': 1.2, 'Fe': 1.2, 'Co': 1.2, 'Ni': 1.2, 'Cu': 1.2, 'Zn': 1.2,
    'H': 1.0,       # never enters the score: see xs_radius_table
}


def xs_radius_table(elements: Sequence[str], radii: Optional[Dict[str, float]] = None) -> List[float]:
    """The radius of every element symbol, from `radii` first and XS_RADII second; an element in neither raises.  A radius of 0
    is allowed: such an atom takes no part in the score (kpd_vina_score reports it with type -1 and status bit 2).
    'H' has an entry so that the class list of hydrogenated molecules (`Sanitized.add_hs`) passes; it holds for ligand and pocket
    class lists alike (a list naming 'H' used to raise here), and its value never enters a score: kpd_vina_score and
    kpd_vina_pocket_types give every hydrogen type -1 whatever its radius."""
    out = []
    for el in elements:
        r = (radii or {}).get(el, XS_RADII.get(el))
        if r is None:
            raise hip.KpdError(f'vina_score: no radius for element {el!r}; pass radii={{{el!r}: R}}')
        r = float(r)
        if not 0 <= r < float('inf'):
            raise hip.KpdError(f'vina_score: the radius of {el!r} must be finite and >= 0 (got {r!r})')
        out.append(r)
    return out


# van der Waals radii for `Sanitized.pose_check`, element -> Angstrom, in the form of Bondi 1964 (with later values where Bondi has
# none).  RECALLED, NOT CHECKED AGAINST THE PAPER: nothing may rely on these being Bondi's values; pass `radii=` to override.
VDW_RADII: Dict[str, float] = {
    'H': 1.2, 'B': 1.92, 'C': 1.7, 'N': 1.55, 'O': 1.52, 'F': 1.47, 'Na': 2.27, 'Mg': 1.73, 'Si': 2.1, 'P': 1.8, 'S': 1.8, 'Cl': 1.75,
    'K': 2.75, 'Ca': 2.31, 'Mn': 2.05, 'Fe': 2.04, 'Co': 2.0, 'Ni': 1.63, 'Cu': 1.4, 'Zn': 1.39, 'As': 1.85, 'Se': 1.9, 'Br': 1.85, 'I': 1.98,
}


def vdw_radius_table(elements: Sequence[str], radii: Optional[Dict[str, float]] = None, with_h: bool = False) -> List[float]:
    """The van der Waals radius of every element symbol, from `radii` first and VDW_RADII second; an element in neither raises.
    'H' gets 0 unless `with_h` (or `radii` names it): a radius of 0 keeps an atom out of the clash and overlap checks of
    kpd_pose_check.  At most hip.CHECK_MAX_RADIUS."""
    out = []
    for el in elements:
        r = (radii or {}).get(el, 0.0 if el == 'H' and not with_h else VDW_RADII.get(el))
        if r is None:
            raise hip.KpdError(f'pose_check: no van der Waals radius for element {el!r}; pass radii={{{el!r}: R}}')
        r = float(r)
        if not 0 <= r <= hip.CHECK_MAX_RADIUS:
            raise hip.KpdError(f'pose_check: the radius of {el!r} must be in 0 .. {hip.CHECK_MAX_RADIUS} (got {r!r})')
        out.append(r)
    return out


# monoisotopic masses for `Molecules.sanitize`, element -> u, to stand where upstream calls Descriptors.ExactMolWt.  RECALLED, NOT
# CHECKED AGAINST A TABLE OF NUCLIDES: nothing may rely on the last digits; pass `masses=` to override.
MONOISOTOPIC_MASS: Dict[str, float] = {
    'H': 1.00782503223, 'B': 11.00930536, 'C': 12.0, 'N': 14.00307400443, 'O': 15.99491461957, 'F': 18.99840316273,
    'Si': 27.97692653465, 'P': 30.97376199842, 'S': 31.9720711744, 'Cl': 34.968852682, 'As': 74.92159457, 'Se': 79.9165218,
    'Br': 78.9183376, 'I': 126.9044719,
}


def mass_table(elements: Sequence[str], masses: Optional[Dict[str, float]] = None):
    """(the mass of every element symbol, the mass of hydrogen), from `masses` first and MONOISOTOPIC_MASS second; an element in
    neither raises."""
    out = []
    for el in list(elements) + ['H']:
        m = (masses or {}).get(el, MONOISOTOPIC_MASS.get(el))
        if m is None:
            raise hip.KpdError(f'sanitize: no mass for element {el!r}; pass masses={{{el!r}: m}}')
        m = float(m)
        if not 0 <= m < 1e6:
            raise hip.KpdError(f'sanitize: the mass of {el!r} must be finite and >= 0 (got {m!r})')
        out.append(m)
    return out[:-1], out[-1]


def _pocket_of(pocket_of, B: int, n_pockets: int, dev) -> torch.Tensor:
    """The pocket of every ligand as an int32 tensor on `dev`: all zeros when one pocket is given and `pocket_of` is None."""
    if pocket_of is None:
        if n_pockets != 1:
            raise ValueError(f'pocket_of is needed to tell which of the {n_pockets} pockets every ligand sits in')
        return torch.zeros(B, dtype=torch.int32, device=dev)
    host = torch.as_tensor(pocket_of).cpu().flatten()
    if host.numel() != B or (host.numel() and (int(host.min()) < -1 or int(host.max()) >= n_pockets)):
        raise ValueError(f'pocket_of must name one of the {n_pockets} pockets (or -1) for each of the {B} ligands')
    return host.to(torch.int32).to(dev)


def _zeros(dev, **spec) -> Dict[str, torch.Tensor]:
    """What a call on no ligands returns: name -> zeros of (dtype, *shape) on `dev`."""
    return {name: torch.zeros(shape, dtype=dtype, device=dev) for name, (dtype, *shape) in spec.items()}


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
                 lig_elements: Optional[Sequence[str]] = None, max_atoms: Optional[int] = None, sizes: Optional[List[int]] = None):
        self.lig_ptr, self.summary, self.status = lig_ptr, summary, status
        self.elem, self.valence, self.frag, self.bonds, self.order, self.bond_ptr = elem, valence, frag, bonds, order, bond_ptr
        self.pos, self.lig_elements = pos, None if lig_elements is None else list(lig_elements)
        self._sizes = None if sizes is None else list(sizes)           # host-known atoms per ligand, if the builder knew them
        self.valid: Optional[torch.Tensor] = None                      # [B] bool, on the molecules `sanitize` returns
        self._allowed: Optional[List[int]] = None                      # the validity table the builder used, if it knew one
        self._allowed_h: Optional[int] = None                          # the entry for 'H' of the caller's table, if it has one
        self._max_atoms = max_atoms if max_atoms is not None or not self._sizes else max(self._sizes)

    def __len__(self) -> int:
        return int(self.lig_ptr.numel()) - 1

    def _mol(self) -> Dict[str, torch.Tensor]:
        """These molecules as the `mol` the `hip` wrappers take: the entries of `hip.MOL_LENGTHS`.  A wrapper checks and reads the
        entries it names, so the same dict serves all of them."""
        return dict(elem=self.elem, valence=self.valence, frag=self.frag, bonds=self.bonds, order=self.order, bond_ptr=self.bond_ptr,
                    status=self.status)

    @classmethod
    def from_sdf(cls, files, lig_elements: Sequence[str], remove_hydrogen: bool = True, allowed_bonds: Optional[Dict[str, object]] = None,
                 device='cuda') -> 'Molecules':
        """The molecules of SDF / MOL V2000 files, with the bonds the files state: `structure.read_sdf`."""
        from . import structure
        return structure.read_sdf(files, lig_elements, remove_hydrogen=remove_hydrogen, allowed_bonds=allowed_bonds, device=device)

    def sdf(self, largest_frag: bool = False, strict: bool = True) -> List[str]:
        """One MOL V2000 block (closed by `$$$$`) per ligand, written on the GPU; `largest_frag`: only the largest fragment,
        renumbered (upstream's `process_molecule(largest_frag=True)`).  A ligand that has no block (left out, a non-finite
        coordinate, a coordinate that does not fit `%10.4f`) raises; with `strict=False` its entry is the empty string."""
        if self.pos is None or self.lig_elements is None or self.bonds is None:
            raise hip.KpdError('these Molecules carry no coordinates: build them with build_molecules')
        if len(self) == 0:
            return []
        text, ptr, status = hip.sdf_emit(self.pos, self.lig_ptr, self.lig_elements, self._mol(), largest_only=largest_frag)
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
        in float64).  Upstream computes `connectivity` over the molecules rdkit could sanitise; here it is over all ligands
        (`sanitize().metrics()` gives upstream's order of operations, `validity` first).
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
            return _zeros(self.lig_ptr.device, key=(torch.int64, 0), fp=(torch.int32, 0, int(nbits) // 32), status=(torch.int32, 0))
        z = [ATOMIC_NUMBERS.get(el, 0) for el in self.lig_elements]
        return hip.mol_keys(self.lig_ptr, z, self._mol(), largest_only=largest_frag, with_orders=with_orders, radius=radius, nbits=nbits)

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

    def _pose_stack(self, pos) -> torch.Tensor:
        """[N,3], [K,N,3] or a list of per-ligand [n_i,3] / [K,n_i,3] tensors -> [K,N,3]."""
        if isinstance(pos, (list, tuple)):
            if len(pos) != len(self):
                raise hip.KpdError(f'pose_rmsd: {len(pos)} per-ligand tensors for {len(self)} ligands')
            parts = [p if p.dim() == 3 else p[None] for p in pos]
            pos = torch.cat(parts, dim=1) if parts else torch.zeros(1, 0, 3, device=self.lig_ptr.device)
        if not isinstance(pos, torch.Tensor) or pos.dim() not in (2, 3) or pos.shape[-1] != 3:
            raise hip.KpdError('pose_rmsd: pos must be [N,3], [K,N,3] or a list of per-ligand tensors')
        return pos if pos.dim() == 3 else pos[None]

    def pose_rmsd(self, pos, ref=None, largest_frag: bool = False, skip_h: bool = True, pairs: bool = False, max_nodes: int = 65536,
                  bond_label: Optional[torch.Tensor] = None, atom_label: Optional[torch.Tensor] = None) -> 'PoseRMSD':
        """The symmetry-corrected RMSD of poses of these molecules, on the GPU (`kpd_pose_rmsd`): the minimum over the automorphisms
        of the bond graph of the unaligned RMSD, what upstream reads off `Chem.CalcRMS` (analysis/pocket_minimization.py), under
        the rule of include/kpd.h; no agreement with RDKit's numbers is claimed.  A flipped phenyl ring or a carboxylate turned by
        one step is the same pose: its value is 0 where the plain atom-by-atom number reports 1 - 2.5 A.
        `pos`: [N,3], [K,N,3] or a list of per-ligand tensors, K poses of the whole batch; `ref`: the pose they are compared with,
        these molecules' own `pos` by default; `pairs=True` (K <= 64): every pose against every other instead; `largest_frag`:
        over the largest fragment alone; `skip_h`: hydrogens take no part; `bond_label` [3N] / `atom_label` [N]: int32 labels an
        automorphism must keep (None: elements and connectivity only, so that the two Kekule patterns of a ring are one graph)."""
        if self.lig_elements is None or self.bonds is None:
            raise hip.KpdError('these Molecules carry no bond graph: build them with build_molecules')
        stack = self._pose_stack(pos)
        K = int(stack.shape[0])
        if K < 1 or (pairs and K > hip.POSE_MAX_PAIR_POSES):
            raise hip.KpdError(f'pose_rmsd: {K} poses; at least 1, and at most {hip.POSE_MAX_PAIR_POSES} with pairs=True')
        if not stack.is_cuda:
            raise hip.KpdError(f'pose_rmsd: poses must live on the GPU (got {stack.device}); there is no CPU implementation')
        if not pairs:
            ref = self.pos if ref is None else ref
            if ref is None:
                raise hip.KpdError('these Molecules carry no coordinates: pass ref')
            ref = self._pose_stack(ref)[0]
        dev = stack.device
        if len(self) == 0:
            shape = (0, K, K) if pairs else (0, K)
            return PoseRMSD(_zeros(dev, rmsd=(torch.float64, *shape), plain=(torch.float64, *shape), nodes=(torch.int64, *shape),
                                   status=(torch.int32, 0), **({} if pairs else dict(map=(torch.int32, K, 0)))), bool(pairs))
        z = [ATOMIC_NUMBERS.get(el, 0) for el in self.lig_elements]
        out = hip.pose_rmsd(self.lig_ptr, z, self._mol(), stack, None if pairs else ref, pairs=pairs, largest_only=largest_frag, skip_h=skip_h,
                            max_nodes=max_nodes, bond_label=bond_label, atom_label=atom_label)
        return PoseRMSD(out, bool(pairs))

    def set_metrics(self, group_ptr: Optional[torch.Tensor] = None, train_keys: Optional[torch.Tensor] = None,
                    connectivity_thresh: float = 0.5, radius: int = 2, nbits: int = 2048, largest_frag: bool = True,
                    with_orders: bool = True, valid_only: bool = False) -> Dict[str, object]:
        """Upstream's numbers about the set of samples, from keys and fingerprints instead of SMILES and RDKit fingerprints:
        uniqueness = distinct keys / connected ligands (`compute_uniqueness`, analysis/metrics.py:135-140; "connected": has a
        molecule and largest fragment atoms / atoms >= `connectivity_thresh`, `compute_connectivity` without the sanitisation
        step before it, as in `metrics`), novelty = share of those distinct keys that are not in `train_keys`
        (`compute_novelty`; only when `train_keys`, e.g. from `training_keys`, is given), and with `group_ptr` [G+1] (int32
        offsets: consecutive ligands of a pocket form a group) diversity_per_group [G] (float64 device tensor: the mean
        Tanimoto distance over the pairs of a group's ligands that have a molecule, 0.0 for fewer than two,
        `MoleculeProperties.calculate_diversity`), diversity (its mean) and diversity_std (`np.std`, as upstream prints).
        An empty set gives upstream's 0.0.  `valid_only` (only on the `Sanitized.molecules` of `sanitize`): every number is
        taken over the ligands that sanitised, which is upstream's order of operations."""
        r = self._keys(largest_frag, with_orders, radius, nbits)
        has = (r['status'] & hip.KEY_NO_MOLECULE) == 0
        if valid_only:
            if self.valid is None:
                raise hip.KpdError('set_metrics(valid_only=True) needs the molecules of Molecules.sanitize()')
            has = has & self.valid
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

    def sanitize(self, largest_frag: bool = False, masses: Optional[Dict[str, float]] = None,
                 allowed_bonds: Optional[Dict[str, object]] = None) -> 'Sanitized':
        """Sanitise every ligand on the GPU in one launch (`kpd_mol_sanitize`): ring bonds, planar rings, Kekule bond orders,
        aromatic rings, implicit hydrogen counts, donor / acceptor flags, `valid` and the per-molecule descriptors, by the rule
        include/kpd.h defines.  Stands where upstream calls Chem.SanitizeMol and MoleculeProperties; NOT RDKit's rule and not
        compared with it.  `largest_frag`: over the largest fragment only; `masses`: element -> mass, consulted before
        MONOISOTOPIC_MASS ('H' for the hydrogens); `allowed_bonds` (an intended extension of the plain signature): the over-valence
        table, in the form `build_molecules` takes; by default the very table these molecules were built with, so that
        `atom_validity` and `valid` judge by one table."""
        if self.pos is None or self.lig_elements is None or self.bonds is None:
            raise hip.KpdError('these Molecules carry no coordinates: build them with build_molecules')
        if not self.pos.is_cuda:
            raise hip.KpdError(f'sanitize: ligands must live on the GPU (got {self.pos.device}); sanitisation has no CPU implementation')
        z, allowed = _class_tables(self.lig_elements, allowed_bonds)
        if allowed_bonds is None and self._allowed is not None:
            allowed = self._allowed
        mass, mass_h = mass_table(self.lig_elements, masses)
        dev = self.pos.device
        if len(self) == 0:
            i32 = (torch.int32, 0)
            out = _zeros(dev, order_k=i32, bond_flags=i32, valence_k=i32, atom_h=i32, atom_flags=i32, desc_i=(torch.int32, 0, 10),
                         desc_f=(torch.float64, 0, 2), valid=i32, status=i32)
        else:
            out = hip.mol_sanitize(self.pos, self.lig_ptr, z, allowed, mass, mass_h, self._mol(), largest_only=largest_frag)
        san = Sanitized(self, out, z, largest_frag)
        if allowed_bonds is not None and 'H' in allowed_bonds:
            san.molecules._allowed_h = _class_tables(['H'], allowed_bonds)[1][0]
        return san

    def _in_pockets(self, where: str, what: str, pocket_pos, pocket_elements, pocket_of):
        """What `relax` and `vina_score` share: the guards, then the pockets as one device batch.  Returns pocket_x [M,3],
        pocket_ptr [P+1], pocket_of [B], the pockets' sizes, the atomic number of every ligand class and the max_atoms bound."""
        if self.pos is None or self.lig_elements is None or self.bonds is None:
            raise hip.KpdError('these Molecules carry no coordinates: build them with build_molecules')
        if len(pocket_pos) != len(pocket_elements):
            raise ValueError('pocket_pos and pocket_elements must have one entry per pocket')
        if not self.pos.is_cuda or any(not p.is_cuda for p in pocket_pos):
            raise hip.KpdError(f'{where}: ligands and pockets must live on the GPU; {what} has no CPU implementation')
        dev = self.pos.device
        for q, (p, els) in enumerate(zip(pocket_pos, pocket_elements)):
            if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] != len(els):
                raise hip.KpdError(f'{where}: pocket {q} has positions {tuple(p.shape)} and {len(els)} element symbols')
        pocket_of = _pocket_of(pocket_of, len(self), len(pocket_pos), dev)
        sizes = [int(p.shape[0]) for p in pocket_pos]
        pocket_x = torch.cat([p.reshape(-1, 3).float() for p in pocket_pos]) if sizes else torch.zeros(0, 3, device=dev)
        pocket_ptr = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
        n_max = self._max_atoms if self._max_atoms is not None else hip.MOL_MAX_ATOMS
        return (pocket_x, pocket_ptr, pocket_of, sizes, [ATOMIC_NUMBERS.get(el, 0) for el in self.lig_elements],
                max(1, min(n_max, hip.MOL_MAX_ATOMS)))


    def relax(self, pocket_pos: List[torch.Tensor], pocket_elements: List[Sequence[str]], pocket_of=None,
              vdw: Optional[Dict[str, tuple]] = None, **params) -> 'Relaxed':
        """Relax every ligand inside its rigid pocket on the GPU, all in one launch (`kpd_relax`): what upstream does per ligand
        in analysis/pocket_minimization.py, with the force field and the L-BFGS minimiser include/kpd.h defines instead of
        RDKit's UFF.  NOT UFF: heavy atoms only, no torsions or inversions, no electrostatics, a rigid pocket; the energies
        are comparable between samples relaxed by this function only.
        `pocket_pos`: a list of [m_p,3] GPU tensors in the ligands' frame, `pocket_elements`: a list of symbol lists, one per
        pocket; `pocket_of`: the pocket of every ligand (-1: none), all zeros by default when one pocket is given; `vdw`:
        element -> (x, D), consulted before VDW_PARAMS (an element in neither raises); `params`: k_b, k_a, r_c, s, w_intra,
        gtol, max_step, max_iters."""
        pocket_x, pocket_ptr, pocket_of, sizes, z, max_atoms = self._in_pockets('relax', 'relaxation', pocket_pos, pocket_elements, pocket_of)
        dev = self.pos.device
        lig_vdw = torch.tensor(vdw_table(self.lig_elements, vdw), dtype=torch.float32, device=dev).reshape(-1, 2)
        rows = [r for els in pocket_elements for r in vdw_table(els, vdw)]
        pocket_vdw = torch.tensor(rows, dtype=torch.float32, device=dev).reshape(-1, 2)
        if len(self) == 0:
            return Relaxed(self, self.pos, **_zeros(dev, report=(torch.float64, 0, 12), status=(torch.int32, 0)))
        pos, report, status = hip.relax(self.pos, self.lig_ptr, z, lig_vdw, self._mol(), pocket_x, pocket_vdw, pocket_ptr, pocket_of,
                                        max_atoms=max_atoms, max_pocket=max(sizes, default=0), **params)
        return Relaxed(self, pos, report, status)

    def _vina_inputs(self, where: str, what: str, pocket_pos, pocket_elements, pocket_of, radii, pocket_types, lig_types):
        """What `vina_score` and `vina_minimize` share beyond `_in_pockets`: the radius tables, the pocket types (perceived once, or
        the caller's, normalised to one [M] int32 device tensor) and the ligand type overrides.  Returns the tuple of `_in_pockets`
        followed by the device, lig_radius [F], pocket_radius [M], pocket_types [M] and lig_types ([N] or None)."""
        pocket_x, pocket_ptr, pocket_of, sizes, z, max_atoms = self._in_pockets(where, what, pocket_pos, pocket_elements, pocket_of)
        dev = self.pos.device
        lig_radius = torch.tensor(xs_radius_table(self.lig_elements, radii), dtype=torch.float32, device=dev)
        pocket_radius = torch.tensor([r for els in pocket_elements for r in xs_radius_table(els, radii)], dtype=torch.float32, device=dev)
        if pocket_types is None:
            pz = torch.tensor([ATOMIC_NUMBERS.get(el, 0) for els in pocket_elements for el in els], dtype=torch.int32, device=dev)
            pocket_types, _ = hip.vina_pocket_types(pocket_x, pz, pocket_ptr)
        else:
            if not isinstance(pocket_types, torch.Tensor):
                pocket_types = torch.tensor([int(t) for row in pocket_types for t in row], dtype=torch.int32)
            pocket_types = pocket_types.to(torch.int32).to(dev).flatten()
            if pocket_types.numel() != sum(sizes):
                raise hip.KpdError(f'{where}: pocket_types has {pocket_types.numel()} entries for {sum(sizes)} pocket atoms')
        if lig_types is not None:
            lig_types = torch.as_tensor(lig_types).to(torch.int32).to(dev).flatten()
        return pocket_x, pocket_ptr, pocket_of, sizes, z, max_atoms, dev, lig_radius, pocket_radius, pocket_types, lig_types

    def vina_score(self, pocket_pos: List[torch.Tensor], pocket_elements: List[Sequence[str]], pocket_of=None,
                   radii: Optional[Dict[str, float]] = None, pocket_types=None, lig_types: Optional[torch.Tensor] = None,
                   grad: bool = False, **params) -> 'VinaScores':
        """Score every ligand in its rigid pocket on the GPU, all in one launch (`kpd_vina_score`): the Vina functional form that
        include/kpd.h defines, with a typing rule of this library's own and recalled weights and radii.  NOT gnina's or Vina's
        numbers: the scores rank samples scored by this function against each other.
        `pocket_pos`, `pocket_elements`, `pocket_of`: as for `relax`; `radii`: element -> radius, consulted before XS_RADII (an
        element in neither raises); `pocket_types`: a `VinaScores.pocket_types` to reuse, or the caller's own flags (1 hydrophobic,
        2 donor, 4 acceptor, -1 takes no part) as one sequence per pocket or one [M] tensor, in place of the perceived ones;
        `lig_types`: [N] int32 whose entries >= 0 replace the perceived ligand flags; `grad`: also return the gradient and the
        per-atom scores; `params`: w_gauss1, w_gauss2, w_repulsion, w_hydrophobic, w_hbond, w_rot, r_c."""
        (pocket_x, pocket_ptr, pocket_of, sizes, z, max_atoms, dev, lig_radius, pocket_radius, pocket_types,
         lig_types) = self._vina_inputs('vina_score', 'scoring', pocket_pos, pocket_elements, pocket_of, radii, pocket_types, lig_types)
        if len(self) == 0:
            empty = _zeros(dev, report=(torch.float64, 0, 8), status=(torch.int32, 0), lig_type=(torch.int32, 0))
            return VinaScores(self, empty, pocket_types)
        out = hip.vina_score(self.pos, self.lig_ptr, z, lig_radius, self._mol(), pocket_x, pocket_radius, pocket_types, pocket_ptr, pocket_of,
                             lig_type_in=lig_types, grad=grad, atom_score=grad, max_atoms=max_atoms, max_pocket=max(sizes, default=0),
                             **params)
        return VinaScores(self, out, pocket_types)

    def vina_minimize(self, pocket_pos: List[torch.Tensor], pocket_elements: List[Sequence[str]], pocket_of=None,
                      radii: Optional[Dict[str, float]] = None, pocket_types=None, lig_types: Optional[torch.Tensor] = None,
                      max_rotors: Optional[int] = None, **params) -> 'VinaMinimized':
        """Minimise every ligand in its rigid pocket under the score of `vina_score`, over rigid-body and torsional degrees of
        freedom, all in one launch (`kpd_vina_minimize`): what upstream does with `gnina --minimize` (gen_docking_cmds.py
        --minimize), with the torsion tree, the intramolecular term and the L-BFGS include/kpd.h defines.  NOT gnina's or Vina's
        numbers: the typing, the weights and the radii are those of `vina_score`.
        `pocket_pos`, `pocket_elements`, `pocket_of`, `radii`, `pocket_types`, `lig_types`: as for `vina_score`; `max_rotors`
        (0 .. 64, 64 by default): the rotors beyond it are frozen, 0 minimises rigid bodies only; `params`: the parameters of
        `vina_score` and w_intra, gtol, max_step, max_iters."""
        (pocket_x, pocket_ptr, pocket_of, sizes, z, max_atoms, dev, lig_radius, pocket_radius, pocket_types,
         lig_types) = self._vina_inputs('vina_minimize', 'minimisation', pocket_pos, pocket_elements, pocket_of, radii, pocket_types, lig_types)
        if len(self) == 0:
            return VinaMinimized(self, self.pos, pocket_types=pocket_types, **_zeros(dev, report=(torch.float64, 0, 16), status=(torch.int32, 0)))
        pos, report, status = hip.vina_minimize(self.pos, self.lig_ptr, z, lig_radius, self._mol(), pocket_x, pocket_radius, pocket_types, pocket_ptr,
                                                pocket_of, lig_type_in=lig_types, max_atoms=max_atoms, max_pocket=max(sizes, default=0),
                                                max_rotors=hip.VINA_MIN_MAX_ROTORS if max_rotors is None else max_rotors, **params)
        return VinaMinimized(self, pos, report, status, pocket_types)

    def _dock_box(self, pocket_of: torch.Tensor, n_pockets: int, box, autobox_ligand, autobox_add: float):
        """The search box of every ligand, (lo, hi) as [B,3] fp32 device tensors: `box` per ligand or per pocket, else the bounding
        box of the pocket's `autobox_ligand` widened by `autobox_add`, else (also for a ligand without a pocket) that of the
        ligand's own input pose."""
        dev, B = self.pos.device, len(self)
        sizes = self.lig_ptr[1:] - self.lig_ptr[:-1]
        idx = torch.repeat_interleave(torch.arange(B, device=dev), sizes.long())[:, None].expand(-1, 3)
        own_lo = torch.full((B, 3), float('inf'), device=dev).scatter_reduce(0, idx, self.pos, 'amin') - float(autobox_add)
        own_hi = torch.full((B, 3), float('-inf'), device=dev).scatter_reduce(0, idx, self.pos, 'amax') + float(autobox_add)
        if box is None and autobox_ligand is None:
            return own_lo, own_hi
        if box is not None:
            lo, hi = (torch.as_tensor(t, dtype=torch.float32).to(dev).reshape(-1, 3) for t in box)
            if lo.shape != hi.shape or lo.shape[0] not in (B, n_pockets):
                raise hip.KpdError(f'vina_dock: box must be (lo, hi) of [{B},3] per ligand or [{n_pockets},3] per pocket, got '
                                   f'{tuple(lo.shape)} and {tuple(hi.shape)}')
            if lo.shape[0] == B:
                return lo.contiguous(), hi.contiguous()
        else:
            if len(autobox_ligand) != n_pockets:
                raise hip.KpdError(f'vina_dock: autobox_ligand must hold one [n,3] reference ligand for each of the {n_pockets} pockets')
            ref = [torch.as_tensor(r, dtype=torch.float32).to(dev).reshape(-1, 3) for r in autobox_ligand]
            lo = torch.stack([r.amin(dim=0) for r in ref]) - float(autobox_add)
            hi = torch.stack([r.amax(dim=0) for r in ref]) + float(autobox_add)
        has, q = (pocket_of >= 0)[:, None], pocket_of.clamp(min=0).long()
        return torch.where(has, lo[q], own_lo).contiguous(), torch.where(has, hi[q], own_hi).contiguous()

    def vina_dock(self, pocket_pos: List[torch.Tensor], pocket_elements: List[Sequence[str]], pocket_of=None, box=None,
                  autobox_ligand=None, autobox_add: float = 4.0, n_chains: int = 8, n_steps: int = 50, n_modes: Optional[int] = None,
                  seed: int = 0, lig_ids=None, radii: Optional[Dict[str, float]] = None, pocket_types=None,
                  lig_types: Optional[torch.Tensor] = None, max_rotors: Optional[int] = None, **params) -> 'VinaDocked':
        """Search poses of every ligand in its rigid pocket under the score of `vina_score`: `n_chains` Monte-Carlo chains per
        ligand (perturb, minimise, Metropolis) inside a box, then ranking and clustering into `n_modes` poses, in two launches
        (`kpd_vina_dock`): what upstream does with full gnina docking inside `--autobox_ligand` (gen_docking_cmds.py without
        --minimize), with the search include/kpd.h DEFINES.  NOT gnina's or Vina's docking and NOT their numbers: the typing, the
        weights and the radii are those of `vina_score`.
        `pocket_pos`, `pocket_elements`, `pocket_of`, `radii`, `pocket_types`, `lig_types`, `max_rotors`: as for `vina_minimize`;
        `box`: (lo, hi), each [B,3] per ligand or [P,3] per pocket; `autobox_ligand`: a reference ligand's [n,3] per pocket, whose
        bounding box widened by `autobox_add` is the box, as gnina's `--autobox_ligand`; with neither, the box is the ligand's own
        input bounding box widened by `autobox_add`; `n_modes`: `min(9, n_chains)` by default; `seed` and `lig_ids` (the name of
        every ligand's random stream, its index by default) fix the random numbers; `params`: the parameters of `vina_minimize`
        (max_iters is the final refinement's) and temperature, amplitude, min_rmsd, step_iters."""
        (pocket_x, pocket_ptr, pocket_of, sizes, z, max_atoms, dev, lig_radius, pocket_radius, pocket_types,
         lig_types) = self._vina_inputs('vina_dock', 'docking', pocket_pos, pocket_elements, pocket_of, radii, pocket_types, lig_types)
        n_chains = int(n_chains)
        n_modes = min(9, n_chains) if n_modes is None else int(n_modes)
        if len(self) == 0:
            m, c, f32, f64 = max(n_modes, 1), max(n_chains, 1), torch.float32, torch.float64
            empty = _zeros(dev, pos=(f32, m, 0, 3), n_found=(torch.int32, 0), report=(f64, 0, m, 8), chain_pos=(f32, c, 0, 3),
                           chain_report=(f64, 0, c, 10), status=(torch.int32, 0))
            z3 = torch.zeros(0, 3, device=dev)
            return VinaDocked(self, empty, pocket_types, (z3, z3))
        lo, hi = self._dock_box(pocket_of, len(pocket_pos), box, autobox_ligand, autobox_add)
        if lig_ids is not None:
            lig_ids = torch.as_tensor(lig_ids).to(torch.int32).to(dev).flatten()
        out = hip.vina_dock(self.pos, self.lig_ptr, z, lig_radius, self._mol(), pocket_x, pocket_radius, pocket_types, pocket_ptr, pocket_of, lo, hi,
                            n_chains=n_chains, n_steps=n_steps, n_modes=n_modes, seed=seed, lig_id=lig_ids, lig_type_in=lig_types,
                            max_atoms=max_atoms, max_pocket=max(sizes, default=0),
                            max_rotors=hip.VINA_MIN_MAX_ROTORS if max_rotors is None else max_rotors, **params)
        return VinaDocked(self, out, pocket_types, (lo, hi))


class PoseRMSD:
    """What `pose_rmsd` returns, device tensors: `.rmsd` and `.plain` (the atom-by-atom number over the same atoms; rmsd <= plain)
    float64 and `.nodes` int64 (candidates the search tried), [B,K], or [B,K,K] for pairs (symmetric, the diagonal 0); `.map`
    [K,N] int32 (the row whose place in the pose answers each atom of the reference, -1 for an atom that took no part; None for
    pairs); `.status` [B] (bits: 1 no molecule -- zeros and map -1 --, 2 some search stopped at max_nodes and gives an upper
    bound, 4 a non-finite coordinate: the searches that read it give zeros)."""

    def __init__(self, out: Dict[str, torch.Tensor], pairs: bool):
        self.rmsd, self.plain, self.nodes, self.status = out['rmsd'], out['plain'], out['nodes'], out['status']
        self.map, self.pairs = out.get('map'), pairs

    def table(self) -> Dict[str, list]:
        """lig_idx, pose (pairs: pose_i, pose_j with i < j), rmsd, plain, nodes as lists; ligands without a molecule have no row."""
        keep = ((self.status.cpu() & hip.POSE_NO_MOLECULE) == 0).nonzero().flatten().tolist()
        K = int(self.rmsd.shape[1])
        rmsd, plain, nodes = self.rmsd.cpu(), self.plain.cpu(), self.nodes.cpu()
        if self.pairs:
            rows = [(b, i, j) for b in keep for i in range(K) for j in range(i + 1, K)]
            return dict(lig_idx=[r[0] for r in rows], pose_i=[r[1] for r in rows], pose_j=[r[2] for r in rows],
                        rmsd=[rmsd[r].item() for r in rows], plain=[plain[r].item() for r in rows], nodes=[int(nodes[r]) for r in rows])
        rows = [(b, k) for b in keep for k in range(K)]
        return dict(lig_idx=[r[0] for r in rows], pose=[r[1] for r in rows], rmsd=[rmsd[r].item() for r in rows],
                    plain=[plain[r].item() for r in rows], nodes=[int(nodes[r]) for r in rows])


class PoseChecks:
    """What `pose_check` returns, device tensors per (ligand, pose): `.passed` [B,K] bool (no check fails, the pose could be
    checked, and the molecule is `Sanitized.valid`), `.fail` [B,K] int32 (bit k: hip.CHECK_FAIL[k]), `.report` [B,K,10] float64 (the
    extreme value behind every check, columns hip.CHECK_REPORT), `.counts` [B,K,17] int32 (items examined and failing, columns
    hip.CHECK_COUNTS), `.atom_fail` [K,N] int32 (per atom the checks it took part in failing), `.status` [B,K] (bits: 1 no molecule,
    2 bad input, 4 some atom took no part in the clash and overlap checks).  The rule is include/kpd.h's, NOT PoseBusters'."""

    def __init__(self, out: Dict[str, torch.Tensor], valid: torch.Tensor):
        self.fail, self.report, self.counts, self.atom_fail, self.status = (out[k] for k in ('fail', 'report', 'counts', 'atom_fail', 'status'))
        checked = (self.status & (hip.CHECK_NO_MOLECULE | hip.CHECK_BAD_INPUT)) == 0
        self.passed = (self.fail == 0) & checked & valid.to(torch.bool)[:, None]

    def table(self) -> Dict[str, list]:
        """lig_idx, pose, passed, one bool column per check (True: it passes), then every report and count column, as lists;
        poses that could not be checked (status bit 0 or 1) have no row."""
        st, fail, rep, cnt, ok = self.status.cpu(), self.fail.cpu(), self.report.cpu(), self.counts.cpu(), self.passed.cpu()
        rows = [(b, k) for b in range(st.shape[0]) for k in range(st.shape[1])
                if not int(st[b, k]) & (hip.CHECK_NO_MOLECULE | hip.CHECK_BAD_INPUT)]
        out: Dict[str, list] = dict(lig_idx=[b for b, _ in rows], pose=[k for _, k in rows], passed=[bool(ok[r]) for r in rows])
        for bit, name in enumerate(hip.CHECK_FAIL):
            out[name + '_ok'] = [not (int(fail[r]) >> bit) & 1 for r in rows]
        for c, name in enumerate(hip.CHECK_REPORT):
            out[name] = [rep[r][c].item() for r in rows]
        for c, name in enumerate(hip.CHECK_COUNTS):
            out[name] = [int(cnt[r][c]) for r in rows]
        return out


class Matches:
    """What `Sanitized.match` returns, for the user's patterns only (the rows lifted out of "$(...)" are not reported), device
    tensors: `.hits` [B,n] int32 (atoms that are the image of the pattern's first atom in some embedding), `.has` [B,n] bool,
    `.first_map` [B,n,16] int32 (the first embedding from the lowest such atom, as atom rows of the batch; -1 beyond the pattern's
    atoms and without a hit), `.n_embed` [B,n] int64 (embeddings as maps, a benzene ring holds c1ccccc1 twelve times; None unless
    `all_embeddings`), `.status` [B] (bits: 1 no molecule, 2 some search stopped at max_nodes: the counts are then lower bounds).
    The rule is include/kpd.h's, NOT RDKit's matcher."""

    def __init__(self, patterns: 'smarts.Patterns', out: Dict[str, torch.Tensor]):
        self.patterns, self.names, self._out = patterns, patterns.names, out
        rows = patterns.row_index(out['hits'].device)
        self.hits, self.status = out['hits'][:, rows], out['status']
        self.has = self.hits > 0
        self.first_map = out['first_map'][:, rows] if 'first_map' in out else None
        self.n_embed = out['n_embed'][:, rows] if 'n_embed' in out else None

    def _bit(self, words: torch.Tensor, p: int) -> torch.Tensor:
        r = self.patterns.rows[p]
        return ((words[:, r >> 5] >> (r & 31)) & 1) != 0

    def anchor_atoms(self, p: int) -> torch.Tensor:
        """[N] bool: the atom is the image of the first atom of pattern p in some embedding."""
        return self._bit(self._out['anchor'], p)

    def cover_atoms(self, p: int) -> torch.Tensor:
        """[N] bool: the atom is the image of any atom of pattern p in any embedding (needs `all_embeddings=True`)."""
        if 'cover' not in self._out:
            raise hip.KpdError('cover_atoms needs match(..., all_embeddings=True)')
        return self._bit(self._out['cover'], p)

    def table(self) -> Dict[str, list]:
        """lig_idx, then one column of hit counts per pattern name; ligands without a molecule have no row."""
        keep = ((self.status.cpu() & hip.MATCH_NO_MOLECULE) == 0).nonzero().flatten().tolist()
        hits = self.hits.cpu()
        out: Dict[str, list] = dict(lig_idx=keep)
        for k, name in enumerate(self.names):
            out[name] = hits[keep, k].tolist()
        return out


class Sanitized:
    """What `Molecules.sanitize` returns: `.molecules` (a `Molecules` whose `order` is order_k and whose `valence` is valence_k, so
    `.sdf()`, `.keys()`, `.relax()`, `.vina_score()`, `.vina_minimize()` and `.vina_dock()` work unchanged on the Kekule orders),
    `.h` [N] (implicit hydrogens), `.aromatic_atoms` [N] and `.aromatic_bonds` [3N] (bool), `.atom_flags` [N] and `.bond_flags`
    [3N] (bits hip.SAN_ATOM_* / hip.SAN_BOND_*), `.valid` [B] (bool), `.status` [B] (bits: 1 no molecule, 2 more than 64 five-
    or six-cycles, 4 a candidate component of more than 24 atoms), device tensors.  The rule is include/kpd.h's, NOT RDKit's."""

    def __init__(self, mols: Molecules, out: Dict[str, torch.Tensor], z: Sequence[int], largest_frag: bool):
        self.molecules = Molecules(mols.lig_ptr, mols.summary, mols.status, mols.elem, out['valence_k'], mols.frag, mols.bonds,
                                   out['order_k'], mols.bond_ptr, mols.pos, mols.lig_elements, mols._max_atoms, sizes=mols._sizes)
        self.valid = out['valid'] != 0
        self.molecules.valid, self.molecules._allowed, self.molecules._allowed_h = self.valid, mols._allowed, mols._allowed_h
        self.h, self.atom_flags, self.bond_flags, self.status = out['atom_h'], out['atom_flags'], out['bond_flags'], out['status']
        self.aromatic_atoms = (out['atom_flags'] & hip.SAN_ATOM_AROMATIC) != 0
        self.aromatic_bonds = (out['bond_flags'] & hip.SAN_BOND_AROMATIC) != 0
        self.largest_frag, self._desc_i, self._desc_f, self._z = bool(largest_frag), out['desc_i'], out['desc_f'], list(z)
        self._out = out

    def add_hs(self) -> 'Hydrogenated':
        """Explicit hydrogens with coordinates for every ligand, on the GPU (`kpd_mol_add_hs`): what upstream gets from
        Chem.AddHs(lig, addCoords=True).  The counts are `.h`; the placement rule (ideal tetrahedral / trigonal / linear sites at
        the X-H rest lengths of `relax`, the first hydrogen of a chain end anti to the chain) is include/kpd.h's, NOT RDKit's.
        The hydrogens take the class 'H' of `lig_elements`, appended if it is absent (its validity entry is the caller's
        `allowed_bonds['H']` if there is one).  Two host synchronisations: the sum of the counts that sizes the outputs, and the
        copy of the B + 1 offsets that gives the new atoms per ligand."""
        return Hydrogenated(self)

    def smiles(self, kekule: bool = False, largest_frag: Optional[bool] = None) -> List[str]:
        """One SMILES string per ligand, written on the GPU (`kpd_mol_smiles`): the aromatic form (`c1ccccc1`), with `kekule=True`
        the Kekule form (`C=1C=CC=CC1`).  `largest_frag`: None, the scope these molecules were sanitised with; True, the largest
        fragment alone (upstream's `Chem.MolToSmiles(largest_mol)`), which molecules sanitised over every atom can give as well,
        their per-atom results covering every fragment; False needs molecules sanitised over every atom.  Canonical under the
        rule of include/kpd.h, NOT RDKit's: equal strings mean the same molecule among strings of this library only.  A ligand
        without a molecule (or with more than 99 ring closures open at once) gives ''; a ligand that is not `valid` still has a
        string.  No charges, no stereo."""
        largest = self.largest_frag if largest_frag is None else bool(largest_frag)
        if self.largest_frag and not largest:
            raise hip.KpdError('smiles(largest_frag=False) needs molecules sanitised over every atom: sanitize(largest_frag=False)')
        m = self.molecules
        if m.lig_elements is None or m.bonds is None:
            raise hip.KpdError('these Molecules carry no bond graph: build them with build_molecules')
        if len(m) == 0:
            return []
        if not m.lig_ptr.is_cuda:
            raise hip.KpdError(f'smiles: ligands must live on the GPU (got {m.lig_ptr.device}); there is no CPU implementation')
        text, ptr, status = hip.mol_smiles(m.lig_ptr, self._z, m.lig_elements, m._mol(), self._out, largest_only=largest, aromatic=not kekule)
        if any(s & hip.SMI_CAPACITY for s in status):
            raise hip.KpdError('smiles: text buffer too small (internal sizing error)')
        return ['' if status[b] else text[ptr[b]:ptr[b + 1]].decode('ascii') for b in range(len(status))]

    def pose_rmsd(self, pos, ref=None, largest_frag: Optional[bool] = None, skip_h: bool = True, pairs: bool = False,
                  max_nodes: int = 65536, bond_label: Optional[torch.Tensor] = None,
                  atom_label: Optional[torch.Tensor] = None) -> 'PoseRMSD':
        """`Molecules.pose_rmsd` on the labelled graph of the SMILES rule: by default atom_label = 2 h + aromatic and bond_label = 4
        on an aromatic bond, else the Kekule order, so an automorphism keeps hydrogen counts and bond orders but does not depend
        on which Kekule pattern the ring was given.  `largest_frag`: None, the scope these molecules were sanitised with."""
        largest = self.largest_frag if largest_frag is None else bool(largest_frag)
        if self.largest_frag and not largest:
            raise hip.KpdError('pose_rmsd(largest_frag=False) needs molecules sanitised over every atom: sanitize(largest_frag=False)')
        m = self.molecules
        if atom_label is None:
            atom_label = (2 * self.h.clamp(min=0) + self.aromatic_atoms.to(torch.int32)).to(torch.int32)
        if bond_label is None:      # rows outside the sanitised scope or beyond bond_ptr[B] carry no order: any label in range will do
            bond_label = torch.where(self.aromatic_bonds, torch.full_like(m.order, 4), m.order.clamp(1, 3)).to(torch.int32)
        return m.pose_rmsd(pos, ref, largest_frag=largest, skip_h=skip_h, pairs=pairs, max_nodes=max_nodes, bond_label=bond_label,
                           atom_label=atom_label)

    def pose_check(self, pos=None, pocket_pos: Optional[List[torch.Tensor]] = None, pocket_elements: Optional[List[Sequence[str]]] = None,
                   pocket_of=None, radii: Optional[Dict[str, float]] = None, with_h: bool = False, largest_frag: Optional[bool] = None,
                   **thresholds) -> 'PoseChecks':
        """Whether poses of these molecules are physically plausible, on the GPU in one launch (`kpd_pose_check`): bond lengths and
        1-3 distances in range, no internal clash, flat aromatic rings, planar centres and double bonds and, with pockets, no clash
        with the pocket and little volume overlap with it.  The list follows PoseBusters; the rule is include/kpd.h's and these are
        NOT PoseBusters' numbers (reference lengths and angles of this library's own, no energy check, no stereo).
        `pos`: [N,3], [K,N,3] or a list of per-ligand tensors, these molecules' own pose by default; relaxed, minimised and docked
        poses are the main customers.  `pocket_pos`, `pocket_elements`, `pocket_of`: as for `Molecules.relax`; without them the two
        pocket checks examine nothing.  `radii`: element -> van der Waals radius, consulted before VDW_RADII (an element in neither
        raises); `with_h`: hydrogens take part in the clash and overlap checks; `largest_frag`: None, the scope these molecules
        were sanitised with; `thresholds`: the fields of `hip.pose_check_params`."""
        largest = self.largest_frag if largest_frag is None else bool(largest_frag)
        if self.largest_frag and not largest:
            raise hip.KpdError('pose_check(largest_frag=False) needs molecules sanitised over every atom: sanitize(largest_frag=False)')
        m = self.molecules
        if m.lig_elements is None or m.bonds is None:
            raise hip.KpdError('these Molecules carry no bond graph: build them with build_molecules')
        pos = m.pos if pos is None else pos
        if pos is None:
            raise hip.KpdError('these Molecules carry no coordinates: pass pos')
        stack = m._pose_stack(pos)
        if not stack.is_cuda or not m.lig_ptr.is_cuda:
            raise hip.KpdError(f'pose_check: poses must live on the GPU (got {stack.device}); there is no CPU implementation')
        if (pocket_pos is None) != (pocket_elements is None):
            raise ValueError('pocket_pos and pocket_elements come together')
        dev = stack.device
        lig_radius = torch.tensor(vdw_radius_table(m.lig_elements, radii, with_h), dtype=torch.float32, device=dev)
        pocket = {}
        if pocket_pos is not None:
            if m.pos is None:
                m = Molecules(m.lig_ptr, m.summary, m.status, m.elem, m.valence, m.frag, m.bonds, m.order, m.bond_ptr, stack[0],
                              m.lig_elements, m._max_atoms, sizes=m._sizes)
            pocket_x, pocket_ptr, pocket_of, sizes, _, _ = m._in_pockets('pose_check', 'checking', pocket_pos, pocket_elements, pocket_of)
            rows = [r for els in pocket_elements for r in vdw_radius_table(els, radii, with_h)]
            pocket = dict(pocket_x=pocket_x, pocket_radius=torch.tensor(rows, dtype=torch.float32, device=dev), pocket_ptr=pocket_ptr,
                          pocket_of=pocket_of, max_pocket=max(sizes, default=0))
        hip.pose_check_params(**thresholds)         # refuse bad thresholds before anything is launched
        K = int(stack.shape[0])
        if len(m) == 0:
            i32 = torch.int32
            empty = _zeros(dev, fail=(i32, 0, K), report=(torch.float64, 0, K, len(hip.CHECK_REPORT)), counts=(i32, 0, K, len(hip.CHECK_COUNTS)),
                           atom_fail=(i32, K, 0), status=(i32, 0, K))
            return PoseChecks(empty, self.valid)
        n_max = m._max_atoms if m._max_atoms is not None else hip.MOL_MAX_ATOMS
        out = hip.pose_check(m.lig_ptr, self._z, m._mol(), self._out, stack, lig_radius, largest_only=largest,
                             max_atoms=max(1, min(n_max, hip.MOL_MAX_ATOMS)), **pocket, **thresholds)
        return PoseChecks(out, self.valid)

    def unique(self, kekule: bool = False, largest_frag: Optional[bool] = None) -> List[int]:
        """The index of the first ligand of every distinct string of `smiles(kekule, largest_frag)`, ascending; ligands without a
        molecule are left out."""
        first: Dict[str, int] = {}
        for b, s in enumerate(self.smiles(kekule, largest_frag)):
            if s:
                first.setdefault(s, b)
        return sorted(first.values())

    def _patterns(self, patterns) -> 'smarts.Patterns':
        if isinstance(patterns, smarts.Patterns):
            return patterns
        return smarts.compile(patterns)

    def _match(self, pats, mode: int, max_nodes: int, want_map: bool = True, type_group=None, value=None) -> Dict[str, torch.Tensor]:
        m = self.molecules
        if m.bonds is None:
            raise hip.KpdError('these Molecules carry no bond graph: build them with build_molecules')
        if not m.lig_ptr.is_cuda:
            raise hip.KpdError(f'match: ligands must live on the GPU (got {m.lig_ptr.device}); there is no CPU implementation')
        return hip.mol_match(m.lig_ptr, self._z, m._mol(), self._out, pats, mode=mode, max_nodes=max_nodes, want_map=want_map,
                             type_group=type_group, value=value, largest_only=self.largest_frag)

    def match(self, patterns, all_embeddings: bool = False, max_nodes: int = 65536) -> 'Matches':
        """Substructure search on the GPU (`kpd_mol_match`): `patterns` is a `smarts.Patterns`, a SMARTS string or a list of them
        (strings are compiled on the spot; `smarts` states the supported subset).  The queries are matched on THIS library's
        sanitised labels: its aromaticity, no charges, no stereo, no ring sizes.  The rule is include/kpd.h's; it is NOT RDKit's
        matcher and is not compared with it.  `all_embeddings`: count every embedding (`.n_embed`, `.cover_atoms`) instead of
        stopping each search at its first.  The scope is the one these molecules were sanitised with.  The first use of a `Patterns` on
        a device copies its table and row numbers there; after that a call makes no host synchronisation."""
        pats = self._patterns(patterns)
        out = self._match(pats, hip.MATCH_ALL if all_embeddings else hip.MATCH_ANCHORS, max_nodes)
        return Matches(pats, out)

    def has_substructure(self, pattern: str) -> torch.Tensor:
        """[B] bool: the ligand contains the SMARTS query (`match`, whose limits apply: NOT RDKit's matcher)."""
        pats = self._patterns(pattern)
        if pats.n != 1:
            raise ValueError('has_substructure takes one pattern; use match() for several')
        return self._match(pats, hip.MATCH_ANCHORS, 65536, want_map=False)['hits'][:, pats.rows[0]] > 0

    def atom_types(self, patterns, values=None):
        """First-match-wins atom typing by a caller-supplied table (the form of a Crippen table; the library ships none): the
        type of an atom is the first pattern of `patterns` it is the first atom of, -1 if none.  `values`: one number per
        pattern (default 0).  Returns (atom_type [N] int32 as the index of the user's pattern, -1 untyped or out of scope;
        type_sum [B] float64, the values of a ligand's typed atoms added in ascending atom index; untyped [B] int32)."""
        pats = self._patterns(patterns)
        values = [0.0] * pats.n if values is None else [float(v) for v in values]
        if len(values) != pats.n:
            raise ValueError(f'atom_types: {len(values)} values for {pats.n} patterns')
        group, value = [-1] * pats.n_rows, [0.0] * pats.n_rows
        for k, r in enumerate(pats.rows):
            group[r], value[r] = 0, values[k]
        out = self._match(pats, hip.MATCH_ANCHORS, 65536, want_map=False, type_group=group, value=value)
        return pats.user_index(out['atom_type'].device)[out['atom_type'][0].long()], out['type_sum'][:, 0], out['untyped'][:, 0]

    def descriptors(self) -> Dict[str, torch.Tensor]:
        """Per ligand, as [B] device tensors: n_heavy, n_h, hbd, hba, n_rot, n_rings, n_arom_rings, n_arom_atoms, lipinski4 (how
        many of mw < 500, hbd <= 5, hba <= 10, n_rot <= 10 hold: upstream's logP rule is not counted), n_cycles (int32) and mw
        (float64).  Zeros for a ligand without a molecule."""
        out = {name: self._desc_i[:, k] for k, name in enumerate(hip.SAN_DESC_I)}
        out['mw'] = self._desc_f[:, 0]
        return out

    def table(self) -> Dict[str, list]:
        """lig_idx, valid and the descriptors as lists; ligands without a molecule (status bit 0) have no row."""
        st = self.status.cpu()
        keep = ((st & hip.SAN_NO_MOLECULE) == 0).nonzero().flatten().tolist()
        out: Dict[str, list] = dict(lig_idx=keep, valid=self.valid.cpu()[keep].tolist())
        for name, col in self.descriptors().items():
            out[name] = col.cpu()[keep].tolist()
        return out

    def vina_types(self) -> torch.Tensor:
        """[N] int32 for `lig_types=` of `vina_score` / `vina_minimize` / `vina_dock`: the flags of kpd_vina_score recomputed
        from the hydrogen counts.  N: donor (2) iff h >= 1, else acceptor (4) under the acceptor rule of include/kpd.h, else 0;
        O: acceptor, and donor iff h >= 1; -1 (keep the rule of kpd_vina_score) for every other element and outside the scope."""
        m = self.molecules
        zt = torch.tensor(self._z, dtype=torch.int32, device=m.elem.device)
        za = torch.where(m.elem >= 0, zt[m.elem.clamp(min=0).long()], torch.zeros_like(m.elem))
        donor = (self.h >= 1).to(torch.int32) * 2
        acc = ((self.atom_flags & hip.SAN_ATOM_ACCEPTOR) != 0).to(torch.int32) * 4
        t = torch.full_like(m.elem, -1)
        t = torch.where(za == 7, torch.where(donor > 0, donor, acc), t)
        t = torch.where(za == 8, donor | 4, t)
        return torch.where(m.valence >= 0, t, torch.full_like(t, -1))

    def metrics(self, type_counts: Optional[torch.Tensor] = None, connectivity_thresh: float = 0.5,
                group_ptr: Optional[torch.Tensor] = None, train_keys: Optional[torch.Tensor] = None, by: str = 'key',
                train_smiles: Optional[Sequence[str]] = None) -> Dict[str, object]:
        """Upstream's order of operations (ModelAnalyzer.sample_and_analyze): validity = ligands that sanitised / ligands that
        were built (as in `Molecules.metrics`, empty and left-out ligands do not count); connectivity over the valid ligands;
        uniqueness, novelty and diversity (`set_metrics(valid_only=True)`) over the valid, connected ones; atom_validity,
        avg_frag_frac and atom_type_kldiv as `Molecules.metrics` gives them; and the mean and standard deviation (np.std) of
        mw, hbd, hba, n_rot and lipinski4 over the valid ligands.  `group_ptr` and `train_keys` are those of `set_metrics` (the
        pockets' groups for diversity, the training keys for novelty), passed through so that one call gives upstream's seven.
        `by='smiles'`: uniqueness (and novelty against `train_smiles`, strings of this library) are counted on the strings of
        `smiles(largest_frag=True)` instead of on the keys: the same scope, the largest fragment, as every other set metric, but a
        string does not depend on the Kekule pattern; every other number is the same.  The default is the key."""
        if by not in ('key', 'smiles'):
            raise ValueError(f"by must be 'key' or 'smiles' (got {by!r})")
        m = self.molecules
        out: Dict[str, object] = m.metrics(type_counts, connectivity_thresh)
        n = (m.lig_ptr[1:] - m.lig_ptr[:-1]).double()
        built = (n > 0) & ((m.status & hip.MOL_BAD_SEGMENT) == 0)
        valid = self.valid & built
        n_built, n_valid = int(built.sum()), int(valid.sum())
        out['validity'] = n_valid / n_built if n_built else 0.0
        frac = m.summary[:, 2].double() / n.clamp(min=1)
        out['connectivity'] = float((frac[valid] >= connectivity_thresh).double().mean()) if n_valid else 0.0
        out.update(m.set_metrics(group_ptr, train_keys, connectivity_thresh, largest_frag=True, valid_only=True))
        if by == 'smiles':
            keep = (valid & (frac >= connectivity_thresh)).cpu().tolist()
            strings = [s for s, k in zip(self.smiles(largest_frag=True), keep) if k and s]
            distinct = set(strings)
            out['uniqueness'] = len(distinct) / len(strings) if strings else 0.0
            if train_smiles is not None:
                known = set(train_smiles)
                out['novelty'] = sum(s not in known for s in distinct) / len(distinct) if distinct else 0.0
        desc = self.descriptors()
        for name in ('mw', 'hbd', 'hba', 'n_rot', 'lipinski4'):
            col = desc[name][valid].double()
            out[name + '_mean'] = float(col.mean()) if n_valid else 0.0
            out[name + '_std'] = float(col.std(unbiased=False)) if n_valid else 0.0
        return out


class Hydrogenated:
    """What `Sanitized.add_hs` returns: `.molecules` (a `Molecules` with the hydrogens appended to every ligand's atoms and bonds,
    Kekule orders, so `.sdf()`, `.keys()`, `.sanitize()`, `.relax()`, `.vina_score()`, `.vina_minimize()` and `.vina_dock()` work
    unchanged; its `lig_elements` are the input's plus 'H' if that was absent), `.parent` [N'] (for an H the row of its heavy
    atom, else the atom's own row), `.source` [N'] (-1 for an H, else the row in `.heavy`), `.is_h` [N'] (bool), `.n_h` [B],
    `.status` [B] (bits hip.HS_*: 1 no molecule, 2 more than 256 atoms with the hydrogens, 8 some atom placed by the general rule,
    16 a non-finite coordinate; with 1, 2 or 16 the ligand is copied through without hydrogens), device tensors, and `.heavy`
    (the `Sanitized.molecules` it came from).  The placement rule is include/kpd.h's, NOT RDKit's."""

    def __init__(self, san: 'Sanitized'):
        m = san.molecules
        if m.pos is None or m.lig_elements is None or m.bonds is None:
            raise hip.KpdError('these Molecules carry no coordinates: build them with build_molecules')
        if not m.pos.is_cuda:
            raise hip.KpdError(f'add_hs: ligands must live on the GPU (got {m.pos.device}); hydrogen placement has no CPU implementation')
        elements = list(m.lig_elements)
        allowed = list(m._allowed) if m._allowed is not None else _class_tables(elements, None)[1]
        if 'H' not in elements:
            elements.append('H')
            allowed.append(ALLOWED_BONDS['H'] if m._allowed_h is None else m._allowed_h)
        h_class = elements.index('H')
        z = [ATOMIC_NUMBERS.get(el, 0) for el in elements]
        dev = m.pos.device
        self.heavy = m
        if len(m) == 0:
            i32 = (torch.int32, 0)
            out = _zeros(dev, lig_ptr=(torch.int32, 1), pos=(torch.float32, 0, 3), elem=i32, valence=i32, frag=i32, bonds=(torch.int32, 0, 2),
                         order=i32, bond_ptr=(torch.int32, 1), summary=(torch.int32, 0, 4), parent=i32, source=i32, n_h=i32, status=i32)
            sizes: Optional[List[int]] = []
        else:
            out = hip.mol_add_hs(m.pos, m.lig_ptr, z, allowed, h_class, m._mol(), san._out, largest_only=san.largest_frag)
            sizes = (out['lig_ptr'][1:] - out['lig_ptr'][:-1]).cpu().tolist()
            for k in ('pos', 'elem', 'valence', 'frag', 'parent', 'source'):       # rows sized for ligands that were copied through
                out[k] = out[k][:sum(sizes)]
        self.molecules = Molecules(out['lig_ptr'], out['summary'], m.status, out['elem'], out['valence'], out['frag'], out['bonds'],
                                   out['order'], out['bond_ptr'], out['pos'], elements, sizes=sizes)
        self.molecules.valid, self.molecules._allowed, self.molecules._allowed_h = san.valid, allowed, m._allowed_h
        self.parent, self.source, self.n_h, self.status = out['parent'], out['source'], out['n_h'], out['status']
        self.is_h = (out['source'] < 0) & (out['elem'] >= 0)

    def sdf(self, largest_frag: bool = False, strict: bool = True) -> List[str]:
        """`.molecules.sdf()`: the blocks with their 'H' atom lines."""
        return self.molecules.sdf(largest_frag=largest_frag, strict=strict)


class VinaDocked:
    """What `Molecules.vina_dock` returns: `.molecules` (a `Molecules` with the same bond graph at mode 0, the best pose found),
    `.mode(k)` (the same at mode k; a ligand with fewer modes keeps its input pose there), `.n_found` [B], `.report`
    [B,n_modes,8] float64 (columns hip.VINA_DOCK_REPORT), `.chain_report` [B,n_chains,10] (columns hip.VINA_DOCK_CHAIN_REPORT),
    `.status` [B] (bits: 1 no molecule, 2 bad input, 4 some atom took no part, 16 rotors frozen, 32 more than 8 fragments, 128 a
    bad box, 256 the input pose is outside the box, 512 fewer than n_modes found; with 1, 2, 32 or 128 the ligand is unchanged),
    `.box` (lo, hi) [B,3] and `.pocket_types` [M], device tensors.  NOT gnina's or Vina's docking or numbers: see include/kpd.h."""

    def __init__(self, mols: Molecules, out: Dict[str, torch.Tensor], pocket_types: torch.Tensor, box):
        self._mols, self._pos, self.chain_pos = mols, out['pos'], out['chain_pos']
        self.n_found, self.report, self.chain_report, self.status = out['n_found'], out['report'], out['chain_report'], out['status']
        self.pocket_types, self.box = pocket_types, box
        self.molecules = self.mode(0)

    @property
    def n_modes(self) -> int:
        return int(self._pos.shape[0])

    def mode(self, k: int) -> Molecules:
        """The batch at mode k (0 is the best) as `Molecules`."""
        if not 0 <= int(k) < self.n_modes:
            raise IndexError(f'mode {k} of {self.n_modes}')
        m = self._mols
        return Molecules(m.lig_ptr, m.summary, m.status, m.elem, m.valence, m.frag, m.bonds, m.order, m.bond_ptr, self._pos[int(k)],
                         m.lig_elements, m._max_atoms, sizes=m._sizes)

    def sdf(self) -> List[str]:
        """Per ligand its found modes in rank order as consecutive MOL blocks, the layout of a gnina output file
        (gen_ligands_docked.sdf); the empty string for a ligand with no mode."""
        found = self.n_found.tolist()
        blocks = [self.mode(k).sdf(strict=False) for k in range(max(found, default=0))]
        return [''.join(blocks[k][b] for k in range(found[b])) for b in range(len(found))]

    def sym_rmsd(self, **kw) -> torch.Tensor:
        """[B,n_modes] float64: the symmetry-corrected RMSD (`Molecules.pose_rmsd`, whose keywords pass through) of every mode to
        the input pose, 0 for a mode that does not exist.  `report[:, :, 4]`, the atom-by-atom number, is never smaller."""
        r = self._mols.pose_rmsd(self._pos, **kw).rmsd
        exists = torch.arange(self.n_modes, device=r.device)[None, :] < self.n_found[:, None]
        return torch.where(exists, r, torch.zeros_like(r))

    def pose_check(self, san: 'Sanitized', *args, **kw) -> 'PoseChecks':
        """`Sanitized.pose_check` of every mode in one call ([B,n_modes] results; a mode that was not found is the input pose).
        `san`: the `Sanitized` whose `.molecules` were docked; the other arguments (pockets, radii, thresholds) pass through."""
        return _check_poses_of(san, self._mols, self._pos, args, kw)

    def mode_rmsd(self, **kw) -> torch.Tensor:
        """[B,n_modes,n_modes] float64: the symmetry-corrected RMSD between the modes of every ligand (symmetric, the diagonal 0);
        0 where either mode does not exist."""
        r = self._mols.pose_rmsd(self._pos, pairs=True, **kw).rmsd
        exists = torch.arange(self.n_modes, device=r.device)[None, :] < self.n_found[:, None]
        return torch.where(exists[:, :, None] & exists[:, None, :], r, torch.zeros_like(r))

    def distinct_modes(self, min_rmsd: float = 1.0, **kw) -> List[List[int]]:
        """Per ligand the modes that stay when the "Modes" rule of include/kpd.h is walked over the found modes in rank order with
        the symmetry-corrected RMSD: a mode is kept iff its `mode_rmsd` to every mode kept before is >= `min_rmsd`.  The modes
        `vina_dock` itself returned were told apart by the atom-by-atom number, so a pose with a flipped phenyl ring or a turned
        carboxylate can be among them twice; this drops the repeat.  A host walk over the [B,n_modes,n_modes] matrix."""
        r, found = self.mode_rmsd(**kw).cpu(), self.n_found.tolist()
        out = []
        for b, n in enumerate(found):
            kept: List[int] = []
            for k in range(n):
                if all(float(r[b, k, j]) >= float(min_rmsd) for j in kept):
                    kept.append(k)
            out.append(kept)
        return out

    def table(self) -> Dict[str, list]:
        """lig_idx, mode, score, rmsd_input, chain, as lists: one row per found mode, ligands in batch order, modes in rank order."""
        found, rep = self.n_found.tolist(), self.report.cpu()
        rows = [(b, k) for b in range(len(found)) for k in range(found[b])]
        return dict(lig_idx=[b for b, _ in rows], mode=[k for _, k in rows], score=[rep[b, k, 0].item() for b, k in rows],
                    rmsd_input=[rep[b, k, 4].item() for b, k in rows], chain=[int(rep[b, k, 6].item()) for b, k in rows])


class VinaMinimized:
    """What `Molecules.vina_minimize` returns: `.molecules` (a `Molecules` with the same bond graph at the minimised pose, so its
    `.sdf()` blocks are the counterpart of upstream's gen_ligands_gnina_minimized.sdf and `.vina_score(...)` gives the five terms
    there), `.pos` (a list of per-ligand [n_i,3] tensors), `.report` [B,16] float64 (columns hip.VINA_MIN_REPORT), `.status` [B]
    (bits: 1 no molecule, 2 bad input, 4 some atom took no part, 8 line search exhausted, 16 rotors frozen, 32 more than 8
    fragments, 64 max_iters reached before gtol; with 1, 2 or 32 the ligand is unchanged) and `.pocket_types` [M], device tensors.
    NOT gnina's or Vina's numbers: see include/kpd.h."""

    def __init__(self, mols: Molecules, pos: torch.Tensor, report: torch.Tensor, status: torch.Tensor, pocket_types: torch.Tensor):
        self.molecules = Molecules(mols.lig_ptr, mols.summary, mols.status, mols.elem, mols.valence, mols.frag, mols.bonds, mols.order,
                                   mols.bond_ptr, pos, mols.lig_elements, mols._max_atoms)
        self.report, self.status, self.pocket_types, self._sizes = report, status, pocket_types, mols._sizes
        self._input = mols

    def sym_rmsd(self, **kw) -> torch.Tensor:
        """[B] float64: the symmetry-corrected RMSD (`Molecules.pose_rmsd`, whose keywords pass through) of the minimised pose to
        the input pose; `report[:, 8]`, the atom-by-atom number, is never smaller.  0 for a ligand without a molecule."""
        return self._input.pose_rmsd(self.molecules.pos, **kw).rmsd[:, 0]

    def pose_check(self, san: 'Sanitized', *args, **kw) -> 'PoseChecks':
        """`Sanitized.pose_check` of the minimised pose.  `san`: the `Sanitized` whose `.molecules` were minimised; the other
        arguments (pockets, radii, thresholds) pass through."""
        return _check_poses_of(san, self._input, self.molecules.pos, args, kw)

    @property
    def pos(self) -> List[torch.Tensor]:
        sizes = self._sizes if self._sizes is not None else (self.molecules.lig_ptr[1:] - self.molecules.lig_ptr[:-1]).tolist()
        return list(torch.split(self.molecules.pos, sizes))

    def table(self) -> Dict[str, list]:
        """lig_idx, score_before, score_after, rmsd, n_rot, iterations, as lists; ligands that were left out (status bit 0, 1 or 5)
        have no row, as in `Relaxed.table`."""
        st, rep = self.status.cpu(), self.report.cpu()
        out_bits = hip.VINA_MIN_NO_MOLECULE | hip.VINA_MIN_BAD_INPUT | hip.VINA_MIN_FRAGMENTS
        keep = ((st & out_bits) == 0).nonzero().flatten().tolist()
        return dict(lig_idx=keep, score_before=rep[keep, 0].tolist(), score_after=rep[keep, 1].tolist(), rmsd=rep[keep, 8].tolist(),
                    n_rot=[int(v) for v in rep[keep, 13].tolist()], iterations=[int(v) for v in rep[keep, 11].tolist()])


class Relaxed:
    """What `Molecules.relax` returns: `.molecules` (a `Molecules` with the same bond graph at the relaxed positions, so `.sdf()`,
    `.metrics()` and `.keys()` work unchanged: its SDF blocks are upstream's pocket_minimized_ligands.sdf), `.pos` (a list of
    per-ligand [n_i,3] tensors), `.report` [B,12] float64 (columns hip.RELAX_REPORT) and `.status` [B] (bits: 1 no molecule,
    2 bad input, 4 max_iters reached before gtol, 8 line search exhausted; with 1 or 2 the ligand is unchanged), device tensors."""

    def __init__(self, mols: Molecules, pos: torch.Tensor, report: torch.Tensor, status: torch.Tensor):
        self.molecules = Molecules(mols.lig_ptr, mols.summary, mols.status, mols.elem, mols.valence, mols.frag, mols.bonds, mols.order,
                                   mols.bond_ptr, pos, mols.lig_elements, mols._max_atoms)
        self.report, self.status, self._sizes = report, status, mols._sizes
        self._input = mols

    def sym_rmsd(self, **kw) -> torch.Tensor:
        """[B] float64: the symmetry-corrected RMSD (`Molecules.pose_rmsd`, whose keywords pass through) of the relaxed pose to the
        input pose, upstream's `Chem.CalcRMS` column under the rule of include/kpd.h; `report[:, 2]`, the atom-by-atom number, is
        never smaller.  0 for a ligand without a molecule."""
        return self._input.pose_rmsd(self.molecules.pos, **kw).rmsd[:, 0]

    def pose_check(self, san: 'Sanitized', *args, **kw) -> 'PoseChecks':
        """`Sanitized.pose_check` of the relaxed pose.  `san`: the `Sanitized` whose `.molecules` were relaxed; the other
        arguments (pockets, radii, thresholds) pass through."""
        return _check_poses_of(san, self._input, self.molecules.pos, args, kw)

    @property
    def pos(self) -> List[torch.Tensor]:
        sizes = self._sizes if self._sizes is not None else (self.molecules.lig_ptr[1:] - self.molecules.lig_ptr[:-1]).tolist()
        return list(torch.split(self.molecules.pos, sizes))

    def table(self) -> Dict[str, list]:
        """Upstream's CSV columns (pocket_minimization.py: lig_idx, rmsd, energy_before, energy_after) plus pocket_energy (the
        ligand-pocket part of energy_after), as lists; ligands that were left out (status bit 0 or 1) have no row, as upstream
        skips a ligand it could not minimise.  Energies in the units of include/kpd.h's force field, not UFF's."""
        st = self.status.cpu()
        rep = self.report.cpu()
        keep = ((st & (hip.RELAX_NO_MOLECULE | hip.RELAX_BAD_INPUT)) == 0).nonzero().flatten().tolist()
        return dict(lig_idx=keep, rmsd=rep[keep, 2].tolist(), energy_before=rep[keep, 0].tolist(), energy_after=rep[keep, 1].tolist(),
                    pocket_energy=rep[keep, 9].tolist())


class VinaScores:
    """What `Molecules.vina_score` returns: `.report` [B,8] float64 (columns hip.VINA_REPORT: score, inter, the five weighted
    terms, n_rot) and `.status` [B] (bits: 1 no molecule, 2 bad input, 4 some atom took no part), `.score` [B] (NaN where status
    bit 0 or 1 is set), `.lig_types` [N] and `.pocket_types` [M] (flags 1 hydrophobic, 2 donor, 4 acceptor; -1 takes no part),
    device tensors; `.grad` / `.atom_score`: lists of per-ligand [n_i,3] / [n_i] float64 tensors, or None when not asked for.
    NOT gnina's or Vina's numbers: see include/kpd.h."""

    def __init__(self, mols: Molecules, out: Dict[str, torch.Tensor], pocket_types: torch.Tensor):
        self.report, self.status, self.lig_types, self.pocket_types = out['report'], out['status'], out['lig_type'], pocket_types
        self._grad, self._atom_score, self._mols = out.get('grad'), out.get('atom_score'), mols

    def _split(self, t):
        if t is None:
            return None
        m = self._mols
        return list(torch.split(t, m._sizes if m._sizes is not None else (m.lig_ptr[1:] - m.lig_ptr[:-1]).tolist()))

    @property
    def score(self) -> torch.Tensor:
        left_out = (self.status & (hip.VINA_NO_MOLECULE | hip.VINA_BAD_INPUT)) != 0
        return torch.where(left_out, torch.full_like(self.report[:, 0], float('nan')), self.report[:, 0])

    @property
    def grad(self):
        return self._split(self._grad)

    @property
    def atom_score(self):
        return self._split(self._atom_score)

    def table(self) -> Dict[str, list]:
        """lig_idx, score, inter, the five weighted terms, n_rot and efficiency = score / heavy atoms taking part, as lists;
        ligands that were left out (status bit 0 or 1) have no row, as in `Relaxed.table`."""
        st, rep = self.status.cpu(), self.report.cpu()
        keep = ((st & (hip.VINA_NO_MOLECULE | hip.VINA_BAD_INPUT)) == 0).nonzero().flatten().tolist()
        taking = [int((t >= 0).sum()) for t in self._split(self.lig_types.cpu())]
        out: Dict[str, list] = dict(lig_idx=keep)
        for k, name in enumerate(hip.VINA_REPORT[:7]):
            out[name] = rep[keep, k].tolist()
        out['n_rot'] = [int(v) for v in rep[keep, 7].tolist()]
        out['efficiency'] = [rep[b, 0].item() / taking[b] if taking[b] else 0.0 for b in keep]
        return out


def _check_poses_of(san: 'Sanitized', mols: Molecules, pos: torch.Tensor, args, kw) -> 'PoseChecks':
    """What the `pose_check` of `Relaxed`, `VinaMinimized` and `VinaDocked` share: the poses belong to the molecules `san` holds."""
    if not isinstance(san, Sanitized) or san.molecules.lig_ptr is not mols.lig_ptr or san.molecules.bonds is not mols.bonds:
        raise hip.KpdError('pose_check: pass the Sanitized whose .molecules these poses were computed from')
    return san.pose_check(pos, *args, **kw)


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
    mols = Molecules(ptr, m['summary'], m['status'], m['elem'], m['valence'], m['frag'], m['bonds'], m['order'], m['bond_ptr'],
                     hip._dev_f32(pos, 'pos'), lig_elements, sizes=sizes)
    mols._allowed = allowed
    if allowed_bonds is not None and 'H' in allowed_bonds:
        mols._allowed_h = _class_tables(['H'], allowed_bonds)[1][0]
    return mols


def training_keys(lig_pos: List[torch.Tensor], lig_feat: List[torch.Tensor], lig_elements: Sequence[str], largest_frag: bool = True,
                  with_orders: bool = True) -> torch.Tensor:
    """The keys of the training ligands as a sorted int64 tensor without repeats, for `set_metrics(train_keys=...)`.
    `lig_pos` / `lig_feat`: the processed dataset's ligand coordinates and one-hot features (GPU tensors, as for
    `build_molecules`).  The ligands are perceived by the same rule as the samples, so novelty compares like with like; pass
    the `largest_frag` / `with_orders` the samples' keys will be computed with.  Ligands without a molecule are left out."""
    mols = build_molecules(lig_pos, lig_feat, lig_elements)
    r = mols._keys(largest_frag, with_orders)
    return torch.unique(r['key'][(r['status'] & hip.KEY_NO_MOLECULE) == 0])


def training_keys_from_sdf(files, lig_elements: Sequence[str], largest_frag: bool = True, with_orders: bool = True,
                           remove_hydrogen: bool = True, device='cuda') -> torch.Tensor:
    """`training_keys` of ligands read from SDF files, with the bonds the files state (not perceived ones): a sorted int64 tensor
    without repeats.  Records without a molecule are left out.  Keys of file bonds compare with keys of samples only as far as
    the perceived bonds of the samples agree with what a file would state; with_orders=False compares connectivity alone."""
    mols = Molecules.from_sdf(files, lig_elements, remove_hydrogen=remove_hydrogen, device=device)
    r = mols._keys(largest_frag, with_orders)
    return torch.unique(r['key'][(r['status'] & hip.KEY_NO_MOLECULE) == 0])


def analyze_samples(samples: List[dict], lig_elements: Sequence[str], type_counts: Optional[torch.Tensor] = None,
                    allowed_bonds: Optional[Dict[str, object]] = None, connectivity_thresh: float = 0.5, device=None,
                    train_keys: Optional[torch.Tensor] = None, set_metrics: bool = False, sanitize: bool = False,
                    masses: Optional[Dict[str, float]] = None, smiles: bool = False, pose_check: bool = False, groups=False) -> Dict[str, float]:
    """The part of `ModelAnalyzer.sample_and_analyze` (analysis/metrics.py:60-100) that needs no rdkit: `samples` is the list
    of {'positions', 'features'} dicts `_sample` returns, one per pocket; the result is `Molecules.metrics` over all of them
    and, with `set_metrics=True`, `Molecules.set_metrics` as well (uniqueness, novelty against `train_keys` if given, and the
    diversity of every pocket's ligands).
    `_sample` hands its ligands back on the host: name the GPU to work on as `device` and they are copied there (one copy of
    the concatenated batch would do as well: `build_molecules` takes GPU tensors only and never computes on the host).
    `sanitize=True`: the numbers of `Sanitized.metrics` instead, upstream's seven in upstream's order of operations (`validity`
    first; connectivity, uniqueness, novelty and diversity over the ligands that sanitised) and the descriptor statistics; the
    rule is include/kpd.h's (`Molecules.sanitize`), NOT RDKit's.  With the default every key and value is what it was.
    `smiles=True` (implies `sanitize=True`): the result also has 'smiles', one list of strings per entry of `samples`: the SMILES
    of every ligand's largest fragment (upstream's `Chem.MolToSmiles(largest_mol)`; `Sanitized.smiles`, NOT RDKit's canonical
    form), '' for a ligand without a molecule.
    `pose_check=True` (implies `sanitize=True`): the result also has 'plausible', the fraction of the sanitised, connected ligands
    (those uniqueness is counted over) whose sampled pose passes `Sanitized.pose_check` without a pocket: NOT PoseBusters' number.
    `groups=True` or a `smarts.Patterns` (implies `sanitize=True`): the result also has 'group_frequency', name -> the fraction of the
    ligands that sanitised (`validity`'s numerator) that contain the query, for `smarts.FUNCTIONAL_GROUPS` or the given patterns
    (`Sanitized.match`: NOT RDKit's matcher).  Every other key and value is what it is without."""
    want_groups = groups is not False and groups is not None
    sanitize = sanitize or smiles or pose_check or want_groups
    lig_pos, lig_feat = [], []
    for rec in samples:
        lig_pos.extend(rec['positions'])
        lig_feat.extend(rec['features'])
    if device is not None:
        lig_pos, lig_feat = [p.to(device) for p in lig_pos], [f.to(device) for f in lig_feat]
    mols = build_molecules(lig_pos, lig_feat, lig_elements, allowed_bonds)
    if sanitize:
        group_ptr = torch.tensor([0] + [len(rec['positions']) for rec in samples], dtype=torch.int64).cumsum(0).to(torch.int32)
        san = mols.sanitize(masses=masses)
        out = san.metrics(type_counts, connectivity_thresh, group_ptr, train_keys)
        if smiles:
            strings, at = san.smiles(largest_frag=True), group_ptr.tolist()
            out['smiles'] = [strings[at[q]:at[q + 1]] for q in range(len(samples))]
        if pose_check:
            m = san.molecules
            n = (m.lig_ptr[1:] - m.lig_ptr[:-1]).double()
            keep = san.valid & (n > 0) & ((m.status & hip.MOL_BAD_SEGMENT) == 0) & (m.summary[:, 2].double() / n.clamp(min=1) >= connectivity_thresh)
            n_keep = int(keep.sum())
            out['plausible'] = float(san.pose_check().passed[:, 0][keep].double().mean()) if n_keep else 0.0
        if want_groups:
            pats = groups if isinstance(groups, smarts.Patterns) else smarts.compile(smarts.FUNCTIONAL_GROUPS)
            m = san.molecules
            ok = san.valid & ((m.lig_ptr[1:] - m.lig_ptr[:-1]) > 0) & ((m.status & hip.MOL_BAD_SEGMENT) == 0)
            n_ok = int(ok.sum())
            has = san.match(pats).has[ok].double().sum(0).cpu().tolist() if n_ok else [0.0] * pats.n
            out['group_frequency'] = {name: has[k] / n_ok if n_ok else 0.0 for k, name in enumerate(pats.names)}
        return out
    out = mols.metrics(type_counts, connectivity_thresh)
    if set_metrics:
        group_ptr = torch.tensor([0] + [len(rec['positions']) for rec in samples], dtype=torch.int64).cumsum(0).to(torch.int32)
        out.update(mols.set_metrics(group_ptr, train_keys, connectivity_thresh))
    return out


def check_samples(lig_pos: List[torch.Tensor], lig_feat: List[torch.Tensor], lig_elements: Sequence[str],
                  pocket_pos: Optional[List[torch.Tensor]] = None, pocket_elements: Optional[List[Sequence[str]]] = None, pocket_of=None,
                  allowed_bonds: Optional[Dict[str, object]] = None, radii: Optional[Dict[str, float]] = None, **thresholds) -> PoseChecks:
    """Perceive, sanitise and check sampled ligands in one go: `build_molecules(...).sanitize().pose_check(...)` on the lists every
    sampling entry point returns.  The limits of `Sanitized.pose_check` apply: NOT PoseBusters' numbers."""
    return build_molecules(lig_pos, lig_feat, lig_elements, allowed_bonds).sanitize().pose_check(
        None, pocket_pos, pocket_elements, pocket_of, radii=radii, **thresholds)


def relax_samples(samples: List[dict], pockets: List[dict], lig_elements: Sequence[str], device=None,
                  allowed_bonds: Optional[Dict[str, object]] = None, vdw: Optional[Dict[str, tuple]] = None, add_hs: bool = False,
                  **params) -> Relaxed:
    """The counterpart of `analyze_samples` for upstream's analysis/pocket_minimization.py: `samples` is the list of
    {'positions', 'features'} dicts `_sample` returns, one per pocket, and `pockets` one {'positions': [m,3] tensor, 'elements':
    m symbols} dict per entry, in the frame of its ligands.  All ligands are perceived and relaxed inside their own pocket in
    one batch (`Molecules.relax`, whose limits apply: the force field of include/kpd.h, NOT UFF); ligand k of the result is
    the k-th ligand in the order of `samples`.  `device`: the GPU to copy host tensors to, as for `analyze_samples`.
    `add_hs=True` (upstream's `pocket_minimization(add_hs=True)`): the ligands are sanitised and given explicit hydrogens
    (`Sanitized.add_hs`) before they are relaxed; the result's `.molecules` then carry the hydrogens."""
    if len(samples) != len(pockets):
        raise ValueError('samples and pockets must have one entry per pocket')
    lig_pos, lig_feat, pocket_of = [], [], []
    for q, rec in enumerate(samples):
        lig_pos.extend(rec['positions'])
        lig_feat.extend(rec['features'])
        pocket_of.extend([q] * len(rec['positions']))
    pocket_pos = [torch.as_tensor(p['positions']) for p in pockets]
    if device is not None:
        lig_pos, lig_feat = [p.to(device) for p in lig_pos], [f.to(device) for f in lig_feat]
        pocket_pos = [p.to(device) for p in pocket_pos]
    mols = build_molecules(lig_pos, lig_feat, lig_elements, allowed_bonds)
    if add_hs:
        mols = mols.sanitize().add_hs().molecules
    return mols.relax(pocket_pos, [list(p['elements']) for p in pockets], pocket_of=pocket_of, vdw=vdw, **params)


def hydrogenate_samples(samples: List[dict], lig_elements: Sequence[str], device=None,
                        allowed_bonds: Optional[Dict[str, object]] = None, largest_frag: bool = False,
                        masses: Optional[Dict[str, float]] = None) -> Hydrogenated:
    """Perceive, sanitise and hydrogenate all sampled ligands in one batch, in the mould of `relax_samples`: `samples` is the
    list of {'positions', 'features'} dicts `_sample` returns, one per pocket; ligand k of the result is the k-th ligand in the
    order of `samples`.  Stands where upstream calls `process_molecule(add_hydrogens=True)`; the rules are include/kpd.h's
    (`Molecules.sanitize`, `Sanitized.add_hs`), NOT RDKit's.  `device`: the GPU to copy host tensors to."""
    lig_pos, lig_feat = [], []
    for rec in samples:
        lig_pos.extend(rec['positions'])
        lig_feat.extend(rec['features'])
    if device is not None:
        lig_pos, lig_feat = [p.to(device) for p in lig_pos], [f.to(device) for f in lig_feat]
    mols = build_molecules(lig_pos, lig_feat, lig_elements, allowed_bonds)
    return mols.sanitize(largest_frag=largest_frag, masses=masses, allowed_bonds=allowed_bonds).add_hs()


def score_samples(samples: List[dict], pockets: List[dict], lig_elements: Sequence[str], device=None, relax: bool = False,
                  allowed_bonds: Optional[Dict[str, object]] = None, radii: Optional[Dict[str, float]] = None,
                  vdw: Optional[Dict[str, tuple]] = None, pocket_types=None, grad: bool = False, vina: Optional[Dict[str, float]] = None,
                  **relax_params):
    """Score every sampled ligand in its own pocket (`Molecules.vina_score`, whose limits apply: NOT gnina's numbers), in the
    mould of `relax_samples`: `samples` is the list of {'positions', 'features'} dicts `_sample` returns, one per pocket, and
    `pockets` one {'positions', 'elements'} dict per entry.  Returns the `VinaScores` of the sampled poses; with `relax=True`
    the ligands are also relaxed in their pockets (`Molecules.relax` with `vdw` and `relax_params`, e.g. max_iters) and the
    result is (scores of the raw poses, scores of the relaxed poses, the `Relaxed`).  The pocket types are computed once.
    `vina`: parameters of the score (w_gauss1 .. r_c)."""
    if len(samples) != len(pockets):
        raise ValueError('samples and pockets must have one entry per pocket')
    lig_pos, lig_feat, pocket_of = [], [], []
    for q, rec in enumerate(samples):
        lig_pos.extend(rec['positions'])
        lig_feat.extend(rec['features'])
        pocket_of.extend([q] * len(rec['positions']))
    pocket_pos = [torch.as_tensor(p['positions']) for p in pockets]
    if device is not None:
        lig_pos, lig_feat = [p.to(device) for p in lig_pos], [f.to(device) for f in lig_feat]
        pocket_pos = [p.to(device) for p in pocket_pos]
    pocket_elements = [list(p['elements']) for p in pockets]
    mols = build_molecules(lig_pos, lig_feat, lig_elements, allowed_bonds)
    raw = mols.vina_score(pocket_pos, pocket_elements, pocket_of=pocket_of, radii=radii, pocket_types=pocket_types, grad=grad, **(vina or {}))
    if not relax:
        return raw
    relaxed = mols.relax(pocket_pos, pocket_elements, pocket_of=pocket_of, vdw=vdw, **relax_params)
    after = relaxed.molecules.vina_score(pocket_pos, pocket_elements, pocket_of=pocket_of, radii=radii, pocket_types=raw.pocket_types,
                                         grad=grad, **(vina or {}))
    return raw, after, relaxed


def minimize_samples(samples: List[dict], pockets: List[dict], lig_elements: Sequence[str], device=None, relax: bool = False,
                     allowed_bonds: Optional[Dict[str, object]] = None, radii: Optional[Dict[str, float]] = None,
                     vdw: Optional[Dict[str, tuple]] = None, pocket_types=None, max_rotors: Optional[int] = None,
                     relax_params: Optional[Dict[str, float]] = None, **params):
    """Minimise every sampled ligand in its own pocket under the Vina-form score (`Molecules.vina_minimize`, whose limits apply:
    NOT gnina's numbers), in the mould of `relax_samples`: the counterpart of upstream's gen_docking_cmds.py --minimize.
    `samples` is the list of {'positions', 'features'} dicts `_sample` returns, one per pocket, and `pockets` one {'positions',
    'elements'} dict per entry.  Returns the `VinaMinimized`; with `relax=True` the ligands are first relaxed in their pockets
    (`Molecules.relax` with `vdw` and `relax_params`, e.g. dict(max_iters=...)), which is upstream's order, and the result is
    (the `Relaxed`, the `VinaMinimized` of the relaxed poses).  The pocket types are computed once.  `params`: the parameters of
    `Molecules.vina_minimize` (w_gauss1 .. r_c, w_intra, gtol, max_step, max_iters)."""
    if len(samples) != len(pockets):
        raise ValueError('samples and pockets must have one entry per pocket')
    lig_pos, lig_feat, pocket_of = [], [], []
    for q, rec in enumerate(samples):
        lig_pos.extend(rec['positions'])
        lig_feat.extend(rec['features'])
        pocket_of.extend([q] * len(rec['positions']))
    pocket_pos = [torch.as_tensor(p['positions']) for p in pockets]
    if device is not None:
        lig_pos, lig_feat = [p.to(device) for p in lig_pos], [f.to(device) for f in lig_feat]
        pocket_pos = [p.to(device) for p in pocket_pos]
    pocket_elements = [list(p['elements']) for p in pockets]
    mols = build_molecules(lig_pos, lig_feat, lig_elements, allowed_bonds)
    relaxed = None
    if relax:
        relaxed = mols.relax(pocket_pos, pocket_elements, pocket_of=pocket_of, vdw=vdw, **(relax_params or {}))
        mols = relaxed.molecules
    out = mols.vina_minimize(pocket_pos, pocket_elements, pocket_of=pocket_of, radii=radii, pocket_types=pocket_types, max_rotors=max_rotors,
                             **params)
    return (relaxed, out) if relax else out


def dock_samples(samples: List[dict], pockets: List[dict], lig_elements: Sequence[str], ref_ligands=None, relax: bool = False, device=None,
                 allowed_bonds: Optional[Dict[str, object]] = None, radii: Optional[Dict[str, float]] = None,
                 vdw: Optional[Dict[str, tuple]] = None, pocket_types=None, max_rotors: Optional[int] = None,
                 relax_params: Optional[Dict[str, float]] = None, **dock):
    """Dock every sampled ligand in its own pocket under the Vina-form score (`Molecules.vina_dock`, whose limits apply: NOT
    gnina's docking or numbers), beside `minimize_samples`: the counterpart of upstream's gen_docking_cmds.py without --minimize.
    `samples` and `pockets` as for `minimize_samples`; `ref_ligands`: one [n,3] reference ligand per pocket, whose bounding box
    widened by `autobox_add` is the search box (`--autobox_ligand`); without it every ligand searches the box of its own input
    pose.  Returns the `VinaDocked`; with `relax=True` the ligands are first relaxed in their pockets and the result is (the
    `Relaxed`, the `VinaDocked` of the relaxed poses).  `dock`: what `Molecules.vina_dock` takes (box, autobox_add, n_chains,
    n_steps, n_modes, seed, lig_ids and the parameters)."""
    if len(samples) != len(pockets):
        raise ValueError('samples and pockets must have one entry per pocket')
    lig_pos, lig_feat, pocket_of = [], [], []
    for q, rec in enumerate(samples):
        lig_pos.extend(rec['positions'])
        lig_feat.extend(rec['features'])
        pocket_of.extend([q] * len(rec['positions']))
    pocket_pos = [torch.as_tensor(p['positions']) for p in pockets]
    if device is not None:
        lig_pos, lig_feat = [p.to(device) for p in lig_pos], [f.to(device) for f in lig_feat]
        pocket_pos = [p.to(device) for p in pocket_pos]
    pocket_elements = [list(p['elements']) for p in pockets]
    mols = build_molecules(lig_pos, lig_feat, lig_elements, allowed_bonds)
    relaxed = None
    if relax:
        relaxed = mols.relax(pocket_pos, pocket_elements, pocket_of=pocket_of, vdw=vdw, **(relax_params or {}))
        mols = relaxed.molecules
    out = mols.vina_dock(pocket_pos, pocket_elements, pocket_of=pocket_of, autobox_ligand=ref_ligands, radii=radii,
                         pocket_types=pocket_types, max_rotors=max_rotors, **dock)
    return (relaxed, out) if relax else out
