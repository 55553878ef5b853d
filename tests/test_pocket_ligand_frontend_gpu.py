"""kpd_relax and kpd_vina_score take "one perceived ligand and its pocket" through one front end (csrc/molecule_core.h): on the same
malformed batch both must leave out the same ligands with the same status bits 0 and 1, and touch nothing of them.  The batch is the
six-ligand one of test_relax_gpu.test_left_out_ligands and test_vina_gpu.test_bad_inputs; every raw call runs with canaries."""
import copy

import numpy as np
import pytest

from . import test_relax_gpu as TR
from . import test_vina_gpu as TV
from .molecule_cases import Z, one_hot
from .relax_cases import grow, make_pocket

pytestmark = pytest.mark.gpu


def edited(inp, **edits):
    """`inp` with the named device tensors of what kpd_mol_perceive left replaced by edited copies; edits: name -> {index: value}."""
    c = copy.copy(inp)
    c.t = dict(inp.t)
    for name, changes in edits.items():
        c.t[name] = inp.t[name].clone()
        for i, v in changes.items():
            c.t[name][i] = v
    return c


def test_relax_and_vina_leave_out_the_same_ligands(cuda):
    rng = np.random.default_rng(3)
    ligs = [(one_hot(s), p) for s, p in (grow(rng, n) for n in (9, 12, 7, 15, 11, 6))]
    anchor = np.concatenate([p for _, p in ligs])
    pockets = [make_pocket(rng, 20, anchor, reach=4.0), make_pocket(rng, 90, anchor, reach=4.0)]
    pocket_of = [0, 1, 0, 1, 1, -1]
    rx, vn = TR.Inputs(cuda, ligs, pockets, pocket_of), TV.Inputs(cuda, ligs, pockets, pocket_of)
    ty, _ = TV.pocket_types_gpu(vn)
    ptr, N, B, F, cap = [int(a) for a in rx.ptr], rx.pos.shape[0], rx.B, len(Z), rx.t['cap']
    nan_pos, inf_px = rx.pos.copy(), rx.px.copy()
    nan_pos[ptr[1] + 3, 1] = np.nan
    inf_px[int(rx.pptr[1]) + 50, 2] = np.inf                     # row 50 of pocket 1: beyond the 10 staged rows
    cases = [                                                    # (edits of the perceived tensors, arguments, status & 3 of every ligand)
        ({}, {}, [0, 0, 0, 0, 0, 0]),
        (dict(ptr={3: N + 5}), {}, [0, 0, 1, 1, 0, 0]),          # ligand 2 ends, ligand 3 starts beyond the atoms
        (dict(bond_ptr={B: cap + 1}), {}, [0, 0, 0, 0, 0, 1]),   # ligand 5: bonds beyond cap_bonds
        ({}, dict(pocket_of=[0, 1, 2, 1, 1, -2]), [0, 0, 2, 0, 0, 2]),      # pocket_of = P, and below -1
        ({}, dict(pos=nan_pos), [0, 2, 0, 0, 0, 0]),
        ({}, dict(px=inf_px, max_pocket=10), [0, 2, 0, 2, 2, 0]),            # every ligand of pocket 1
        (dict(elem={ptr[0]: -1, ptr[4] + 2: F}), {}, [1, 0, 0, 0, 1, 0]),    # a class below 0, and F
    ]
    for edits, args, want in cases:
        out, rep, st = TR.relax_gpu(edited(rx, **edits), max_atoms=16, max_iters=10, **args)
        o = TV.score_gpu(edited(vn, **edits), ty, max_atoms=16, **args)
        assert (st & 3).tolist() == (o['status'] & 3).tolist() == want, (edits, list(args), st, o['status'])
        pos_in = np.asarray(args.get('pos', rx.pos), dtype=np.float32)
        for b in range(B):
            if want[b]:
                rows = slice(ptr[b], ptr[b + 1])
                assert TV.bits(out[rows]) == TV.bits(pos_in[rows]) and not rep[b].any(), (edits, list(args), b)
                assert not o['report'][b].any(), (edits, list(args), b)
