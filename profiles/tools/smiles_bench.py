"""Timing of kpd_mol_smiles next to kpd_mol_sanitize and kpd_mol_perceive (profiles/smiles.md).
    python profiles/tools/smiles_bench.py    HIP events around the raw C calls (buffers preallocated, no host sync inside)
The workloads are those of profiles/tools/sanitize_bench.py: 6 400 generated ring-bearing ligands of about 25 atoms (400 distinct
ones, repeated) and 64 two-fragment ligands of about 60 atoms.  Also printed: how many rounds the tie-breaking loop of the rule
takes on the distinct ligands (counted by the restatement tests/smiles_ref.py on the device's own sanitised graphs).
The generator and the restatement live in the tests package: run this from a full checkout of the repository."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule
from tests import sanitize_cases as C
from tests import smiles_ref as S
from tests.molecule_cases import ELEMENTS, one_hot

dev = torch.device('cuda:0')
L = hip.lib()

def pool(lo, hi, want):
    out, seed = [], 90000
    while len(out) < want:
        sym, pos, _ = C.generate(seed)
        seed += 1
        if lo <= len(sym) <= hi:
            out.append((sym, pos))
    return out

def setup(ligs):
    sizes = [len(s) for s, _ in ligs]
    B, N = len(ligs), sum(sizes)
    pos = torch.from_numpy(np.concatenate([p for _, p in ligs]).astype(np.float32)).to(dev)
    feat = torch.from_numpy(np.concatenate([one_hot(s) for s, _ in ligs])).to(dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    mass, mass_h = molecule.mass_table(ELEMENTS)
    o = dict(B=B, N=N, pos=pos, feat=feat, ptr=torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev),
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev),
             mass=torch.tensor(mass, dtype=torch.float64, device=dev), mass_h=mass_h, elem=i32(N), valence=i32(N), frag=i32(N),
             bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B), order_k=i32(3 * N),
             bond_flags=i32(3 * N), valence_k=i32(N), atom_h=i32(N), atom_flags=i32(N), desc_i=i32(B, 10),
             desc_f=torch.empty(B, 2, dtype=torch.float64, device=dev), valid=i32(B), san_status=i32(B),
             symbols=hip._packed_symbols(ELEMENTS, dev), cap=8 * N, text=torch.empty(8 * N, dtype=torch.uint8, device=dev),
             text_ptr=torch.empty(B + 1, dtype=torch.int64, device=dev), smi_status=i32(B), zlist=z)
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    o['s2'] = torch.empty(int(L.kpd_smiles_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    return o

def perceive(o):
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * o['N'], o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))

def sanitize(o, largest=0):
    hip.check(L.kpd_mol_sanitize(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), o['mass'].data_ptr(), o['mass_h'], o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(),
              o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), largest, o['order_k'].data_ptr(), o['bond_flags'].data_ptr(),
              o['valence_k'].data_ptr(), o['atom_h'].data_ptr(), o['atom_flags'].data_ptr(), o['desc_i'].data_ptr(), o['desc_f'].data_ptr(),
              o['valid'].data_ptr(), o['san_status'].data_ptr(), None))

def smiles(o, largest=0, aromatic=1):
    hip.check(L.kpd_mol_smiles(o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(), o['symbols'].data_ptr(),
              o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order_k'].data_ptr(), o['bond_flags'].data_ptr(), o['bond_ptr'].data_ptr(),
              3 * o['N'], o['status'].data_ptr(), o['san_status'].data_ptr(), o['atom_h'].data_ptr(), o['atom_flags'].data_ptr(), largest,
              aromatic, o['text'].data_ptr(), o['cap'], o['text_ptr'].data_ptr(), o['smi_status'].data_ptr(), o['s2'].data_ptr(), None))

def timed(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), f'median {np.median(ts):.1f} us, min {ts.min():.1f}, max {ts.max():.1f} ({reps} runs)'

def tie_rounds(o, count):
    """Rounds of the tie-breaking loop on the first `count` ligands, by the restatement on the device's sanitised graphs."""
    ptr, bp = o['ptr'].tolist(), o['bond_ptr'].tolist()
    elem, h, fl = o['elem'].tolist(), o['atom_h'].tolist(), o['atom_flags'].tolist()
    bonds, ok, bf = o['bonds'].tolist(), o['order_k'].tolist(), o['bond_flags'].tolist()
    rounds = []
    for b in range(count):
        a0, a1, p0, p1 = ptr[b], ptr[b + 1], bp[b], bp[b + 1]
        rows = [(i - a0, j - a0) for i, j in bonds[p0:p1]]
        labels = [4 if f & 4 else k for k, f in zip(ok[p0:p1], bf[p0:p1])]
        rounds.append(S.canonical_ranks([o['zlist'][e] for e in elem[a0:a1]], h[a0:a1], [f >> 1 & 1 for f in fl[a0:a1]], rows, labels)[1])
    return rounds

small = pool(20, 30, 400)
mid = pool(25, 35, 128)
far = np.array([30.0, 0.0, 0.0], dtype=np.float32)
cases = (('B = 6400 x about 25 atoms', [small[k % len(small)] for k in range(6400)], 400),
         ('B = 64 x about 60 atoms (two fragments each)', [(mid[2 * k][0] + mid[2 * k + 1][0], np.concatenate([mid[2 * k][1], mid[2 * k + 1][1] + far])) for k in range(64)], 64))
for name, ligs, distinct in cases:
    o = setup(ligs)
    perceive(o); sanitize(o); smiles(o); torch.cuda.synchronize()
    at = o['text_ptr'].tolist()
    text = bytes(o['text'][:at[-1]].cpu().numpy()).decode()
    r = tie_rounds(o, distinct)
    print(f'{name}: {o["N"]} atoms ({o["N"] / o["B"]:.1f} per ligand), {at[-1]} bytes of text ({at[-1] / o["B"]:.1f} per ligand), status '
          f'{int(o["smi_status"].max())}; tie-breaking rounds over {distinct} distinct ligands: max {max(r)}, mean {sum(r) / len(r):.2f}')
    print('  first strings:', [text[at[b]:at[b + 1]] for b in range(3)])
    tp, sp = timed(lambda: perceive(o))
    ts, ss = timed(lambda: sanitize(o))
    ta, sa = timed(lambda: smiles(o))
    tk, sk = timed(lambda: smiles(o, 0, 0))
    sanitize(o, 1); torch.cuda.synchronize()
    tl, sl = timed(lambda: smiles(o, 1, 1))
    print('  kpd_mol_perceive                   ', sp)
    print('  kpd_mol_sanitize, every atom       ', ss)
    print('  kpd_mol_smiles, aromatic form      ', sa, f'= {ta / ts:.2f} x sanitize')
    print('  kpd_mol_smiles, Kekule form        ', sk, f'= {tk / ts:.2f} x sanitize')
    print('  kpd_mol_smiles, largest fragment   ', sl, f'= {tl / ts:.2f} x sanitize')
