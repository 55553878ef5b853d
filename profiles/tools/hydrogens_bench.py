"""Timing of kpd_mol_add_hs next to kpd_mol_sanitize (profiles/hydrogens.md).
    python profiles/tools/hydrogens_bench.py    HIP events around the raw C calls (buffers preallocated, no host sync inside)
The protocol and the ligands of profiles/tools/sanitize_bench.py: the seeded generator of tests/sanitize_cases.py, 6 400 ligands
of about 25 atoms (400 distinct ones, repeated) and 64 two-fragment ligands of about 60 atoms; median of 50 calls after 5 warm-up
calls.  The generator lives in the tests package: run this from a full checkout of the repository."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule
from tests import sanitize_cases as C
from tests.molecule_cases import ELEMENTS, one_hot

dev = torch.device('cuda:0')
L = hip.lib()
ELEMENTS_H = ELEMENTS + ['H']
F = len(ELEMENTS_H)

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
    feat = torch.from_numpy(np.concatenate([np.pad(one_hot(s), ((0, 0), (0, 1))) for s, _ in ligs])).to(dev)      # an empty H column
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS_H, None)
    mass, mass_h = molecule.mass_table(ELEMENTS_H)
    o = dict(B=B, N=N, pos=pos, feat=feat, ptr=torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev),
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev),
             mass=torch.tensor(mass, dtype=torch.float64, device=dev), mass_h=mass_h, elem=i32(N), valence=i32(N), frag=i32(N),
             bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B), order_k=i32(3 * N),
             bond_flags=i32(3 * N), valence_k=i32(N), atom_h=i32(N), atom_flags=i32(N), desc_i=i32(B, 10),
             desc_f=torch.empty(B, 2, dtype=torch.float64, device=dev), valid=i32(B), san_status=i32(B))
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    o['s2'] = torch.empty(int(L.kpd_mol_add_hs_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    return o

def perceive(o):
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], F, o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * o['N'], o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))

def sanitize(o, largest=0):
    hip.check(L.kpd_mol_sanitize(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), F, o['z'].data_ptr(),
              o['allowed'].data_ptr(), o['mass'].data_ptr(), o['mass_h'], o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(),
              o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), largest, o['order_k'].data_ptr(), o['bond_flags'].data_ptr(),
              o['valence_k'].data_ptr(), o['atom_h'].data_ptr(), o['atom_flags'].data_ptr(), o['desc_i'].data_ptr(), o['desc_f'].data_ptr(),
              o['valid'].data_ptr(), o['san_status'].data_ptr(), None))

def outputs(o):
    """Sized as hip.mol_add_hs sizes them: from one device sum of atom_h."""
    n_h = int(o['atom_h'].sum().item())
    ca, cb = o['N'] + n_h, 3 * o['N'] + n_h
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    o.update(ca=ca, cb=cb, out_ptr=i32(o['B'] + 1), out_pos=torch.empty(ca, 3, device=dev), out_elem=i32(ca), out_valence=i32(ca),
             out_frag=i32(ca), out_bonds=i32(cb, 2), out_order=i32(cb), out_bond_ptr=i32(o['B'] + 1), out_summary=i32(o['B'], 4),
             parent=i32(ca), source=i32(ca), n_h=i32(o['B']), hs_status=i32(o['B']))

def add_hs(o, largest=0):
    hip.check(L.kpd_mol_add_hs(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), F, o['z'].data_ptr(),
              o['allowed'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order_k'].data_ptr(), o['bond_ptr'].data_ptr(),
              3 * o['N'], o['status'].data_ptr(), o['san_status'].data_ptr(), o['valence_k'].data_ptr(), o['atom_h'].data_ptr(),
              o['atom_flags'].data_ptr(), largest, F - 1, o['ca'], o['cb'],
              *[o[k].data_ptr() for k in ('out_ptr', 'out_pos', 'out_elem', 'out_valence', 'out_frag', 'out_bonds', 'out_order', 'out_bond_ptr',
                                          'out_summary', 'parent', 'source', 'n_h', 'hs_status')], o['s2'].data_ptr(), None))

def timed(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), f'median {np.median(ts):.1f} us, min {ts.min():.1f}, max {ts.max():.1f} ({reps} runs)'

small = pool(20, 30, 400)
mid = pool(25, 35, 128)
far = np.array([30.0, 0.0, 0.0], dtype=np.float32)
cases = (('B = 6400 x about 25 atoms', [small[k % len(small)] for k in range(6400)]),
         ('B = 64 x about 60 atoms (two fragments each)', [(mid[2 * k][0] + mid[2 * k + 1][0], np.concatenate([mid[2 * k][1], mid[2 * k + 1][1] + far])) for k in range(64)]))
for name, ligs in cases:
    o = setup(ligs)
    perceive(o); sanitize(o); outputs(o); add_hs(o); torch.cuda.synchronize()
    st = o['hs_status']
    print(f'{name}: {o["N"]} atoms ({o["N"] / o["B"]:.1f} per ligand), {int(o["summary"][:, 0].sum())} bonds; hydrogens added {int(o["n_h"].sum())} '
          f'({float(o["n_h"].double().mean()):.1f} per ligand), output {int(o["out_ptr"][-1])} atoms, {int(o["out_bond_ptr"][-1])} bonds; ligands with the '
          f'general rule {int(((st & hip.HS_GENERAL) != 0).sum())}, copied through {int(((st & 19) != 0).sum())}, no room {int(((st & 4) != 0).sum())}')
    ts, ss = timed(lambda: sanitize(o))
    th, sh = timed(lambda: add_hs(o))
    sanitize(o, 1); torch.cuda.synchronize()
    tl, sl = timed(lambda: add_hs(o, 1))
    print('  kpd_mol_sanitize, every atom      ', ss)
    print('  kpd_mol_add_hs, every atom        ', sh, f'= {th / ts:.2f} x sanitize')
    print('  kpd_mol_add_hs, largest fragment  ', sl, f'= {tl / ts:.2f} x sanitize')
