"""Timing of kpd_relax next to kpd_mol_perceive (profiles/relax.md).
    python profiles/tools/relax_bench.py      HIP events around the raw C calls (buffers preallocated, no host sync inside)
The ligands are those of profiles/tools/molset_bench.py: seeded normal clouds of 1.6 A x (n / 20)^(1/3), one-hot features over
ten element classes; 6 400 ligands of 25 atoms, 100 per pocket, in 64 pockets of 300 atoms, and 64 ligands of 60 atoms in one
pocket of 300.  A pocket is 300 atoms drawn uniformly from the shell 4.5 .. 11 A around the origin, where the clouds sit."""
import sys, os, ctypes
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule

dev = torch.device('cuda:0')
L = hip.lib()
ELEMENTS = ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B']
POOL = [0, 0, 0, 1, 2, 3, 6, 5, 4, 7]
POCKET_ELEMENTS = ['C', 'C', 'C', 'N', 'O', 'S']
M = 300

def setup(B, n, group):
    g = torch.Generator().manual_seed(B * 1000 + n)
    N, P = B * n, B // group
    pos = (torch.randn(N, 3, generator=g) * 1.6 * (n / 20.0) ** (1.0 / 3.0)).to(dev)
    cls = torch.tensor(POOL)[torch.randint(0, len(POOL), (N,), generator=g)]
    feat = torch.nn.functional.one_hot(cls, len(ELEMENTS)).float().to(dev)
    r = (4.5 ** 3 + (11.0 ** 3 - 4.5 ** 3) * torch.rand(P * M, generator=g)) ** (1.0 / 3.0)
    d = torch.randn(P * M, 3, generator=g)
    px = (d / d.norm(dim=1, keepdim=True) * r[:, None]).to(dev)
    pel = [POCKET_ELEMENTS[k] for k in torch.randint(0, len(POCKET_ELEMENTS), (P * M,), generator=g).tolist()]
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    o = dict(B=B, N=N, n=n, P=P, pos=pos, feat=feat, ptr=(torch.arange(B + 1, dtype=torch.int32) * n).to(dev),
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev), elem=i32(N),
             valence=i32(N), frag=i32(N), bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B),
             lig_vdw=torch.tensor(molecule.vdw_table(ELEMENTS), dtype=torch.float32, device=dev), px=px,
             pv=torch.tensor(molecule.vdw_table(pel), dtype=torch.float32, device=dev),
             pptr=(torch.arange(P + 1, dtype=torch.int32) * M).to(dev), pof=(torch.arange(B, dtype=torch.int32) // group).to(dev),
             out=torch.empty(N, 3, device=dev), report=torch.empty(B, 12, dtype=torch.float64, device=dev), rstatus=i32(B))
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    return o

def perceive(o):
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * o['N'], o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))

def relax(o, max_iters=400):
    p = hip.relax_params(max_iters=max_iters)
    hip.check(L.kpd_relax(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['n'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(),
              o['lig_vdw'].data_ptr(), o['bonds'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), o['px'].data_ptr(),
              o['pv'].data_ptr(), o['pptr'].data_ptr(), o['P'] * M, o['P'], M, o['pof'].data_ptr(), ctypes.byref(p), o['out'].data_ptr(),
              o['report'].data_ptr(), o['rstatus'].data_ptr(), None))

def timed(fn, reps, warm):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    return np.array(ts)

def show(ts):
    return f'median {np.median(ts):.1f} us, min {ts.min():.1f}, max {ts.max():.1f} ({len(ts)} runs)'

for B, n, group in ((6400, 25, 100), (64, 60, 64)):
    o = setup(B, n, group)
    perceive(o); relax(o); torch.cuda.synchronize()
    rep, st = o['report'], o['rstatus']
    nb = (o['bond_ptr'][1:] - o['bond_ptr'][:-1]).double()
    evals = float(rep[:, 5].sum())
    # non-bonded pairs one evaluation visits: every ligand atom x its pocket, and every ordered pair of ligand atoms
    pairs = B * n * (M + n - 1)
    print(f'B={B} x {n} atoms in {o["P"]} pockets of {M}: status bits {[int((st & b).ne(0).sum()) for b in (1, 2, 4, 8)]}, mean iterations '
          f'{float(rep[:, 4].mean()):.1f}, mean evaluations {float(rep[:, 5].mean()):.1f}, mean E before {float(rep[:, 0].mean()):.1f} after '
          f'{float(rep[:, 1].mean()):.1f}, mean pocket part before {float(rep[:, 10].mean()):.1f} after {float(rep[:, 9].mean()):.1f}, mean rmsd '
          f'{float(rep[:, 2].mean()):.3f}, median gmax after {float(rep[:, 3].median()):.2e}, bonds per ligand {float(nb.mean()):.1f}')
    tp = timed(lambda: perceive(o), 50, 5)
    tr = timed(lambda: relax(o), 5, 1)
    t1 = timed(lambda: relax(o, 0), 20, 3)
    med = float(np.median(tr))
    print('  kpd_mol_perceive           ', show(tp))
    print('  kpd_relax, max_iters = 400 ', show(tr))
    print('  kpd_relax, max_iters = 0   ', show(t1))
    print(f'  per evaluation of the batch {med / (evals / B):.1f} us; {evals * n * (M + n - 1) / (med * 1e-6) / 1e9:.1f} G pair visits/s '
          f'({pairs} pair visits per evaluation of the batch)')
