"""Timing of kpd_pose_rmsd next to kpd_mol_sanitize and kpd_mol_keys (profiles/pose_rmsd.md).
    python profiles/tools/pose_rmsd_bench.py    HIP events around the raw C calls (buffers preallocated, no host sync inside)
The workloads are those of profiles/tools/smiles_bench.py: 6 400 generated ring-bearing ligands of about 25 atoms (400 distinct
ones, repeated) and 64 two-fragment ligands of about 60 atoms, each with K = 1 pose against the reference; and 640 of the first
kind with 9 poses each and pairs = 1 (36 searches per ligand), the shape of a docking run's modes.  A pose is the reference
displaced by a seeded Gaussian of 0.3 A per coordinate (K = 1) or 0.5 A (the nine).  Also printed: the node counts of the
searches and how many of them found a map better than the identity.
The generator lives in the tests package: run this from a full checkout of the repository."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule
from tests import sanitize_cases as C
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

def setup(ligs, K, pairs, sigma):
    sizes = [len(s) for s, _ in ligs]
    B, N = len(ligs), sum(sizes)
    ref = np.concatenate([p for _, p in ligs]).astype(np.float32)
    rng = np.random.default_rng(7)
    poses = (ref[None] + rng.standard_normal((K, N, 3)) * sigma).astype(np.float32)
    feat = torch.from_numpy(np.concatenate([one_hot(s) for s, _ in ligs])).to(dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    mass, mass_h = molecule.mass_table(ELEMENTS)
    per = (K, K) if pairs else (K,)
    o = dict(B=B, N=N, K=K, pairs=int(pairs), pos=torch.from_numpy(ref).to(dev), poses=torch.from_numpy(poses).to(dev), feat=feat,
             ptr=torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev),
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev),
             mass=torch.tensor(mass, dtype=torch.float64, device=dev), mass_h=mass_h, elem=i32(N), valence=i32(N), frag=i32(N),
             bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B), order_k=i32(3 * N),
             bond_flags=i32(3 * N), valence_k=i32(N), atom_h=i32(N), atom_flags=i32(N), desc_i=i32(B, 10), desc_f=f64(B, 2), valid=i32(B),
             san_status=i32(B), key=torch.empty(B, dtype=torch.int64, device=dev), fp=i32(B, 64), key_status=i32(B),
             rmsd=f64(B, *per), plain=f64(B, *per), nodes=torch.empty(B, *per, dtype=torch.int64, device=dev), map=i32(K, N), pr_status=i32(B))
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    o['s2'] = torch.empty(int(L.kpd_pose_rmsd_scratch_bytes(N, K, int(pairs))), dtype=torch.uint8, device=dev)
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

def keys(o):
    hip.check(L.kpd_mol_keys(o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(), o['frag'].data_ptr(),
              o['bonds'].data_ptr(), o['order'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), 0, 0, 2, 2048,
              o['key'].data_ptr(), o['fp'].data_ptr(), None, o['key_status'].data_ptr(), None))

def pose_rmsd(o, with_map=True):
    hip.check(L.kpd_pose_rmsd(o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(), o['frag'].data_ptr(),
              o['bonds'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), None, None, 0, 1,
              None if o['pairs'] else o['pos'].data_ptr(), o['poses'].data_ptr(), o['K'], o['pairs'], 65536, o['rmsd'].data_ptr(),
              o['plain'].data_ptr(), o['map'].data_ptr() if with_map and not o['pairs'] else None, o['nodes'].data_ptr(),
              o['pr_status'].data_ptr(), o['s2'].data_ptr(), None))

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
two = [(mid[2 * k][0] + mid[2 * k + 1][0], np.concatenate([mid[2 * k][1], mid[2 * k + 1][1] + far])) for k in range(64)]
cases = (('B = 6400 x about 25 atoms, K = 1', [small[k % len(small)] for k in range(6400)], 1, False, 0.3),
         ('B = 64 x about 60 atoms (two fragments each), K = 1', two, 1, False, 0.3),
         ('B = 640 x about 25 atoms, 9 poses, pairs = 1', [small[k % len(small)] for k in range(640)], 9, True, 0.5))
for name, ligs, K, pairs, sigma in cases:
    o = setup(ligs, K, pairs, sigma)
    perceive(o); sanitize(o); keys(o); pose_rmsd(o); torch.cuda.synchronize()
    nodes, rmsd, plain = o['nodes'].cpu().numpy(), o['rmsd'].cpu().numpy(), o['plain'].cpu().numpy()
    used = np.triu(np.ones((K, K), dtype=bool), 1)[None].repeat(o['B'], 0) if pairs else np.ones_like(nodes, dtype=bool)
    print(f'{name}: {o["N"]} atoms ({o["N"] / o["B"]:.1f} per ligand), {int(used.sum())} searches, scratch {o["s2"].numel()} bytes, status '
          f'{int(o["pr_status"].max())}; nodes per search: max {int(nodes[used].max())}, mean {nodes[used].mean():.1f}; rmsd < plain in '
          f'{int((rmsd[used] < plain[used]).sum())} searches; mean rmsd {rmsd[used].mean():.3f}, mean plain {plain[used].mean():.3f}')
    ts, ss = timed(lambda: sanitize(o))
    tk, sk = timed(lambda: keys(o))
    tr, sr = timed(lambda: pose_rmsd(o))
    tn, sn = timed(lambda: pose_rmsd(o, False))
    print('  kpd_mol_sanitize, every atom       ', ss)
    print('  kpd_mol_keys, every atom           ', sk)
    print('  kpd_pose_rmsd                      ', sr, f'= {tr / ts:.2f} x sanitize, {tr / tk:.2f} x keys')
    print('  kpd_pose_rmsd, map = NULL          ', sn, f'= {tn / ts:.2f} x sanitize, {tn / tk:.2f} x keys')
