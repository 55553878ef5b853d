"""Timing of kpd_pose_check next to kpd_vina_score (profiles/pose_check.md).
    python profiles/tools/pose_check_bench.py    HIP events around the raw C calls (buffers preallocated, no host sync inside)
The ligands are those of profiles/tools/pose_rmsd_bench.py: 6 400 generated ring-bearing ligands of about 25 atoms (400 distinct
ones, repeated) in 64 pockets of 300 atoms, 100 ligands to a pocket; 64 two-fragment ligands of about 60 atoms in one pocket of 300;
and 640 of the first kind with 9 poses each (a docking run's modes), 10 ligands to a pocket.  A pocket is 300 seeded points (C, N, O,
S) in a ball of 12 A around its first ligand, none within 3 A of that ligand's atoms; the other ligands of the pocket lie where the
generator put them, so some clash.  Pose k > 0 is pose 0 displaced by a seeded Gaussian of 0.5 A per coordinate.  kpd_vina_score (pose
0, no gradient) is timed in the same run as the yardstick.  Also printed: how many poses fail which check and the lattice counts.
The generator lives in the tests package: run this from a full checkout of the repository."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule
from tests import sanitize_cases as C
from tests.molecule_cases import ELEMENTS, one_hot

dev = torch.device('cuda:0')
L = hip.lib()
POCKET_ATOMS, POOL = 300, ('C', 'C', 'C', 'N', 'O', 'S')

def pool(lo, hi, want):
    out, seed = [], 90000
    while len(out) < want:
        sym, pos, _ = C.generate(seed)
        seed += 1
        if lo <= len(sym) <= hi:
            out.append((sym, pos))
    return out

def make_pocket(rng, anchor):
    c, pts = anchor.mean(0), []
    while len(pts) < POCKET_ATOMS:
        v = rng.standard_normal(3)
        q = c + v / np.linalg.norm(v) * 12.0 * rng.random() ** (1.0 / 3.0)
        if np.linalg.norm(anchor - q, axis=1).min() >= 3.0:
            pts.append(q)
    return [POOL[int(rng.integers(len(POOL)))] for _ in pts], np.array(pts, dtype=np.float32)

def setup(ligs, K, per_pocket):
    sizes = [len(s) for s, _ in ligs]
    B, N = len(ligs), sum(sizes)
    rng = np.random.default_rng(7)
    ref = np.concatenate([p for _, p in ligs]).astype(np.float32)
    poses = np.stack([ref] + [(ref + rng.standard_normal((N, 3)) * 0.5).astype(np.float32) for _ in range(K - 1)])
    P = (B + per_pocket - 1) // per_pocket
    pockets = [make_pocket(rng, np.asarray(ligs[q * per_pocket][1], dtype=np.float64)) for q in range(P)]
    psym = [s for sy, _ in pockets for s in sy]
    M = len(psym)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    f32t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    mass, mass_h = molecule.mass_table(ELEMENTS)
    o = dict(B=B, N=N, K=K, M=M, P=P, pos=torch.from_numpy(ref).to(dev), poses=torch.from_numpy(poses).to(dev),
             feat=torch.from_numpy(np.concatenate([one_hot(s) for s, _ in ligs])).to(dev),
             ptr=torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev),
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev),
             mass=torch.tensor(mass, dtype=torch.float64, device=dev), mass_h=mass_h, elem=i32(N), valence=i32(N), frag=i32(N),
             bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B), order_k=i32(3 * N),
             bond_flags=i32(3 * N), valence_k=i32(N), atom_h=i32(N), atom_flags=i32(N), desc_i=i32(B, 10), desc_f=f64(B, 2), valid=i32(B),
             san_status=i32(B), max_atoms=max(sizes),
             pocket_x=torch.from_numpy(np.concatenate([p for _, p in pockets])).to(dev),
             pocket_ptr=torch.arange(P + 1, dtype=torch.int32, device=dev) * POCKET_ATOMS,
             pocket_of=(torch.arange(B, dtype=torch.int32, device=dev) // per_pocket).to(torch.int32),
             pocket_z=torch.tensor([molecule.ATOMIC_NUMBERS[s] for s in psym], dtype=torch.int32, device=dev),
             vdw_lig=f32t(molecule.vdw_radius_table(ELEMENTS)), vdw_pocket=f32t(molecule.vdw_radius_table(psym)),
             xs_lig=f32t(molecule.xs_radius_table(ELEMENTS, {'B': 2.0})), xs_pocket=f32t(molecule.xs_radius_table(psym)),
             pocket_type=i32(M), pocket_status=i32(P), fail=i32(B, K), report=f64(B, K, len(hip.CHECK_REPORT)),
             counts=i32(B, K, len(hip.CHECK_COUNTS)), atom_fail=i32(K, N), pc_status=i32(B, K), v_report=f64(B, 8), v_type=i32(N), v_status=i32(B))
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    return o

def perceive(o):
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * o['N'], o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))

def sanitize(o):
    hip.check(L.kpd_mol_sanitize(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), o['mass'].data_ptr(), o['mass_h'], o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(),
              o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), 0, o['order_k'].data_ptr(), o['bond_flags'].data_ptr(),
              o['valence_k'].data_ptr(), o['atom_h'].data_ptr(), o['atom_flags'].data_ptr(), o['desc_i'].data_ptr(), o['desc_f'].data_ptr(),
              o['valid'].data_ptr(), o['san_status'].data_ptr(), None))

def pocket_types(o):
    hip.check(L.kpd_vina_pocket_types(o['pocket_x'].data_ptr(), o['pocket_z'].data_ptr(), o['pocket_ptr'].data_ptr(), o['M'], o['P'],
              o['pocket_type'].data_ptr(), o['pocket_status'].data_ptr(), None))

def vina_score(o):
    hip.check(L.kpd_vina_score(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['max_atoms'], o['elem'].data_ptr(), len(ELEMENTS),
              o['z'].data_ptr(), o['xs_lig'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'],
              o['status'].data_ptr(), None, o['pocket_x'].data_ptr(), o['xs_pocket'].data_ptr(), o['pocket_type'].data_ptr(),
              o['pocket_ptr'].data_ptr(), o['M'], o['P'], POCKET_ATOMS, o['pocket_of'].data_ptr(), None, o['v_report'].data_ptr(), None, None,
              o['v_type'].data_ptr(), o['v_status'].data_ptr(), None))

def pose_check(o, pocket=True):
    none = torch.full((o['B'],), -1, dtype=torch.int32, device=dev) if not pocket else None
    def call():
        hip.check(L.kpd_pose_check(o['ptr'].data_ptr(), o['N'], o['B'], o['max_atoms'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(),
                  o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order_k'].data_ptr(), o['bond_flags'].data_ptr(), o['bond_ptr'].data_ptr(),
                  3 * o['N'], o['status'].data_ptr(), o['san_status'].data_ptr(), o['atom_h'].data_ptr(), o['atom_flags'].data_ptr(), 0,
                  o['poses'].data_ptr(), o['K'], o['vdw_lig'].data_ptr(), o['pocket_x'].data_ptr(), o['vdw_pocket'].data_ptr(),
                  o['pocket_ptr'].data_ptr(), o['M'], o['P'], POCKET_ATOMS, (o['pocket_of'] if pocket else none).data_ptr(), None,
                  o['fail'].data_ptr(), o['report'].data_ptr(), o['counts'].data_ptr(), o['atom_fail'].data_ptr(), o['pc_status'].data_ptr(), None))
    return call

def timed(fn, reps=20):
    for _ in range(3): fn()
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
cases = (('B = 6400 x about 25 atoms, K = 1, 64 pockets of 300', [small[k % len(small)] for k in range(6400)], 1, 100),
         ('B = 64 x about 60 atoms (two fragments each), K = 1, one pocket of 300', two, 1, 64),
         ('B = 640 x about 25 atoms, 9 poses, 64 pockets of 300', [small[k % len(small)] for k in range(640)], 9, 10))
for name, ligs, K, per_pocket in cases:
    o = setup(ligs, K, per_pocket)
    perceive(o); sanitize(o); pocket_types(o); vina_score(o); pose_check(o)(); torch.cuda.synchronize()
    fail, cnt, st = o['fail'].cpu().numpy(), o['counts'].cpu().numpy().astype(np.int64), o['pc_status'].cpu().numpy()
    per_check = ', '.join(f'{n} {int(((fail >> k) & 1).sum())}' for k, n in enumerate(hip.CHECK_FAIL))
    print(f'{name}: {o["N"]} atoms ({o["N"] / o["B"]:.1f} per ligand), {o["B"] * K} poses, status bits {int(np.bitwise_or.reduce(st.reshape(-1)))}, '
          f'vina status {int(o["v_status"].max())}; poses failing: {per_check}; passing everything {int((fail == 0).sum())}; lattice points per pose '
          f'{cnt[:, :, 15].mean():.0f} (max {cnt[:, :, 15].max()}), in the pocket {cnt[:, :, 16].mean():.1f}; pocket pairs per pose {cnt[:, :, 13].mean():.0f}')
    tv, sv = timed(lambda: vina_score(o))
    tc, sc = timed(pose_check(o))
    tn, sn = timed(pose_check(o, pocket=False))
    print('  kpd_vina_score (pose 0, no gradient) ', sv)
    print('  kpd_pose_check                       ', sc, f'= {tc / tv:.2f} x vina_score')
    print('  kpd_pose_check, pocket_of = -1       ', sn, f'= {tn / tv:.2f} x vina_score')
