"""Timing of kpd_mol_match next to kpd_mol_perceive and kpd_mol_sanitize (profiles/match.md).
    python profiles/tools/match_bench.py    HIP events around the raw C calls (buffers preallocated, no host sync inside)
The workloads are those of profiles/tools/pose_rmsd_bench.py: 6 400 generated ring-bearing ligands of about 25 atoms (400 distinct
ones, repeated) and 64 two-fragment ligands of about 60 atoms.  Three tables: smarts.FUNCTIONAL_GROUPS with every search stopped at
its first embedding, the same with all embeddings, and a synthetic first-match-wins typing table of 110 user rows of which 30 hold
a "$(...)" (the shape of a Crippen table, NOT one: its values are seeded noise).  Also printed: the time the plain-Python
restatement (tests/match_ref.py, NOT RDKit) takes on the first 64 ligands of each workload.
The generator lives in the tests package: run this from a full checkout of the repository."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule, smarts
from tests import sanitize_cases as C
from tests import match_ref as R
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


def typing_table():
    """110 user rows in first-match-wins order, specific before general, 30 of them with a "$(...)"; one typing group."""
    inner = ['C=O', 'CN', 'CO', 'Cc', 'C[F,Cl,Br,I]', 'cn', 'co', 'cs', 'NC=O', 'C#N', 'CS', 'c[OX2H]', 'cN', 'C(=O)O', 'CC=O']
    rec = [f'[{a};$({i})]' for a in ('#6', '#7') for i in inner]                                       # 30
    plain = [f'[{e}{q}]' for e in ('C', 'c', 'N', 'n', 'O', 'o', 'S', 's') for q in ('X4H3', 'X4H2', 'X4H1', 'X4H0', 'X3H2', 'X3H1', 'X3H0', 'X2H1', 'X2H0')]
    plain += ['[F]', '[Cl]', '[Br]', '[I]', '[#6]', '[#7]', '[#8]', '*']                                # 72 + 8 = 80
    pats = smarts.compile(rec + plain)
    assert pats.n == 110, pats.n
    rng = np.random.default_rng(5)
    group, value = [-1] * pats.n_rows, [0.0] * pats.n_rows
    for r in pats.rows:
        group[r], value[r] = 0, float(rng.standard_normal())
    return pats, group, value


def setup(ligs):
    sizes = [len(s) for s, _ in ligs]
    B, N = len(ligs), sum(sizes)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    mass, mass_h = molecule.mass_table(ELEMENTS)
    o = dict(B=B, N=N, pos=torch.from_numpy(np.concatenate([p for _, p in ligs]).astype(np.float32)).to(dev),
             feat=torch.from_numpy(np.concatenate([one_hot(s) for s, _ in ligs])).to(dev),
             ptr=torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev), zs=z,
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev),
             mass=torch.tensor(mass, dtype=torch.float64, device=dev), mass_h=mass_h, elem=i32(N), valence=i32(N), frag=i32(N),
             bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B), order_k=i32(3 * N),
             bond_flags=i32(3 * N), valence_k=i32(N), atom_h=i32(N), atom_flags=i32(N), desc_i=i32(B, 10), desc_f=f64(B, 2), valid=i32(B),
             san_status=i32(B), mm_status=i32(B))
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


def match_buffers(o, pats, mode, group=None, value=None):
    P, B, N = pats.n_rows, o['B'], o['N']
    W = (P + 31) // 32
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    m = dict(pats=pats, table=pats.host.to(dev), mode=mode, G=1 if group else 0, anchor=i32(N, W), hits=i32(B, P), first_map=i32(B, P, 16),
             n_embed=torch.empty(B, P, dtype=torch.int64, device=dev), cover=i32(N, W), atom_type=i32(1, N),
             type_sum=torch.empty(B, 1, dtype=torch.float64, device=dev), untyped=i32(B, 1),
             tg=torch.tensor(group, dtype=torch.int32, device=dev) if group else None,
             value=torch.tensor(value, dtype=torch.float64, device=dev) if group else None)
    return m


def match(o, m, with_map=True):
    p = lambda t: None if t is None else t.data_ptr()
    hip.check(L.kpd_mol_match(o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(), o['frag'].data_ptr(),
              o['bonds'].data_ptr(), o['order_k'].data_ptr(), o['bond_flags'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'],
              o['status'].data_ptr(), o['san_status'].data_ptr(), o['valence_k'].data_ptr(), o['atom_h'].data_ptr(), o['atom_flags'].data_ptr(), 0,
              m['pats'].host.data_ptr(), m['table'].data_ptr(), m['pats'].host.numel(), m['mode'], 65536, p(m['tg']), p(m['value']), m['G'],
              m['anchor'].data_ptr(), m['hits'].data_ptr(), m['first_map'].data_ptr() if with_map else None, m['n_embed'].data_ptr(),
              m['cover'].data_ptr(), m['atom_type'].data_ptr(), m['type_sum'].data_ptr(), m['untyped'].data_ptr(), o['mm_status'].data_ptr(), None))


def timed(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), f'median {np.median(ts):.1f} us, min {ts.min():.1f}, max {ts.max():.1f} ({reps} runs)'


def restatement_seconds(o, pats, mode, count=64):
    host = lambda t: t.cpu().numpy().astype(np.int64)
    B = min(count, o['B'])
    ptr = host(o['ptr'])[:B + 1]
    mol = dict(elem=host(o['elem']), frag=host(o['frag']), bonds=host(o['bonds']), order=host(o['order']), bond_ptr=host(o['bond_ptr']), status=host(o['status']))
    san = {k: host(o[k]) for k in ('order_k', 'bond_flags', 'valence_k', 'atom_h', 'atom_flags')}
    san['status'] = host(o['san_status'])
    t = time.time()
    ref = R.match_batch(ptr, mol, san, o['zs'], pats.host.tolist(), mode)
    return time.time() - t, B, ref


small = pool(20, 30, 400)
mid = pool(25, 35, 128)
far = np.array([30.0, 0.0, 0.0], dtype=np.float32)
two = [(mid[2 * k][0] + mid[2 * k + 1][0], np.concatenate([mid[2 * k][1], mid[2 * k + 1][1] + far])) for k in range(64)]
groups = smarts.compile(smarts.FUNCTIONAL_GROUPS)
typing, t_group, t_value = typing_table()
print(f'tables: functional groups {groups.n} user rows, {groups.n_rows} rows, {groups.host.numel()} words; typing {typing.n} user rows, '
      f'{typing.n_rows} rows, {typing.host.numel()} words')
for name, ligs in (('B = 6400 x about 25 atoms', [small[k % len(small)] for k in range(6400)]), ('B = 64 x about 60 atoms (two fragments each)', two)):
    o = setup(ligs)
    perceive(o); sanitize(o)
    runs = (('functional groups, anchors', match_buffers(o, groups, 0)), ('functional groups, all embeddings', match_buffers(o, groups, 1)),
            ('typing table, 110 + lifted rows, anchors', match_buffers(o, typing, 0, t_group, t_value)))
    for _, m in runs:
        match(o, m)
    torch.cuda.synchronize()
    print(f'{name}: {o["N"]} atoms ({o["N"] / o["B"]:.1f} per ligand), match status max {int(o["mm_status"].max())}, sanitize status max '
          f'{int(o["san_status"].max())}')
    tp, sp = timed(lambda: perceive(o))
    ts, ss = timed(lambda: sanitize(o))
    print('  kpd_mol_perceive                   ', sp)
    print('  kpd_mol_sanitize, every atom       ', ss)
    for label, m in runs:
        tm, sm = timed(lambda: match(o, m))
        tn, _ = timed(lambda: match(o, m, False))
        extra = f', hits per ligand {m["hits"].double().sum().item() / o["B"]:.1f}'
        if m['mode']:
            extra += f', embeddings per ligand {m["n_embed"].double().sum().item() / o["B"]:.1f}'
        if m['G']:
            extra += f', untyped atoms {int(m["untyped"].sum())}'
        print(f'  kpd_mol_match, {label:42s}', sm, f'= {tm / ts:.2f} x sanitize, {tm / tp:.2f} x perceive; first_map = NULL {tn:.1f} us{extra}')
    for label, pats, mode in (('functional groups, anchors', groups, 0), ('typing table, anchors', typing, 0)):
        sec, nb, ref = restatement_seconds(o, pats, mode)
        print(f'  restatement (tests/match_ref.py, plain Python), {label}: {sec:.2f} s for the first {nb} ligands = {sec / nb * 1e3:.1f} ms per ligand')
