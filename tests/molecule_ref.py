"""Float64 numpy restatement of the molecule rule of include/kpd.h (kpd_mol_perceive, kpd_sdf_emit), the yardstick of
test_molecule_gpu.py.  Same arithmetic as the kernels: d2 = (dx*dx + dy*dy) + dz*dz in float64 on exact differences of the
fp32 coordinates, thresholds (T*T) * 1e-4 from integer picometres; so every comparison against the GPU is exact equality.
The SDF formatter uses Python's own `%` formatting."""
import numpy as np

# Z: (r1, r2, r3, cap), radii in pm (0 = no bond of that order)
TABLE = {1: (32, 0, 0, 1), 5: (85, 78, 0, 3), 6: (75, 67, 60, 4), 7: (71, 60, 54, 3), 8: (63, 57, 0, 2), 9: (64, 0, 0, 1),
         14: (116, 0, 0, 4), 15: (111, 102, 0, 5), 16: (103, 94, 0, 6), 17: (99, 0, 0, 1), 33: (121, 0, 0, 3), 35: (114, 0, 0, 1),
         53: (133, 0, 0, 1)}
EMPTY, CAPACITY, BAD_ATOM, BAD_SEGMENT = 1, 2, 4, 8
SDF_NONFINITE, SDF_WIDE, SDF_NO_MOLECULE, SDF_CAPACITY = 1, 2, 4, 8
MAX_ATOMS = 256


def argmax_first(row) -> int:
    """torch.argmax on the CPU: the first maximum; a NaN is a maximum."""
    best, bv = 0, row[0]
    if bv != bv:
        return 0
    for k in range(1, len(row)):
        x = row[k]
        if x != x:
            return k
        if x > bv:
            best, bv = k, x
    return best


def _test(d2, ri, rj, margin):
    T = ri[:, None].astype(np.int64) + rj[None, :].astype(np.int64) + margin
    with np.errstate(invalid='ignore'):
        return (d2 <= (T * T).astype(np.float64) * 1e-4) & (ri[:, None] > 0) & (rj[None, :] > 0)


def perceive(pos, feat, z, allowed):
    """One ligand.  pos [n,3] float32, feat [n,F] float32, z / allowed: F integers.  Returns a dict: elem, valence, frag [n],
    bonds [m,2] (local, i < j, sorted), order [m], summary (4 ints), status, and the counters of what the rule did (stats)."""
    pos, feat = np.asarray(pos, dtype=np.float32).reshape(-1, 3), np.asarray(feat, dtype=np.float32)
    n = pos.shape[0]
    stats = dict(candidates=0, pruned=0, demoted=0)
    if n == 0:
        e = np.zeros(0, dtype=np.int64)
        return dict(elem=e, valence=e, frag=e, bonds=e.reshape(0, 2), order=e, summary=[0, 0, 0, 0], status=EMPTY, stats=stats)
    elem = np.array([argmax_first(feat[a]) for a in range(n)], dtype=np.int64)
    rows = np.array([TABLE.get(int(z[c]), (0, 0, 0, 0)) for c in elem], dtype=np.int64)
    finite = np.isfinite(pos).all(axis=1)
    status = BAD_ATOM if (not finite.all() or (rows[:, 0] == 0).any()) else 0
    cap = rows[:, 3].copy()
    r = rows[:, :3].copy()
    r[~finite] = 0
    p = pos.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy, dz = (p[:, None, c] - p[None, :, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        A = (d2 > 0.16) & _test(d2, r[:, 0], r[:, 0], 45)                                       # step 1
    np.fill_diagonal(A, False)
    stats['candidates'] = int(A.sum()) // 2
    for i in range(n):                                                                       # step 2
        while A[i].sum() > cap[i]:
            js = np.nonzero(A[i])[0]
            far = d2[i, js].max()
            j = js[d2[i, js] == far].max()
            A[i, j] = A[j, i] = False
            stats['pruned'] += 1
    t3, t2 = _test(d2, r[:, 2], r[:, 2], 3), _test(d2, r[:, 1], r[:, 1], 5)                    # step 3
    O = np.where(A, np.where(t3, 3, np.where(t2, 2, 1)), 0).astype(np.int64)
    for i in range(n):                                                                       # step 4
        while O[i].sum() > cap[i]:
            top = O[i].max()
            assert top >= 2, 'degree <= cap after step 2'
            js = np.nonzero(O[i] == top)[0]
            far = d2[i, js].max()
            j = js[d2[i, js] == far].max()
            O[i, j] -= 1
            O[j, i] -= 1
            stats['demoted'] += 1
    frag = np.full(n, -1, dtype=np.int64)                                                    # step 5
    sizes = []
    for a in range(n):
        if frag[a] >= 0:
            continue
        frag[a] = len(sizes)
        todo, size = [a], 0
        while todo:
            u = todo.pop()
            size += 1
            for v in np.nonzero(A[u])[0]:
                if frag[v] < 0:
                    frag[v] = len(sizes)
                    todo.append(int(v))
        sizes.append(size)
    valence = O.sum(axis=1)
    al = np.array([int(allowed[c]) for c in elem], dtype=np.int64)
    invalid = (valence == 0) | (valence > al) | (rows[:, 0] == 0)                             # step 6
    ii, jj = np.nonzero(np.triu(A, 1))
    return dict(elem=elem, valence=valence, frag=frag, bonds=np.stack([ii, jj], axis=1).astype(np.int64), order=O[ii, jj],
                summary=[len(ii), len(sizes), max(sizes), int(invalid.sum())], status=status, stats=stats)


def perceive_batch(pos, feat, ptr, z, allowed, cap_bonds=None):
    """The outputs of kpd_mol_perceive for a batch, in its layout: elem / valence / frag [N] (-1 where a ligand is left out),
    bonds [m,2] (global rows; only the ligands that fit cap_bonds, at their bond_ptr rows, -1 elsewhere), order [m], bond_ptr
    [B+1], summary [B,4], status [B]; `stats`: the counters summed, `mols`: the per-ligand dicts (None where left out)."""
    pos, feat = np.asarray(pos, dtype=np.float32).reshape(-1, 3), np.asarray(feat, dtype=np.float32)
    N, B = pos.shape[0], len(ptr) - 1
    cap_bonds = 3 * N if cap_bonds is None else cap_bonds
    out = dict(elem=np.full(N, -1, dtype=np.int64), valence=np.full(N, -1, dtype=np.int64), frag=np.full(N, -1, dtype=np.int64),
               bond_ptr=np.zeros(B + 1, dtype=np.int64), summary=np.zeros((B, 4), dtype=np.int64), status=np.zeros(B, dtype=np.int64),
               stats=dict(candidates=0, pruned=0, demoted=0), mols=[])
    for b in range(B):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        if not (0 <= a0 <= a1 <= N) or a1 - a0 > MAX_ATOMS:
            out['status'][b] = BAD_SEGMENT
            out['bond_ptr'][b + 1] = out['bond_ptr'][b]
            out['mols'].append(None)
            continue
        m = perceive(pos[a0:a1], feat[a0:a1], z, allowed)
        out['mols'].append(m)
        for k in ('elem', 'valence', 'frag'):
            out[k][a0:a1] = m[k]
        out['summary'][b], out['status'][b] = m['summary'], m['status']
        out['bond_ptr'][b + 1] = out['bond_ptr'][b] + len(m['order'])
        for k in out['stats']:
            out['stats'][k] += m['stats'][k]
    total = int(out['bond_ptr'][B])
    out['bonds'] = np.full((max(total, cap_bonds), 2), -1, dtype=np.int64)
    out['order'] = np.full(max(total, cap_bonds), -1, dtype=np.int64)
    out['written'] = np.zeros(max(total, cap_bonds), dtype=bool)
    for b, m in enumerate(out['mols']):
        p0, p1 = int(out['bond_ptr'][b]), int(out['bond_ptr'][b + 1])
        if m is None or p1 == p0:
            continue
        if p1 > cap_bonds:
            out['status'][b] |= CAPACITY
            continue
        out['bonds'][p0:p1] = m['bonds'] + int(ptr[b])
        out['order'][p0:p1] = m['order']
        out['written'][p0:p1] = True
    return out


def sdf_block(pos, symbols, bonds, order, keep=None):
    """The MOL V2000 block of one ligand, or (None, flag) if it cannot be written.  pos [n,3] float32, symbols: n strings,
    bonds [m,2] local and 0-based, keep: boolean mask of the atoms to write (None: all)."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    n = pos.shape[0]
    flag = 0
    for v in pos.flatten():
        if not np.isfinite(v):
            flag |= SDF_NONFINITE
        elif len('%.4f' % float(v)) > 10:
            flag |= SDF_WIDE
    if flag:
        return None, flag
    keep = np.ones(n, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    number = np.cumsum(keep) * keep                     # 1-based, 0 = left out
    lines = ['', '  kpd_hip ' + ' ' * 10 + '3D', '']
    kept = [(int(number[i]), int(number[j]), int(o)) for (i, j), o in zip(bonds, order) if number[i] and number[j]]
    lines.append('%3d%3d  0  0  0  0  0  0  0  0999 V2000' % (int(keep.sum()), len(kept)))
    for a in range(n):
        if keep[a]:
            x, y, zc = (float(v) for v in pos[a])
            lines.append('%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0' % (x, y, zc, symbols[a]))
    lines += ['%3d%3d%3d  0' % t for t in kept]
    lines += ['M  END', '$$$$']
    return ''.join(line + '\n' for line in lines), 0


def sdf_batch(pos, ptr, elements, ref, largest_only=False):
    """Blocks and status of kpd_sdf_emit for the batch `ref` = perceive_batch(...) describes: (list of strings, list of ints)."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    blocks, status = [], []
    for b, m in enumerate(ref['mols']):
        if m is None or ref['status'][b] & (CAPACITY | BAD_SEGMENT):
            blocks.append('')
            status.append(SDF_NO_MOLECULE)
            continue
        keep = None
        if largest_only and len(m['frag']):
            sizes = np.bincount(m['frag'])
            keep = m['frag'] == int(np.argmax(sizes))   # the first maximum: the lowest rank on a tie
        text, flag = sdf_block(pos[int(ptr[b]):int(ptr[b + 1])], [elements[c] for c in m['elem']], m['bonds'], m['order'], keep)
        blocks.append(text or '')
        status.append(flag)
    return blocks, status
