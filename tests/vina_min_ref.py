"""Float64 numpy restatement of kpd_vina_minimize as include/kpd.h defines it: the torsion tree (active rotors, their orientation
and depth, rigid pieces), the intramolecular pair list, the chart `move` with its gradient projection and first-order velocity, the
objective E = inter + w_intra intra and the L-BFGS over the pose coordinates.  Typing, the rotor rule and the pair function are
those of tests/vina_ref.py.  `reverse=True` sums every energy, gradient, projection and dot-product term in the opposite order,
which is how the tests measure what a different summation order alone can do to a trajectory; the minimiser records the margin of
every accept / reject / reset decision, as relax_ref.minimize does."""
import numpy as np

from . import vina_ref as V

NO_MOLECULE, BAD_INPUT, ATOM_OUT, LINE_SEARCH, FROZEN, FRAGMENTS, ITER_CAP = 1, 2, 4, 8, 16, 32, 64
DEFAULTS = dict(V.DEFAULTS, w_intra=1.0, gtol=1e-3, max_step=0.2, max_iters=200)
REPORT = ('score_before', 'score_after', 'E_before', 'E_after', 'inter_before', 'inter_after', 'intra_before', 'intra_after', 'rmsd',
          'gnorm_before', 'gnorm_after', 'iterations', 'evaluations', 'n_rot', 'n_active', 'n_frag')
MAX_FRAGS, MAX_ROTORS = 8, 64


def _sum(a, reverse, axis=None):
    a = np.asarray(a, dtype=np.float64)
    if reverse:
        a = a[::-1] if axis is None else np.flip(a, axis=axis)
    return np.add.reduce(a, axis=axis) if axis is not None else np.add.reduce(a.ravel())


def _reach(nb, start, other):
    """The atoms reached from `start` when its bond to `other` is removed."""
    seen, todo = {start}, [start]
    while todo:
        u = todo.pop()
        for v in nb[u]:
            if (u == start and v == other) or v in seen:
                continue
            seen.add(v)
            todo.append(v)
    return seen


def tree(z_atoms, bonds, orders, frag, max_rotors=MAX_ROTORS, types=None):
    """The torsion tree of one ligand: z_atoms [n], bonds [m,2] local with i < j in bond_ij order, orders [m], frag [n] (labels as
    kpd_mol_perceive writes them).  Returns a dict: n_rot (all rotors), rotors [(a, b)] of the T active ones, M [T,n] bool (moved
    sets), depth [T], order (active indices from the deepest to the shallowest), piece [n] (lowest atom of the rigid piece), frag,
    F, and pairs [n,n] bool, the symmetric mask of the intramolecular pairs (`types` [n]: atoms with -1 take no part)."""
    n = len(z_atoms)
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2).tolist()
    frag = np.asarray(frag, dtype=np.int64)
    nb = [[] for _ in range(n)]
    for i, j in bonds:
        nb[i].append(j)
        nb[j].append(i)
    hdeg = [sum(1 for j in nb[a] if int(z_atoms[j]) != 1) for a in range(n)]
    found = []
    for (i, j), o in zip(bonds, list(orders)):
        if int(o) != 1 or hdeg[i] < 2 or hdeg[j] < 2:
            continue
        if i not in _reach(nb, j, i):
            found.append((i, j))
    active = found[:max_rotors]
    low = {int(f): int(np.nonzero(frag == f)[0].min()) for f in set(frag.tolist())}
    rotors, M = [], np.zeros((len(active), n), dtype=bool)
    for k, (i, j) in enumerate(active):
        seen = _reach(nb, j, i)
        if low[int(frag[j])] in seen:
            M[k] = frag == frag[j]
            M[k, list(seen)] = False
            rotors.append((j, i))
        else:
            M[k, list(seen)] = True
            rotors.append((i, j))
    depth = np.array([int(sum(M[q, b] for q in range(len(active)))) for _, b in rotors], dtype=np.int64)
    order = sorted(range(len(active)), key=lambda k: (-depth[k], k))
    cut = {frozenset(r) for r in rotors}
    piece = np.full(n, -1, dtype=np.int64)
    for a in range(n):
        if piece[a] >= 0:
            continue
        piece[a] = a
        todo = [a]
        while todo:
            u = todo.pop()
            for v in nb[u]:
                if piece[v] < 0 and frozenset((u, v)) not in cut:
                    piece[v] = a
                    todo.append(v)
    near = np.eye(n, dtype=bool)                              # three or fewer bonds apart
    step = near.copy()
    adj = np.zeros((n, n), dtype=bool)
    for i, j in bonds:
        adj[i, j] = adj[j, i] = True
    for _ in range(3):
        step = (step.astype(np.int64) @ adj.astype(np.int64)) > 0
        near |= step
    part = np.ones(n, dtype=bool) if types is None else np.asarray(types) >= 0
    pairs = ~near & (piece[:, None] != piece[None, :]) & part[:, None] & part[None, :]
    return dict(n=n, n_rot=len(found), rotors=rotors, M=M, depth=depth, order=order, piece=piece, frag=frag, F=int(frag.max()) + 1 if n else 0,
                pairs=pairs, T=len(active))


def pair_list(t):
    """The intramolecular pairs i < j as a sorted list."""
    ii, jj = np.nonzero(np.triu(t['pairs'], 1))
    return list(zip(ii.tolist(), jj.tolist()))


def _pair_sums(x, ti, Ri, q, tj, Rj, on, P, reverse):
    """Unweighted term sums [5], the gradient [n,3] of their weighted sum with respect to x, and the sum of the absolute weighted
    terms and, per atom of x, of the norms of its gradient contributions, over the pairs (i, j) of x [n,3] and q [m,3] that `on`
    admits and that lie inside the cutoff."""
    w = np.array([P[k] for k in V.WEIGHTS], dtype=np.float64)
    n = len(x)
    if len(q) == 0 or n == 0:
        return np.zeros(5), np.zeros((n, 3)), 0.0, np.zeros(n)
    diff = x[:, None, :] - q[None, :, :]
    d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    on = on & (d2 < P['r_c'] * P['r_c'])
    r = np.sqrt(d2)
    d = (r - Ri[:, None]) - Rj[None, :]
    hyd = ((ti[:, None] & V.H) != 0) & ((tj[None, :] & V.H) != 0)
    hb = (((ti[:, None] & V.D) != 0) & ((tj[None, :] & V.A) != 0)) | (((ti[:, None] & V.A) != 0) & ((tj[None, :] & V.D) != 0))
    t, dt = V.pair_terms(d, hyd, hb)
    t, dt = np.where(on[None], t, 0.0), np.where(on[None], dt, 0.0)
    sums = np.array([_sum(_sum(t[k], reverse, axis=1), reverse) for k in range(5)])
    far = r >= 1e-6
    k = np.where(far, (w[:, None, None] * dt).sum(axis=0) / np.where(far, r, 1.0), 0.0)
    return sums, _sum(k[..., None] * diff, reverse, axis=1), float(np.abs(w[:, None, None] * t).sum()), (np.abs(k) * r).sum(axis=1)


def evaluate(x, t, types, radius, ppos, ptypes, pradius, params=None, reverse=False):
    """One evaluation at x [n,3] float64.  Returns dict: inter, intra, E, g [n,3] (Cartesian, un-normalised), abs_terms (the sum of
    the absolute weighted pair terms of inter and of w_intra intra, the scale of the tolerances), abs_g [n] (per atom, the sum of
    the norms of its gradient contributions)."""
    P = dict(DEFAULTS, **(params or {}))
    w = np.array([P[k] for k in V.WEIGHTS], dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    types, ptypes = np.asarray(types, dtype=np.int64), np.asarray(ptypes, dtype=np.int64)
    Rl = np.asarray(radius, dtype=np.float32).astype(np.float64)
    q, Q = np.asarray(ppos, dtype=np.float32).astype(np.float64).reshape(-1, 3), np.asarray(pradius, dtype=np.float32).astype(np.float64)
    part_i, part_j = types >= 0, (ptypes >= 0) & (Q > 0)
    ti, tj = np.where(part_i, types, 0), np.where(part_j, ptypes & 7, 0)
    s_inter, g_inter, a_inter, ag_inter = _pair_sums(x, ti, Rl, q, tj, Q, part_i[:, None] & part_j[None, :], P, reverse)
    s_intra, g_intra, a_intra, ag_intra = _pair_sums(x, ti, Rl, x, ti, Rl, t['pairs'], P, reverse)
    ws, wi = w * s_inter, w * s_intra
    inter = (((ws[0] + ws[1]) + ws[2]) + ws[3]) + ws[4]
    intra = 0.5 * ((((wi[0] + wi[1]) + wi[2]) + wi[3]) + wi[4])
    return dict(inter=inter, intra=intra, E=inter + P['w_intra'] * intra, g=g_inter + P['w_intra'] * g_intra,
                abs_terms=a_inter + 0.5 * P['w_intra'] * a_intra, abs_inter=a_inter, abs_intra=0.5 * a_intra,
                abs_g=ag_inter + P['w_intra'] * ag_intra)


def centres(x, t):
    c = np.zeros((t['F'], 3))
    for f in range(t['F']):
        s = np.zeros(3)
        for i in np.nonzero(t['frag'] == f)[0]:
            s = s + x[i]
        c[f] = s / int((t['frag'] == f).sum())
    return c


def axes(x, t):
    u = np.zeros((t['T'], 3))
    for k, (a, b) in enumerate(t['rotors']):
        v = x[b] - x[a]
        ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        u[k] = v / ln if ln >= 1e-6 else 0.0
    return u


def project(x, g, t, reverse=False):
    """g_delta [6F + T] at delta = 0 in the chart at x, from the Cartesian gradient g."""
    c, u = centres(x, t), axes(x, t)
    out = np.zeros(6 * t['F'] + t['T'])
    for f in range(t['F']):
        idx = np.nonzero(t['frag'] == f)[0]
        out[6 * f:6 * f + 3] = _sum(g[idx], reverse, axis=0)
        out[6 * f + 3:6 * f + 6] = _sum(np.cross(x[idx] - c[f], g[idx]), reverse, axis=0)
    for k, (a, b) in enumerate(t['rotors']):
        idx = np.nonzero(t['M'][k])[0]
        s = _sum(np.cross(x[idx] - x[b], g[idx]), reverse, axis=0)
        out[6 * t['F'] + k] = (u[k, 0] * s[0] + u[k, 1] * s[1]) + u[k, 2] * s[2]
    return out


def _rot(r, u, c, s):
    return (r * c + np.cross(u, r) * s) + u * (((u[0] * r[0] + u[1] * r[1]) + u[2] * r[2]) * (1.0 - c))


def move(x, delta, t):
    """move(x, delta) of include/kpd.h."""
    x = np.asarray(x, dtype=np.float64)
    c, u = centres(x, t), axes(x, t)
    F = t['F']
    out = np.zeros_like(x)
    for i in range(len(x)):
        p = x[i].copy()
        for k in t['order']:
            if not t['M'][k, i]:
                continue
            b = t['rotors'][k][1]
            th = delta[6 * F + k]
            p = x[b] + _rot(p - x[b], u[k], np.cos(th), np.sin(th))
        f = int(t['frag'][i])
        om = np.asarray(delta[6 * f + 3:6 * f + 6], dtype=np.float64)
        th = np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
        r = p - c[f]
        if th >= 1e-12:
            r = _rot(r, om / th, np.cos(th), np.sin(th))
        out[i] = (c[f] + r) + delta[6 * f:6 * f + 3]
    return out


def velocity(x, p, t):
    """The first-order velocity [n,3] of every atom under the pose velocity p."""
    c, u = centres(x, t), axes(x, t)
    F = t['F']
    v = np.zeros_like(x)
    for i in range(len(x)):
        f = int(t['frag'][i])
        v[i] = p[6 * f:6 * f + 3] + np.cross(p[6 * f + 3:6 * f + 6], x[i] - c[f])
        for k, (a, b) in enumerate(t['rotors']):
            if t['M'][k, i]:
                v[i] = v[i] + p[6 * F + k] * np.cross(u[k], x[i] - x[b])
    return v


def _dot(a, b, reverse):
    return _sum(a * b, reverse)


def minimize(pos0, t, types, radius, ppos, ptypes, pradius, params=None, reverse=False):
    """The minimiser of include/kpd.h from the fp32 geometry pos0.  Returns dict: pos_out float32, x64 (the minimiser's own last
    point before the fp32 rounding), report (a dict with the keys REPORT), status (bits 2, 3, 4, 6), first / last (evaluations),
    margins (name, value) of every decision."""
    P = dict(DEFAULTS, **(params or {}))
    x0 = np.asarray(pos0, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = len(x0)

    def ev(y):
        e = evaluate(y, t, types, radius, ppos, ptypes, pradius, P, reverse)
        return e

    def chart(y, e):
        e['gd'] = project(y, e['g'], t, reverse)
        e['gnorm'] = float(np.abs(e['gd']).max())
        return e

    first = chart(x0, ev(x0))
    cur, x, E = first, x0.copy(), first['E']
    S, Y, RHO = [], [], []
    gamma, iters, evals, status = 1.0, 0, 1, 0
    margins = []
    rel = lambda v: abs(v) / max(1.0, abs(E))
    for _ in range(int(P['max_iters'])):
        margins.append(('converged', rel(cur['gnorm'] - P['gtol'])))
        if cur['gnorm'] <= P['gtol']:
            break
        iters += 1
        g = cur['gd']
        p = g.copy()
        al = []
        for k in range(len(S) - 1, -1, -1):                   # newest first
            a = RHO[k] * _dot(S[k], p, reverse)
            al.append(a)
            p = p - a * Y[k]
        if S:
            p = p * gamma
        for k in range(len(S)):                               # oldest first
            be = RHO[k] * _dot(Y[k], p, reverse)
            p = p + (al[len(S) - 1 - k] - be) * S[k]
        p = -p
        gp = _dot(g, p, reverse)
        margins.append(('descent', rel(gp)))
        if not gp < 0.0:
            S, Y, RHO = [], [], []
            p = -g
            gp = -_dot(g, g, reverse)
        v = velocity(x, p, t)
        vmax = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).max()
        with np.errstate(divide='ignore'):
            alpha = min(1.0, P['max_step'] / vmax)
        accepted = None
        for _ls in range(21):
            xt = move(x, alpha * p, t)
            tr = ev(xt)
            evals += 1
            bound = E + 1e-4 * alpha * gp
            margins.append(('armijo', rel(tr['E'] - bound) if np.isfinite(tr['E']) else np.inf))
            if np.isfinite(tr['E']) and tr['E'] <= bound:
                accepted = tr
                break
            alpha *= 0.5
        if accepted is None:
            if S:
                S, Y, RHO = [], [], []
                continue
            status |= LINE_SEARCH
            break
        chart(xt, accepted)
        s_new, y_new = alpha * p, accepted['gd'] - g
        sy, yy = _dot(s_new, y_new, reverse), _dot(y_new, y_new, reverse)
        gg = _dot(accepted['gd'], accepted['gd'], reverse)
        margins.append(('pair', rel(sy - 1e-10 * yy)))
        margins.append(('noise', rel(yy - 1e-20 * gg)))
        if sy > 1e-10 * yy and yy > 1e-20 * gg:
            S.append(s_new)
            Y.append(y_new)
            RHO.append(1.0 / sy)
            gamma = sy / yy
            if len(S) > 8:
                S.pop(0)
                Y.pop(0)
                RHO.pop(0)
        x, E, cur = xt, accepted['E'], accepted
    x64 = x.copy()
    if iters:
        xr = x.astype(np.float32).astype(np.float64)
        ulp = np.spacing(np.abs(xr).astype(np.float32)).astype(np.float64)
        margins.append(('ulp', float((0.5 * ulp - np.abs(x - xr)).min()) if n else np.inf))       # in Angstrom, not relative
        fin = chart(xr, ev(xr))
        evals += 1
        margins.append(('round', rel(fin['E'] - first['E'])))
        if fin['E'] <= first['E']:
            x, cur = xr, fin
        else:
            x, cur = x0.copy(), first
    if cur['gnorm'] > P['gtol'] and not status & LINE_SEARCH:
        status |= ITER_CAP
    if t['n_rot'] > t['T']:
        status |= FROZEN
    if (np.asarray(types) < 0).any() or (np.asarray(ptypes) < 0).any() or not (np.asarray(pradius, dtype=np.float32) > 0).all():
        status |= ATOM_OUT
    out = x.astype(np.float32)
    d = out.astype(np.float64) - x0
    norm = 1.0 + P['w_rot'] * t['n_rot']
    rep = dict(score_before=first['inter'] / norm, score_after=cur['inter'] / norm, E_before=first['E'], E_after=cur['E'],
               inter_before=first['inter'], inter_after=cur['inter'], intra_before=first['intra'], intra_after=cur['intra'],
               rmsd=np.sqrt((d * d).sum() / n) if n else 0.0, gnorm_before=first['gnorm'], gnorm_after=cur['gnorm'], iterations=iters,
               evaluations=evals, n_rot=t['n_rot'], n_active=t['T'], n_frag=t['F'])
    return dict(pos_out=out, x64=x64, report=rep, status=status, first=first, last=cur, margins=margins)


def min_margin(margins, names=None):
    vals = [v for k, v in margins if names is None or k in names]
    return min(vals) if vals else np.inf


def minimize_ligand(pos, z_atoms, bonds, orders, frag, radius, ppos, ptypes, pradius, params=None, type_in=None, max_rotors=MAX_ROTORS,
                    reverse=False):
    """Typing, the tree and the minimisation of one ligand in one typed pocket."""
    types = V.ligand_types(z_atoms, bonds, orders, radius, type_in)
    t = tree(z_atoms, bonds, orders, frag, max_rotors, types)
    out = minimize(pos, t, types, radius, ppos, ptypes, pradius, params, reverse)
    out.update(tree=t, types=types)
    return out
