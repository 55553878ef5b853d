"""Float64 numpy restatement of the relaxation rule of include/kpd.h (kpd_relax): rest values, the energy with its four parts,
the analytic gradient and the L-BFGS minimiser, the yardstick of test_relax_config.py and test_relax_gpu.py.  Plain numpy on the
fp32 inputs widened to float64; `reverse=True` sums every energy, gradient and dot-product term in the opposite order, which is
how the tests measure what a different summation order alone can do to a trajectory.  The minimiser records the margin of every
accept / reject / reset decision (distance of the tested quantity from its threshold, relative to max(1, |E|)): a trajectory is
only comparable between two implementations where no decision is a coin toss."""
import numpy as np

from .molecule_ref import TABLE

COS100, COS150, COS114, COS_TET = -0.1736481776669303, -0.8660254037844387, -0.4184314830435483, -0.3333333228927115
DEFAULTS = dict(k_b=700.0, k_a=200.0, r_c=10.0, s=0.6, w_intra=1.0, gtol=1e-3, max_step=0.2, max_iters=400)
NO_MOLECULE, BAD_INPUT, ITER_CAP, LINE_SEARCH = 1, 2, 4, 8
CLASS_COS = {1: COS_TET, 2: -0.5, 3: -1.0}


def _sum(a, reverse, axis=None):
    a = np.asarray(a, dtype=np.float64)
    if reverse:
        a = a[::-1] if axis is None else np.flip(a, axis=axis)
    return np.add.reduce(a, axis=axis) if axis is not None else np.add.reduce(a.ravel())


def _cos(v, a, c, b):
    """cos of the angles a - c - b (index arrays) in the coordinates v, the header's formula; ok = both arms >= 1e-6."""
    u, w = v[a] - v[c], v[b] - v[c]
    uu = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]
    ww = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
    ok = ~((uu < 1e-12) | (ww < 1e-12))
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = 1.0 / np.sqrt(uu * ww)
        cs = (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1] + u[:, 2] * w[:, 2]) * inv
    return u, w, uu, ww, inv, cs, ok


def topology(pos0, z_atoms, bonds):
    """Rest values of one ligand.  pos0 [n,3] float32 (the sampled geometry), z_atoms [n] atomic numbers, bonds [m,2] local
    i < j.  Returns a dict: bonds, r0 [m], angles (a, c, b index arrays, cos0, cls), excl [n,n] bool (pairs that are no
    non-bonded pairs), margins (distance of every rest-value decision from its threshold)."""
    x = np.asarray(pos0, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = x.shape[0]
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    nbr = [[] for _ in range(n)]
    for i, j in bonds:
        nbr[i].append(int(j))
        nbr[j].append(int(i))
    nbr = [sorted(l) for l in nbr]
    margins = []
    r0 = np.zeros(len(bonds))
    for k, (i, j) in enumerate(bonds):
        ri, rj = TABLE[int(z_atoms[i])], TABLE[int(z_atoms[j])]
        d = x[i] - x[j]
        d = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        h1 = 2 * (ri[0] + rj[0])
        h2 = 2 * (ri[1] + rj[1]) if ri[1] and rj[1] else 0
        h3 = 2 * (ri[2] + rj[2]) if ri[2] and rj[2] else 0
        best, bd, offs = 0, 0.0, []
        for h in (h3, h2, (h1 + h2) // 2 if h2 else 0, h1):
            if not h:
                continue
            off = abs(d - 0.005 * h)
            offs.append(off)
            if not best or off < bd or (off == bd and h > best):
                best, bd = h, off
        r0[k] = 0.005 * best
        offs.sort()
        if len(offs) > 1:
            margins.append(offs[1] - offs[0])
    A, C, B = [], [], []
    for c in range(n):
        l = nbr[c]
        for s in range(len(l)):
            for t in range(s + 1, len(l)):
                A.append(l[s])
                C.append(c)
                B.append(l[t])
    A, C, B = (np.array(v, dtype=np.int64) for v in (A, C, B))
    cls = np.zeros(len(A), dtype=np.int64)
    cos0 = np.zeros(len(A))
    if len(A):
        _, _, _, _, _, cs, ok = _cos(x, A, C, B)
        deg = np.array([len(l) for l in nbr])
        for q in range(len(A)):
            if not ok[q] or cs[q] > COS100:
                cls[q], cos0[q] = 0, cs[q] if ok[q] else 0.0
            elif deg[C[q]] >= 4:
                cls[q] = 1
            elif cs[q] <= COS150:
                cls[q] = 3
            elif cs[q] <= COS114:
                cls[q] = 2
            else:
                cls[q] = 1
            if cls[q]:
                cos0[q] = CLASS_COS[int(cls[q])]
            if ok[q]:
                ths = [COS100] if deg[C[q]] >= 4 or cs[q] > COS100 else [COS100, COS150, COS114]
                margins.append(min(abs(cs[q] - t) for t in ths))
    excl = np.eye(n, dtype=bool)
    for i in range(n):
        for j in nbr[i]:
            excl[i, j] = True
            for k in nbr[j]:
                excl[i, k] = True
    return dict(n=n, bonds=bonds, r0=r0, A=A, C=C, B=B, cos0=cos0, cls=cls, excl=excl, nbr=nbr, margins=margins)


def _lj(d2, xij, Dij, P):
    """Energy e and gradient factor k (dE/dx_i = k (x_i - x_j)) of the non-bonded pairs, elementwise."""
    rc2 = P['r_c'] * P['r_c']
    inv_rc2 = 1.0 / rc2
    s = P['s']
    s6 = 1.0 / (s * s * s * s * s * s)
    ce, cf = s6 * s6 - 2.0 * s6, s6 * s6 - s6
    x2 = xij * xij
    q = x2 * inv_rc2
    q3 = q * q * q
    shift = Dij * (q3 * q3 - 2.0 * q3)
    d0 = s * xij
    inside = d2 < rc2
    soft = inside & (d2 < d0 * d0)
    hard = inside & ~soft
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        d = np.sqrt(d2)
        slope = -12.0 * Dij * cf / d0
        e_soft = Dij * ce + slope * (d - d0) - shift
        k_soft = np.where(d >= 1e-6, slope / d, 0.0)
        u = x2 / d2
        u3 = u * u * u
        e_hard = Dij * (u3 * u3 - 2.0 * u3) - shift
        k_hard = -12.0 * Dij * (u3 * u3 - u3) / d2
    e = np.where(soft, e_soft, np.where(hard, e_hard, 0.0))
    k = np.where(soft, k_soft, np.where(hard, k_hard, 0.0))
    return e, k


def energy(x, topo, lig_vdw, pocket_x, pocket_vdw, P, reverse=False):
    """Energy and gradient at x [n,3] float64.  lig_vdw [n,2] per ATOM, pocket_x [m,3], pocket_vdw [m,2] (fp32 values).
    Returns dict: parts [4] (bond, angle, intra, pocket), E, g [n,3], gmax, abs_E (sum of the absolute energy terms),
    abs_g [n] (sum over an atom's gradient terms of their norms), and the conditioning of the bonded terms, which are small
    differences of large numbers at a minimum: cond_E = sum k_b |d - r0| d + sum k_a |cos - cos0| (what one relative rounding
    of d or cos does to the energy), cond_g [n] = sum k_b d + sum k_a / arm (what it does to an atom's gradient)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    n = x.shape[0]
    g = np.zeros((n, 3))
    abs_g = np.zeros(n)
    cond_g = np.zeros(n)
    cond_E = 0.0
    lv = np.asarray(lig_vdw, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    sx, sD = np.sqrt(lv[:, 0]), np.sqrt(lv[:, 1])
    abs_E = 0.0
    # pocket
    px = np.asarray(pocket_x, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    e_pocket = 0.0
    if len(px):
        pv = np.asarray(pocket_vdw, dtype=np.float32).astype(np.float64).reshape(-1, 2)
        D = x[:, None, :] - px[None, :, :]
        d2 = D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2]
        e, k = _lj(d2, sx[:, None] * np.sqrt(pv[:, 0])[None, :], sD[:, None] * np.sqrt(pv[:, 1])[None, :], P)
        e_pocket = _sum(_sum(e, reverse, axis=1), reverse)
        g += _sum(k[..., None] * D, reverse, axis=1)
        abs_E += np.abs(e).sum()
        abs_g += (np.abs(k) * np.sqrt(d2)).sum(axis=1)
    # intra
    D = x[:, None, :] - x[None, :, :]
    d2 = D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2]
    e, k = _lj(d2, sx[:, None] * sx[None, :], sD[:, None] * sD[None, :], P)
    e = np.where(topo['excl'], 0.0, e)
    k = np.where(topo['excl'], 0.0, k) * P['w_intra']
    e_intra = _sum(_sum(0.5 * P['w_intra'] * e, reverse, axis=1), reverse)
    g += _sum(k[..., None] * D, reverse, axis=1)
    abs_E += 0.5 * P['w_intra'] * np.abs(e).sum()
    abs_g += (np.abs(k) * np.sqrt(d2)).sum(axis=1)
    # bonds
    e_bond = 0.0
    b = topo['bonds']
    if len(b):
        D = x[b[:, 0]] - x[b[:, 1]]
        d = np.sqrt(D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2])
        dl = d - topo['r0']
        eb = 0.5 * P['k_b'] * dl * dl
        e_bond = _sum(eb, reverse)
        with np.errstate(divide='ignore', invalid='ignore'):
            k = np.where(d >= 1e-6, P['k_b'] * dl / d, 0.0)
        order = range(len(b) - 1, -1, -1) if reverse else range(len(b))
        for q in order:
            g[b[q, 0]] += k[q] * D[q]
            g[b[q, 1]] -= k[q] * D[q]
            abs_g[b[q, 0]] += abs(k[q]) * d[q]
            abs_g[b[q, 1]] += abs(k[q]) * d[q]
            cond_g[b[q, 0]] += P['k_b'] * d[q]
            cond_g[b[q, 1]] += P['k_b'] * d[q]
        abs_E += eb.sum()
        cond_E += (P['k_b'] * np.abs(dl) * d).sum()
    # angles
    e_angle = 0.0
    if len(topo['A']):
        A, C, B = topo['A'], topo['C'], topo['B']
        u, w, uu, ww, inv, cs, ok = _cos(x, A, C, B)
        dl = np.where(ok, cs - topo['cos0'], 0.0)
        ea = 0.5 * P['k_a'] * dl * dl
        e_angle = _sum(ea, reverse)
        f = P['k_a'] * dl
        with np.errstate(divide='ignore', invalid='ignore'):
            ga = np.where(ok[:, None], f[:, None] * (w * inv[:, None] - cs[:, None] * u / uu[:, None]), 0.0)
            gb = np.where(ok[:, None], f[:, None] * (u * inv[:, None] - cs[:, None] * w / ww[:, None]), 0.0)
        order = range(len(A) - 1, -1, -1) if reverse else range(len(A))
        for q in order:
            g[A[q]] += ga[q]
            g[B[q]] += gb[q]
            g[C[q]] -= ga[q] + gb[q]
            na, nb = np.linalg.norm(ga[q]), np.linalg.norm(gb[q])
            abs_g[A[q]] += na
            abs_g[B[q]] += nb
            abs_g[C[q]] += na + nb
            if ok[q]:
                ra, rb = P['k_a'] / np.sqrt(uu[q]), P['k_a'] / np.sqrt(ww[q])
                cond_g[A[q]] += ra
                cond_g[B[q]] += rb
                cond_g[C[q]] += ra + rb
        abs_E += ea.sum()
        cond_E += (P['k_a'] * np.abs(dl)).sum()
    parts = np.array([e_bond, e_angle, e_intra, e_pocket])
    E = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    gn = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    return dict(parts=parts, E=E, g=g, gmax=gn.max() if n else 0.0, abs_E=abs_E, abs_g=abs_g, cond_E=cond_E, cond_g=cond_g)


def tolerances(e, rel):
    """Allowed deviation of an implementation from the evaluation `e` of `energy`: (energy and parts, gmax).  rel x the sum of
    the absolute terms, plus 16 roundings (16 x 2.2e-16) of the inputs of the bonded terms: at a minimum 1/2 k (d - r0)^2 is the
    square of a difference that has lost all but a few digits, which no order of summation can give back."""
    eps16 = 16 * np.finfo(np.float64).eps
    return (rel * e['abs_E'] + eps16 * e['cond_E'],
            (rel * e['abs_g'].max() + eps16 * e['cond_g'].max()) if len(e['abs_g']) else 0.0)


def _dot(a, b, reverse):
    return _sum(a.ravel() * b.ravel(), reverse)


def minimize(pos0, topo, lig_vdw, pocket_x, pocket_vdw, params=None, reverse=False):
    """The minimiser of include/kpd.h from the fp32 geometry pos0.  Returns dict: x [n,3] float64 (the rows written, widened),
    x64 (the minimiser's own last point, before the fp32 rounding), pos_out float32, E_before,
    E, parts, pocket_before, gmax_before, gmax, iters, evals, status, rmsd, history (E after every accepted step), margins
    (name, value) of every decision."""
    P = dict(DEFAULTS)
    P.update(params or {})
    x0 = np.asarray(pos0, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = x0.shape[0]
    ev = lambda y: energy(y, topo, lig_vdw, pocket_x, pocket_vdw, P, reverse)
    cur = ev(x0)
    x, g, E = x0.copy(), cur['g'], cur['E']
    first = cur
    S, Y, RHO = [], [], []
    gamma = 1.0
    iters, evals, status = 0, 1, 0
    margins, history = [], [E]
    rel = lambda v: abs(v) / max(1.0, abs(E))
    for _ in range(int(P['max_iters'])):
        margins.append(('converged', rel(cur['gmax'] - P['gtol'])))
        if cur['gmax'] <= P['gtol']:
            break
        iters += 1
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
        pmax = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]).max()
        with np.errstate(divide='ignore'):
            alpha = min(1.0, P['max_step'] / pmax)
        accepted = None
        for _ls in range(21):
            xt = x + alpha * p
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
        s_new, y_new = xt - x, accepted['g'] - g
        sy, yy = _dot(s_new, y_new, reverse), _dot(y_new, y_new, reverse)
        gg = _dot(accepted['g'], accepted['g'], reverse)
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
        x, g, E, cur = xt, accepted['g'], accepted['E'], accepted
        history.append(E)
    x64 = x.copy()
    if iters:               # the report describes the rows written: one more evaluation at the fp32-rounded positions
        xr = x.astype(np.float32).astype(np.float64)
        ulp = np.spacing(np.abs(xr).astype(np.float32)).astype(np.float64)
        margins.append(('ulp', float((0.5 * ulp - np.abs(x - xr)).min()) if n else np.inf))       # in Angstrom, not relative
        fin = ev(xr)
        evals += 1
        margins.append(('round', rel(fin['E'] - first['E'])))
        if fin['E'] <= first['E']:
            x, cur, E = xr, fin, fin['E']
        else:
            x, cur, E = x0.copy(), first, first['E']
    if cur['gmax'] > P['gtol'] and not status & LINE_SEARCH:
        status |= ITER_CAP
    out = x.astype(np.float32)
    d = out.astype(np.float64) - x0
    rmsd = np.sqrt((d * d).sum() / n) if n else 0.0
    return dict(x=x, pos_out=out, E_before=first['E'], E=E, parts=cur['parts'], pocket_before=first['parts'][3],
                gmax_before=first['gmax'], gmax=cur['gmax'], iters=iters, evals=evals, status=status, rmsd=rmsd, history=history,
                margins=margins, first=first, last=cur, x64=x64)


def min_margin(margins, names=None):
    vals = [v for k, v in margins if names is None or k in names]
    return min(vals) if vals else np.inf
