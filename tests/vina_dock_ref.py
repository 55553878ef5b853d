"""Float64 numpy restatement of kpd_vina_dock as include/kpd.h defines it, built on tests/vina_min_ref.py: its `tree`, `evaluate`,
`project`, `move` and `velocity` are used as they are; the iteration loop of its `minimize` is restated here as `minimise(x, K)`,
because `minimize` rounds its start to fp32 and closes with the fp32 step, which a step of the search must not do (the config test
checks that the two loops agree to the bit from an fp32 start).  Philox4x32-10 in Python integers.  `reverse=True` sums every
energy, gradient, projection, dot product, centre, radius of gyration and RMSD in the opposite order; `margins` records how far
every decision was from going the other way."""
import math

import numpy as np

from . import vina_min_ref as R
from . import vina_ref as V

NO_MOLECULE, BAD_INPUT, ATOM_OUT, FROZEN, FRAGMENTS, BAD_BOX, START_OUTSIDE, FEW_MODES = 1, 2, 4, 16, 32, 128, 256, 512
DEFAULTS = dict(R.DEFAULTS, temperature=1.2, amplitude=2.0, min_rmsd=1.0, step_iters=20)
REPORT = ('score', 'E', 'inter', 'intra', 'rmsd_input', 'rmsd_best', 'chain', 'gnorm')
CHAIN_REPORT = ('E', 'inter', 'intra', 'best_step', 'accepted', 'box_rejected', 'evaluations', 'found', 'gnorm', 'score')
Q_MUTATION, Q_METROPOLIS, Q_FRAGMENT, Q_ROTORS = 0, 1, 2, 18
M32 = 0xFFFFFFFF


def philox(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter (4 words), key (2 words) -> 4 words."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniforms(q, s, c, lig_id, seed):
    """The four uniforms of block (q, s, c, lig_id): u = (w + 0.5) 2^-32."""
    return [(w + 0.5) * 2.0 ** -32 for w in philox((q, s, c, lig_id), (seed & M32, (seed >> 32) & M32))]


def ball(u1, u2, u3):
    z, phi, rho = 2.0 * u1 - 1.0, (2.0 * math.pi) * u2, float(np.cbrt(u3))
    sq = math.sqrt(1.0 - z * z)
    return np.array([rho * (sq * math.cos(phi)), rho * (sq * math.sin(phi)), rho * z])


def centre(x, reverse=False):
    return R._sum(x, reverse, axis=0) / len(x)


def box_margin(x, lo, hi, reverse=False):
    """min over the coordinates of the distance of the ligand's centre to the box faces: negative iff outside."""
    c = centre(x, reverse)
    return float(min((c - lo).min(), (hi - c).min()))


def gyration(x, t, f, reverse=False):
    idx = np.nonzero(t['frag'] == f)[0]
    d = x[idx] - R.centres(x, t)[f]
    return math.sqrt(R._sum((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], reverse) / len(idx))


def rmsd(a, b, reverse=False):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return math.sqrt(R._sum((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], reverse) / len(d))


def minimise(x, K, ev, t, P, reverse, margins):
    """minimise(x, K) of include/kpd.h: the loop of vina_min_ref.minimize from the float64 point x, without its closing step.
    `ev(y)` evaluates.  Returns the last point and its evaluation (with gd and gnorm) and the number of evaluations."""
    def chart(y, e):
        e['gd'] = R.project(y, e['g'], t, reverse)
        e['gnorm'] = float(np.abs(e['gd']).max()) if len(e['gd']) else 0.0
        return e

    cur, x = chart(x, ev(x)), np.array(x, dtype=np.float64)
    E, evals = cur['E'], 1
    S, Y, RHO, gamma = [], [], [], 1.0
    rel = lambda v: abs(v) / max(1.0, abs(E))
    for _ in range(int(K)):
        margins.append(('converged', rel(cur['gnorm'] - P['gtol'])))
        if cur['gnorm'] <= P['gtol']:
            break
        g = cur['gd']
        p = g.copy()
        al = []
        for k in range(len(S) - 1, -1, -1):
            a = RHO[k] * R._dot(S[k], p, reverse)
            al.append(a)
            p = p - a * Y[k]
        if S:
            p = p * gamma
        for k in range(len(S)):
            be = RHO[k] * R._dot(Y[k], p, reverse)
            p = p + (al[len(S) - 1 - k] - be) * S[k]
        p = -p
        gp = R._dot(g, p, reverse)
        margins.append(('descent', rel(gp)))
        if not gp < 0.0:
            S, Y, RHO = [], [], []
            p = -g
            gp = -R._dot(g, g, reverse)
        v = R.velocity(x, p, t)
        vmax = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).max()
        with np.errstate(divide='ignore'):
            alpha = min(1.0, P['max_step'] / vmax)
        accepted = None
        for _ls in range(21):
            xt = R.move(x, alpha * p, t)
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
            break
        chart(xt, accepted)
        s_new, y_new = alpha * p, accepted['gd'] - g
        sy, yy = R._dot(s_new, y_new, reverse), R._dot(y_new, y_new, reverse)
        gg = R._dot(accepted['gd'], accepted['gd'], reverse)
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
    return x, cur, evals


def start_delta(x, t, lo, hi, c, lig_id, seed):
    """The delta of the random start of chain c >= 1."""
    F, T = t['F'], t['T']
    cen, d = R.centres(x, t), np.zeros(6 * t['F'] + t['T'])
    for f in range(F):
        u = uniforms(Q_FRAGMENT + 2 * f, 0, c, lig_id, seed)
        d[6 * f + 3:6 * f + 6] = math.pi * ball(u[0], u[1], u[2])
        u = np.array(uniforms(Q_FRAGMENT + 2 * f + 1, 0, c, lig_id, seed)[:3])
        d[6 * f:6 * f + 3] = (lo + u * (hi - lo)) - cen[f]
    for k in range(T):
        d[6 * F + k] = math.pi * (2.0 * uniforms(Q_ROTORS + k // 4, 0, c, lig_id, seed)[k % 4] - 1.0)
    return d


def mutation_delta(x, t, s, c, lig_id, seed, amplitude, reverse=False):
    """The delta of step s from the current pose x, and the entity it moves."""
    F, T = t['F'], t['T']
    u = uniforms(Q_MUTATION, s, c, lig_id, seed)
    e = min(int(math.floor(u[0] * (2 * F + T))), 2 * F + T - 1)
    d, v = np.zeros(6 * F + T), ball(u[1], u[2], u[3])
    if e < F:
        d[6 * e:6 * e + 3] = amplitude * v
    elif e < 2 * F:
        f = e - F
        r = gyration(x, t, f, reverse)
        if r >= 1e-6:
            d[6 * f + 3:6 * f + 6] = (amplitude / r) * v
    else:
        d[6 * F + e - 2 * F] = math.pi * (2.0 * u[1] - 1.0)
    return d, e


def run_chain(pos0, t, types, radius, ppos, ptypes, pradius, lo, hi, c, lig_id, seed, n_steps, P, reverse=False):
    """Chain c of one ligand.  Returns dict: found, pos (float32 rows), x64 (the float64 point whose rounding the rows are: the refined one, or the best), report (keys
    CHAIN_REPORT), margins."""
    x0 = np.asarray(pos0, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    margins, n_rot = [], t['n_rot']
    ev = lambda y: R.evaluate(y, t, types, radius, ppos, ptypes, pradius, P, reverse)
    out = dict(found=0, pos=x0.astype(np.float32), x64=x0.copy(), margins=margins)
    rep = dict(E=0.0, inter=0.0, intra=0.0, best_step=-1, accepted=0, box_rejected=0, evaluations=0, found=0, gnorm=0.0, score=0.0)
    out['report'] = rep
    x = x0 if c == 0 else R.move(x0, start_delta(x0, t, lo, hi, c, lig_id, seed), t)
    x, e, n = minimise(x, P['step_iters'], ev, t, P, reverse, margins)
    rep['evaluations'] += n
    if not np.isfinite(e['E']):
        return out
    if c > 0:                                                 # a random start that left the box ends the chain
        m = box_margin(x, lo, hi, reverse)
        margins.append(('box', abs(m)))
        if m < 0:
            rep['box_rejected'] += 1
            return out
    cur, E_cur, best, E_best = x, e['E'], x, e['E']
    rep.update(found=1, best_step=0)
    out['found'] = 1
    for s in range(1, int(n_steps) + 1):
        delta, _ = mutation_delta(cur, t, s, c, lig_id, seed, P['amplitude'], reverse)
        x = R.move(cur, delta, t)
        m = box_margin(x, lo, hi, reverse)
        margins.append(('box', abs(m)))
        if m < 0:
            rep['box_rejected'] += 1
            continue
        x, e, n = minimise(x, P['step_iters'], ev, t, P, reverse, margins)
        rep['evaluations'] += n
        m = box_margin(x, lo, hi, reverse)
        margins.append(('box', abs(m)))
        if m < 0:
            rep['box_rejected'] += 1
            continue
        E = e['E']
        fin = bool(np.isfinite(E))
        if fin:
            margins.append(('best', abs(E - E_best) / max(1.0, abs(E_best))))
        if fin and E < E_best:
            best, E_best = x, E
            rep['best_step'] = s
        u = uniforms(Q_METROPOLIS, s, c, lig_id, seed)[0]
        if fin:
            gap = math.log(u) * P['temperature'] - (E_cur - E)              # accepted by the draw iff gap < 0
            margins.append(('metropolis', (max(E_cur - E, -gap) if E < E_cur else abs(gap)) / max(1.0, abs(E_cur - E))))
            if E < E_cur or u < math.exp(min((E_cur - E) / P['temperature'], 700.0)):
                cur, E_cur = x, E
                rep['accepted'] += 1
    x, e, n = minimise(best, P['max_iters'], ev, t, P, reverse, margins)
    rep['evaluations'] += n
    out['x64'] = x.copy()
    xr = x.astype(np.float32).astype(np.float64)
    ulp = np.spacing(np.abs(xr).astype(np.float32)).astype(np.float64)
    margins.append(('ulp', float((0.5 * ulp - np.abs(x - xr)).min())))                # in Angstrom, not relative
    fin = ev(xr)
    rep['evaluations'] += 1
    margins.append(('round', abs(fin['E'] - E_best) / max(1.0, abs(E_best))))
    keep = bool(fin['E'] <= E_best)
    if keep and c > 0:                                        # chain 0 is the minimiser: no box
        m = box_margin(xr, lo, hi, reverse)
        margins.append(('box', abs(m)))
        keep = m >= 0
    if not keep:
        out['x64'] = best.copy()
        xr = best.astype(np.float32).astype(np.float64)
        fin = ev(xr)
        rep['evaluations'] += 1
    gd = R.project(xr, fin['g'], t, reverse)
    rep.update(E=fin['E'], inter=fin['inter'], intra=fin['intra'], gnorm=float(np.abs(gd).max()) if len(gd) else 0.0,
               score=fin['inter'] / (1.0 + P['w_rot'] * n_rot))
    out['pos'] = xr.astype(np.float32)
    return out


def modes(chains, pos0, n_modes, min_rmsd, reverse=False):
    """Ranking and clustering of the chains' poses.  Returns (the kept chain indices in rank order, report rows (dicts with the keys
    REPORT), margins)."""
    margins = []
    order = sorted((c for c, ch in enumerate(chains) if ch['found']), key=lambda c: (chains[c]['report']['E'], c))
    for a, b in zip(order, order[1:]):
        Ea, Eb = chains[a]['report']['E'], chains[b]['report']['E']
        margins.append(('rank', abs(Eb - Ea) / max(1.0, abs(Ea))))
    kept = []
    for c in order:
        if len(kept) == n_modes:
            break
        ds = [rmsd(chains[c]['pos'], chains[k]['pos'], reverse) for k in kept]
        margins.extend(('rmsd', abs(d - min_rmsd)) for d in ds)
        if all(d >= min_rmsd for d in ds):
            kept.append(c)
    x0 = np.asarray(pos0, dtype=np.float32)
    rows = []
    for c in kept:
        r = chains[c]['report']
        rows.append(dict(score=r['score'], E=r['E'], inter=r['inter'], intra=r['intra'], rmsd_input=rmsd(chains[c]['pos'], x0, reverse),
                         rmsd_best=rmsd(chains[c]['pos'], chains[kept[0]]['pos'], reverse) if c != kept[0] else 0.0, chain=c,
                         gnorm=r['gnorm']))
    return kept, rows, margins


def dock_ligand(pos, z_atoms, bonds, orders, frag, radius, ppos, ptypes, pradius, box_lo, box_hi, lig_id=0, seed=0, n_chains=2, n_steps=0,
                n_modes=1, params=None, type_in=None, max_rotors=R.MAX_ROTORS, reverse=False):
    """The whole search of one well-formed ligand in one typed pocket.  Returns dict: chains (run_chain's), kept, report (rows of
    modes), n_found, status, margins (all of them), tree, types."""
    P = dict(DEFAULTS, **(params or {}))
    types = V.ligand_types(z_atoms, bonds, orders, radius, type_in)
    t = R.tree(z_atoms, bonds, orders, frag, max_rotors, types)
    lo = np.asarray(box_lo, dtype=np.float32).astype(np.float64)
    hi = np.asarray(box_hi, dtype=np.float32).astype(np.float64)
    x0 = np.asarray(pos, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    chains = [run_chain(pos, t, types, radius, ppos, ptypes, pradius, lo, hi, c, lig_id, seed, n_steps, P, reverse) for c in range(n_chains)]
    kept, rows, margins = modes(chains, pos, n_modes, P['min_rmsd'], reverse)
    m0 = box_margin(x0, lo, hi, reverse)
    margins.append(('box', abs(m0)))
    for ch in chains:
        margins.extend(ch['margins'])
    status = (START_OUTSIDE if m0 < 0 else 0) | (FEW_MODES if len(kept) < n_modes else 0) | (FROZEN if t['n_rot'] > t['T'] else 0)
    if (np.asarray(types) < 0).any() or (np.asarray(ptypes) < 0).any() or not (np.asarray(pradius, dtype=np.float32) > 0).all():
        status |= ATOM_OUT
    return dict(chains=chains, kept=kept, report=rows, n_found=len(kept), status=status, margins=margins, tree=t, types=types)
