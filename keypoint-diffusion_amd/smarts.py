"""Queries for `kpd_mol_match`: a subset of SMARTS compiled on the host into the int32 table that include/kpd.h defines.

Pure Python, no RDKit, no GPU.  The table is the interface of the C call; this module only writes it.  What is compiled is matched on
the labels of THIS library's sanitised molecules (`kpd_mol_sanitize`): its aromaticity, no charges, no stereo, no ring sizes.  It is
not RDKit's matcher and is not compared with it.

Subset.  Outside brackets: C N O S P F Cl Br I B Si As (aliphatic), c n o s p (aromatic), * a A.  Inside brackets: element symbols
(upper case: aliphatic, c n o s p: aromatic), #n, * a A, D<n> (heavy neighbours), H<n> (hydrogens, implicit and explicit; a bare
[H] is the element, use [#1] anywhere else), X<n> (neighbours + implicit H), v<n> (valence + implicit H), R (in a ring), R0 (in none),
x<n> (ring bonds; bare x: at least one), +0 / -0 (always true; every other charge is never true, with a note), @ / @@ (ignored, with a
note), $(...) (the atom is the image of atom 0 of the inner pattern), and ! & , ; with the precedence of SMARTS.  A number beyond 15
means "15 or more".  Bonds: - = # : ~ @ with ! & , ; and nothing for "single or aromatic".  Branches, ring closures 1 .. 9 and %nn.
Everything else is a ValueError that names the pattern and the column (0-based) of the first thing that cannot be taken:
disconnected queries, r<n>, R<n> with n > 0, k z Z d ^, isotopes, atom maps, / and \\, reactions.
"""
import copy
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import torch

Q_ATOMS, Q_BONDS, Q_ALT, Q_PATTERNS, Q_TOP, Q_MAGIC = 16, 24, 8, 512, 15, 0x4b505101         # KPD_Q_* of include/kpd.h
Q_HEAD, Q_ROW_HEAD, Q_ATOM_WORDS, Q_CLOSE_WORDS, Q_ALT_WORDS, Q_REFS = 4, 4, 4, 4, 16, 2

ALL_Z, ALL16 = (1 << 128) - 1, 0xffff
ALIPHATIC, AROMATIC, NO_RING, RING = 1, 2, 1, 2         # what an alternative allows: bits 0 - 1 and 2 - 3 of its class word
BOND_ANY, BOND_RING, BOND_DEFAULT = 0xff, 0xf0, 0x99    # bit = kind + 4 ring; kind 0 .. 2 = order 1 .. 3, 3 = aromatic
BOND_KIND = {'-': 0x11, '=': 0x22, '#': 0x44, ':': 0x88, '~': BOND_ANY, '@': BOND_RING}
NUMBERS = {'H': 1, 'B': 5, 'C': 6, 'N': 7, 'O': 8, 'F': 9, 'Si': 14, 'P': 15, 'S': 16, 'Cl': 17, 'As': 33, 'Se': 34, 'Br': 35, 'I': 53}
BARE = ('Cl', 'Br', 'Si', 'As', 'C', 'N', 'O', 'S', 'P', 'F', 'I', 'B')       # outside brackets, two letters first
# two-letter element symbols that are not in NUMBERS: refused inside brackets, where their letters would read as two primitives
OTHER_ELEMENTS = frozenset(
    'He Li Be Ne Na Mg Al Ar Ca Sc Ti Cr Mn Fe Co Ni Cu Zn Ga Ge Kr Rb Sr Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te Xe Cs Ba La Ce Pr Nd Pm Sm Eu '
    'Gd Tb Dy Ho Er Tm Yb Lu Hf Ta Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa Np Pu Am Cm Bk Cf Es Fm Md No Lr'.split())
AROMATIC_SYMBOLS = {'c': 6, 'n': 7, 'o': 8, 's': 16, 'p': 15}
FIELDS = ('z', 'ar', 'ring', 'D', 'H', 'X', 'v', 'x')
FULL = dict(z=ALL_Z, ar=3, ring=3, D=ALL16, H=ALL16, X=ALL16, v=ALL16, x=ALL16)


# ---- atom expressions as a disjunction of conjunctions --------------------------------------------------------------------------
def _conj(**fields):
    c = dict(FULL, need=frozenset(), forbid=frozenset())
    c.update(fields)
    return c


def _covers(a, b):
    """Everything that satisfies b satisfies a."""
    return all(b[f] & ~a[f] == 0 for f in FIELDS) and a['need'] <= b['need'] and a['forbid'] <= b['forbid']


def _tidy(dnf):
    """Without duplicates and without a conjunction that another one covers; the order of the rest is kept."""
    out = []
    for c in dnf:
        if not any(_covers(o, c) for o in out):
            out = [o for o in out if not _covers(c, o)] + [c]
    return out


def _and(x, y):
    out = []
    for a in x:
        for b in y:
            c = {f: a[f] & b[f] for f in FIELDS}
            c['need'], c['forbid'] = a['need'] | b['need'], a['forbid'] | b['forbid']
            if all(c[f] for f in FIELDS) and not (c['need'] & c['forbid']):
                out.append(c)
    return _tidy(out)


def _not(x):
    out = [_conj()]
    for c in x:
        parts = [_conj(**{f: FULL[f] & ~c[f]}) for f in FIELDS if c[f] != FULL[f]]
        parts += [_conj(forbid=frozenset([r])) for r in sorted(c['need'])] + [_conj(need=frozenset([r])) for r in sorted(c['forbid'])]
        out = _and(out, [p for p in parts if all(p[f] for f in FIELDS)])
    return out


def _count_mask(k: int) -> int:
    return 1 << min(k, Q_TOP)


class Query:
    """One row: atoms in depth-first order (a disjunction each), parent and parent bond mask per atom, closures (s, t, mask)."""

    def __init__(self):
        self.atoms, self.parent, self.pmask, self.closures, self.cols = [], [], [], [], []


class _Compiler:
    def __init__(self):
        self.rows: List[Query] = []
        self.lifted: Dict[str, int] = {}
        self.notes: List[str] = []

    def lift(self, inner: str, top: str, base: int) -> int:
        if inner not in self.lifted:
            q = _Parser(self, inner, top, base).parse()
            self.rows.append(q)
            self.lifted[inner] = len(self.rows) - 1
        return self.lifted[inner]


class _Parser:
    def __init__(self, comp: _Compiler, text: str, top: str, base: int):
        self.comp, self.s, self.top, self.base, self.i = comp, text, top, base, 0

    def fail(self, what: str, at: Optional[int] = None):
        raise ValueError(f'smarts: pattern {self.top!r}, column {self.base + (self.i if at is None else at)}: {what}')

    def note(self, what: str, at: int):
        self.comp.notes.append(f'pattern {self.top!r}, column {self.base + at}: {what}')

    def peek(self) -> str:
        return self.s[self.i] if self.i < len(self.s) else ''

    def number(self) -> Optional[int]:
        j = self.i
        while self.peek().isdigit():
            self.i += 1
        return int(self.s[j:self.i]) if self.i > j else None

    # ---- the chain ---------------------------------------------------------------------------------------------------------------
    def parse(self) -> Query:
        q, s = Query(), self.s
        stack, prev, bond, opened = [], -1, None, {}
        while self.i < len(s):
            ch = s[self.i]
            if ch == '(':
                if prev < 0:
                    self.fail('a branch before the first atom')
                stack.append(prev)
                self.i += 1
            elif ch == ')':
                if not stack or bond is not None:
                    self.fail('a ")" without its "(", or behind a bond')
                prev = stack.pop()
                self.i += 1
            elif ch == '.':
                self.fail('disconnected queries (".") are not supported')
            elif ch in '/\\':
                self.fail('stereo bonds are not supported')
            elif ch == '>':
                self.fail('reaction queries are not supported')
            elif ch in BOND_KIND or ch == '!':
                if bond is not None or prev < 0:
                    self.fail('a bond without an atom in front of it')
                bond = self.bond_low()
            elif ch.isdigit() or ch == '%':
                at = self.i
                if prev < 0:
                    self.fail('a ring closure before the first atom')
                if ch == '%':
                    if not (s[self.i + 1:self.i + 3].isdigit() and len(s[self.i + 1:self.i + 3]) == 2):
                        self.fail('"%" needs two digits')
                    num, self.i = int(s[self.i + 1:self.i + 3]), self.i + 3
                else:
                    num, self.i = int(ch), self.i + 1
                if num in opened:
                    a, m, _ = opened.pop(num)
                    if m is not None and bond is not None and m != bond:
                        self.fail('the two ends of a ring closure carry different bonds', at)
                    lo, hi = min(a, prev), max(a, prev)           # behind a closed branch the closing atom is the earlier one
                    if lo == hi or q.parent[hi] == lo or any(c[:2] == (lo, hi) for c in q.closures):
                        self.fail('a ring closure onto the atom itself or onto a bond that is there already', at)
                    q.closures.append((lo, hi, BOND_DEFAULT if m is None and bond is None else m if bond is None else bond))
                else:
                    opened[num] = (prev, bond, at)
                bond = None
            else:
                at = self.i
                dnf = self.bracket() if ch == '[' else self.bare()
                if len(q.atoms) >= Q_ATOMS:
                    self.fail(f'more than {Q_ATOMS} atoms in one query', at)
                if prev < 0 and q.atoms:
                    self.fail('an atom without a bond to the atoms before it', at)
                q.atoms.append(dnf)
                q.cols.append(self.base + at)
                q.parent.append(prev)
                q.pmask.append(0 if prev < 0 else BOND_DEFAULT if bond is None else bond)
                prev, bond = len(q.atoms) - 1, None
        if stack:
            self.fail('a "(" is never closed')
        if opened:
            self.fail('a ring closure is never closed', min(v[2] for v in opened.values()))
        if bond is not None:
            self.fail('a bond without an atom behind it')
        if not q.atoms:
            self.fail('no atom')
        if len(q.atoms) - 1 + len(q.closures) > Q_BONDS:
            self.fail(f'more than {Q_BONDS} bonds in one query', 0)
        return q

    def bare(self):
        s = self.s
        for sym in BARE:
            if s.startswith(sym, self.i):
                self.i += len(sym)
                return [_conj(z=1 << NUMBERS[sym], ar=ALIPHATIC)]
        ch = s[self.i]
        if ch in AROMATIC_SYMBOLS:
            self.i += 1
            return [_conj(z=1 << AROMATIC_SYMBOLS[ch], ar=AROMATIC)]
        if ch in '*aA':
            self.i += 1
            return [_conj() if ch == '*' else _conj(ar=AROMATIC if ch == 'a' else ALIPHATIC)]
        self.fail(f'{ch!r} is not an atom, a bond or a branch of the supported subset')

    # ---- bonds: masks are a Boolean algebra of their own -----------------------------------------------------------------------------
    def bond_low(self) -> int:
        m = self.bond_or()
        while self.peek() == ';':
            self.i += 1
            m &= self.bond_or()
        return m

    def bond_or(self) -> int:
        m = self.bond_and()
        while self.peek() == ',':
            self.i += 1
            m |= self.bond_and()
        return m

    def bond_and(self) -> int:
        m = self.bond_unary()
        while self.peek() == '&' or self.peek() in BOND_KIND or self.peek() == '!':
            if self.peek() == '&':
                self.i += 1
            m &= self.bond_unary()
        return m

    def bond_unary(self) -> int:
        if self.peek() == '!':
            self.i += 1
            return BOND_ANY & ~self.bond_unary()
        ch = self.peek()
        if ch in '/\\':
            self.fail('stereo bonds are not supported')
        if ch not in BOND_KIND or not ch:
            self.fail('a bond symbol is expected here')
        self.i += 1
        return BOND_KIND[ch]

    # ---- a bracket atom ------------------------------------------------------------------------------------------------------------------
    def bracket(self):
        self.open_at = self.i
        self.i += 1
        if self.peek().isdigit():
            self.fail('isotopes are not supported')
        dnf = self.atom_low()
        if self.peek() != ']':
            self.fail('"]" is expected here' if self.peek() else 'a "[" is never closed')
        self.i += 1
        return dnf

    def atom_low(self):
        d = self.atom_or()
        while self.peek() == ';':
            self.i += 1
            d = _and(d, self.atom_or())
        return d

    def atom_or(self):
        d = self.atom_and()
        while self.peek() == ',':
            self.i += 1
            d = _tidy(d + self.atom_and())
        return d

    def atom_and(self):
        d = self.atom_unary()
        while self.peek() not in (']', ',', ';', ''):
            if self.peek() == '&':
                self.i += 1
            d = _and(d, self.atom_unary())
        return d

    def atom_unary(self):
        if self.peek() == '!':
            self.i += 1
            return _not(self.atom_unary())
        return self.primitive()

    def primitive(self):
        s, at = self.s, self.i
        ch = self.peek()
        if not ch:
            self.fail('a "[" is never closed')
        if ch == '$':
            if s[at + 1:at + 2] != '(':
                self.fail('"$" needs "(...)"')
            depth, j = 0, at + 1
            while j < len(s):
                depth += (s[j] == '(') - (s[j] == ')')
                if depth == 0:
                    break
                j += 1
            if j >= len(s):
                self.fail('the "(" of a "$(" is never closed')
            self.i = j + 1
            return [_conj(need=frozenset([self.comp.lift(s[at + 2:j], self.top, self.base + at + 2)]))]
        if ch == '#':
            self.i += 1
            n = self.number()
            if n is None or n > 127:
                self.fail('"#" needs an atomic number in 0 .. 127', at)
            return [_conj(z=1 << n)]
        if ch == '*':
            self.i += 1
            return [_conj()]
        if ch in '+-':
            while self.peek() == ch:
                self.i += 1
            signs, n = self.i - at, self.number()
            charge = signs if n is None else n
            if signs > 1 and n is not None:
                self.fail('a charge is written with signs or with a number, not both', at)
            if charge == 0:
                return [_conj()]
            self.note('a charge other than 0 is never true: the sanitised molecules carry none', at)
            return []
        if ch == '@':
            while self.peek() == '@':
                self.i += 1
            self.note('chirality is ignored', at)
            return [_conj()]
        if ch == ':':
            self.fail('atom maps are not supported')
        if ch in 'rkzZd^':
            self.fail(f'the primitive {ch!r} is not supported (no ring sizes, heteroatom counts or hybridisation)')
        two = s[at:at + 2]
        if two in OTHER_ELEMENTS:
            self.fail(f'the element {two!r} is outside the supported subset (write #n for its atomic number)')
        if len(two) == 2 and two in NUMBERS:
            self.i += 2
            return [_conj(z=1 << NUMBERS[two], ar=ALIPHATIC)]
        if ch == 'H':
            self.i += 1
            if s[self.open_at:self.i + 1] == '[H]':
                return [_conj(z=1 << 1)]
            n = self.number()
            return [_conj(H=_count_mask(1 if n is None else n))]
        if ch in 'DXv':
            self.i += 1
            n = self.number()
            return [_conj(**{ch: _count_mask(1 if n is None else n)})]
        if ch == 'x':
            self.i += 1
            n = self.number()
            return [_conj(x=ALL16 & ~1 if n is None else _count_mask(n))]
        if ch == 'R':
            self.i += 1
            n = self.number()
            if n:
                self.fail('R<n> with n > 0 (a number of rings) is not supported', at)
            return [_conj(ring=RING if n is None else NO_RING)]
        if ch in 'aA':
            self.i += 1
            return [_conj(ar=AROMATIC if ch == 'a' else ALIPHATIC)]
        if ch in NUMBERS:
            self.i += 1
            return [_conj(z=1 << NUMBERS[ch], ar=ALIPHATIC)]
        if ch in AROMATIC_SYMBOLS:
            self.i += 1
            return [_conj(z=1 << AROMATIC_SYMBOLS[ch], ar=AROMATIC)]
        if ch.isdigit():
            self.fail('a number without a primitive in front of it (isotopes are not supported)')
        self.fail(f'{ch!r} is not a primitive of the supported subset')


# ---- the table -----------------------------------------------------------------------------------------------------------------
def _signed(w: int) -> int:
    return w - (1 << 32) if w >= 1 << 31 else w


def _row_words(q: Query, top: str) -> List[int]:
    atoms, alts = [], []
    for t, dnf in enumerate(q.atoms):
        if len(dnf) > Q_ALT:
            raise ValueError(f'smarts: pattern {top!r}, column {q.cols[t]}: this atom expands to {len(dnf)} alternatives, more than {Q_ALT}')
        first = len(alts) // Q_ALT_WORDS
        for c in dnf or [dict(FULL, z=0, need=frozenset(), forbid=frozenset())]:          # nothing left: an alternative that never holds
            if len(c['need']) > Q_REFS or len(c['forbid']) > Q_REFS:
                raise ValueError(f'smarts: pattern {top!r}, column {q.cols[t]}: more than {Q_REFS} "$(...)" (or "!$(...)") in one alternative')
            need, forbid = sorted(c['need']) + [-1, -1], sorted(c['forbid']) + [-1, -1]
            alts += [_signed((c['z'] >> (32 * w)) & 0xffffffff) for w in range(4)]
            alts += [c['ar'] | c['ring'] << 2, c['D'], c['H'], c['X'], c['v'], c['x']] + need[:2] + forbid[:2] + [0, 0]
        atoms += [q.parent[t], q.pmask[t], first, max(1, len(dnf))]
    closes = [w for s, t, m in q.closures for w in (s, t, m, 0)]
    return [len(q.atoms), len(q.closures), len(alts) // Q_ALT_WORDS, 0] + atoms + closes + alts


def table_words(rows: Sequence[Sequence[int]]) -> List[int]:
    """The whole table from the words of its rows (the head and the offsets in front)."""
    P = len(rows)
    at, offsets = Q_HEAD + P, []
    for r in rows:
        offsets.append(at)
        at += len(r)
    return [Q_MAGIC, P, at, 0] + offsets + [w for r in rows for w in r]


class Patterns:
    """A compiled list of queries.  `table`: the int32 tensor `kpd_mol_match` reads (`host`: the same words on the CPU, which the call
    checks); `n` user patterns with `names`; `rows[k]`: the row of the table user pattern k became (the rows lifted out of "$(...)"
    lie in between and are not reported); `n_rows`: all rows; `notes`: what was ignored or can never be true."""

    def __init__(self, words: Sequence[int], names: Sequence[str], rows: Sequence[int], notes: Sequence[str], smarts: Sequence[str] = ()):
        self.host = torch.tensor(list(words), dtype=torch.int32)
        self.table, self._on = self.host, {}
        self.names, self.rows, self.notes, self.smarts = list(names), list(rows), list(notes), list(smarts)
        self.n, self.n_rows = len(self.rows), int(self.host[1])

    def _cached(self, device, what: str, make):
        key = (str(device), what)
        if key not in self._on:
            self._on[key] = make().to(device)
        return self._on[key]

    def to(self, device) -> 'Patterns':
        """These Patterns with `table` on `device`: a view that shares everything else (one copy per device, made once); the
        object it is called on keeps its own `table`."""
        view = copy.copy(self)
        view.table = self._cached(device, 'table', lambda: self.host)
        return view

    def row_index(self, device) -> torch.Tensor:
        """`rows` as an int64 tensor on `device` (copied once per device)."""
        return self._cached(device, 'rows', lambda: torch.tensor(self.rows, dtype=torch.long))

    def user_index(self, device) -> torch.Tensor:
        """[n_rows + 1] int32 on `device`: row -> the user's pattern, -1 for a lifted row; the last entry (index -1) is -1."""
        def make():
            user = torch.full((self.n_rows + 1,), -1, dtype=torch.int32)
            user[torch.tensor(self.rows, dtype=torch.long)] = torch.arange(self.n, dtype=torch.int32)
            return user
        return self._cached(device, 'user', make)

    def __len__(self) -> int:
        return self.n


def compile(patterns: Sequence[str], names: Optional[Sequence[str]] = None) -> Patterns:       # noqa: A001 (the name the callers read)
    """SMARTS strings -> Patterns.  ValueError names the pattern and the column of the first thing outside the subset."""
    if isinstance(patterns, str):
        patterns = [patterns]
    if isinstance(patterns, dict):
        names, patterns = list(patterns), list(patterns.values())
    patterns = list(patterns)
    if not patterns:
        raise ValueError('smarts: no pattern')
    names = list(patterns) if names is None else list(names)
    if len(names) != len(patterns):
        raise ValueError(f'smarts: {len(names)} names for {len(patterns)} patterns')
    comp, user, tops = _Compiler(), [], []
    for text in patterns:
        if not isinstance(text, str):
            raise ValueError(f'smarts: a pattern must be a string, got {type(text).__name__}')
        before = len(comp.rows)
        q = _Parser(comp, text, text, 0).parse()
        tops += [text] * (len(comp.rows) - before + 1)
        comp.rows.append(q)
        user.append(len(comp.rows) - 1)
        if len(comp.rows) > Q_PATTERNS:
            raise ValueError(f'smarts: pattern {text!r}: the table would have more than {Q_PATTERNS} rows (the rows lifted out of "$(...)" count)')
    return Patterns(table_words([_row_words(q, top) for q, top in zip(comp.rows, tops)]), names, user, comp.notes, patterns)


# Named queries written for THIS library's sanitised form: no charges, so a nitro group appears in its demoted form (N with three
# single bonds, both O read as hydroxyls: the limit kpd_mol_sanitize states); aromaticity is kpd_mol_sanitize's.
FUNCTIONAL_GROUPS = OrderedDict([
    ('hydroxyl', '[OX2H][#6]'),
    ('phenol', '[OX2H]c'),
    ('carboxylic acid', '[CX3](=O)[OX2H]'),
    ('ester', '[CX3](=O)[OX2H0][#6]'),
    ('ether', '[OD2]([#6;!$(C=O)])[#6;!$(C=O)]'),
    ('aldehyde', '[CX3H1](=O)[#6]'),
    ('ketone', '[#6][CX3](=O)[#6]'),
    ('amide', '[CX3](=O)[NX3]'),
    ('primary amine', '[N;X3;H2;!$(NC=O)]'),
    ('secondary amine', '[N;X3;H1;!$(NC=O)]'),
    ('tertiary amine', '[N;X3;H0;!$(NC=O);!$(NO)]'),
    ('nitrile', '[CX2]#[NX1]'),
    ('nitro (demoted)', '[NX3]([OX2H])([OX2H])[#6]'),
    ('sulfonamide', '[SX4](=O)(=O)[NX3]'),
    ('sulfone', '[SX4](=O)(=O)([#6])[#6]'),
    ('thiol', '[SX2H]'),
    ('thioether', '[SX2]([#6])[#6]'),
    ('halide', '[F,Cl,Br,I]'),
    ('phenyl', 'c1ccccc1'),
    ('pyridine-type N', '[nX2]'),
    ('pyrrole-type NH', '[nX3H1]'),
])
