"""The plausibility checks of include/kpd.h (kpd_pose_check) without a GPU: the restatement (tests/pose_check_ref.py) on molecules
written by hand, where every distortion must set exactly its own bits; the lattice count of check 6 against a brute force; the
distance of every compared value from its threshold, so that the GPU test may compare flags exactly; and the refusals of the
Python surface."""
import os
import re

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import pose_check_cases as PC
from . import pose_check_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6


@pytest.fixture(scope='module')
def results():
    """name -> (case, the restatement's output, the margins of its comparisons)."""
    out = {}
    for c in PC.all_cases():
        m = []
        out[c['name']] = (c, PC.run_case(c, margins=m), m)
    return out


def bits_of(fail):
    return [n for k, n in enumerate(R.FAIL_NAMES) if (int(fail) >> k) & 1]


# ---- hand molecules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in PC.ideal()])
def test_ideal_molecules_pass_everything(results, name):
    c, out, _ = results[name]
    assert out['fail'][0, 0] == 0 and not out['atom_fail'].any(), (name, bits_of(out['fail'][0, 0]))
    assert out['status'][0, 0] == (R.ATOM_OUT if 'H' in c['sym'] else 0)          # hydrogens have radius 0 unless asked for
    cnt = dict(zip(R.COUNTS, out['counts'][0, 0]))
    assert cnt['bonds'] == len(c['bonds']) and not any(cnt[k] for k in R.COUNTS if k.endswith('_fail'))


def test_what_the_ideal_molecules_examine(results):
    count = lambda name: dict(zip(R.COUNTS, results[name][1]['counts'][0, 0]))
    assert count('benzene')['rings'] == 1 and count('benzene')['angles'] == 6 and count('benzene')['pairs'] == 0
    assert count('ethene')['centres'] == 2 and count('ethene')['torsions'] == 4 and count('ethene')['torsions_skipped'] == 0
    assert count('acetamide')['centres'] == 1 and count('acetamide')['angles'] == 3 and count('acetamide')['torsions'] == 0
    assert count('hexane')['pairs'] == 3 and count('hexane')['angles'] == 4           # 1-5, 2-6 and 1-6
    rep = dict(zip(R.REPORT, results['ethene'][1]['report'][0, 0]))
    assert rep['bond_min'] == pytest.approx(1.0, abs=1e-6) and rep['twist_min'] == pytest.approx(1.0, abs=1e-9)


@pytest.mark.parametrize('name', [c['name'] for c in PC.distorted()])
def test_every_distortion_sets_exactly_its_bits(results, name):
    c, out, _ = results[name]
    assert out['fail'][0, 0] == c['expect'], (name, bits_of(out['fail'][0, 0]), bits_of(c['expect']))
    marked = np.bitwise_or.reduce(out['atom_fail'][0]) if out['atom_fail'].size else 0
    assert marked == c['expect'], (name, 'the atoms carry the bits of the checks that fail, and no other')


def test_values_behind_the_distortions(results):
    rep = lambda name: dict(zip(R.REPORT, results[name][1]['report'][0, 0]))
    assert rep('acetamide, carbonyl carbon lifted 0.4 A')['centre_max'] == pytest.approx(0.4, abs=1e-6)
    assert rep('ethene twisted 45 degrees')['twist_min'] == pytest.approx(0.5, abs=1e-6)
    assert rep('propane, a bond stretched x 1.3')['bond_max'] == pytest.approx(1.3 * 1.53 / 1.50, abs=1e-6)
    assert rep('hexane folded, 1-6 contact at 2.0 A')['clash_min'] == pytest.approx(2.0 / 3.4, abs=1e-3)
    assert rep('hexane, 2.0 A from a pocket carbon')['pocket_min'] == pytest.approx(2.0 / 3.4, abs=1e-6)
    assert rep('benzene, one atom lifted 0.6 A')['ring_max'] > 0.25
    c, out, _ = results['benzene, one atom lifted 0.6 A']
    assert (out['atom_fail'][0] == R.F_RING).all()                                     # every atom of the ring
    c, out, _ = results['hexane folded, 1-6 contact at 2.0 A']
    assert out['atom_fail'][0].tolist() == [R.F_CLASH, 0, 0, 0, 0, R.F_CLASH]


def test_no_pocket_means_no_points(results):
    for name in ('benzene', 'hexane'):
        cnt = dict(zip(R.COUNTS, results[name][1]['counts'][0, 0]))
        assert cnt['pocket_pairs'] == 0 and cnt['n_lig_points'] == 0 and cnt['n_overlap_points'] == 0


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in PC.all_cases() if c['pocket'] is not None])
def test_enumeration_equals_brute_force(results, name):
    c, out, _ = results[name]
    brute = PC.run_case(c, lattice=R.lattice_brute)
    for k in ('n_lig_points', 'n_overlap_points'):
        col = R.COUNTS.index(k)
        assert out['counts'][0, 0, col] == brute['counts'][0, 0, col], (name, k)
    assert out['counts'][0, 0, R.COUNTS.index('n_lig_points')] > 0


def test_points_at_exactly_the_radius_count(results):
    """R = 1.5 and h = 0.5 with the atom on a lattice point: the points are the integer triples with i^2 + j^2 + k^2 <= 9, the six at
    exactly d = R among them, and every d2 is exact in fp64."""
    c, out, _ = results['one carbon on a lattice point, R = 1.5']
    want = sum(i * i + j * j + k * k <= 9 for i in range(-4, 5) for j in range(-4, 5) for k in range(-4, 5))
    inside = sum(i * i + j * j + k * k < 9 for i in range(-4, 5) for j in range(-4, 5) for k in range(-4, 5))
    assert want == 123 and inside < want
    assert out['counts'][0, 0, R.COUNTS.index('n_lig_points')] == want


def test_a_ligand_straddling_the_origin(results):
    c, out, _ = results['benzene straddling the origin']
    assert (c['pose'] < 0).any() and (c['pose'] > 0).any()
    # truncation instead of floor would lose the layer of points at the lowest negative index: the range must reach it, and the
    # brute force of test_enumeration_equals_brute_force (which has its own floor) must agree with the enumeration on this case
    assert R._axis_range(-0.2, 1.7, 0.5) == (-4, 3) and int(-3.8) == -3
    takes = [(a, tuple(float(v) for v in c['pose'][a]), float(np.float32(PC.VDW['C']))) for a in range(6)]
    n_lig, _, _ = R.lattice_counts(takes, [], 0.5, 0.8)
    assert n_lig == out['counts'][0, 0, R.COUNTS.index('n_lig_points')] == R.lattice_brute(takes, [], 0.5, 0.8)[0]


# ---- margins -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in PC.all_cases()])
def test_no_compared_value_sits_on_its_threshold(results, name):
    _, _, margins = results[name]
    assert margins and min(margins) >= MARGIN, (name, min(margins))


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 256])
def test_no_compared_value_of_the_chains_sits_on_its_threshold(n):
    """The chains of the GPU tests: their flags are compared exactly there as well."""
    margins = []
    out = PC.run_case(PC.chain_case(n), margins=margins)
    assert out['status'][0, 0] == 0 and (n == 1 or min(margins) >= MARGIN), (n, min(margins, default=None))


# ---- the header and the Python layer -------------------------------------------------------------------------------------------------------
def test_header_declares_the_call_and_its_limits():
    text = open(os.path.join(ROOT, 'include', 'kpd.h')).read()
    assert 'kpd_status kpd_pose_check(' in text and 'void kpd_pose_check_defaults(' in text
    assert "NOT PoseBusters' NUMBERS" in text and 'AS RECALLED, NOT' in text
    fields = re.search(r'typedef struct kpd_pose_check_params \{(.*?)\}', text, re.S).group(1)
    assert [f.strip() for f in fields.replace('double', '').replace(';', '').split(',')] == [f[0] for f in hip.KpdPoseCheckParams._fields_]
    assert list(R.DEFAULTS) == [f[0] for f in hip.KpdPoseCheckParams._fields_]
    assert 'kpd_pose_check' in hip.EXPORTS and 'kpd_pose_check_defaults' in hip.EXPORTS
    mk = open(os.path.join(ROOT, 'keypoint-diffusion_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'pose_check\.o.*: CXXFLAGS \+= -ffp-contract=off', mk)


def test_defaults_of_the_library_are_the_restatement_s():
    p = hip.pose_check_params()
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert hip.CHECK_FAIL == R.FAIL_NAMES and hip.CHECK_REPORT == R.REPORT and hip.CHECK_COUNTS == R.COUNTS


@pytest.mark.parametrize('bad', [dict(h=0.01), dict(h=5.0), dict(bond_lo=-1.0), dict(pocket_scale=9.0), dict(bond_lo=1.5, bond_hi=1.0),
                                 dict(overlap_max=float('nan')), dict(no_such_threshold=1.0)])
def test_bad_thresholds_are_refused(bad):
    with pytest.raises(hip.KpdError):
        hip.pose_check_params(**bad)


def test_host_tensors_are_refused():
    ptr, mol, san, pos, pocket = PC.arrays([PC.benzene()])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32)
    mol_t = dict(elem=t(mol['elem']), frag=t(mol['frag']), bonds=t(mol['bonds']), bond_ptr=t(mol['bond_ptr']), status=t(mol['status']))
    san_t = {k: t(v) for k, v in san.items()}
    with pytest.raises(hip.KpdError):
        hip.pose_check(t(ptr), PC.Z_H, mol_t, san_t, torch.from_numpy(pos), torch.from_numpy(PC.lig_radius()))


def test_radius_table():
    assert molecule.vdw_radius_table(['C', 'H']) == [molecule.VDW_RADII['C'], 0.0]
    assert molecule.vdw_radius_table(['C', 'H'], with_h=True) == [molecule.VDW_RADII['C'], molecule.VDW_RADII['H']]
    assert molecule.vdw_radius_table(['C', 'Xx'], radii={'Xx': 2.0, 'C': 1.5}) == [1.5, 2.0]
    with pytest.raises(hip.KpdError):
        molecule.vdw_radius_table(['C', 'Xx'])
    with pytest.raises(hip.KpdError):
        molecule.vdw_radius_table(['C'], radii={'C': 9.0})
    for name in ('pose_check',):
        assert all(hasattr(cls, name) for cls in (molecule.Sanitized, molecule.Relaxed, molecule.VinaMinimized, molecule.VinaDocked))
    assert callable(molecule.check_samples)
