#!/usr/bin/env python
"""Generate tests/golden/allowed_bonds.json, the fixture of tests/test_molecule_config.py.  It holds settings only: upstream's
`allowed_bonds` table (constants.py; the table `check_atom_valency`, analysis/metrics.py:156-190, reads) and the `lig_elements`
list of every configuration file upstream ships (configs/dev_config.yml and trained_models/*/config.yml).

Run in the build container only (it imports the reference file, which never travels to the GPU box):
    python tests/golden/make_molecule_golden.py"""
import glob
import importlib.util
import json
import os

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'


def _upstream_constants():
    spec = importlib.util.spec_from_file_location('ref_constants', os.path.join(REF, 'constants.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    allowed = _upstream_constants().allowed_bonds
    files = sorted(glob.glob(os.path.join(REF, 'configs', '*.yml')) + glob.glob(os.path.join(REF, 'trained_models', '*', 'config.yml')))
    elements = {}
    for f in files:
        with open(f) as fh:
            cfg = yaml.safe_load(fh)
        elements[os.path.relpath(f, REF)] = list(cfg['dataset']['lig_elements'])
    out = {'allowed_bonds': allowed, 'lig_elements': elements}
    with open(os.path.join(HERE, 'allowed_bonds.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f'{len(allowed)} elements, {len(elements)} configuration files')


if __name__ == '__main__':
    main()
