"""kpd_pdb_parse on the GPU against its Python restatement (tests/structure_ref.py): every integer and every bit of every output,
file by file and batched, on the hand-written records, on the edges of the line scan, with capacities one too small and on
hostile bytes.  Every call goes through guarded buffers."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, structure

from . import structure_cases as SC
from . import structure_ref as R
from .util import GUARD, guarded, intact

pytestmark = pytest.mark.gpu
T = hip.STRUCT_TILE
SCAN_T = 1024           # SCAN_THREADS of csrc/scan_core.h (tests/test_pocket_gpu.py holds the two together)
FILL = -7
WIDTH = dict(pos=3, occ_b=2)
TORCH_DT = {np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64}


def raw_parse(dev, data: bytes, ptr, cap_lines=None, cap_atoms=None, shift=0):
    """One call of kpd_pdb_parse with every output and the scratch between guard bands.  `shift`: the text starts that many bytes
    into its allocation.  Returns the outputs as numpy arrays over the whole capacity, and the host lists."""
    B = len(ptr) - 1
    cap_lines = data.count(b'\n') + B + 1 if cap_lines is None else cap_lines           # a line ends with '\n' or with its file
    cap_atoms = data.count(b'ATOM  ') + data.count(b'HETATM') if cap_atoms is None else cap_atoms
    whole = torch.frombuffer(bytearray(b'\n' * shift + data + b'\n' * 16), dtype=torch.uint8).to(dev)       # '\n' around the text: a read past it would show
    text = whole[shift:shift + len(data)]
    fp = torch.tensor(ptr, dtype=torch.int64, device=dev)
    sym = hip._packed_symbols(SC.REC_EL, dev, longest=2)
    rn = hip._packed_symbols(SC.RESNAMES, dev, longest=3)
    bufs, ptrs = {}, []
    for name, dt in R.FIELDS:
        buf, p = guarded(cap_atoms * WIDTH.get(name, 1), TORCH_DT[dt], dev, FILL)
        bufs[name] = buf
        ptrs.append(p)
    meta, p_meta = guarded(3 * B + 2, torch.int32, dev, FILL)
    L = hip.lib()
    nb = int(L.kpd_pdb_scratch_bytes(len(data), B, cap_lines))
    scratch, p_scr = guarded(nb, torch.uint8, dev, 0x5a)
    hip.check(L.kpd_pdb_parse(text.data_ptr(), len(data), fp.data_ptr(), B, sym.data_ptr(), len(SC.REC_EL), rn.data_ptr(), len(SC.RESNAMES),
                              cap_lines, cap_atoms, *ptrs, p_meta, p_meta + 4 * (B + 1), p_meta + 4 * (2 * B + 1), p_meta + 4 * (3 * B + 1),
                              p_scr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert intact(meta, 3 * B + 2, FILL) and intact(scratch, nb, 0x5a)
    out = {}
    for name, dt in R.FIELDS:
        w = WIDTH.get(name, 1)
        assert intact(bufs[name], cap_atoms * w, FILL), name
        a = bufs[name][GUARD:GUARD + cap_atoms * w].cpu().numpy()
        out[name] = a.reshape(cap_atoms, w) if w > 1 else a
    host = meta[GUARD:GUARD + 3 * B + 2].cpu().tolist()
    out.update(atom_ptr=host[:B + 1], n_res=host[B + 1:2 * B + 1], status=host[2 * B + 1:3 * B + 1], n_lines=host[-1], cap_atoms=cap_atoms)
    return out


def same_bits(got, want, name):
    if got.dtype == np.float32:
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        assert np.array_equal(got.view(np.int32)[ok], want.view(np.int32)[ok]), name
    else:
        assert np.array_equal(got, want), (name, got[:8], want[:8])


def check_against(got, ref):
    """Everything the call returned equals the restatement; rows beyond the atoms are untouched."""
    assert got['atom_ptr'] == ref['atom_ptr'] and got['n_res'] == ref['n_res'] and got['n_lines'] == ref['n_lines']
    cap = got['cap_atoms']
    fits = [b1 <= cap for b1 in ref['atom_ptr'][1:]]
    want_status = [s | (R.CAPACITY if not f and b1 > b0 else 0) for s, f, b0, b1 in zip(ref['status'], fits, ref['atom_ptr'], ref['atom_ptr'][1:])]
    assert got['status'] == want_status
    written = np.zeros(cap, dtype=bool)
    for f, b0, b1 in zip(fits, ref['atom_ptr'], ref['atom_ptr'][1:]):
        if f:
            written[b0:b1] = True
    for name, _ in R.FIELDS:
        same_bits(got[name][written], ref[name][np.nonzero(written)[0]], name)
        rest = got[name][~written]
        assert (rest == FILL).all(), name            # nothing is written for what does not fit
    return got


def run(dev, files, **kw):
    data, ptr = SC.concat(files)
    return check_against(raw_parse(dev, data, ptr, **kw), R.parse_pdb(data, ptr, SC.REC_EL, SC.RESNAMES))


def arrays_file(n_res, seed):
    g = np.random.default_rng(seed)
    per = g.integers(4, 10, n_res)
    res = np.repeat(np.arange(n_res), per)
    n = len(res)
    return SC.pdb_from_arrays(g.uniform(-150, 150, (n, 3)), g.integers(0, 11, n), res), n


@pytest.fixture(scope='module')
def hand_files():
    return [SC.hand_main(), SC.two_models(), SC.crlf_no_final_newline(), SC.split_residue(), b'', b'\n\n\n\n\n', arrays_file(40, 1)[0],
            b'ATOM', b'ATOM  ', b'HETATM\n']


def test_hand_cases_file_by_file_and_as_one_batch(cuda, hand_files):
    for f in hand_files:
        run(cuda, [f])
    got = run(cuda, hand_files)
    assert got['status'][0] == R.BAD_RECORD and got['status'][1] == R.MODELS and got['status'][4] == R.EMPTY == got['status'][5]
    assert got['status'][8] == R.BAD_RECORD and got['atom_ptr'][9] - got['atom_ptr'][8] == 1         # 'ATOM  ' alone is a (bad) record


def test_text_written_from_coordinates_reads_back_rounded(cuda):
    g = torch.Generator().manual_seed(5)
    pos = (torch.randn(300, 3, generator=g) * 40).float()
    data = SC.pdb_from_arrays(pos.numpy(), np.zeros(300, dtype=int), np.arange(300) // 7)
    got = run(cuda, [data])
    want = np.array([[np.float32(float('%8.3f' % v)) for v in p] for p in pos.tolist()], dtype=np.float32)
    assert got['pos'][:300].tobytes() == want.tobytes()


def test_bitwise_batch_invariance(cuda, hand_files):
    files = hand_files + [arrays_file(25, 2)[0]]
    alone = [raw_parse(cuda, f, [0, len(f)]) for f in files]
    for order in (list(range(len(files))), [3, 0, 10, 6, 1, 9, 2, 8, 4, 7, 5]):
        data, ptr = SC.concat([files[i] for i in order])
        for _ in range(2):                                   # and a second run
            got = raw_parse(cuda, data, ptr)
            for k, i in enumerate(order):
                a0, a1 = got['atom_ptr'][k], got['atom_ptr'][k + 1]
                n = alone[i]['atom_ptr'][1]
                assert a1 - a0 == n and got['n_res'][k] == alone[i]['n_res'][0] and got['status'][k] == alone[i]['status'][0]
                for name, _ in R.FIELDS:
                    w = alone[i][name][:n] + ptr[k] if name == 'line_off' else alone[i][name][:n]         # -0.0 + 0 would lose its sign
                    same_bits(got[name][a0:a1], w, name)


def test_no_files_and_no_bytes(cuda):
    got = run(cuda, [])
    assert got['atom_ptr'] == [0] and got['status'] == [] and got['n_lines'] == 0
    got = run(cuda, [b'', b''])
    assert got['atom_ptr'] == [0, 0, 0] and got['status'] == [R.EMPTY, R.EMPTY]
    out = hip.pdb_parse(torch.zeros(0, dtype=torch.uint8, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda), SC.REC_EL)
    assert out['atom_ptr'] == [0] and out['pos'].shape == (0, 3)


@pytest.mark.parametrize('n', [T - 1, T, T + 1])
def test_file_boundaries_and_line_ends_on_the_tile_edges(cuda, n):
    # a file boundary at n, with and without a '\n' in front of it; an empty file on the boundary; a line end at n - 1, n, n + 1
    a = SC.file_of_length(n, seed=n)
    run(cuda, [a, SC.split_residue()])
    run(cuda, [a, b'', SC.split_residue(), b'', b''])
    run(cuda, [a[:-1] + b'\n', SC.split_residue()])
    run(cuda, [SC.simple_file(n // 80, 3) + b'X' * (n % 80 - 1) + b'\n' + SC.split_residue()])
    run(cuda, [b'\n' * n, SC.crlf_no_final_newline()])
    for shift in (1, 3, 7):                                 # an unaligned text base moves the tiles, not the answer
        run(cuda, [a, b'', SC.hand_main()], shift=shift)


def test_a_line_longer_than_a_tile(cuda):
    long_line = SC.rec('ATOM', '1', ' C', ' ', 'GLY', 'A', '1', ' ', '1.000', '2.000', '3.000', el='C') + 'x' * (2 * T + 100)
    got = run(cuda, [SC.split_residue() + long_line.encode() + b'\n' + SC.split_residue(), b'REMARK ' + b'y' * (T + 5)])
    assert got['atom_ptr'] == [0, 9, 9]


@pytest.fixture(scope='module')
def many_small_files():
    files = []
    for i in range(2 * SCAN_T + 1):
        files.append(b'' if i % 97 == 40 else b'REMARK\n' if i % 101 == 5 else SC.simple_file(1 + i % 3, seed=i, line_len=60 + i % 25))
    return files, [R.parse_pdb(f, [0, len(f)], SC.REC_EL, SC.RESNAMES) for f in files]


@pytest.mark.parametrize('B', [SCAN_T - 1, SCAN_T, SCAN_T + 1, 2 * SCAN_T + 1])
def test_file_counts_across_the_chunks_of_the_scan(cuda, many_small_files, B):
    files, refs = many_small_files
    data, ptr = SC.concat(files[:B])
    got = raw_parse(cuda, data, ptr)
    assert got['atom_ptr'] == [0] + list(np.cumsum([r['atom_ptr'][1] for r in refs[:B]]))
    assert got['status'] == [r['status'][0] for r in refs[:B]] and got['n_res'] == [r['n_res'][0] for r in refs[:B]]
    n = got['atom_ptr'][-1]
    same_bits(got['pos'][:n], np.concatenate([r['pos'] for r in refs[:B]]), 'pos')
    assert np.array_equal(got['line_off'][:n], np.concatenate([r['line_off'] + ptr[k] for k, r in enumerate(refs[:B])]))


@pytest.mark.parametrize('tiles', [SCAN_T - 1, SCAN_T, SCAN_T + 1])
def test_tile_counts_across_the_chunks_of_the_scan(cuda, tiles):
    data = SC.simple_file(tiles * T // 512, seed=9, line_len=512)[:tiles * T - 40]
    got = run(cuda, [data[:len(data) // 2], data[len(data) // 2:]])
    assert got['n_lines'] == tiles * T // 512 + 1


def test_capacities_one_too_small(cuda):
    files = [SC.split_residue(), SC.crlf_no_final_newline(), arrays_file(6, 4)[0]]
    full = run(cuda, files)
    need_atoms, need_lines = full['atom_ptr'][-1], full['n_lines']
    got = run(cuda, files, cap_atoms=need_atoms - 1)                        # the last file does not fit; the others are unaffected
    assert got['status'][2] & R.CAPACITY and not got['status'][0] & R.CAPACITY and got['atom_ptr'][-1] == need_atoms
    got = run(cuda, files, cap_atoms=5)                                     # the second does not fit either
    assert [bool(s & R.CAPACITY) for s in got['status']] == [False, True, True]
    run(cuda, files, cap_atoms=0)
    data, ptr = SC.concat(files)
    low = raw_parse(cuda, data, ptr, cap_lines=need_lines - 1)              # the line table: no file is parsed, the size is reported
    assert low['n_lines'] == need_lines and low['status'] == [R.LINES] * 3 and low['atom_ptr'] == [0, 0, 0, 0] and low['n_res'] == [0, 0, 0]
    assert all((low[name] == FILL).all() for name, _ in R.FIELDS)
    run(cuda, files, cap_lines=need_lines)


def test_malformed_segments(cuda):
    a = SC.split_residue()
    for ptr in ([0, len(a) + 1], [5, 3], [-1, 10]):
        got = raw_parse(cuda, a, ptr, cap_lines=64, cap_atoms=16)
        assert got['status'] == [R.BAD_SEGMENT] and got['atom_ptr'] == [0, 0] and all((got[name] == FILL).all() for name, _ in R.FIELDS)


def test_hostile_bytes(cuda):
    """Bounds, not faults: any bytes end in statuses, inside the capacities, and the restatement reads them the same way."""
    h = SC.hostile_bytes(65536, seed=11)
    run(cuda, [h])
    run(cuda, [h[:30000], h[30000:30001], h[30001:]], shift=5)
    run(cuda, [h], cap_atoms=3)
    valid = SC.hand_main() + arrays_file(12, 8)[0]
    run(cuda, SC.truncations(valid, 200, seed=12))


def test_wrapper_sizes_itself_and_receptors(cuda, hand_files):
    rec = structure.read_pdb(hand_files[:4] + [arrays_file(30, 6)[0]], SC.REC_EL, resnames=SC.RESNAMES, device=cuda)
    data, ptr = SC.concat(hand_files[:4] + [arrays_file(30, 6)[0]])
    ref = R.parse_pdb(data, ptr, SC.REC_EL, SC.RESNAMES)
    assert rec.segments == ref['atom_ptr'] and rec.n_res == ref['n_res'] and rec.status == ref['status']
    for name, _ in R.FIELDS:
        same_bits(getattr(rec, name).cpu().numpy(), ref[name], name)
    flags = torch.from_numpy(ref['flags'])
    keep = rec.mask().cpu()
    assert torch.equal(keep, (flags & (R.BAD | R.HYDROGEN | R.WATER | R.ALTLOC)) == 0)
    assert torch.equal(rec.mask(remove_hydrogen=False, remove_water=False, altloc=False, hetatm=False).cpu(), (flags & (R.BAD | R.HETATM)) == 0)
    feat, other = rec.features()
    assert feat.shape == (len(flags), len(SC.REC_EL)) and torch.equal(other.cpu(), torch.from_numpy(ref['elem']) == len(SC.REC_EL))
    assert torch.equal(feat.sum(1).cpu() == 0, other.cpu())
    lines = rec.lines(keep)
    want = [l for l, w in SC.HAND_MAIN if w is not None]
    kept0 = keep[:ref['atom_ptr'][1]].tolist()
    assert lines[0] == ''.join(l + '\n' for l, k in zip(want, kept0) if k).encode('latin-1')
    assert lines[2] == SC.crlf_no_final_newline().replace(b'REMARK\r\n', b'').replace(b'\r', b'') + b'\n'
    # a tiny capacity estimate: the wrapper repeats itself once with the sizes the first call reports
    short = b'ATOM  \n' * 500
    out = hip.pdb_parse(torch.frombuffer(bytearray(short), dtype=torch.uint8).to(cuda), torch.tensor([0, len(short)], device=cuda), SC.REC_EL)
    assert out['atom_ptr'] == [0, 500] and out['n_lines'] == 500 and out['flags'].shape[0] == 500 and out['status'] == [R.BAD_RECORD]


# ==== kpd_sdf_parse ===================================================================================================================
from keypoint_diffusion_amd import molecule  # noqa: E402

from .molecule_cases import ALLOWED, ELEMENTS, TEXTBOOK, TWO_ETHANOLS_CL, Z, one_hot  # noqa: E402

ATOM_FIELDS = (('pos', torch.float32, 3), ('sym', torch.int32, 1), ('elem', torch.int32, 1), ('valence', torch.int32, 1), ('frag', torch.int32, 1))


def raw_sdf(dev, data, ptr, remove_h=True, cap_lines=None, cap_mols=None, cap_atoms=None, cap_bonds=None, shift=0):
    """One call of kpd_sdf_parse with every output and the scratch between guard bands; numpy arrays over the whole capacities."""
    B = len(ptr) - 1
    cap_lines = data.count(b'\n') + B + 1 if cap_lines is None else cap_lines
    cap_mols = data.count(b'$$$$') + B if cap_mols is None else cap_mols
    cap_atoms = data.count(b'\n') if cap_atoms is None else cap_atoms
    cap_bonds = data.count(b'\n') if cap_bonds is None else cap_bonds
    whole = torch.frombuffer(bytearray(b'\n' * shift + data + b'\n' * 16), dtype=torch.uint8).to(dev)
    text = whole[shift:shift + len(data)]
    fp = torch.tensor(ptr, dtype=torch.int64, device=dev)
    sym = hip._packed_symbols(ELEMENTS, dev, longest=3)
    zt, at = torch.tensor(Z, dtype=torch.int32, device=dev), torch.tensor(ALLOWED, dtype=torch.int32, device=dev)
    spec = [('mol_ptr', torch.int32, B + 1), ('file_status', torch.int32, B), ('lig_ptr', torch.int32, cap_mols + 1)]
    spec += [(n, dt, cap_atoms * w) for n, dt, w in ATOM_FIELDS]
    spec += [('bonds', torch.int32, cap_bonds * 2), ('order', torch.int32, cap_bonds), ('bond_ptr', torch.int32, cap_mols + 1),
             ('summary', torch.int32, cap_mols * 4), ('title_off', torch.int64, cap_mols * 2), ('status', torch.int32, cap_mols),
             ('n_lines', torch.int32, 1)]
    bufs, ptrs = {}, []
    for name, dt, n in spec:
        bufs[name], p = guarded(n, dt, dev, FILL)
        ptrs.append(p)
    L = hip.lib()
    nb = int(L.kpd_sdf_parse_scratch_bytes(len(data), B, cap_lines, cap_mols))
    scratch, p_scr = guarded(nb, torch.uint8, dev, 0x5a)
    hip.check(L.kpd_sdf_parse(text.data_ptr(), len(data), fp.data_ptr(), B, sym.data_ptr(), len(ELEMENTS), zt.data_ptr(), at.data_ptr(),
                              1 if remove_h else 0, cap_lines, cap_mols, cap_atoms, cap_bonds, *ptrs, p_scr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert intact(scratch, nb, 0x5a)
    out = dict(cap_mols=cap_mols, cap_atoms=cap_atoms, cap_bonds=cap_bonds)
    for name, dt, n in spec:
        assert intact(bufs[name], n, FILL), name
        out[name] = bufs[name][GUARD:GUARD + n].cpu().numpy()
    for name, w in (('pos', 3), ('bonds', 2), ('summary', 4), ('title_off', 2)):
        out[name] = out[name].reshape(-1, w)
    return out


def check_sdf(got, ref):
    """What the call returned equals the restatement under the call's capacities; what does not fit is reported, not written."""
    cm, ca, cb = got['cap_mols'], got['cap_atoms'], got['cap_bonds']
    B, M = len(ref['mol_ptr']) - 1, ref['mol_ptr'][-1]
    assert got['mol_ptr'].tolist() == ref['mol_ptr'] and got['n_lines'][0] == ref['n_lines']
    file_fits = [ref['mol_ptr'][b + 1] <= cm for b in range(B)]
    assert got['file_status'].tolist() == [s | (0 if f or ref['mol_ptr'][b + 1] == ref['mol_ptr'][b] else R.CAPACITY)
                                           for b, (s, f) in enumerate(zip(ref['file_status'], file_fits))]
    parsed = [False] * cm
    for b in range(B):
        if file_fits[b]:
            for m in range(ref['mol_ptr'][b], ref['mol_ptr'][b + 1]):
                parsed[m] = True
    size = [ref['lig_ptr'][m + 1] - ref['lig_ptr'][m] if parsed[m] else 0 for m in range(cm)]
    nbond = [ref['bond_ptr'][m + 1] - ref['bond_ptr'][m] if parsed[m] else 0 for m in range(cm)]
    lig_ptr, bond_ptr = [0] + list(np.cumsum(size)), [0] + list(np.cumsum(nbond))
    assert got['lig_ptr'].tolist() == lig_ptr and got['bond_ptr'].tolist() == bond_ptr
    wa, wb = np.zeros(ca, dtype=bool), np.zeros(cb, dtype=bool)
    for m in range(cm):
        fits = lig_ptr[m + 1] <= ca and bond_ptr[m + 1] <= cb
        st = ref['status'][m] if parsed[m] else 0
        assert got['status'][m] == st | (R.MOL_CAPACITY if size[m] and not fits else 0), m
        assert got['summary'][m].tolist() == (ref['summary'][m].tolist() if parsed[m] and fits else [0, 0, 0, 0]), m
        assert got['title_off'][m].tolist() == (ref['title_off'][m].tolist() if parsed[m] else [0, 0]), m
        if not (parsed[m] and fits and size[m]):
            continue
        a0, a1, r0, r1 = lig_ptr[m], lig_ptr[m + 1], ref['lig_ptr'][m], ref['lig_ptr'][m + 1]
        wa[a0:a1] = True
        for name, _, _ in ATOM_FIELDS:
            same_bits(got[name][a0:a1], ref[name][r0:r1], name)
        p0, p1, q0, q1 = bond_ptr[m], bond_ptr[m + 1], ref['bond_ptr'][m], ref['bond_ptr'][m + 1]
        wb[p0:p1] = True
        assert np.array_equal(got['bonds'][p0:p1], ref['bonds'][q0:q1] - r0 + a0) and np.array_equal(got['order'][p0:p1], ref['order'][q0:q1])
    for name, _, _ in ATOM_FIELDS:
        assert (got[name][~wa] == FILL).all(), name
    assert (got['bonds'][~wb] == FILL).all() and (got['order'][~wb] == FILL).all()
    return got


def run_sdf(dev, files, remove_h=True, **kw):
    data, ptr = SC.concat(files)
    return check_sdf(raw_sdf(dev, data, ptr, remove_h=remove_h, **kw), R.parse_sdf(data, ptr, ELEMENTS, Z, ALLOWED, remove_h=remove_h))


@pytest.fixture(scope='module')
def sdf_files():
    return [f for _, (f, _) in sorted(SC.HAND_SDF.items())] + [SC.big_molecule(256, 1), SC.big_molecule(257, 2), SC.big_molecule(20, 3, degree7=True),
                                                               SC.big_molecule(70, 4)]


def test_sdf_hand_cases_file_by_file_and_as_one_batch(cuda, sdf_files):
    for f in sdf_files:
        run_sdf(cuda, [f])
        run_sdf(cuda, [f], remove_h=False)
    run_sdf(cuda, sdf_files)
    run_sdf(cuda, sdf_files, remove_h=False, shift=3)


@pytest.fixture(scope='module')
def textbook(cuda):
    cases = [(sym, pos) for _, sym, pos, _ in TEXTBOOK] + [TWO_ETHANOLS_CL[:2]]
    return molecule.build_molecules([torch.from_numpy(p).to(cuda) for _, p in cases], [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in cases], ELEMENTS)


def test_round_trip_through_sdf_text(cuda, textbook):
    blocks = textbook.sdf()
    back = structure.read_sdf(blocks, ELEMENTS, device=cuda)
    nb = int(textbook.bond_ptr[-1])
    assert torch.equal(back.lig_ptr, textbook.lig_ptr) and torch.equal(back.bond_ptr, textbook.bond_ptr)
    for k in ('elem', 'valence', 'frag', 'summary'):
        assert torch.equal(getattr(back, k), getattr(textbook, k)), k
    assert torch.equal(back.bonds[:nb], textbook.bonds[:nb]) and torch.equal(back.order[:nb], textbook.order[:nb])
    assert back.status.tolist() == textbook.status.tolist() and back.mol_ptr == list(range(len(blocks) + 1)) and back.titles == [''] * len(blocks)
    want = np.array([[np.float32(float('%10.4f' % v)) for v in p] for p in textbook.pos.cpu().tolist()], dtype=np.float32)
    assert back.pos.cpu().numpy().tobytes() == want.tobytes()
    assert back.sdf() == blocks                              # re-emitting the parsed molecules gives the same bytes
    one = molecule.Molecules.from_sdf([''.join(blocks)], ELEMENTS, device=cuda)      # all records in one file
    assert one.mol_ptr == [0, len(blocks)] and torch.equal(one.bonds[:nb], textbook.bonds[:nb]) and one.sdf() == blocks
    # the molecules of a file go wherever perceived ones go
    assert torch.equal(back.keys(), textbook.keys())
    rmsd = back.pose_rmsd(back.pos)
    assert float(rmsd.rmsd.max()) == 0.0
    keys = molecule.training_keys_from_sdf(blocks, ELEMENTS, device=cuda)
    pos, feat = [textbook.pos[a:b] for a, b in zip(textbook.lig_ptr[:-1].tolist(), textbook.lig_ptr[1:].tolist())], None
    feat = [torch.nn.functional.one_hot(textbook.elem[a:b].long(), len(ELEMENTS)).float() for a, b in zip(textbook.lig_ptr[:-1].tolist(), textbook.lig_ptr[1:].tolist())]
    assert torch.equal(keys, molecule.training_keys(pos, feat, ELEMENTS))


def test_sdf_bitwise_batch_invariance(cuda, sdf_files):
    refs = [R.parse_sdf(f, [0, len(f)], ELEMENTS, Z, ALLOWED) for f in sdf_files]
    order = list(range(len(sdf_files)))[::-1][3:] + list(range(len(sdf_files)))[::-1][:3]
    for _ in range(2):
        got = run_sdf(cuda, [sdf_files[i] for i in order])
        assert got['mol_ptr'].tolist() == [0] + list(np.cumsum([refs[i]['mol_ptr'][1] for i in order]))
        assert got['status'][:got['mol_ptr'][-1]].tolist() == [s for i in order for s in refs[i]['status']]


def test_sdf_scan_edges(cuda):
    got = run_sdf(cuda, [])
    assert got['mol_ptr'].tolist() == [0]
    eth = SC.HAND_SDF['shuffled bonds, explicit hydrogens'][0]
    for n in (T - 1, T, T + 1):
        pad = SC.mol_block('x' * 70, [(0.0, 0.0, 0.0, 'C')], [])
        a = (pad * (n // len(pad) + 1))[:n]
        run_sdf(cuda, [a, b'', eth, b''])                   # a file boundary on the tile edge cuts a record
        run_sdf(cuda, [a[:-1] + b'\n', eth], shift=7)
    small = SC.mol_block('s', [(0.0, 0.0, 0.0, 'C'), (1.5, 0.0, 0.0, 'O')], [(2, 1, 1)])
    for count in (SCAN_T - 1, SCAN_T, SCAN_T + 1, 2 * SCAN_T + 1):      # records and files on both sides of the scan's chunk width
        got = raw_sdf(cuda, small * count, [0, len(small) * count])
        assert got['mol_ptr'].tolist() == [0, count] and got['lig_ptr'][:count + 1].tolist() == list(range(0, 2 * count + 1, 2))
        assert (got['lig_ptr'][count:] == 2 * count).all()                      # entries behind the records repeat the total
        assert got['bonds'][:count].tolist() == [[2 * k, 2 * k + 1] for k in range(count)] and (got['status'] == 0).all()
        got = raw_sdf(cuda, small * count, [len(small) * k for k in range(count + 1)])
        assert got['mol_ptr'].tolist() == list(range(count + 1)) and got['bond_ptr'][:count + 1].tolist() == list(range(count + 1))


def test_sdf_capacities_one_too_small(cuda):
    files = [SC.HAND_SDF['two records and a bare block'][0], SC.HAND_SDF['aromatic type 4'][0], SC.HAND_SDF['M  CHG and a charge field'][0]]
    full = run_sdf(cuda, files)
    M, na, nb = full['mol_ptr'][-1], full['lig_ptr'][-1], full['bond_ptr'][-1]
    assert (M, na, nb) == (5, 13, 10)
    run_sdf(cuda, files, cap_mols=M, cap_atoms=na, cap_bonds=nb)
    got = run_sdf(cuda, files, cap_mols=M, cap_atoms=na - 1, cap_bonds=nb)
    assert got['status'][4] & R.MOL_CAPACITY and not got['status'][3] & R.MOL_CAPACITY
    got = run_sdf(cuda, files, cap_mols=M, cap_atoms=na, cap_bonds=nb - 1)
    assert got['status'][4] & R.MOL_CAPACITY and not got['status'][3] & R.MOL_CAPACITY
    got = run_sdf(cuda, files, cap_mols=M - 1, cap_atoms=na, cap_bonds=nb)          # the last file's record does not fit: that file is not parsed
    assert got['file_status'].tolist() == [0, 0, R.CAPACITY] and got['mol_ptr'][-1] == M
    got = run_sdf(cuda, files, cap_mols=2)                                          # the first file (three records) does not fit either
    assert got['file_status'].tolist() == [R.CAPACITY] * 3 and got['lig_ptr'].tolist() == [0, 0, 0]
    run_sdf(cuda, files, cap_mols=0, cap_atoms=0, cap_bonds=0)
    data, ptr = SC.concat(files)
    low = raw_sdf(cuda, data, ptr, cap_lines=full['n_lines'][0] - 1)
    assert low['n_lines'][0] == full['n_lines'][0] and low['file_status'].tolist() == [R.LINES] * 3 and low['mol_ptr'].tolist() == [0, 0, 0, 0]


def test_sdf_hostile_bytes(cuda, sdf_files):
    import random
    g = random.Random(21)
    h = bytearray(SC.hostile_bytes(65536, seed=22))
    for _ in range(300):
        p = g.randrange(len(h) - 64)
        w = g.choice([b'\n$$$$\n', b'\n  3  2  0  0  0  0  0  0  0  0999 V2000\n', b'\nM  END\n', b'\n    0.0000    1.0000    2.0000 C   0  0\n', b'\n  1  2  1  0\n',
                      b'\n999999  0  0  0  0  0  0  0  0999 V2000\n'])
        h[p:p + len(w)] = w
    run_sdf(cuda, [bytes(h)])
    run_sdf(cuda, [bytes(h[:20000]), bytes(h[20000:])], remove_h=False, shift=1, cap_atoms=5, cap_bonds=2)
    valid = b''.join(sdf_files[:6])
    run_sdf(cuda, SC.truncations(valid, 200, seed=23))


def test_files_to_pockets_to_samples(cuda):
    """Text written from arrays goes through load_complexes and gives the dict extract_pockets gives on the arrays rounded to the
    printed precision; the dataset built from it samples; the samples' own SDF text reads back onto them."""
    from keypoint_diffusion_amd import dataset as kdata, pocket as P, synth
    from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
    from . import util
    from .test_pocket_gpu import REC_EL, synthetic_structures
    s = synthetic_structures([60, 80], [9, 12], seed=5)
    rnd = lambda t, fmt: torch.tensor([[float(fmt % v) for v in p] for p in t.tolist()], dtype=torch.float32)
    el = torch.where(s['other'], len(REC_EL), s['rec_feat'].float().argmax(1))
    lig_el = s['lig_feat'].float().argmax(1)
    rec_files, lig_files = [], []
    for b in range(2):
        r0, r1, l0, l1 = s['rec_seg'][b], s['rec_seg'][b + 1], s['lig_seg'][b], s['lig_seg'][b + 1]
        rec_files.append(SC.pdb_from_arrays(s['rec_pos'][r0:r1].numpy(), el[r0:r1].tolist(), s['rec_res'][r0:r1].tolist(), elements=REC_EL))
        lig_files.append(SC.mol_block('lig %d' % b, [(float(x), float(y), float(z), ELEMENTS[e]) for (x, y, z), e in zip(s['lig_pos'][l0:l1].tolist(), lig_el[l0:l1].tolist())],
                                      [(k + 1, k + 2, 1) for k in range(l1 - l0 - 1)]))
    data, skipped = structure.load_complexes(rec_files, lig_files, REC_EL, ELEMENTS, device=cuda)
    d = {k: (v.to(cuda) if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
    want, want_skipped = P.extract_pockets(rnd(s['rec_pos'], '%8.3f').to(cuda), d['rec_feat'], d['rec_res'], d['rec_seg'], rnd(s['lig_pos'], '%10.4f').to(cuda),
                                           d['lig_feat'], d['lig_seg'], other_atoms_mask=d['other'])
    assert skipped == want_skipped == []
    for k, v in want.items():
        assert torch.equal(data[k], v) if isinstance(v, torch.Tensor) else True, k
    assert data['rec_files'] == rec_files and data['rec_pos'].shape[0] > 0
    # one more complex per reason to skip
    two = lig_files[0] + lig_files[1]
    iron = SC.HAND_SDF['unsupported element'][0]
    _, skipped = structure.load_complexes(rec_files + [rec_files[0], rec_files[0], b'REMARK\n'], lig_files + [two, iron, lig_files[0]], REC_EL, ELEMENTS, device=cuda)
    assert [i for i, _ in skipped] == [2, 3, 4] and 'NotImplementedError' in skipped[0][1] and 'Unparsable' in skipped[1][1] and 'receptor' in skipped[2][1]
    cut = dict(util.CUTOFFS_ALL_ATOM, kl=8, ll=5)
    ds = kdata.ProteinLigandDataset('byop', data, REC_EL, ELEMENTS, n_keypoints=8, graph_cutoffs=cut)
    assert len(ds) == 2
    model = KeypointDiffusion(10, 10, None, n_timesteps=4, architecture='egnn', rec_encoder_type='fixed',
                              graph_config=dict(n_keypoints=8, graph_cutoffs=cut), dynamics_config=dict(util.EGNN_C2, n_layers=2),
                              rec_encoder_config={'vector_size': 16}, precision=1e-5)
    synth.fill_state_dict_(model, 13)
    model = model.eval().cuda()
    g1, _ = ds[1]
    pos, feat = model.sample_given_pocket(g1, torch.tensor([9, 11]))
    assert all(torch.isfinite(p).all() for p in pos)
    mols = molecule.build_molecules([p.cuda() for p in pos], [f.cuda() for f in feat], ELEMENTS)
    blocks = mols.sdf()
    back = structure.read_sdf(blocks, ELEMENTS, device=cuda)
    assert back.sdf() == blocks and float(back.pose_rmsd(back.pos).rmsd.max()) == 0.0
    assert torch.equal(molecule.training_keys_from_sdf(blocks, ELEMENTS, device=cuda), molecule.training_keys([p.cuda() for p in pos], [f.cuda() for f in feat], ELEMENTS))
