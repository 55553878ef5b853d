"""ctypes binding of libkpd_hip.so (C ABI in include/kpd.h).

The library is the product: there is no PyTorch / CPU fallback.  If the shared object has
not been built (`python __graft_entry__.py` or `make -C keypoint-diffusion_amd/csrc`) every
entry point raises.
"""
import ctypes as C
import os
from typing import Dict, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# KPD_LIB: another copy of the same library (for example a parent commit's, to compare against);
# bench.py refuses to run with it set and checks kpd_build_flags() == 0
LIB_PATH = os.environ.get('KPD_LIB') or os.path.join(_HERE, 'csrc', 'libkpd_hip.so')
_lib = None

c_int_p = C.POINTER(C.c_int32)
c_float_p = C.POINTER(C.c_float)


class KpdBatch(C.Structure):
    _fields_ = [('B', C.c_int32), ('n_lig', C.c_int32), ('n_kp', C.c_int32), ('max_lig', C.c_int32),
                ('max_kp', C.c_int32), ('lig_ptr', C.c_void_p), ('kp_ptr', C.c_void_p), ('lig_x', C.c_void_p),
                ('lig_h', C.c_void_p), ('kp_x', C.c_void_p), ('kp_h', C.c_void_p), ('kp_v', C.c_void_p),
                ('n_kk', C.c_int32), ('kk_src', C.c_void_p), ('kk_dst', C.c_void_p), ('kk_rowptr', C.c_void_p)]


class KpdLigGraph(C.Structure):
    _fields_ = [('cap_ll', C.c_int32), ('cap_kl', C.c_int32),
                ('ll_src', C.c_void_p), ('ll_dst', C.c_void_p), ('ll_rowptr', C.c_void_p),
                ('kl_src', C.c_void_p), ('kl_dst', C.c_void_p), ('kl_rowptr', C.c_void_p),
                ('lk_src', C.c_void_p), ('lk_dst', C.c_void_p), ('lk_rowptr', C.c_void_p),
                ('ll_per_graph', C.c_void_p), ('counts', C.c_void_p)]


class KpdEgnnConfig(C.Structure):
    _fields_ = [('atom_nf', C.c_int32), ('rec_nf', C.c_int32), ('n_layers', C.c_int32), ('hidden_nf', C.c_int32),
                ('use_tanh', C.c_int32), ('norm', C.c_int32), ('update_kp_feat', C.c_int32),
                ('message_norm', C.c_float), ('ll_k', C.c_int32), ('kl_k', C.c_int32),
                ('ll_cutoff', C.c_float), ('kl_cutoff', C.c_float), ('coords_range', C.c_float)]


class KpdGvpConfig(C.Structure):
    _fields_ = [('n_lig_scalars', C.c_int32), ('n_kp_scalars', C.c_int32), ('vector_size', C.c_int32),
                ('n_convs', C.c_int32), ('n_hidden_scalars', C.c_int32), ('update_kp', C.c_int32),
                ('message_norm_mode', C.c_int32), ('message_norm', C.c_float), ('ll_k', C.c_int32), ('kl_k', C.c_int32),
                ('ll_cutoff', C.c_float), ('kl_cutoff', C.c_float), ('n_message_gvps', C.c_int32),
                ('n_update_gvps', C.c_int32), ('n_noise_gvps', C.c_int32)]


class KpdRecencConfig(C.Structure):
    _fields_ = [('in_scalar_size', C.c_int32), ('out_scalar_size', C.c_int32), ('vector_size', C.c_int32),
                ('n_rr_convs', C.c_int32), ('n_rk_convs', C.c_int32), ('n_message_gvps', C.c_int32),
                ('n_update_gvps', C.c_int32), ('message_norm_mode', C.c_int32), ('message_norm', C.c_float),
                ('k_closest', C.c_int32), ('n_keypoints', C.c_int32), ('rr_cutoff', C.c_float), ('rk_cutoff', C.c_float),
                ('kk_cutoff', C.c_float), ('kp_rad', C.c_float)]


class KpdRecegnnConfig(C.Structure):
    _fields_ = [('n_convs', C.c_int32), ('n_keypoints', C.c_int32), ('in_n_node_feat', C.c_int32),
                ('hidden_n_node_feat', C.c_int32), ('out_n_node_feat', C.c_int32), ('use_sameres_feat', C.c_int32),
                ('use_tanh', C.c_int32), ('norm', C.c_int32), ('fix_pos', C.c_int32), ('coords_range', C.c_float),
                ('message_norm', C.c_float), ('k_closest', C.c_int32), ('kk_cutoff', C.c_float), ('kp_rad', C.c_float)]


class KpdWgradItem(C.Structure):
    _fields_ = [('A', C.c_void_p), ('B', C.c_void_p), ('lda', C.c_int32), ('ldb', C.c_int32), ('K', C.c_int32), ('C', C.c_void_p), ('ldc', C.c_int32),
                ('B2', C.c_void_p), ('ldb2', C.c_int32), ('nb2', C.c_int32), ('Cx1', C.c_void_p), ('ldx1', C.c_int32), ('colsum', C.c_void_p),
                ('A2', C.c_void_p), ('lda2', C.c_int32), ('na2', C.c_int32), ('Cx2', C.c_void_p), ('ldx2', C.c_int32), ('colsum2', C.c_void_p),
                ('B3', C.c_void_p), ('ldb3', C.c_int32), ('nb3', C.c_int32), ('Cx3', C.c_void_p), ('ldx3', C.c_int32)]


class KpdRecBatch(C.Structure):
    _fields_ = [('B', C.c_int32), ('n_rec', C.c_int32), ('max_rec', C.c_int32), ('rec_ptr', C.c_void_p),
                ('rec_x', C.c_void_p), ('rec_h', C.c_void_p), ('n_rr', C.c_int32), ('rr_src', C.c_void_p),
                ('rr_dst', C.c_void_p), ('rr_rowptr', C.c_void_p)]


class KpdRecOut(C.Structure):
    _fields_ = [('kp_x', C.c_void_p), ('kp_h', C.c_void_p), ('kp_v', C.c_void_p), ('rk_src', C.c_void_p),
                ('rk_dst', C.c_void_p), ('cap_kk', C.c_int32), ('kk_src', C.c_void_p), ('kk_dst', C.c_void_p),
                ('kk_per_graph', C.c_void_p), ('counts', C.c_void_p)]


class KpdRelaxParams(C.Structure):
    _fields_ = [('k_b', C.c_double), ('k_a', C.c_double), ('r_c', C.c_double), ('s', C.c_double), ('w_intra', C.c_double),
                ('gtol', C.c_double), ('max_step', C.c_double), ('max_iters', C.c_int32)]


class KpdVinaParams(C.Structure):
    _fields_ = [(name, C.c_double) for name in ('w_gauss1', 'w_gauss2', 'w_repulsion', 'w_hydrophobic', 'w_hbond', 'w_rot', 'r_c')]


class KpdPoseCheckParams(C.Structure):
    _fields_ = [(name, C.c_double) for name in ('bond_lo', 'bond_hi', 'angle_lo', 'angle_hi', 'clash_min', 'ring_max', 'centre_max',
                                                 'twist_min', 'pocket_min', 'pocket_scale', 'overlap_max', 'h')]


class KpdVinaMinParams(C.Structure):
    _fields_ = ([(name, C.c_double) for name in ('w_gauss1', 'w_gauss2', 'w_repulsion', 'w_hydrophobic', 'w_hbond', 'w_rot', 'r_c', 'w_intra',
                                                  'gtol', 'max_step')] + [('max_iters', C.c_int32)])


class KpdVinaDockParams(C.Structure):
    _fields_ = (KpdVinaMinParams._fields_ + [(name, C.c_double) for name in ('temperature', 'amplitude', 'min_rmsd')] +
                [('step_iters', C.c_int32)])


class KpdError(RuntimeError):
    pass


# The prototype of every function include/kpd.h declares: name -> (result type, argument types).  This table is the only place a
# prototype is written: `lib()` sets restype / argtypes from it, EXPORTS is its keys, and tests/test_abi.py compares it with the
# header's text parameter by parameter (count, order and kind) and the Structure classes above field by field.
_P, _I32, _I64, _U64, _F32, _F64, _STR, _STATUS, _ref = (C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_char_p,
                                                         C.c_int, C.POINTER)
_LIGANDS_IN_POCKETS = [_P, _P] + [_I32] * 3 + [_P, _I32]      # pos, lig_ptr, N, B, max_atoms, elem, F: the head of relax and the vina calls
PROTOTYPES = {
    'kpd_last_error': (_STR, []),
    'kpd_version': (C.c_int, []),
    'kpd_build_flags': (C.c_int, []),
    'kpd_build_lig_graph': (_STATUS, [_ref(KpdBatch), _F32, _I32, _F32, _I32, _ref(KpdLigGraph), _P]),
    'kpd_egnn_forward': (_STATUS, [_P, _ref(KpdBatch)] + [_P] * 4),
    'kpd_egnn_debug_state': (_STATUS, [_P, _STR, _P, _I64, _P]),
    'kpd_egnn_last_counts': (_STATUS, [_P, _ref(_I32), _P]),
    'kpd_egnn_profile': (_STATUS, [_P, _I32]),
    'kpd_egnn_profile_read': (_STATUS, [_P, _ref(_F64), _ref(_I32)]),
    'kpd_sample_update': (_STATUS, [_I32, _P, _P, _I32] + [_P] * 8 + [_I32, _P]),
    'kpd_step_coefficients': (_STATUS, [_P, _I32, _P, _P, _I32, _P, _P]),
    'kpd_complex_noise': (_STATUS, [_I32, _P, _I32, _P, _U64, _I32, _I32, _P, _P]),
    'kpd_inpaint_coefficients': (_STATUS, [_P, _I32, _P, _P, _I32, _P, _P]),
    'kpd_sample_update_inpaint': (_STATUS, [_I32, _P, _P, _I32] + [_P] * 14 + [_I32, _P]),
    'kpd_sample_renoise': (_STATUS, [_I32, _P, _P, _I32] + [_P] * 6 + [_I32, _P]),
    'kpd_guided_coefficients': (_STATUS, [_P, _I32, _P, _P, _I32, _F32, _F32, _P, _P]),
    'kpd_sample_update_guided': (_STATUS, [_I32, _P, _P, _I32] + [_P] * 16 + [_F32, _I32, _P]),
    'kpd_clash_score': (_STATUS, [_I32] + [_P] * 4 + [_F32, _P, _P]),
    'kpd_gvp_forward': (_STATUS, [_P, _ref(KpdBatch)] + [_P] * 4),
    'kpd_gvp_debug_state': (_STATUS, [_P, _STR, _P, _I64, _P]),
    'kpd_gvp_profile': (_STATUS, [_P, _I32]),
    'kpd_gvp_profile_read': (_STATUS, [_P, _ref(_F64), _ref(_I32)]),
    'kpd_gvp_last_counts': (_STATUS, [_P, _ref(_I32), _P]),
    'kpd_recenc_forward': (_STATUS, [_P, _ref(KpdRecBatch), _ref(KpdRecOut), _P]),
    'kpd_recegnn_forward': (_STATUS, [_P, _ref(KpdRecBatch), _P, _ref(KpdRecOut)] + [_P] * 3),
    'kpd_xyz_scratch_bytes': (_I64, [_I32, _I32]),
    'kpd_xyz_emit': (_STATUS, [_P] * 3 + [_I32] * 3 + [_P] * 3 + [_I64] + [_P] * 4),
    'kpd_rec_graph_scratch_bytes': (_I64, [_I32, _I32]),
    'kpd_build_rec_graph': (_STATUS, [_P, _P] + [_I32] * 3 + [_F32, _I32, _P, _I32] + [_P] * 8),
    'kpd_egnn_trainer_forward': (_STATUS, [_P, _ref(KpdBatch)] + [_P] * 4),
    'kpd_egnn_trainer_backward': (_STATUS, [_P] * 8),
    'kpd_egnn_trainer_profile': (_STATUS, [_P, _I32]),
    'kpd_egnn_trainer_profile_read': (_STATUS, [_P, _ref(_F64), _ref(_I32), _ref(_F64)]),
    'kpd_gvp_trainer_last_counts': (_STATUS, [_P, _ref(_I32)]),
    'kpd_gvp_trainer_message_path': (_STATUS, [_P, _ref(_I32)]),
    'kpd_wgrad_batch': (_STATUS, [_I32, _I32, _ref(KpdWgradItem), _P, _I64, _P]),
    'kpd_adam_step': (_STATUS, [_P, _I32, _I64, _I32] + [_F64] * 5 + [_I64, _F64, _P]),
    'kpd_gvp_trainer_forward': (_STATUS, [_P, _ref(KpdBatch)] + [_P] * 4),
    'kpd_gvp_trainer_backward': (_STATUS, [_P] * 9),
    'kpd_gvp_trainer_set_dropout': (_STATUS, [_P, _F32, _U64]),
    'kpd_dropout_mask': (_STATUS, [_U64] + [_I32] * 4 + [_I64, _F32, _P, _P]),
    'kpd_recenc_trainer_set_dropout': (_STATUS, [_P, _F32, _U64]),
    'kpd_recenc_trainer_forward': (_STATUS, [_P, _ref(KpdRecBatch), _ref(KpdRecOut), _P]),
    'kpd_recenc_trainer_backward': (_STATUS, [_P] * 5),
    'kpd_recegnn_trainer_forward': (_STATUS, [_P, _ref(KpdRecBatch), _P, _ref(KpdRecOut)] + [_P] * 3),
    'kpd_recegnn_trainer_backward': (_STATUS, [_P] * 4),
    'kpd_ot_emd_uniform': (_STATUS, [_I32] + [_P] * 5 + [_I32]),
    'kpd_sgemm': (_STATUS, [_I32] * 5 + [_F32, _P, _I32, _P, _I32, _F32, _P, _I32, _P, _P, _I64, _P]),
    'kpd_dist_hinge': (_STATUS, [_P, _P, _I32, _P, _P, _I32, _I32, _F32] + [_P] * 5),
    'kpd_pocket_scratch_bytes': (_I64, [_I32, _I32]),
    'kpd_pocket_select': (_STATUS, [_P] * 5 + [_I32, _I32, _P, _P, _I32, _I32, _F32, _F32, _I32] + [_P] * 8),
    'kpd_interface_points_scratch_bytes': (_I64, [_I32] * 3),
    'kpd_interface_points': (_STATUS, [_P] * 3 + [_I32, _P, _P, _I32, _I32, _F32, _F32, _I32, _I32] + [_P] * 6),
    'kpd_mol_scratch_bytes': (_I64, [_I32, _I32]),
    'kpd_mol_perceive': (_STATUS, [_P] * 3 + [_I32] * 3 + [_P, _P, _I32] + [_P] * 10),
    'kpd_sdf_scratch_bytes': (_I64, [_I32, _I32]),
    'kpd_sdf_emit': (_STATUS, [_P, _P, _I32, _I32, _P, _I32] + [_P] * 5 + [_I32, _P, _I32, _P, _I64] + [_P] * 4),
    'kpd_mol_keys': (_STATUS, [_P, _I32, _I32, _P, _I32] + [_P] * 5 + [_I32, _P] + [_I32] * 4 + [_P] * 5),
    'kpd_fp_diversity': (_STATUS, [_P, _P, _I32, _I32, _P, _I32] + [_P] * 4),
    'kpd_mol_sanitize': (_STATUS, [_P, _P, _I32, _I32, _P, _I32] + [_P] * 3 + [_F64] + [_P] * 4 + [_I32, _P, _I32] + [_P] * 10),
    'kpd_mol_add_hs_scratch_bytes': (_I64, [_I32, _I32]),
    'kpd_mol_add_hs': (_STATUS, [_P, _P, _I32, _I32, _P, _I32] + [_P] * 6 + [_I32] + [_P] * 5 + [_I32] * 4 + [_P] * 15),
    'kpd_smiles_scratch_bytes': (_I64, [_I32, _I32]),
    'kpd_mol_smiles': (_STATUS, [_P, _I32, _I32, _P, _I32] + [_P] * 7 + [_I32] + [_P] * 4 + [_I32, _I32, _P, _I64] + [_P] * 4),
    'kpd_pose_rmsd_scratch_bytes': (_I64, [_I32] * 3),
    'kpd_pose_rmsd': (_STATUS, [_P, _I32, _I32, _P, _I32] + [_P] * 4 + [_I32] + [_P] * 3 + [_I32, _I32, _P, _P, _I32, _I32, _I64] +
                      [_P] * 7),
    'kpd_mol_match': (_STATUS, [_P, _I32, _I32, _P, _I32] + [_P] * 6 + [_I32] + [_P] * 5 + [_I32, _P, _P, _I32, _I32, _I64, _P, _P, _I32] +
                      [_P] * 10),
    'kpd_pose_check_defaults': (None, [_ref(KpdPoseCheckParams)]),
    'kpd_pose_check': (_STATUS, [_P] + [_I32] * 3 + [_P, _I32] + [_P] * 6 + [_I32] + [_P] * 4 + [_I32, _P, _I32] + [_P] * 4 + [_I32] * 3 +
                       [_P, _ref(KpdPoseCheckParams)] + [_P] * 6),
    'kpd_relax_defaults': (None, [_ref(KpdRelaxParams)]),
    'kpd_relax': (_STATUS, _LIGANDS_IN_POCKETS + [_P] * 4 + [_I32] + [_P] * 4 + [_I32] * 3 + [_P, _ref(KpdRelaxParams)] + [_P] * 4),
    'kpd_vina_defaults': (None, [_ref(KpdVinaParams)]),
    'kpd_vina_pocket_types': (_STATUS, [_P] * 3 + [_I32, _I32] + [_P] * 3),
    'kpd_vina_score': (_STATUS, _LIGANDS_IN_POCKETS + [_P] * 5 + [_I32] + [_P] * 6 + [_I32] * 3 + [_P, _ref(KpdVinaParams)] + [_P] * 6),
    'kpd_vina_min_defaults': (None, [_ref(KpdVinaMinParams)]),
    'kpd_vina_minimize': (_STATUS, _LIGANDS_IN_POCKETS + [_P] * 6 + [_I32] + [_P] * 6 + [_I32] * 3 + [_P, _I32, _ref(KpdVinaMinParams)] +
                          [_P] * 4),
    'kpd_vina_dock_defaults': (None, [_ref(KpdVinaDockParams)]),
    'kpd_vina_dock': (_STATUS, _LIGANDS_IN_POCKETS + [_P] * 6 + [_I32] + [_P] * 6 + [_I32] * 3 + [_P, _I32] + [_P] * 3 + [_U64] +
                      [_I32] * 3 + [_ref(KpdVinaDockParams)] + [_P] * 7),
    'kpd_pdb_scratch_bytes': (_I64, [_I64, _I32, _I32]),
    'kpd_pdb_parse': (_STATUS, [_P, _I64, _P, _I32, _P, _I32, _P] + [_I32] * 3 + [_P] * 18),
    'kpd_sdf_parse_scratch_bytes': (_I64, [_I64] + [_I32] * 3),
    'kpd_sdf_parse': (_STATUS, [_P, _I64, _P, _I32, _P, _I32, _P, _P] + [_I32] * 5 + [_P] * 17),
}
# the handle functions every family has: identical up to the config struct and the number of sizes `reserve` takes
for _family, _cfg, _n_sizes in (('egnn', KpdEgnnConfig, 6), ('gvp', KpdGvpConfig, 6), ('recenc', KpdRecencConfig, 4),
                                ('recegnn', KpdRecegnnConfig, 4)):
    for _prefix in (f'kpd_{_family}_', f'kpd_{_family}_trainer_'):
        PROTOTYPES[_prefix + 'create'] = (_STATUS, [_ref(_cfg), _ref(_P)])
        PROTOTYPES[_prefix + 'destroy'] = (None, [_P])
        PROTOTYPES[_prefix + 'reserve'] = (_STATUS, [_P] + [_I32] * _n_sizes)
    PROTOTYPES[f'kpd_{_family}_load_weight'] = (_STATUS, [_P, _STR, _P, _ref(_I64), _I32, _P])
    PROTOTYPES[f'kpd_{_family}_commit'] = (_STATUS, [_P])
    PROTOTYPES[f'kpd_{_family}_trainer_bind'] = (_STATUS, [_P, _STR, _P, _P, _ref(_I64), _I32])
EXPORTS = list(PROTOTYPES)


def lib():
    """Load (once) and return the HIP library; raise loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KpdError(f'{LIB_PATH} not found: the HIP extension must be built first '
                       f'(python -c "import __graft_entry__ as g; g.build()"). There is no CPU fallback.')
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)     # AttributeError if a declared symbol is not exported
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L




def check(status: int):
    if status != 0:
        raise KpdError(f'kpd status {status}: {lib().kpd_last_error().decode()}')


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise KpdError(f'{name} must live on the GPU (got {t.device}); the hot path has no CPU implementation')
    return t.contiguous().float()


def _offsets(t, name: str, count: str = 'B') -> int:
    """`t` must be a contiguous 1-D int32 GPU tensor of `count` + 1 offsets; returns that count."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.numel() >= 1 and t.is_contiguous()):
        raise KpdError(f'{name} must be a contiguous int32 GPU tensor of {count} + 1 offsets')
    return t.numel() - 1


def _per_entry(t, name: str, n: int, what: str, contiguous: bool = False) -> torch.Tensor:
    """`t` must be a 1-D int32 GPU tensor with one entry per `what` (n of them); returns it contiguous.  `contiguous`: a strided
    tensor is refused, not copied (the sites that always refused one)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n and
            (t.is_contiguous() or not contiguous)):
        raise KpdError(f'{name} must be a {"contiguous " if contiguous else ""}1-D int32 GPU tensor with one entry per {what}')
    return t.contiguous()


# How many elements every entry of what `mol_perceive` (MOL_LENGTHS) and `mol_sanitize` (SAN_LENGTHS) return has, for N atoms, B
# ligands and a bond list of cap_bonds rows.  The library cannot see a tensor's length: `_mol_args` is the only guard.
MOL_LENGTHS = dict(elem='N', valence='N', frag='N', bonds='2 * cap_bonds', order='cap_bonds', bond_ptr='B + 1', status='B')
SAN_LENGTHS = dict(order_k='cap_bonds', bond_flags='cap_bonds', valence_k='N', atom_h='N', atom_flags='N', status='B')


def _numel(t) -> int:
    """Elements of a tensor, 0 for anything else (which `_mol_args` then refuses by name)."""
    return t.numel() if isinstance(t, torch.Tensor) else 0


def _mol_args(where: str, mol: dict, fields, B: int, N: int, san: Optional[dict] = None, san_fields=()) -> int:
    """The entries `fields` of `mol` (what `mol_perceive` returned) and `san_fields` of `san` (what `mol_sanitize` returned) must be
    contiguous int32 GPU tensors of the lengths MOL_LENGTHS / SAN_LENGTHS state.  Returns cap_bonds, the rows of mol['bonds']."""
    n_bonds = _numel(mol.get('bonds'))
    if n_bonds % 2:
        raise KpdError(f'{where}: bonds has {n_bonds} elements, an odd number: it must hold two atoms per row')
    size = {'N': N, 'B': B, 'B + 1': B + 1, 'cap_bonds': n_bonds // 2, '2 * cap_bonds': n_bonds}
    for what, src, names, lengths in (('perceived', mol, fields, MOL_LENGTHS), ('sanitised', san, san_fields, SAN_LENGTHS)):
        for name in names:
            t = src.get(name)
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
                raise KpdError(f'{where}: {name} must be a contiguous int32 GPU tensor')
            if t.numel() != size[lengths[name]]:
                raise KpdError(f'{where}: {name} of the {what} molecules has {t.numel()} elements, not {lengths[name]} = '
                               f'{size[lengths[name]]} (N = {N} atoms, B = {B} ligands, cap_bonds = {n_bonds // 2} bond rows)')
    return n_bonds // 2


def _class_table(device, *rows) -> torch.Tensor:
    """The integer per-class tables of a call (atomic numbers, largest valences), one row each, as an int32 device tensor [len(rows), F]."""
    return torch.tensor([list(map(int, row)) for row in rows], dtype=torch.int32, device=device)


class PreparedBatch:
    """Device-side, int32, dst-sorted view of the static part of a batch (built once per batch)."""

    def __init__(self, lig_counts: torch.Tensor, kp_counts: torch.Tensor, kk_src: torch.Tensor, kk_dst: torch.Tensor,
                 device):
        lig_counts = lig_counts.cpu().long()
        kp_counts = kp_counts.cpu().long()
        self.B = int(lig_counts.numel())
        self.n_lig = int(lig_counts.sum())
        self.n_kp = int(kp_counts.sum())
        self.max_lig = int(lig_counts.max())
        self.max_kp = int(kp_counts.max())
        if int(lig_counts.min()) < 1 or int(kp_counts.min()) < 1:
            raise KpdError('every complex needs at least one ligand atom and one keypoint')
        zero = torch.zeros(1, dtype=torch.long)
        self.lig_ptr = torch.cat([zero, lig_counts.cumsum(0)]).int().to(device)
        self.kp_ptr = torch.cat([zero, kp_counts.cumsum(0)]).int().to(device)
        kk_src = kk_src.to(device).long()
        kk_dst = kk_dst.to(device).long()
        if kk_src.numel():
            order = torch.argsort(kk_dst * (self.n_kp + 1) + kk_src)      # (dst, src) lexicographic
            kk_src, kk_dst = kk_src[order], kk_dst[order]
        self.n_kk = int(kk_src.numel())
        self.kk_src = kk_src.int().contiguous()
        self.kk_dst = kk_dst.int().contiguous()
        deg = torch.bincount(kk_dst, minlength=self.n_kp) if self.n_kk else torch.zeros(self.n_kp, dtype=torch.long, device=device)
        self.kk_rowptr = torch.cat([torch.zeros(1, dtype=torch.long, device=device), deg.cumsum(0)]).int().contiguous()

    def struct(self, lig_x, lig_h, kp_x, kp_h, kp_v=None) -> KpdBatch:
        return KpdBatch(self.B, self.n_lig, self.n_kp, self.max_lig, self.max_kp, _ptr(self.lig_ptr), _ptr(self.kp_ptr),
                        _ptr(lig_x), _ptr(lig_h), _ptr(kp_x), _ptr(kp_h), _ptr(kp_v), self.n_kk, _ptr(self.kk_src),
                        _ptr(self.kk_dst), _ptr(self.kk_rowptr))


def build_lig_graph(pb: PreparedBatch, lig_x: torch.Tensor, kp_x: torch.Tensor, ll_cutoff: float, kl_k: int, ll_k: int = 0,
                    kl_cutoff: float = 0.0):
    """Standalone graph build (kpd_build_lig_graph); returns a dict of int32 device tensors.  ll_k > 0: kNN lig-lig graph
    instead of the radius graph; kl_k == 0: radius keypoint->ligand graph of radius kl_cutoff instead of kNN."""
    dev = lig_x.device
    lig_x, kp_x = _dev_f32(lig_x, 'lig_x'), _dev_f32(kp_x, 'kp_x')
    cap_ll = max(pb.n_lig * min(pb.max_lig - 1, ll_k if ll_k > 0 else 200), 1)
    cap_kl = max(pb.n_kp * (kl_k if kl_k > 0 else min(pb.max_lig, 100)), 1)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    out = dict(ll_src=i32(cap_ll), ll_dst=i32(cap_ll), ll_rowptr=i32(pb.n_lig + 1),
               kl_src=i32(cap_kl), kl_dst=i32(cap_kl), kl_rowptr=i32(pb.n_lig + 1),
               lk_src=i32(cap_kl), lk_dst=i32(cap_kl), lk_rowptr=i32(pb.n_kp + 1),
               ll_per_graph=i32(pb.B), counts=i32(8))
    lg = KpdLigGraph(cap_ll, cap_kl, *[_ptr(out[k]) for k in
                                      ('ll_src', 'll_dst', 'll_rowptr', 'kl_src', 'kl_dst', 'kl_rowptr',
                                       'lk_src', 'lk_dst', 'lk_rowptr', 'll_per_graph', 'counts')])
    bt = pb.struct(lig_x, None, kp_x, None)
    check(lib().kpd_build_lig_graph(C.byref(bt), float(ll_cutoff), int(ll_k), float(kl_cutoff), int(kl_k), C.byref(lg), _stream()))
    return out


class _Handle:
    """Owns one kpd_<prefix>_* handle of the library (`prefix`: 'egnn', 'gvp_trainer', ...), created from its ctypes config."""

    def __init__(self, prefix: str, cfg):
        self._prefix, self.cfg = prefix, cfg
        self._h = C.c_void_p()
        check(self._fn('create')(C.byref(self.cfg), C.byref(self._h)))

    def _fn(self, name: str):
        return getattr(lib(), f'kpd_{self._prefix}_{name}')

    def __del__(self):
        if getattr(self, '_h', None) and _lib is not None:
            getattr(_lib, f'kpd_{self._prefix}_destroy')(self._h)
            self._h = None


class _Engine(_Handle):
    """An inference handle: weights are packed once from a state dict."""

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        load, st = self._fn('load_weight'), _stream()
        keep = []                                  # the converted copies live until the packing kernels have read them
        for name, t in sd.items():
            if t.numel() == 0:                     # dropout.vector_dropout.dummy_param
                continue
            t = _dev_f32(t.detach(), name)
            keep.append(t)
            shape = (C.c_int64 * t.dim())(*t.shape)
            check(load(self._h, name.encode(), t.data_ptr(), shape, t.dim(), st))
        torch.cuda.current_stream().synchronize()     # packing kernels read the source tensors
        check(self._fn('commit')(self._h))


class _Trainer(_Handle):
    """A training handle: parameters are bound by reference name to their live storage (read in place every step); gradients
    are written into the buffers bound for the backward call."""

    def bind(self, names, weights, grads):
        bind = self._fn('bind')
        for name, w, g in zip(names, weights, grads):
            if w.numel() == 0:                     # dropout.vector_dropout.dummy_param
                continue
            if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()):
                raise KpdError(f'parameter {name} must be a contiguous fp32 GPU tensor')
            shape = (C.c_int64 * w.dim())(*w.shape)
            check(bind(self._h, name.encode(), w.data_ptr(), None if g is None else g.data_ptr(), shape, w.dim()))


class _Denoiser:
    """What the denoiser handles (engines and trainers) share: the grow-only workspace and the edge counts of the last forward."""
    _reserved = None

    def reserve(self, pb: PreparedBatch):
        key = (pb.B, pb.n_lig, pb.n_kp, pb.n_kk, pb.max_lig, pb.max_kp)
        if self._reserved is not None and all(a <= b for a, b in zip(key, self._reserved)):
            return
        torch.cuda.synchronize()                   # not stream-ordered: it frees the workspace kernels in flight may still use
        check(self._fn('reserve')(self._h, *key))
        self._reserved = key if self._reserved is None else tuple(max(a, b) for a, b in zip(key, self._reserved))

    def _counts(self):
        arr = (C.c_int32 * 8)()
        check(self._fn('last_counts')(self._h, arr, _stream()))
        return arr

    def last_counts(self):
        return dict(zip(('E_ll', 'E_kl', 'E_lk', 'E_kk', 'tiles', 'tiles_last', 'E_last'), self._counts()))


class _DenoiserEngine(_Denoiser, _Engine):
    """The diagnostics of the two inference denoisers."""

    def debug(self, what: str, n_floats: int = 0, device=None) -> Optional[torch.Tensor]:
        out = torch.empty(max(n_floats, 1), device=device or 'cuda')
        check(self._fn('debug_state')(self._h, what.encode(), out.data_ptr(), n_floats, _stream()))
        return out if n_floats else None

    def profile(self, enable: bool):
        check(self._fn('profile')(self._h, int(enable)))

    def profile_read(self):
        """(total ms, launches) of the fused edge kernel (EGNN) / the message-chain kernel (GVP) since profile(True)."""
        ms, n = C.c_double(), C.c_int32()
        check(self._fn('profile_read')(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def gemm_mode(self) -> str:
        """The GEMM mode the engine runs in, as the library reports it ('f32' = exact fp32 MFMA, 'f16x2' = split f16 products;
        the GVP denoiser has 'f16x2' at 256 hidden scalars only)."""
        return 'f16x2' if self._counts()[7] else 'f32'

    def set_gemm_mode(self, mode: str):
        self.debug(f'gemm={mode}')


class EgnnEngine(_DenoiserEngine):
    """Owns one kpd_egnn handle: packed weights + workspace for LigRecDynamics.forward."""

    def __init__(self, cfg: KpdEgnnConfig):
        super().__init__('egnn', cfg)
        self.atom_nf, self.rec_nf = int(cfg.atom_nf), int(cfg.rec_nf)

    def forward(self, pb: PreparedBatch, lig_x, lig_h, kp_x, kp_h, t):
        self.reserve(pb)
        lig_x, lig_h = _dev_f32(lig_x, 'lig x_0'), _dev_f32(lig_h, 'lig h_0')
        kp_x, kp_h = _dev_f32(kp_x, 'kp x_0'), _dev_f32(kp_h, 'kp h_0')
        # the kernels read atom_nf / rec_nf columns per row: a narrower feature tensor would be read past its end
        # (upstream's encoder Linears raise on the same mismatch)
        if tuple(lig_h.shape) != (pb.n_lig, self.atom_nf) or tuple(kp_h.shape) != (pb.n_kp, self.rec_nf):
            raise KpdError(f'feature shapes lig {tuple(lig_h.shape)} / kp {tuple(kp_h.shape)} do not match the denoiser '
                           f'(expected ({pb.n_lig}, atom_nf={self.atom_nf}) / ({pb.n_kp}, rec_nf={self.rec_nf}))')
        t = _dev_f32(t, 'timestep')
        eps_h = torch.empty(pb.n_lig, self.atom_nf, device=lig_x.device)
        eps_x = torch.empty(pb.n_lig, 3, device=lig_x.device)
        bt = pb.struct(lig_x, lig_h, kp_x, kp_h)
        check(lib().kpd_egnn_forward(self._h, C.byref(bt), t.data_ptr(), eps_h.data_ptr(), eps_x.data_ptr(), _stream()))
        return eps_h, eps_x


_PARAM_GEN = [0]


def _on_register_parameter(module, name, param):
    _PARAM_GEN[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_on_register_parameter)


def param_generation() -> int:
    """Counts `register_parameter` calls of every module in the process (a global torch hook): the cached parameter lists of the
    engine-owning modules are rebuilt when it moves, so a swapped Parameter object is never read through a stale list."""
    return _PARAM_GEN[0]


class EgnnTrainer(_Denoiser, _Trainer):
    """Owns one kpd_egnn_trainer handle: forward with saved layer states + backward of LigRecDynamics.forward.
    Gradients are written into fresh zero tensors per backward call and handed to autograd."""

    def __init__(self, cfg: KpdEgnnConfig):
        super().__init__('egnn_trainer', cfg)
        self.atom_nf, self.rec_nf = int(cfg.atom_nf), int(cfg.rec_nf)

    def forward(self, pb: PreparedBatch, lig_x, lig_h, kp_x, kp_h, t):
        self.reserve(pb)
        eps_h = torch.empty(pb.n_lig, self.atom_nf, device=lig_x.device)
        eps_x = torch.empty(pb.n_lig, 3, device=lig_x.device)
        bt = pb.struct(lig_x, lig_h, kp_x, kp_h)
        check(lib().kpd_egnn_trainer_forward(self._h, C.byref(bt), t.data_ptr(), eps_h.data_ptr(), eps_x.data_ptr(), _stream()))
        return eps_h, eps_x

    def backward(self, d_eps_h, d_eps_x, d_lig_h, d_lig_x, d_kp_h, d_kp_x):
        check(lib().kpd_egnn_trainer_backward(self._h, d_eps_h.data_ptr(), d_eps_x.data_ptr(), _ptr(d_lig_h), _ptr(d_lig_x),
                                              _ptr(d_kp_h), _ptr(d_kp_x), _stream()))

    def profile(self, enable: bool):
        check(lib().kpd_egnn_trainer_profile(self._h, int(enable)))

    def profile_read(self):
        """{'fwd' | 'bwd': (total ms, launches, edges)} of k_egnn_edge_train / k_egnn_edge_bwd since profile(True)."""
        ms, n, e = (C.c_double * 2)(), (C.c_int32 * 2)(), (C.c_double * 2)()
        check(lib().kpd_egnn_trainer_profile_read(self._h, ms, n, e))
        return {'fwd': (ms[0], n[0], e[0]), 'bwd': (ms[1], n[1], e[1])}


class GvpEngine(_DenoiserEngine):
    """Owns one kpd_gvp handle: packed weights + workspace for LigRecDynamicsGVP.forward."""

    def __init__(self, cfg: KpdGvpConfig):
        super().__init__('gvp', cfg)
        self.n_lig_scalars = int(cfg.n_lig_scalars)

    def forward(self, pb: PreparedBatch, lig_x, lig_h, kp_x, kp_h, kp_v, t):
        self.reserve(pb)
        lig_x, lig_h = _dev_f32(lig_x, 'lig x_0'), _dev_f32(lig_h, 'lig h_0')
        kp_x, kp_h, kp_v = _dev_f32(kp_x, 'kp x_0'), _dev_f32(kp_h, 'kp h_0'), _dev_f32(kp_v, 'kp v_0')
        t = _dev_f32(t, 'timestep')
        if tuple(kp_v.shape) != (pb.n_kp, int(self.cfg.vector_size), 3):
            raise KpdError(f'kp v_0 has shape {tuple(kp_v.shape)}, expected ({pb.n_kp}, {int(self.cfg.vector_size)}, 3)')
        eps_h = torch.empty(pb.n_lig, self.n_lig_scalars, device=lig_x.device)
        eps_x = torch.empty(pb.n_lig, 3, device=lig_x.device)
        bt = pb.struct(lig_x, lig_h, kp_x, kp_h, kp_v)
        check(lib().kpd_gvp_forward(self._h, C.byref(bt), t.data_ptr(), eps_h.data_ptr(), eps_x.data_ptr(), _stream()))
        return eps_h, eps_x


class GvpTrainer(_Denoiser, _Trainer):
    """Owns one kpd_gvp_trainer handle: forward with saved conv states + backward of LigRecDynamicsGVP.forward."""

    def __init__(self, cfg: KpdGvpConfig):
        super().__init__('gvp_trainer', cfg)

    def set_dropout(self, rate: float, seed: int):
        check(lib().kpd_gvp_trainer_set_dropout(self._h, float(rate), int(seed) & (2 ** 64 - 1)))

    def forward(self, pb: PreparedBatch, lig_x, lig_h, kp_x, kp_h, kp_v, t):
        self.reserve(pb)
        eps_h = torch.empty(pb.n_lig, self.cfg.n_lig_scalars, device=lig_x.device)
        eps_x = torch.empty(pb.n_lig, 3, device=lig_x.device)
        bt = pb.struct(lig_x, lig_h, kp_x, kp_h, kp_v)
        check(lib().kpd_gvp_trainer_forward(self._h, C.byref(bt), t.data_ptr(), eps_h.data_ptr(), eps_x.data_ptr(), _stream()))
        return eps_h, eps_x

    def backward(self, d_eps_h, d_eps_x, d_lig_h, d_kp_h, d_kp_v, d_lig_x=None, d_kp_x=None):
        check(lib().kpd_gvp_trainer_backward(self._h, d_eps_h.data_ptr(), d_eps_x.data_ptr(), _ptr(d_lig_h), _ptr(d_kp_h), _ptr(d_kp_v),
                                             _ptr(d_lig_x), _ptr(d_kp_x), _stream()))

    def _counts(self):
        arr = (C.c_int32 * 4)()                    # the four edge counts only: `last_counts` has four entries here
        check(lib().kpd_gvp_trainer_last_counts(self._h, arr))
        return arr

    def message_path(self) -> int:
        """1: the convs' edge messages run through the register-chained kernels (hidden width 256), 0: one GVP at a time."""
        v = C.c_int32(0)
        check(lib().kpd_gvp_trainer_message_path(self._h, C.byref(v)))
        return int(v.value)


def dropout_mask(seed: int, conv: int, node_type: int, position: int, kind: int, n: int, rate: float, device='cuda') -> torch.Tensor:
    """One dropout stream of the GVP training path (kpd_dropout_mask): n entries in {0, 1 / (1 - rate)}."""
    out = torch.empty(int(n), device=device, dtype=torch.float32)
    check(lib().kpd_dropout_mask(int(seed) & (2 ** 64 - 1), int(conv), int(node_type), int(position), int(kind), int(n), float(rate),
                                 out.data_ptr(), _stream()))
    return out


def _norm_mode(message_norm):
    if message_norm == 'mean':
        return 1, 1.0
    if message_norm == 0:
        return 2, 0.0
    return 0, float(message_norm)


def sorted_csr(src: torch.Tensor, dst: torch.Tensor, n_dst: int, device, return_order: bool = False):
    """(src, dst) sorted by (dst, src) as int32 + CSR row pointer over dst (+ the permutation for edge data)."""
    src, dst = src.to(device).long(), dst.to(device).long()
    order = torch.arange(src.numel(), device=device)
    if src.numel():
        order = torch.argsort(dst * (int(src.max()) + 1) + src)
        src, dst = src[order], dst[order]
    deg = torch.bincount(dst, minlength=n_dst) if src.numel() else torch.zeros(n_dst, dtype=torch.long, device=device)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long, device=device), deg.cumsum(0)])
    out = (src.int().contiguous(), dst.int().contiguous(), rowptr.int().contiguous())
    return out + (order,) if return_order else out


def _rec_batch(eng, rec_counts, rec_x, rec_h, rr_src, rr_dst):
    """The head the two encoder calls share: sizes and offsets of the batch, the dst-sorted rr graph with its permutation (for edge
    data), the workspace of `eng` reserved for them, and the batch struct."""
    dev = rec_x.device
    rec_counts = rec_counts.cpu().long()
    B, n_rec, max_rec = int(rec_counts.numel()), int(rec_counts.sum()), int(rec_counts.max())
    rec_ptr = torch.cat([torch.zeros(1, dtype=torch.long), rec_counts.cumsum(0)]).int().to(dev)
    rec_x, rec_h = _dev_f32(rec_x, 'rec x_0'), _dev_f32(rec_h, 'rec h_0')
    s, d, rowptr, order = sorted_csr(rr_src, rr_dst, n_rec, dev, return_order=True)
    torch.cuda.synchronize()                       # as in _Denoiser.reserve
    check(eng._fn('reserve')(eng._h, B, n_rec, int(s.numel()), max_rec))
    bt = KpdRecBatch(B, n_rec, max_rec, _ptr(rec_ptr), _ptr(rec_x), _ptr(rec_h), int(s.numel()), _ptr(s), _ptr(d), _ptr(rowptr))
    return B, n_rec, max_rec, rec_ptr, rec_x, rec_h, s, d, rowptr, order, bt


def _trim_edges(out):
    """The tail the two encoder calls share: cut the kk / rk edge lists to the counts the library wrote."""
    e_kk, e_rk = out['counts'].tolist()            # once per pocket: a host sync here is fine
    out['kk_src'], out['kk_dst'] = out['kk_src'][:e_kk], out['kk_dst'][:e_kk]
    out['rk_src'], out['rk_dst'] = out['rk_src'][:e_rk], out['rk_dst'][:e_rk]


def _recenc_call(eng, rec_counts, rec_x, rec_h, rr_src, rr_dst):
    """RecEncEngine.forward and RecEncTrainer.forward: batch structs, output buffers, one library call."""
    dev = rec_x.device
    if int(rec_counts.min()) < 1:
        raise KpdError('every pocket needs at least one receptor atom')
    B, n_rec, max_rec, rec_ptr, rec_x, rec_h, s, d, rowptr, _, bt = _rec_batch(eng, rec_counts, rec_x, rec_h, rr_src, rr_dst)
    n_kp = B * eng.K
    cap_kk = max(n_kp * min(eng.K - 1, 100), 1)
    f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    i32 = lambda n: torch.zeros(n, device=dev, dtype=torch.int32)
    out = dict(kp_x=f32(n_kp, 3), kp_h=f32(n_kp, eng.S), kp_v=f32(n_kp, int(eng.cfg.vector_size), 3), rk_src=i32(n_kp * eng.k),
               rk_dst=i32(n_kp * eng.k), kk_src=i32(cap_kk), kk_dst=i32(cap_kk), kk_per_graph=i32(B), counts=i32(2))
    ro = KpdRecOut(_ptr(out['kp_x']), _ptr(out['kp_h']), _ptr(out['kp_v']), _ptr(out['rk_src']), _ptr(out['rk_dst']),
                   cap_kk, _ptr(out['kk_src']), _ptr(out['kk_dst']), _ptr(out['kk_per_graph']), _ptr(out['counts']))
    check(eng._fn('forward')(eng._h, C.byref(bt), C.byref(ro), _stream()))
    _trim_edges(out)
    out['_keep'] = (rec_ptr, rec_x, rec_h, s, d, rowptr)      # the training engine reads these again in its backward pass
    return out


class _RecEnc:
    """What RecEncEngine and RecEncTrainer share: the sizes read from the config, and forward."""

    def __init__(self, prefix: str, cfg: KpdRecencConfig):
        super().__init__(prefix, cfg)
        # rk edges per keypoint: k of the kNN graph, or at most 10 of the radius graph (receptor_encoder_gvp.py:306)
        self.S, self.K, self.k = int(cfg.out_scalar_size), int(cfg.n_keypoints), int(cfg.k_closest) if cfg.k_closest else 10

    def forward(self, rec_counts: torch.Tensor, rec_x, rec_h, rr_src, rr_dst):
        return _recenc_call(self, rec_counts, rec_x, rec_h, rr_src, rr_dst)


class RecEncEngine(_RecEnc, _Engine):
    """Owns one kpd_recenc handle: packed weights + workspace for ReceptorEncoderGVP.forward."""

    def __init__(self, cfg: KpdRecencConfig):
        super().__init__('recenc', cfg)


class RecEncTrainer(_RecEnc, _Trainer):
    """Owns one kpd_recenc_trainer handle: ReceptorEncoderGVP.forward with saved node states + its backward pass."""

    def __init__(self, cfg: KpdRecencConfig):
        super().__init__('recenc_trainer', cfg)

    def set_dropout(self, rate: float, seed: int):
        check(lib().kpd_recenc_trainer_set_dropout(self._h, float(rate), int(seed) & (2 ** 64 - 1)))

    def backward(self, d_kp_x, d_kp_h, d_kp_v):
        check(lib().kpd_recenc_trainer_backward(self._h, _ptr(d_kp_x), _ptr(d_kp_h), _ptr(d_kp_v), _stream()))


def _recegnn_call(eng, rec_counts, rec_x, rec_h, rr_src, rr_dst, same_res):
    """RecEgnnEngine.forward and RecEgnnTrainer.forward."""
    dev = rec_x.device
    if int(rec_counts.min()) < eng.k:
        raise KpdError(f'every pocket needs at least k_closest={eng.k} receptor atoms (the reference stacks exactly k '
                       f'neighbour distances per keypoint)')
    if eng.ef and same_res is None:
        raise KpdError("use_sameres_feat needs g.edges['rr'].data['same_res']")
    B, n_rec, max_rec, rec_ptr, rec_x, rec_h, s, d, rowptr, order, bt = _rec_batch(eng, rec_counts, rec_x, rec_h, rr_src, rr_dst)
    a = same_res.to(dev).reshape(-1)[order].float().contiguous() if eng.ef else None
    n_kp = B * eng.K
    cap_kk = max(n_kp * min(eng.K - 1, 100), 1)
    f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    i32 = lambda n: torch.zeros(n, device=dev, dtype=torch.int32)
    cap_rk = n_kp * min(eng.rk_cap, max_rec)
    out = dict(kp_x=f32(n_kp, 3), kp_h=f32(n_kp, eng.D), rk_src=i32(cap_rk), rk_dst=i32(cap_rk),
               kk_src=i32(cap_kk), kk_dst=i32(cap_kk), kk_per_graph=i32(B), counts=i32(2), rec_h=f32(n_rec, eng.D),
               rec_x=f32(n_rec, 3))
    ro = KpdRecOut(_ptr(out['kp_x']), _ptr(out['kp_h']), None, _ptr(out['rk_src']), _ptr(out['rk_dst']), cap_kk,
                   _ptr(out['kk_src']), _ptr(out['kk_dst']), _ptr(out['kk_per_graph']), _ptr(out['counts']))
    check(eng._fn('forward')(eng._h, C.byref(bt), _ptr(a), C.byref(ro), _ptr(out['rec_h']), _ptr(out['rec_x']), _stream()))
    _trim_edges(out)
    out['_keep'] = (rec_ptr, rec_x, rec_h, s, d, rowptr, a)      # the training engine reads these again in its backward pass
    return out


class _RecEgnn:
    """What RecEgnnEngine and RecEgnnTrainer share: the sizes read from the config, and forward."""

    def __init__(self, prefix: str, cfg: KpdRecegnnConfig):
        super().__init__(prefix, cfg)
        self.D, self.K, self.k, self.ef = int(cfg.out_n_node_feat), int(cfg.n_keypoints), int(cfg.k_closest), bool(cfg.use_sameres_feat)
        self.rk_cap = self.k if self.k else 100    # rk edges per keypoint: k, or at most 100 within kp_rad (:246)

    def forward(self, rec_counts: torch.Tensor, rec_x, rec_h, rr_src, rr_dst, same_res=None):
        return _recegnn_call(self, rec_counts, rec_x, rec_h, rr_src, rr_dst, same_res)


class RecEgnnEngine(_RecEgnn, _Engine):
    """Owns one kpd_recegnn handle: weights + workspace for ReceptorEncoder.forward (models/receptor_encoder.py)."""

    def __init__(self, cfg: KpdRecegnnConfig):
        super().__init__('recegnn', cfg)


class RecEgnnTrainer(_RecEgnn, _Trainer):
    """Owns one kpd_recegnn_trainer handle: ReceptorEncoder.forward with saved layer states + its backward pass."""

    def __init__(self, cfg: KpdRecegnnConfig):
        super().__init__('recegnn_trainer', cfg)

    def backward(self, d_kp_x, d_kp_h):
        check(lib().kpd_recegnn_trainer_backward(self._h, _ptr(d_kp_x), _ptr(d_kp_h), _stream()))


def ot_emd_uniform(costs, n_threads: int = 0):
    """Exact transport plans (uniform masses) for a list of [n_i, m_i] cost matrices (numpy float64, host): kpd_ot_emd_uniform.
    Host-side like the reference's POT call; the library spreads the problems over host threads (ctypes releases the GIL)."""
    import numpy as np
    if not costs:
        return []
    ns = np.asarray([c.shape[0] for c in costs], dtype=np.int32)
    ms = np.asarray([c.shape[1] for c in costs], dtype=np.int32)
    sizes = ns.astype(np.int64) * ms.astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    flat = np.concatenate([np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in costs])
    plan = np.empty_like(flat)
    if n_threads <= 0:
        # one thread per problem where the host has the hardware threads (the solves of a batch are a burst of ~20 ms each: a CPU quota
        # averaged over a scheduling period still lets them all start at once; measured 67 -> ~20 ms per B = 64 batch on a 16-CPU quota)
        n_threads = max(1, min(len(os.sched_getaffinity(0)), 64))
    check(lib().kpd_ot_emd_uniform(len(costs), ns.ctypes.data, ms.ctypes.data, offs.ctypes.data, flat.ctypes.data, plan.ctypes.data,
                                   int(n_threads)))
    return [plan[o:o + s].reshape(int(a), int(b)) for o, s, a, b in zip(offs, sizes, ns, ms)]


def zero_grads_like(params, wanted):
    """Zero-filled gradient buffers for the parameters whose flag in `wanted` is set (None for the others), carved out of ONE flat
    allocation with one fill -- a model has a few hundred parameter tensors, and a fill kernel each is most of a millisecond per step.
    Offsets are multiples of 64 floats (256 B), so every view is as aligned as a tensor of its own."""
    sizes = [((p.numel() + 63) // 64) * 64 if (w and p.numel()) else 0 for p, w in zip(params, wanted)]
    total = sum(sizes)
    if total == 0:
        return [None] * len(params)
    ref = next(p for p, n in zip(params, sizes) if n)
    flat = torch.zeros(total, device=ref.device, dtype=ref.dtype)
    out, off = [], 0
    for p, n in zip(params, sizes):
        out.append(flat[off:off + p.numel()].view(p.shape) if n else None)
        off += n
    return out


def sgemm(a: torch.Tensor, b: torch.Tensor, trans_a=False, trans_b=False, alpha=1.0, beta=0.0, out: torch.Tensor = None,
          workspace: torch.Tensor = None, colsum: torch.Tensor = None) -> torch.Tensor:
    """out = alpha op(a) op(b) + beta out through kpd_sgemm (the GEMM of the training engines).  a, b, out: 2-D fp32 device tensors whose
    last dimension is contiguous; row strides and storage offsets are passed as they are (views of wider arrays are the tested case).
    `workspace`: contiguous fp32 device scratch that lets a K-dominated product be split along K.  `colsum` (trans_a and not trans_b):
    contiguous [M] tensor that receives += the column sums of a."""
    for t, name in ((a, 'a'), (b, 'b')):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)):
            raise KpdError(f'sgemm: {name} must be a 2-D fp32 device tensor with a contiguous last dimension')
    M, K = (a.shape[1], a.shape[0]) if trans_a else tuple(a.shape)
    K2, N = (b.shape[1], b.shape[0]) if trans_b else tuple(b.shape)
    if K != K2:
        raise KpdError(f'sgemm: inner sizes {K} and {K2} differ')
    if out is None:
        out = torch.zeros(M, N, device=a.device)
    if tuple(out.shape) != (M, N) or not out.is_cuda or out.dtype != torch.float32 or (N > 1 and out.stride(1) != 1):
        raise KpdError('sgemm: out must be an fp32 device tensor [M, N] with a contiguous last dimension')
    ld = lambda t: int(t.stride(0)) if t.shape[0] > 1 else max(int(t.shape[1]), 1)
    check(lib().kpd_sgemm(int(trans_a), int(trans_b), M, N, K, float(alpha), a.data_ptr(), ld(a), b.data_ptr(), ld(b), float(beta),
                          out.data_ptr(), ld(out), colsum.data_ptr() if colsum is not None else None,
                          workspace.data_ptr() if workspace is not None else None,
                          int(workspace.numel()) if workspace is not None else 0, _stream()))
    return out


def adam_step(table_dev: torch.Tensor, max_numel: int, mode: int, lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, clip_value=0.0):
    """kpd_adam_step over a device table [n, 5] of int64 (parameter, gradient, exp_avg, exp_avg_sq pointers, element count): optim.py builds it."""
    if not (table_dev.is_cuda and table_dev.dtype == torch.int64 and table_dev.dim() == 2 and table_dev.shape[1] == 5 and table_dev.is_contiguous()):
        raise KpdError('adam_step: the table must be a contiguous int64 device tensor [n, 5]')
    check(lib().kpd_adam_step(table_dev.data_ptr(), int(table_dev.shape[0]), int(max_numel), int(mode), float(lr), float(beta1), float(beta2), float(eps),
                              float(weight_decay), int(step), float(clip_value), _stream()))


def wgrad_batch(kind: int, items, workspace: torch.Tensor):
    """kpd_wgrad_batch: `items` = list of dicts with the fields of kpd_wgrad_item (tensors or None, ints); leading dimensions are taken from
    the tensors' row strides.  Outputs are accumulated in place."""
    arr = (KpdWgradItem * len(items))()
    ld = lambda t: int(t.stride(0)) if t.shape[0] > 1 else max(int(t.shape[-1]), 1)
    p = lambda t: t.data_ptr() if t is not None else None
    for k, it in enumerate(items):
        e = arr[k]
        e.A, e.B, e.lda, e.ldb, e.K = p(it['A']), p(it['B']), ld(it['A']), ld(it['B']), int(it['A'].shape[0])
        c = it.get('C')
        e.C, e.ldc = p(c), ld(c) if c is not None else 0
        for src, ldf, nf, dst, ldd in (('B2', 'ldb2', 'nb2', 'Cx1', 'ldx1'), ('A2', 'lda2', 'na2', 'Cx2', 'ldx2'), ('B3', 'ldb3', 'nb3', 'Cx3', 'ldx3')):
            t, o = it.get(src), it.get(dst)
            setattr(e, src, p(t)); setattr(e, ldf, ld(t) if t is not None else 0); setattr(e, nf, int(it.get(nf, 0)))
            setattr(e, dst, p(o)); setattr(e, ldd, ld(o) if o is not None else 0)
        e.colsum, e.colsum2 = p(it.get('colsum')), p(it.get('colsum2'))
    check(lib().kpd_wgrad_batch(int(kind), len(items), arr, workspace.data_ptr(), int(workspace.numel()), _stream()))


def step_coefficients(gamma: torch.Tensor, s: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """[B,3] reverse-step coefficients from the gamma table (kpd_step_coefficients): one launch per step."""
    gamma, s, t = _dev_f32(gamma, 'gamma'), _dev_f32(s, 's'), _dev_f32(t, 't')
    if s.shape != t.shape or s.dim() != 1:
        raise KpdError(f'step_coefficients: s {tuple(s.shape)} and t {tuple(t.shape)} must be equal 1-D tensors')
    coef = torch.empty(s.shape[0], 3, device=s.device)
    check(lib().kpd_step_coefficients(gamma.data_ptr(), int(gamma.shape[0]), s.data_ptr(), t.data_ptr(), int(s.shape[0]),
                                      coef.data_ptr(), _stream()))
    return coef


def inpaint_coefficients(gamma: torch.Tensor, s: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """[B,6] coefficients of an inpainting step (kpd_inpaint_coefficients): the three of `step_coefficients`, bit for bit, then
    alpha_s, sigma_s, sigma_t|s."""
    gamma, s, t = _dev_f32(gamma, 'gamma'), _dev_f32(s, 's'), _dev_f32(t, 't')
    if s.shape != t.shape or s.dim() != 1:
        raise KpdError(f'inpaint_coefficients: s {tuple(s.shape)} and t {tuple(t.shape)} must be equal 1-D tensors')
    coef = torch.empty(s.shape[0], 6, device=s.device)
    check(lib().kpd_inpaint_coefficients(gamma.data_ptr(), int(gamma.shape[0]), s.data_ptr(), t.data_ptr(), int(s.shape[0]),
                                         coef.data_ptr(), _stream()))
    return coef


def complex_noise(pb: PreparedBatch, width: int, complex_ids: torch.Tensor, seed: int, step: int, tag: int) -> torch.Tensor:
    """[n_lig, width] N(0,1) noise that depends only on (seed, complex id, step, tag, position in the complex)
    (kpd_complex_noise): a sharded run draws what the single-process run draws."""
    if not (complex_ids.is_cuda and complex_ids.dtype == torch.int64 and complex_ids.numel() == pb.B):
        raise KpdError('complex_ids must be an int64 GPU tensor with one id per complex')
    out = torch.empty(pb.n_lig, int(width), device=complex_ids.device, dtype=torch.float32)
    check(lib().kpd_complex_noise(pb.B, _ptr(pb.lig_ptr), int(width), _ptr(complex_ids.contiguous()), int(seed) & (2 ** 64 - 1),
                                  int(step), int(tag), _ptr(out), _stream()))
    return out


def dist_hinge(a: torch.Tensor, a_ptr: torch.Tensor, b: Optional[torch.Tensor], b_ptr: Optional[torch.Tensor], threshold: float,
               grad_a: bool = False, grad_b: bool = False):
    """Segmented distance hinge (kpd_dist_hinge): a [n_a,3] and b [n_b,3] fp32 GPU tensors split into S segments by the int32 GPU
    offsets a_ptr / b_ptr [S+1]; b = None is self mode (pairs i < j of each A segment).  Returns (seg_loss [S], total [1],
    grad_a [n_a,3] or None, grad_b [n_b,3] or None): the unscaled gradients of the total, zero on rows outside every segment."""
    def pos(t, name):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise KpdError(f'dist_hinge: {name} must be a GPU tensor (the hinge has no CPU implementation)')
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
            raise KpdError(f'dist_hinge: {name} must be fp32 [n, 3] (got {t.dtype} {tuple(t.shape)})')
        return t.contiguous()

    def offsets(p, name, dev):
        if not (isinstance(p, torch.Tensor) and p.device == dev and p.dtype == torch.int32 and p.dim() == 1 and p.numel() >= 1):
            raise KpdError(f'dist_hinge: {name} must be a 1-D int32 tensor [S+1] on {dev}')
        return p.contiguous()

    a = pos(a, 'a')
    a_ptr = offsets(a_ptr, 'a_ptr', a.device)
    S = a_ptr.numel() - 1
    if b is not None:
        b = pos(b, 'b')
        if b.device != a.device:
            raise KpdError('dist_hinge: a and b must be on the same device')
        b_ptr = offsets(b_ptr, 'b_ptr', a.device)
        if b_ptr.numel() != S + 1:
            raise KpdError(f'dist_hinge: a_ptr and b_ptr must have the same length (got {S + 1} and {b_ptr.numel()})')
    elif b_ptr is not None or grad_b:
        raise KpdError('dist_hinge: self mode (b = None) takes no b_ptr and no grad_b')
    seg = torch.empty(S, device=a.device, dtype=torch.float32)
    total = torch.empty(1, device=a.device, dtype=torch.float32)
    ga = torch.zeros_like(a) if grad_a else None
    gb = torch.zeros_like(b) if grad_b else None
    check(lib().kpd_dist_hinge(_ptr(a), _ptr(a_ptr), int(a.shape[0]), _ptr(b), _ptr(b_ptr), int(b.shape[0]) if b is not None else 0, S,
                               float(threshold), _ptr(seg), _ptr(total), _ptr(ga), _ptr(gb), _stream()))
    return seg, total, ga, gb


def build_rec_graph(rec_x: torch.Tensor, rec_ptr: torch.Tensor, max_rec: int, r: float, res_idx: Optional[torch.Tensor] = None,
                    max_nn: int = 100, return_rowptr: bool = False):
    """rr radius graph (+ same-residue flags) of a batch of pockets on the GPU (kpd_build_rec_graph).
    rec_x [n_rec,3] fp32, rec_ptr [B+1] int32, res_idx [n_rec] int32 or None, all on the GPU.
    Returns (src, dst, per_graph [B], same_res bool [E] or None), dst-major with global row numbers.  One host sync
    (the edge count) — this is input-pipeline work, once per batch, not step-path work.  return_rowptr appends the CSR row
    pointers [n_rec + 1] of the list to the tuple."""
    rec_x = _dev_f32(rec_x, 'rec_x')
    n_rec, B = rec_x.shape[0], _offsets(rec_ptr, 'rec_ptr')
    if res_idx is not None:
        res_idx = _per_entry(res_idx, 'res_idx', n_rec, 'receptor atom')
    dev = rec_x.device
    cap = n_rec * max(1, min(int(max_nn), int(max_rec) - 1))
    src = torch.empty(cap, dtype=torch.int32, device=dev)
    dst = torch.empty(cap, dtype=torch.int32, device=dev)
    rowptr = torch.empty(n_rec + 1, dtype=torch.int32, device=dev)
    per_graph = torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    same = torch.empty(cap, dtype=torch.uint8, device=dev) if res_idx is not None else None
    scratch = torch.empty(int(lib().kpd_rec_graph_scratch_bytes(n_rec, B)), dtype=torch.uint8, device=dev)
    check(lib().kpd_build_rec_graph(_ptr(rec_x), _ptr(rec_ptr), B, n_rec, int(max_rec), float(r), int(max_nn), _ptr(res_idx),
                                    cap, _ptr(src), _ptr(dst), _ptr(rowptr), _ptr(per_graph), _ptr(same), _ptr(counts), _ptr(scratch), _stream()))
    E = int(counts[0].item())
    if E > cap:
        raise KpdError(f'rr graph: {E} edges exceed the capacity {cap} (internal sizing error)')
    out = (src[:E], dst[:E], per_graph, (same[:E].bool() if same is not None else None))
    return out + (rowptr,) if return_rowptr else out


POCKET_EMPTY, POCKET_CAPACITY, POCKET_BAD_RES, POCKET_BAD_SEGMENT = 1, 2, 4, 8     # status bits of the two pocket entry points
POCKET_MAX_LIG = 1024


def _pocket_args(rec_x, rec_ptr, lig_x, lig_ptr, masks):
    rec_x, lig_x = _dev_f32(rec_x, 'rec_x'), _dev_f32(lig_x, 'lig_x')
    n_rec, B = rec_x.shape[0], _offsets(rec_ptr, 'rec_ptr')
    if rec_x.shape != (n_rec, 3) or lig_x.dim() != 2 or lig_x.shape[1] != 3 or _offsets(lig_ptr, 'lig_ptr') != B:
        raise KpdError(f'rec_x {tuple(rec_x.shape)}, lig_x {tuple(lig_x.shape)}, {B + 1} / {lig_ptr.numel()} offsets')
    out = []
    for name, t in masks:
        if not (t.is_cuda and t.numel() == n_rec and t.dtype in (torch.bool, torch.uint8)):
            raise KpdError(f'{name} must be a bool or uint8 GPU tensor with one entry per receptor atom')
        out.append(t.contiguous().view(torch.uint8) if t.dtype == torch.bool else t.contiguous())
    return rec_x, lig_x, n_rec, B, out


def pocket_select(rec_x: torch.Tensor, rec_ptr: torch.Tensor, res_idx: torch.Tensor, probe: torch.Tensor, emit: torch.Tensor,
                  lig_x: torch.Tensor, lig_ptr: torch.Tensor, max_rec: int, box_padding: float, pocket_cutoff: float,
                  cap_rows: Optional[int] = None):
    """Pocket atoms of a batch of whole receptors on the GPU (kpd_pocket_select; include/kpd.h has the contract).
    rec_x [n_rec,3], res_idx [n_rec] int32, probe / emit [n_rec] bool or uint8, lig_x [n_lig,3], rec_ptr / lig_ptr [B+1]
    int32, all on the GPU; box_padding < 0 or None: no box.  Returns a dict: rows (global atom numbers, ascending),
    pocket_res, pocket_ptr (list of B + 1 offsets; the last is the size needed), status (list of B), in_box, pocket_mask
    (bool [n_rec]).  One host read (offsets + status together)."""
    rec_x, lig_x, n_rec, B, (probe, emit) = _pocket_args(rec_x, rec_ptr, lig_x, lig_ptr, (('probe', probe), ('emit', emit)))
    res_idx = _per_entry(res_idx, 'res_idx', n_rec, 'receptor atom')
    dev = rec_x.device
    cap = n_rec if cap_rows is None else int(cap_rows)
    in_box = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    mask = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    rows = torch.empty(cap, dtype=torch.int32, device=dev)
    pocket_res = torch.empty(cap, dtype=torch.int32, device=dev)
    meta = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)         # pocket_ptr [B + 1], status [B]
    scratch = torch.empty(int(lib().kpd_pocket_scratch_bytes(n_rec, B)), dtype=torch.uint8, device=dev)
    check(lib().kpd_pocket_select(_ptr(rec_x), _ptr(rec_ptr), _ptr(res_idx), _ptr(probe), _ptr(emit), n_rec, int(max_rec),
                                  _ptr(lig_x), _ptr(lig_ptr), int(lig_x.shape[0]), B, -1.0 if box_padding is None else float(box_padding),
                                  float(pocket_cutoff), cap, _ptr(in_box), _ptr(mask), _ptr(rows), _ptr(pocket_res), _ptr(meta),
                                  meta.data_ptr() + 4 * (B + 1), _ptr(scratch), _stream()))
    host = meta.cpu().tolist()
    ptr, status = host[:B + 1], host[B + 1:]
    n = min(ptr[-1], cap)
    return dict(rows=rows[:n], pocket_res=pocket_res[:n], pocket_ptr=ptr, status=status, in_box=in_box.bool(), pocket_mask=mask.bool())


def interface_points(rec_x: torch.Tensor, rec_ptr: torch.Tensor, cand_mask: torch.Tensor, lig_x: torch.Tensor, lig_ptr: torch.Tensor,
                     dist_thr: float, excl_thr: float, cap_cand: int = 2048, cap_points: Optional[int] = None):
    """Interface points of a batch on the GPU (kpd_interface_points).  cand_mask [n_rec] bool or uint8: the candidate
    receptor atoms.  cap_cand: candidate capacity per complex, cap_points: capacity for the points of all complexes
    (default: B * min(cap_cand, 4096), which cannot overflow).  Returns a dict: points [n,3], ip_ptr (list of B + 1 offsets;
    the last is the size needed), n_cand (list of B, exact also beyond cap_cand), status (list of B).  One host read."""
    rec_x, lig_x, n_rec, B, (cand_mask,) = _pocket_args(rec_x, rec_ptr, lig_x, lig_ptr, (('cand_mask', cand_mask),))
    dev = rec_x.device
    cap_cand = int(cap_cand)
    cap_pts = B * min(cap_cand, 4096) if cap_points is None else int(cap_points)
    points = torch.empty(cap_pts, 3, dtype=torch.float32, device=dev)
    meta = torch.empty(3 * B + 1, dtype=torch.int32, device=dev)         # ip_ptr [B + 1], n_cand [B], status [B]
    scratch = torch.empty(int(lib().kpd_interface_points_scratch_bytes(n_rec, B, cap_cand)), dtype=torch.uint8, device=dev)
    base = meta.data_ptr()
    check(lib().kpd_interface_points(_ptr(rec_x), _ptr(rec_ptr), _ptr(cand_mask), n_rec, _ptr(lig_x), _ptr(lig_ptr), int(lig_x.shape[0]), B,
                                     float(dist_thr), float(excl_thr), cap_cand, cap_pts, _ptr(points), base, base + 4 * (B + 1),
                                     base + 4 * (2 * B + 1), _ptr(scratch), _stream()))
    host = meta.cpu().tolist()
    ptr = host[:B + 1]
    return dict(points=points[:min(ptr[-1], cap_pts)], ip_ptr=ptr, n_cand=host[B + 1:2 * B + 1], status=host[2 * B + 1:])


def _packed_symbols(elements, device, longest: int = 4) -> torch.Tensor:
    """Element symbols as NUL-padded little-endian words, the form kpd_xyz_emit and kpd_sdf_emit read."""
    packed = []
    for el in elements:
        b = el.encode('ascii')
        if not 1 <= len(b) <= longest:
            raise KpdError(f'element symbol {el!r} must be 1-{longest} ASCII characters')
        packed.append(int.from_bytes(b.ljust(4, b'\0'), 'little'))
    return torch.tensor(packed, dtype=torch.int32, device=device)        # ASCII: the top bit is never set


def xyz_emit(pos: torch.Tensor, feat: torch.Tensor, lig_ptr: torch.Tensor, elements):
    """Element decode + XYZ text of a batch of ligands on the GPU (kpd_xyz_emit).
    pos [N,3], feat [N,F] fp32 GPU tensors, lig_ptr [B+1] int32 GPU tensor, elements: F symbols.
    Returns (element index per atom [N] int32 GPU tensor, text bytes, text_ptr list of B+1 offsets); the only host
    synchronisation is the copy of the finished text."""
    pos, feat = _dev_f32(pos, 'pos'), _dev_f32(feat, 'feat')
    N, B, F = pos.shape[0], _offsets(lig_ptr, 'lig_ptr'), feat.shape[1] if feat.dim() == 2 else -1
    if pos.shape != (N, 3) or feat.shape[0] != N or F != len(elements):
        raise KpdError(f'xyz_emit: pos {tuple(pos.shape)}, feat {tuple(feat.shape)}, {len(elements)} element symbols')
    dev = pos.device
    symbols = _packed_symbols(elements, dev)
    elem = torch.empty(N, dtype=torch.int32, device=dev)
    capacity = 72 * N + 16 * B + 16         # a line is at most 71 bytes, a header at most 12
    text = torch.empty(capacity, dtype=torch.uint8, device=dev)
    text_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib().kpd_xyz_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    check(lib().kpd_xyz_emit(_ptr(pos), _ptr(feat), _ptr(lig_ptr), N, B, F, _ptr(symbols), _ptr(elem), _ptr(text), capacity,
                             _ptr(text_ptr), _ptr(status), _ptr(scratch), _stream()))
    ptr = text_ptr.cpu().tolist()
    st = int(status.item())
    if st & 2:
        raise KpdError('xyz_emit: text buffer too small (internal sizing error)')
    if st & 1:
        raise KpdError('xyz_emit: a coordinate with |x| >= 2^53 cannot be printed (diverged sample?)')
    return elem, bytes(text[:ptr[-1]].cpu().numpy()), ptr


MOL_EMPTY, MOL_CAPACITY, MOL_BAD_ATOM, MOL_BAD_SEGMENT = 1, 2, 4, 8          # status bits of kpd_mol_perceive
SDF_NONFINITE, SDF_WIDE, SDF_NO_MOLECULE, SDF_CAPACITY = 1, 2, 4, 8         # status bits of kpd_sdf_emit
MOL_MAX_ATOMS = 256


def mol_perceive(pos: torch.Tensor, feat: torch.Tensor, lig_ptr: torch.Tensor, z, allowed, cap_bonds: Optional[int] = None):
    """Bond graph, valences, fragments and validity counts of a batch of ligands on the GPU (kpd_mol_perceive; include/kpd.h
    states the rule).  pos [N,3], feat [N,F] fp32 GPU tensors, lig_ptr [B+1] int32 GPU tensor, z / allowed: the atomic number
    and the largest allowed valence of every feature class (F integers each).  cap_bonds: capacity of the bond list (default
    3 N, which cannot overflow).  Returns a dict of device tensors: elem, valence, frag [N], bonds [cap_bonds,2], order
    [cap_bonds], bond_ptr [B+1], summary [B,4], status [B].  No host synchronisation."""
    pos, feat = _dev_f32(pos, 'pos'), _dev_f32(feat, 'feat')
    B = _offsets(lig_ptr, 'lig_ptr')
    N, F = pos.shape[0], feat.shape[1] if feat.dim() == 2 else -1
    if pos.shape != (N, 3) or feat.shape[0] != N or F < 1 or len(z) != F or len(allowed) != F:
        raise KpdError(f'mol_perceive: pos {tuple(pos.shape)}, feat {tuple(feat.shape)}, {len(z)} atomic numbers, {len(allowed)} valences')
    dev = pos.device
    cap = 3 * N if cap_bonds is None else int(cap_bonds)
    table = _class_table(dev, z, allowed)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = dict(elem=i32(N), valence=i32(N), frag=i32(N), bonds=i32(cap, 2), order=i32(cap), bond_ptr=i32(B + 1), summary=i32(B, 4),
               status=i32(B))
    scratch = torch.empty(int(lib().kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    check(lib().kpd_mol_perceive(_ptr(pos), _ptr(feat), _ptr(lig_ptr), N, B, F, _ptr(table[0]), _ptr(table[1]), cap, _ptr(out['elem']),
                                 _ptr(out['valence']), _ptr(out['frag']), _ptr(out['bonds']), _ptr(out['order']), _ptr(out['bond_ptr']),
                                 _ptr(out['summary']), _ptr(out['status']), _ptr(scratch), _stream()))
    return out


def sdf_emit(pos: torch.Tensor, lig_ptr: torch.Tensor, elements, mol: dict, largest_only: bool = False, capacity: Optional[int] = None):
    """MOL V2000 / SDF text of a batch of ligands on the GPU (kpd_sdf_emit) from what `mol_perceive` returned.
    elements: F symbols of at most three characters.  Returns (text bytes, text_ptr list of B + 1 offsets, status list of B);
    ligand b's block is text[text_ptr[b]:text_ptr[b + 1]], empty when its status is not 0.  The only host synchronisation is
    the copy of the finished text."""
    pos = _dev_f32(pos, 'pos')
    B = _offsets(lig_ptr, 'lig_ptr')
    N, F = pos.shape[0], len(elements)
    cap_bonds = _mol_args('sdf_emit', mol, ('elem', 'frag', 'bonds', 'order', 'bond_ptr', 'status'), B, N)
    if pos.shape != (N, 3) or F < 1:
        raise KpdError(f'sdf_emit: pos {tuple(pos.shape)} must be [N,3] and there must be element symbols (got {F})')
    dev = pos.device
    symbols = _packed_symbols(elements, dev, 3)
    cap = 70 * N + 13 * cap_bonds + 77 * B if capacity is None else int(capacity)      # fixed-width lines: the exact upper bound
    text = torch.empty(cap, dtype=torch.uint8, device=dev)
    text_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib().kpd_sdf_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    check(lib().kpd_sdf_emit(_ptr(pos), _ptr(lig_ptr), N, B, _ptr(mol['elem']), F, _ptr(symbols), _ptr(mol['frag']), _ptr(mol['bonds']),
                             _ptr(mol['order']), _ptr(mol['bond_ptr']), cap_bonds, _ptr(mol['status']), int(bool(largest_only)), _ptr(text),
                             cap, _ptr(text_ptr), _ptr(status), _ptr(scratch), _stream()))
    ptr = text_ptr.cpu().tolist()
    return bytes(text[:min(ptr[-1], cap)].cpu().numpy()), ptr, status.cpu().tolist()


KEY_NO_MOLECULE = 1         # status bit of kpd_mol_keys
DIV_BAD_SEGMENT = 1         # status bit of kpd_fp_diversity


def mol_keys(lig_ptr: torch.Tensor, z, mol: dict, largest_only: bool = True, with_orders: bool = True, radius: int = 2, nbits: int = 2048,
             atom_inv: bool = False):
    """Isomorphism keys and substructure fingerprints of a batch of perceived molecules on the GPU (kpd_mol_keys; include/kpd.h
    states the rule).  `mol`: what `mol_perceive` returned, z: the atomic number of every feature class.  Returns a dict of
    device tensors: key [B] int64 (the uint64 bit pattern), fp [B, nbits/32] int32 (the uint32 bit pattern), status [B] (bit 0:
    no molecule, key 0 and an all-zero row) and, on request, atom_inv [N] int64.  No host synchronisation."""
    B = _offsets(lig_ptr, 'lig_ptr')
    N, F = _numel(mol.get('elem')), len(z)
    cap_bonds = _mol_args('mol_keys', mol, ('elem', 'frag', 'bonds', 'order', 'bond_ptr', 'status'), B, N)
    nbits, radius = int(nbits), int(radius)
    if not (F >= 1 and 0 <= radius <= 4 and 64 <= nbits <= 4096 and nbits & (nbits - 1) == 0):
        raise KpdError(f'mol_keys: {F} atomic numbers must be at least one, radius {radius} 0 .. 4 and nbits {nbits} a power of two in '
                       f'64 .. 4096')
    dev = lig_ptr.device
    zt = _class_table(dev, z)
    out = dict(key=torch.empty(B, dtype=torch.int64, device=dev), fp=torch.empty(B, nbits // 32, dtype=torch.int32, device=dev),
               status=torch.empty(B, dtype=torch.int32, device=dev))
    if atom_inv:
        out['atom_inv'] = torch.empty(N, dtype=torch.int64, device=dev)
    check(lib().kpd_mol_keys(_ptr(lig_ptr), N, B, _ptr(mol['elem']), F, _ptr(zt), _ptr(mol['frag']), _ptr(mol['bonds']), _ptr(mol['order']),
                             _ptr(mol['bond_ptr']), cap_bonds, _ptr(mol['status']), int(bool(largest_only)), int(bool(with_orders)), radius,
                             nbits, _ptr(out['key']), _ptr(out['fp']), _ptr(out.get('atom_inv')), _ptr(out['status']), _stream()))
    return out

SAN_NO_MOLECULE, SAN_TOO_MANY_RINGS, SAN_COMPONENT_TOO_LARGE = 1, 2, 4      # status bits of kpd_mol_sanitize
SAN_BOND_RING, SAN_BOND_PLANAR, SAN_BOND_AROMATIC = 1, 2, 4                # bond_flags
SAN_ATOM_RING, SAN_ATOM_AROMATIC, SAN_ATOM_DONOR, SAN_ATOM_ACCEPTOR, SAN_ATOM_UNSATISFIED, SAN_ATOM_OVERVALENT = 1, 2, 4, 8, 16, 32
SAN_DESC_I = ('n_heavy', 'n_h', 'hbd', 'hba', 'n_rot', 'n_rings', 'n_arom_rings', 'n_arom_atoms', 'lipinski4', 'n_cycles')


def mol_sanitize(pos: torch.Tensor, lig_ptr: torch.Tensor, z, allowed, mass, mass_h: float, mol: dict, largest_only: bool = False):
    """Ring perception, Kekule orders, aromaticity, implicit hydrogens, validity and descriptors of a batch of perceived
    molecules on the GPU (kpd_mol_sanitize; include/kpd.h states the rule).  `mol`: what `mol_perceive` returned; z / allowed /
    mass: the atomic number, the largest allowed valence and the mass of every feature class, mass_h: the mass of hydrogen.
    Returns a dict of device tensors: order_k / bond_flags [cap_bonds], valence_k / atom_h / atom_flags [N], desc_i [B,10]
    (columns SAN_DESC_I), desc_f [B,2] float64 (mw, reserved), valid [B], status [B].  No host synchronisation."""
    pos = _dev_f32(pos, 'pos')
    B = _offsets(lig_ptr, 'lig_ptr')
    N, F = pos.shape[0], len(z)
    cap_bonds = _mol_args('mol_sanitize', mol, ('elem', 'frag', 'bonds', 'order', 'bond_ptr', 'status'), B, N)
    if pos.shape != (N, 3) or F < 1 or len(allowed) != F or len(mass) != F:
        raise KpdError(f'mol_sanitize: pos {tuple(pos.shape)} must be [N,3], and {F} atomic numbers, {len(allowed)} valences, {len(mass)} '
                       f'masses one per class')
    dev = pos.device
    table = _class_table(dev, z, allowed)
    mt = torch.tensor(list(map(float, mass)), dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = dict(order_k=i32(cap_bonds), bond_flags=i32(cap_bonds), valence_k=i32(N), atom_h=i32(N), atom_flags=i32(N), desc_i=i32(B, 10),
               desc_f=torch.empty(B, 2, dtype=torch.float64, device=dev), valid=i32(B), status=i32(B))
    check(lib().kpd_mol_sanitize(_ptr(pos), _ptr(lig_ptr), N, B, _ptr(mol['elem']), F, _ptr(table[0]), _ptr(table[1]), _ptr(mt), float(mass_h),
                                 _ptr(mol['frag']), _ptr(mol['bonds']), _ptr(mol['order']), _ptr(mol['bond_ptr']), cap_bonds,
                                 _ptr(mol['status']), int(bool(largest_only)),
                                 *[_ptr(out[k]) for k in ('order_k', 'bond_flags', 'valence_k', 'atom_h', 'atom_flags', 'desc_i', 'desc_f',
                                                          'valid', 'status')], _stream()))
    return out


HS_NO_MOLECULE, HS_TOO_MANY_ATOMS, HS_NO_ROOM, HS_GENERAL, HS_NONFINITE = 1, 2, 4, 8, 16       # status bits of kpd_mol_add_hs


def mol_add_hs(pos: torch.Tensor, lig_ptr: torch.Tensor, z, allowed, h_class: int, mol: dict, san: dict, largest_only: bool = False):
    """Explicit hydrogens with coordinates on a batch of sanitised molecules on the GPU (kpd_mol_add_hs; include/kpd.h states the
    placement rule).  `mol`: what `mol_perceive` returned, `san`: what `mol_sanitize` returned for it with the same
    `largest_only`; z / allowed: the atomic number and the largest allowed valence of every class, `h_class`: the class the new
    atoms get (z[h_class] must be 1).  The outputs are sized from one device sum of atom_h, the only host synchronisation of this function.  Returns a dict of device tensors in the layout of `mol_perceive` -- lig_ptr [B+1],
    pos [cap_atoms,3], elem / valence / frag [cap_atoms], bonds [cap_bonds,2], order [cap_bonds], bond_ptr [B+1], summary [B,4]
    -- and parent / source [cap_atoms], n_h [B], status [B] (bits HS_*)."""
    pos = _dev_f32(pos, 'pos')
    B = _offsets(lig_ptr, 'lig_ptr')
    N, F = pos.shape[0], len(z)
    cap_in = _mol_args('mol_add_hs', mol, ('elem', 'frag', 'bonds', 'bond_ptr', 'status'), B, N,
                       san, ('order_k', 'valence_k', 'atom_h', 'atom_flags', 'status'))
    if pos.shape != (N, 3) or F < 1 or len(allowed) != F:
        raise KpdError(f'mol_add_hs: pos {tuple(pos.shape)} must be [N,3], and {F} atomic numbers, {len(allowed)} valences one per class')
    h_class = int(h_class)
    if not (0 <= h_class < F and int(z[h_class]) == 1):
        raise KpdError(f'mol_add_hs: h_class {h_class} must name a class of atomic number 1')
    dev = pos.device
    n_h = int(san['atom_h'].clamp(min=0).sum().item()) if N else 0          # an upper bound: ligands copied through add none
    cap_atoms, cap_bonds = N + n_h, cap_in + n_h
    table = _class_table(dev, z, allowed)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = dict(lig_ptr=i32(B + 1), pos=torch.empty(cap_atoms, 3, dtype=torch.float32, device=dev), elem=i32(cap_atoms),
               valence=i32(cap_atoms), frag=i32(cap_atoms), bonds=i32(cap_bonds, 2), order=i32(cap_bonds), bond_ptr=i32(B + 1),
               summary=i32(B, 4), parent=i32(cap_atoms), source=i32(cap_atoms), n_h=i32(B), status=i32(B))
    scratch = torch.empty(int(lib().kpd_mol_add_hs_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    check(lib().kpd_mol_add_hs(_ptr(pos), _ptr(lig_ptr), N, B, _ptr(mol['elem']), F, _ptr(table[0]), _ptr(table[1]), _ptr(mol['frag']),
                               _ptr(mol['bonds']), _ptr(san['order_k']), _ptr(mol['bond_ptr']), cap_in, _ptr(mol['status']),
                               _ptr(san['status']), _ptr(san['valence_k']), _ptr(san['atom_h']), _ptr(san['atom_flags']),
                               int(bool(largest_only)), h_class, cap_atoms, cap_bonds,
                               *[_ptr(out[k]) for k in ('lig_ptr', 'pos', 'elem', 'valence', 'frag', 'bonds', 'order', 'bond_ptr', 'summary',
                                                        'parent', 'source', 'n_h', 'status')], _ptr(scratch), _stream()))
    return out


SMI_NO_MOLECULE, SMI_EXHAUSTED, SMI_CAPACITY = 1, 2, 4        # status bits of kpd_mol_smiles


def mol_smiles(lig_ptr: torch.Tensor, z, elements, mol: dict, san: dict, largest_only: bool = False, aromatic: bool = True,
               capacity: Optional[int] = None):
    """Canonical SMILES of a batch of sanitised molecules on the GPU (kpd_mol_smiles; include/kpd.h states the rule, which is NOT
    RDKit's).  `mol`: what `mol_perceive` returned, `san`: what `mol_sanitize` returned for it with the same `largest_only` (or over every
    atom); z / elements: the atomic number and the symbol (at most four characters) of every class; `aromatic=False`: the Kekule form.
    Returns (text bytes, text_ptr list of B + 1 offsets, status list of B); ligand b's string is text[text_ptr[b]:text_ptr[b + 1]],
    empty when its status has bit SMI_NO_MOLECULE or SMI_EXHAUSTED.  The buffer is sized at 8 bytes per atom and the call is
    repeated once with the size the first one reports if that was too small (`capacity`: the first size); the host
    synchronisations are the copies of the offsets and of the finished text."""
    B = _offsets(lig_ptr, 'lig_ptr')
    N, F = _numel(mol.get('elem')), len(z)
    cap_bonds = _mol_args('mol_smiles', mol, ('elem', 'frag', 'bonds', 'bond_ptr', 'status'), B, N,
                          san, ('order_k', 'bond_flags', 'atom_h', 'atom_flags', 'status'))
    if F < 1 or len(elements) != F:
        raise KpdError(f'mol_smiles: {F} atomic numbers and {len(elements)} element symbols must be one per class')
    dev = lig_ptr.device
    zt = _class_table(dev, z)
    symbols = _packed_symbols(elements, dev)
    text_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib().kpd_smiles_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    cap = 8 * N + 16 if capacity is None else int(capacity)
    for attempt in range(2):
        text = torch.empty(cap, dtype=torch.uint8, device=dev)
        check(lib().kpd_mol_smiles(_ptr(lig_ptr), N, B, _ptr(mol['elem']), F, _ptr(zt), _ptr(symbols), _ptr(mol['frag']), _ptr(mol['bonds']),
                                   _ptr(san['order_k']), _ptr(san['bond_flags']), _ptr(mol['bond_ptr']), cap_bonds, _ptr(mol['status']),
                                   _ptr(san['status']), _ptr(san['atom_h']), _ptr(san['atom_flags']), int(bool(largest_only)),
                                   int(bool(aromatic)), _ptr(text), cap, _ptr(text_ptr), _ptr(status), _ptr(scratch), _stream()))
        ptr = text_ptr.cpu().tolist()
        if ptr[-1] <= cap:
            break
        cap = ptr[-1]                               # the size needed: the second call cannot miss
    return bytes(text[:min(ptr[-1], cap)].cpu().numpy()), ptr, status.cpu().tolist()


POSE_NO_MOLECULE, POSE_MAX_NODES, POSE_NONFINITE = 1, 2, 4      # status bits of kpd_pose_rmsd
POSE_MAX_PAIR_POSES = 64


def pose_rmsd(lig_ptr: torch.Tensor, z, mol: dict, pos: torch.Tensor, ref_pos: Optional[torch.Tensor] = None, pairs: bool = False,
              largest_only: bool = False, skip_h: bool = True, max_nodes: int = 65536, bond_label: Optional[torch.Tensor] = None,
              atom_label: Optional[torch.Tensor] = None, want_map: bool = True):
    """Symmetry-corrected RMSD between poses of a batch of perceived molecules on the GPU (kpd_pose_rmsd; include/kpd.h states the
    rule): the minimum over the automorphisms of the bond graph of the unaligned RMSD.  `mol`: what `mol_perceive` returned, z: the
    atomic number of every feature class; pos [K,N,3]: K poses of the whole batch; `pairs=False`: every pose against `ref_pos`
    [N,3], `pairs=True` (K <= 64): every pose against every other; bond_label [cap_bonds] (1 .. 15) / atom_label [N] (0 .. 2^20 - 1):
    int32 labels an automorphism must keep, None: connectivity and elements alone.  Returns a dict of device tensors: rmsd / plain
    float64 and nodes int64, [B,K] or [B,K,K]; map [K,N] int32 (pairs=False and `want_map`); status [B] (bits POSE_*).  No host
    synchronisation."""
    B = _offsets(lig_ptr, 'lig_ptr')
    if not (isinstance(pos, torch.Tensor) and pos.dim() == 3 and pos.shape[2] == 3):
        raise KpdError(f'pose_rmsd: pos must be [K,N,3], got {tuple(getattr(pos, "shape", ()))}')
    pos = _dev_f32(pos, 'pos')
    K, N, F = pos.shape[0], pos.shape[1], len(z)
    pairs, max_nodes = bool(pairs), int(max_nodes)
    if K < 1 or F < 1 or (pairs and K > POSE_MAX_PAIR_POSES) or max_nodes < 1:
        raise KpdError(f'pose_rmsd: K={K} must be >= 1 (<= {POSE_MAX_PAIR_POSES} with pairs), max_nodes={max_nodes} >= 1, and there must '
                       f'be atomic numbers (got {F})')
    cap_bonds = _mol_args('pose_rmsd', mol, ('elem', 'frag', 'bonds', 'bond_ptr', 'status'), B, N)
    if not pairs:
        if ref_pos is None:
            raise KpdError('pose_rmsd: ref_pos is needed unless pairs=True')
        ref_pos = _dev_f32(ref_pos, 'ref_pos')
        if ref_pos.shape != (N, 3):
            raise KpdError(f'pose_rmsd: ref_pos must be [{N},3], got {tuple(ref_pos.shape)}')
    if bond_label is not None:
        bond_label = _per_entry(bond_label, 'bond_label', cap_bonds, 'bond row')
    if atom_label is not None:
        atom_label = _per_entry(atom_label, 'atom_label', N, 'atom')
    dev = pos.device
    zt = _class_table(dev, z)
    shape = (B, K, K) if pairs else (B, K)
    out = dict(rmsd=torch.empty(shape, dtype=torch.float64, device=dev), plain=torch.empty(shape, dtype=torch.float64, device=dev),
               nodes=torch.empty(shape, dtype=torch.int64, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev))
    if not pairs and want_map:
        out['map'] = torch.empty(K, N, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib().kpd_pose_rmsd_scratch_bytes(N, K, int(pairs))), dtype=torch.uint8, device=dev)
    check(lib().kpd_pose_rmsd(_ptr(lig_ptr), N, B, _ptr(mol['elem']), F, _ptr(zt), _ptr(mol['frag']), _ptr(mol['bonds']), _ptr(mol['bond_ptr']),
                              cap_bonds, _ptr(mol['status']), _ptr(bond_label), _ptr(atom_label), int(bool(largest_only)), int(bool(skip_h)),
                              None if pairs else _ptr(ref_pos), _ptr(pos), K, int(pairs), max_nodes, _ptr(out['rmsd']), _ptr(out['plain']),
                              _ptr(out.get('map')), _ptr(out['nodes']), _ptr(out['status']), _ptr(scratch), _stream()))
    return out


MATCH_NO_MOLECULE, MATCH_MAX_NODES = 1, 2                       # status bits of kpd_mol_match
MATCH_ANCHORS, MATCH_ALL = 0, 1                                 # its modes
MATCH_Q_ATOMS = 16                                              # KPD_Q_ATOMS: the columns of first_map


def mol_match(lig_ptr: torch.Tensor, z, mol: dict, san: dict, patterns, mode: int = MATCH_ANCHORS, max_nodes: int = 65536,
              want_map: bool = True, type_group=None, value=None, largest_only: bool = False):
    """Substructure search on a batch of sanitised molecules on the GPU (kpd_mol_match; include/kpd.h states the rule, which is NOT
    RDKit's matcher).  `mol`: what `mol_perceive` returned, `san`: what `mol_sanitize` returned for it with the same `largest_only` (or
    over every atom); z: the atomic number of every class; `patterns`: a `smarts.Patterns` (its table is checked on the host and
    read on the GPU; its rows lifted out of "$(...)" are rows of the outputs like any other).  mode MATCH_ANCHORS: every search
    stops at its first embedding; MATCH_ALL: all embeddings are counted (n_embed, cover).  type_group [P] (-1: no part in a typing,
    else the group) and value [P]: a first-match-wins typing table, host sequences or tensors.  Returns a dict of device tensors:
    anchor [N,W] (int32 words holding the uint32 bits, W = ceil(P / 32)), hits [B,P], status [B] (bits MATCH_*); first_map [B,P,16]
    with `want_map`; n_embed [B,P] int64 and cover [N,W] with MATCH_ALL; atom_type [G,N], type_sum [B,G] float64 and untyped [B,G]
    with a typing table.  No host synchronisation once the table is on the device (a typing table given as host data is copied)."""
    B = _offsets(lig_ptr, 'lig_ptr')
    N, F = _numel(mol.get('elem')), len(z)
    cap_bonds = _mol_args('mol_match', mol, ('elem', 'frag', 'bonds', 'bond_ptr', 'status'), B, N,
                          san, ('order_k', 'bond_flags', 'valence_k', 'atom_h', 'atom_flags', 'status'))
    mode, max_nodes = int(mode), int(max_nodes)
    if F < 1 or mode not in (MATCH_ANCHORS, MATCH_ALL) or max_nodes < 1:
        raise KpdError(f'mol_match: mode={mode} must be MATCH_ANCHORS or MATCH_ALL, max_nodes={max_nodes} >= 1, and there must be atomic '
                       f'numbers (got {F})')
    dev = lig_ptr.device
    host = patterns.host
    table = patterns.to(dev).table
    P = patterns.n_rows
    W = (P + 31) // 32
    G, tg, val = 0, None, None
    if type_group is not None:
        tg_host = torch.as_tensor(type_group).to('cpu', torch.int32).contiguous()
        if value is None or tg_host.numel() != P or _numel(torch.as_tensor(value)) != P:
            raise KpdError(f'mol_match: type_group and value must have one entry per row of the table ({P})')
        G = max(int(tg_host.max()) + 1, 0)
        tg, val = tg_host.to(dev), torch.as_tensor(value).to(dev, torch.float64).contiguous()
    zt = _class_table(dev, z)
    out = dict(anchor=torch.empty(N, W, dtype=torch.int32, device=dev), hits=torch.empty(B, P, dtype=torch.int32, device=dev),
               status=torch.empty(B, dtype=torch.int32, device=dev))
    if want_map:
        out['first_map'] = torch.empty(B, P, MATCH_Q_ATOMS, dtype=torch.int32, device=dev)
    if mode == MATCH_ALL:
        out['n_embed'] = torch.empty(B, P, dtype=torch.int64, device=dev)
        out['cover'] = torch.empty(N, W, dtype=torch.int32, device=dev)
    if G:
        out.update(atom_type=torch.empty(G, N, dtype=torch.int32, device=dev), type_sum=torch.empty(B, G, dtype=torch.float64, device=dev),
                   untyped=torch.empty(B, G, dtype=torch.int32, device=dev))
    check(lib().kpd_mol_match(_ptr(lig_ptr), N, B, _ptr(mol['elem']), F, _ptr(zt), _ptr(mol['frag']), _ptr(mol['bonds']), _ptr(san['order_k']),
                              _ptr(san['bond_flags']), _ptr(mol['bond_ptr']), cap_bonds, _ptr(mol['status']), _ptr(san['status']),
                              _ptr(san['valence_k']), _ptr(san['atom_h']), _ptr(san['atom_flags']), int(bool(largest_only)), _ptr(host),
                              _ptr(table), host.numel(), mode, max_nodes, _ptr(tg), _ptr(val), G, _ptr(out['anchor']), _ptr(out['hits']),
                              _ptr(out.get('first_map')), _ptr(out.get('n_embed')), _ptr(out.get('cover')), _ptr(out.get('atom_type')),
                              _ptr(out.get('type_sum')), _ptr(out.get('untyped')), _ptr(out['status']), _stream()))
    return out


CHECK_NO_MOLECULE, CHECK_BAD_INPUT, CHECK_ATOM_OUT = 1, 2, 4     # status bits of kpd_pose_check
CHECK_FAIL = ('bond', 'angle', 'clash', 'ring', 'centre', 'twist', 'pocket', 'overlap')       # bit k of `fail` and `atom_fail`
CHECK_REPORT = ('bond_min', 'bond_max', 'angle_min', 'angle_max', 'clash_min', 'ring_max', 'centre_max', 'twist_min', 'pocket_min', 'overlap')
CHECK_COUNTS = ('bonds', 'bonds_fail', 'angles', 'angles_fail', 'pairs', 'pairs_fail', 'rings', 'rings_fail', 'centres', 'centres_fail',
                'torsions', 'torsions_fail', 'torsions_skipped', 'pocket_pairs', 'pocket_pairs_fail', 'n_lig_points', 'n_overlap_points')
CHECK_MAX_RADIUS = 8.0


def pose_check_params(**params) -> KpdPoseCheckParams:
    """The thresholds of kpd_pose_check: the library's defaults (kpd_pose_check_defaults: PoseBusters' published thresholds as
    recalled, not checked against the paper) with the given fields replaced."""
    p, names = _struct_params('pose_check', KpdPoseCheckParams, lib().kpd_pose_check_defaults, params)
    if not (all(0 <= getattr(p, k) <= 1e6 for k in names) and 0.1 <= p.h <= 4 and p.pocket_scale <= 4 and p.bond_lo <= p.bond_hi and
            p.angle_lo <= p.angle_hi):
        raise KpdError('pose_check: ' + ', '.join(f'{k} {getattr(p, k)}' for k in names) + ': every threshold must be in 0 .. 1e6, '
                       'h in 0.1 .. 4, pocket_scale at most 4, and the lower bounds not above the upper ones')
    return p


def pose_check(lig_ptr: torch.Tensor, z, mol: dict, san: dict, pos: torch.Tensor, lig_radius: torch.Tensor,
               pocket_x: Optional[torch.Tensor] = None, pocket_radius: Optional[torch.Tensor] = None, pocket_ptr: Optional[torch.Tensor] = None,
               pocket_of: Optional[torch.Tensor] = None, largest_only: bool = False, max_atoms: int = MOL_MAX_ATOMS,
               max_pocket: Optional[int] = None, **params):
    """Plausibility checks of K poses of a batch of sanitised molecules on the GPU (kpd_pose_check; include/kpd.h states every
    check: bond lengths, 1-3 distances, internal clash, flat aromatic rings, planar centres and double bonds, pocket clash and
    volume overlap; NOT PoseBusters' numbers).  `mol`: what `mol_perceive` returned, `san`: what `mol_sanitize` returned for it;
    z: the atomic number of every class; pos [K,N,3] (or [N,3]) fp32; lig_radius [F] fp32 van der Waals radii (not > 0: the class
    takes no part in the clash and overlap checks); pocket_x [M,3], pocket_radius [M] fp32, pocket_ptr [P+1] and pocket_of [B]
    int32 (-1: no pocket), all four None for no pockets at all; all GPU tensors.  `params`: the thresholds of `pose_check_params`.
    Returns a dict of device tensors: fail [B,K] int32 (bit k: CHECK_FAIL[k]), report [B,K,10] float64 (CHECK_REPORT), counts
    [B,K,17] int32 (CHECK_COUNTS), atom_fail [K,N] int32, status [B,K] int32 (bits CHECK_*).  No host synchronisation."""
    if pocket_x is None:
        if not (pocket_radius is None and pocket_ptr is None and pocket_of is None):
            raise KpdError('pose_check: pocket_radius, pocket_ptr and pocket_of need pocket_x')
        B, dev = _offsets(lig_ptr, 'lig_ptr'), lig_ptr.device
        pocket_x, pocket_radius = torch.zeros(0, 3, device=dev), torch.zeros(0, device=dev)
        pocket_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
        pocket_of = torch.full((B,), -1, dtype=torch.int32, device=dev)
    pos, pocket_x, pocket_of, B, N, F, M, P, cap_bonds, zt, max_atoms, max_pocket = _ligand_pocket_args(
        'pose_check', pos, lig_ptr, z, mol, ('elem', 'frag', 'bonds', 'bond_ptr', 'status'), pocket_x, pocket_ptr, pocket_of, max_atoms,
        max_pocket, san, ('order_k', 'bond_flags', 'atom_h', 'atom_flags', 'status'), stack=True)
    K, dev = pos.shape[0], pos.device
    lig_radius, pocket_radius = _dev_f32(lig_radius, 'lig_radius'), _dev_f32(pocket_radius, 'pocket_radius')
    if lig_radius.shape != (F,) or pocket_radius.shape != (M,):
        raise KpdError(f'pose_check: lig_radius {tuple(lig_radius.shape)} must be [{F}] and pocket_radius {tuple(pocket_radius.shape)} [{M}]')
    p = pose_check_params(**params)
    out = dict(fail=torch.empty(B, K, dtype=torch.int32, device=dev), report=torch.empty(B, K, len(CHECK_REPORT), dtype=torch.float64, device=dev),
               counts=torch.empty(B, K, len(CHECK_COUNTS), dtype=torch.int32, device=dev),
               atom_fail=torch.empty(K, N, dtype=torch.int32, device=dev), status=torch.empty(B, K, dtype=torch.int32, device=dev))
    check(lib().kpd_pose_check(_ptr(lig_ptr), N, B, max_atoms, _ptr(mol['elem']), F, _ptr(zt), _ptr(mol['frag']), _ptr(mol['bonds']),
                               _ptr(san['order_k']), _ptr(san['bond_flags']), _ptr(mol['bond_ptr']), cap_bonds, _ptr(mol['status']),
                               _ptr(san['status']), _ptr(san['atom_h']), _ptr(san['atom_flags']), int(bool(largest_only)), _ptr(pos), K,
                               _ptr(lig_radius), _ptr(pocket_x), _ptr(pocket_radius), _ptr(pocket_ptr), M, P,
                               max_pocket, _ptr(pocket_of), C.byref(p), _ptr(out['fail']),
                               _ptr(out['report']), _ptr(out['counts']), _ptr(out['atom_fail']), _ptr(out['status']), _stream()))
    return out


def fp_diversity(fp: torch.Tensor, use: torch.Tensor, group_ptr: torch.Tensor):
    """Sum of the Tanimoto distances over the pairs of used ligands of every group on the GPU (kpd_fp_diversity).
    fp [B,W] int32 GPU tensor (fingerprint rows), use [B] bool / uint8, group_ptr [G+1] int32 GPU tensor.  Returns device
    tensors (div_sum [G] float64, n_pairs [G] int64, status [G]: bit 0 = malformed segment).  No host synchronisation."""
    if not (fp.is_cuda and fp.dtype == torch.int32 and fp.dim() == 2 and fp.shape[1] >= 1 and fp.is_contiguous()):
        raise KpdError('fp_diversity: fp must be a contiguous int32 GPU tensor [B, W]')
    G = _offsets(group_ptr, 'fp_diversity: group_ptr', 'G')
    B, W = fp.shape
    if not (use.is_cuda and use.dtype in (torch.bool, torch.uint8) and use.shape == (B,)):
        raise KpdError(f'fp_diversity: use must be a bool or uint8 GPU tensor of {B} entries')
    use = use.contiguous().view(torch.uint8)
    dev = fp.device
    div_sum = torch.empty(G, dtype=torch.float64, device=dev)
    n_pairs = torch.empty(G, dtype=torch.int64, device=dev)
    status = torch.empty(G, dtype=torch.int32, device=dev)
    check(lib().kpd_fp_diversity(_ptr(fp), _ptr(use), B, W, _ptr(group_ptr), G, _ptr(div_sum), _ptr(n_pairs), _ptr(status), _stream()))
    return div_sum, n_pairs, status


RELAX_NO_MOLECULE, RELAX_BAD_INPUT, RELAX_ITER_CAP, RELAX_LINE_SEARCH = 1, 2, 4, 8      # status bits of kpd_relax
RELAX_REPORT = ('E_before', 'E_after', 'rmsd', 'gmax_after', 'iterations', 'evaluations', 'E_bond', 'E_angle', 'E_intra', 'E_pocket',
                'E_pocket_before', 'gmax_before')


def _struct_params(where: str, Struct, defaults_fn, params: dict, ints=()):
    """A `Struct` with the library's defaults (`defaults_fn`) and the fields named in `params` replaced (`ints`: the integer
    ones); an unknown name raises.  Returns the struct and its field names."""
    p = Struct()
    defaults_fn(C.byref(p))
    names = [f[0] for f in Struct._fields_]
    for k, v in params.items():
        if k not in names:
            raise KpdError(f'{where}: unknown parameter {k!r} (known: {sorted(names)})')
        setattr(p, k, int(v) if k in ints else float(v))
    return p, names


def _ligand_pocket_args(where: str, pos, lig_ptr, z, mol: dict, fields, pocket_x, pocket_ptr, pocket_of, max_atoms, max_pocket,
                        san: Optional[dict] = None, san_fields=(), stack: bool = False):
    """What `relax`, the vina calls and `pose_check` share: perceived ligands (the `fields` of `mol`, the `san_fields` of `san`: see
    `_mol_args`) and their pockets as the library takes them; M = 0 atoms in P = 0 pockets with every pocket_of -1 is no pocket at
    all.  `stack`: pos is K poses [K,N,3], or one as [N,3], and is returned as [K,N,3]; else it must be [N,3].  Returns pos,
    pocket_x and pocket_of normalised, B, N, F, M, P, cap_bonds, zt (z on the device), max_atoms and max_pocket (M if None)."""
    if not (isinstance(pos, torch.Tensor) and pos.dim() in ((2, 3) if stack else (2,)) and pos.shape[-1] == 3):
        raise KpdError(f'{where}: pos must be {"[K,N,3] or " if stack else ""}[N,3], got {tuple(getattr(pos, "shape", ()))}')
    pos = _dev_f32(pos[None] if stack and pos.dim() == 2 else pos, 'pos')
    B = _offsets(lig_ptr, 'lig_ptr')
    N, F = pos.shape[-2], len(z)
    cap_bonds = _mol_args(where, mol, fields, B, N, san, san_fields)
    P = _offsets(pocket_ptr, f'{where}: pocket_ptr', 'P')
    pocket_of = _per_entry(pocket_of, f'{where}: pocket_of', B, 'ligand', contiguous=True)
    pocket_x = _dev_f32(pocket_x, 'pocket_x')
    M, max_atoms = pocket_x.shape[0], int(max_atoms)
    if (stack and pos.shape[0] < 1) or F < 1 or pocket_x.shape != (M, 3) or not 1 <= max_atoms <= MOL_MAX_ATOMS:
        raise KpdError(f'{where}: pos {tuple(pos.shape)} must hold at least one pose, z at least one class (got {F}), pocket_x '
                       f'{tuple(pocket_x.shape)} be [M,3] and max_atoms {max_atoms} be 1 .. {MOL_MAX_ATOMS}')
    return (pos, pocket_x, pocket_of, B, N, F, M, P, cap_bonds, _class_table(pos.device, z), max_atoms,
            M if max_pocket is None else int(max_pocket))


def relax_params(**params) -> KpdRelaxParams:
    """The parameters of kpd_relax: the library's defaults (kpd_relax_defaults) with the given fields replaced."""
    p, _ = _struct_params('relax', KpdRelaxParams, lib().kpd_relax_defaults, params, ints=('max_iters',))
    if not (p.k_b >= 0 and p.k_a >= 0 and p.r_c > 0 and 0 < p.s < 1 and p.w_intra >= 0 and p.gtol >= 0 and p.max_step > 0 and
            p.max_iters >= 0):
        raise KpdError(f'relax: k_b {p.k_b}, k_a {p.k_a}, w_intra {p.w_intra}, gtol {p.gtol} must be >= 0, r_c {p.r_c} and max_step '
                       f'{p.max_step} > 0, s {p.s} in (0, 1), max_iters {p.max_iters} >= 0')
    return p


def relax(pos: torch.Tensor, lig_ptr: torch.Tensor, z, lig_vdw: torch.Tensor, mol: dict, pocket_x: torch.Tensor, pocket_vdw: torch.Tensor,
          pocket_ptr: torch.Tensor, pocket_of: torch.Tensor, max_atoms: int = MOL_MAX_ATOMS, max_pocket: Optional[int] = None, **params):
    """Relax a batch of perceived ligands inside their rigid pockets on the GPU (kpd_relax; include/kpd.h states the force field
    and the minimiser: this library's own, NOT UFF).  pos [N,3] fp32, lig_ptr [B+1] int32, z: the atomic number of every feature
    class, lig_vdw [F,2] fp32 {x, D} per class, `mol`: what `mol_perceive` returned, pocket_x [M,3], pocket_vdw [M,2] fp32,
    pocket_ptr [P+1] and pocket_of [B] int32 (-1: no pocket); all GPU tensors.  max_atoms / max_pocket: host-known upper bounds
    that size the kernel's LDS (a larger ligand is left out, a larger pocket is merely read from global memory).  Returns
    (pos_out [N,3] fp32, report [B,12] float64 with the columns RELAX_REPORT, status [B] int32).  No host synchronisation."""
    pos, pocket_x, pocket_of, B, N, F, M, P, cap_bonds, zt, max_atoms, max_pocket = _ligand_pocket_args(
        'relax', pos, lig_ptr, z, mol, ('elem', 'bonds', 'bond_ptr', 'status'), pocket_x, pocket_ptr, pocket_of, max_atoms, max_pocket)
    lig_vdw, pocket_vdw = _dev_f32(lig_vdw, 'lig_vdw'), _dev_f32(pocket_vdw, 'pocket_vdw')
    if lig_vdw.shape != (F, 2) or pocket_vdw.shape != (M, 2):
        raise KpdError(f'relax: lig_vdw {tuple(lig_vdw.shape)} must be [{F},2] and pocket_vdw {tuple(pocket_vdw.shape)} [{M},2]')
    p = relax_params(**params)
    dev = pos.device
    pos_out = torch.empty_like(pos)
    report = torch.empty(B, 12, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().kpd_relax(_ptr(pos), _ptr(lig_ptr), N, B, max_atoms, _ptr(mol['elem']), F, _ptr(zt), _ptr(lig_vdw), _ptr(mol['bonds']),
                          _ptr(mol['bond_ptr']), cap_bonds, _ptr(mol['status']), _ptr(pocket_x), _ptr(pocket_vdw), _ptr(pocket_ptr), M, P,
                          max_pocket, _ptr(pocket_of), C.byref(p), _ptr(pos_out), _ptr(report), _ptr(status), _stream()))
    return pos_out, report, status


VINA_NO_MOLECULE, VINA_BAD_INPUT, VINA_ATOM_OUT = 1, 2, 4       # status bits of kpd_vina_score
VINA_POCKET_BAD_SEGMENT, VINA_POCKET_NONFINITE = 1, 2           # status bits of kpd_vina_pocket_types
VINA_H, VINA_D, VINA_A = 1, 2, 4                                # type flags: hydrophobic, hydrogen-bond donor, acceptor
VINA_REPORT = ('score', 'inter', 'gauss1', 'gauss2', 'repulsion', 'hydrophobic', 'hbond', 'n_rot')


def vina_params(**params) -> KpdVinaParams:
    """The parameters of kpd_vina_score: the library's defaults (kpd_vina_defaults: Vina's published weights as recalled, not
    checked against the paper or Vina's source) with the given fields replaced."""
    p, names = _struct_params('vina', KpdVinaParams, lib().kpd_vina_defaults, params)
    if not (all(abs(getattr(p, k)) < 1e12 for k in names) and 0 < p.r_c < 1e6 and p.w_rot >= 0):
        raise KpdError('vina: ' + ', '.join(f'{k} {getattr(p, k)}' for k in names) + ': the weights must be finite, w_rot >= 0, r_c > 0')
    return p


def vina_pocket_types(pocket_x: torch.Tensor, pocket_z: torch.Tensor, pocket_ptr: torch.Tensor):
    """The H / D / A flags of every pocket atom on the GPU (kpd_vina_pocket_types; include/kpd.h states the rule, this library's
    own).  pocket_x [M,3] fp32, pocket_z [M] int32 atomic numbers, pocket_ptr [P+1] int32; all GPU tensors.  Returns
    (pocket_type [M] int32, -1 for an atom that takes no part; status [P] int32: bit 0 malformed segment, bit 1 a non-finite
    coordinate).  Quadratic per pocket; done once per pocket set.  No host synchronisation."""
    pocket_x = _dev_f32(pocket_x, 'pocket_x')
    P = _offsets(pocket_ptr, 'vina_pocket_types: pocket_ptr', 'P')
    M = pocket_x.shape[0]
    pocket_z = _per_entry(pocket_z, 'vina_pocket_types: pocket_z', M, 'pocket atom')
    if pocket_x.shape != (M, 3):
        raise KpdError(f'vina_pocket_types: pocket_x {tuple(pocket_x.shape)} must be [M,3]')
    types = torch.empty(M, dtype=torch.int32, device=pocket_x.device)
    status = torch.empty(P, dtype=torch.int32, device=pocket_x.device)
    check(lib().kpd_vina_pocket_types(_ptr(pocket_x), _ptr(pocket_z), _ptr(pocket_ptr), M, P, _ptr(types), _ptr(status), _stream()))
    return types, status


def vina_score(pos: torch.Tensor, lig_ptr: torch.Tensor, z, lig_radius: torch.Tensor, mol: dict, pocket_x: torch.Tensor,
               pocket_radius: torch.Tensor, pocket_type: torch.Tensor, pocket_ptr: torch.Tensor, pocket_of: torch.Tensor,
               lig_type_in: Optional[torch.Tensor] = None, grad: bool = False, atom_score: bool = False, max_atoms: int = MOL_MAX_ATOMS,
               max_pocket: Optional[int] = None, **params):
    """Score a batch of perceived ligands in their rigid pockets on the GPU (kpd_vina_score; include/kpd.h states the function:
    the Vina functional form with a typing rule of this library's own, NOT gnina's or Vina's numbers).  pos [N,3] fp32, lig_ptr
    [B+1] int32, z: the atomic number of every feature class, lig_radius [F] fp32, `mol`: what `mol_perceive` returned, pocket_x
    [M,3], pocket_radius [M] fp32, pocket_type [M] int32 (from `vina_pocket_types` or the caller), pocket_ptr [P+1] and pocket_of
    [B] int32 (-1: no pocket), lig_type_in: None or [N] int32 whose entries >= 0 replace the perceived flags; all GPU tensors.
    Returns a dict of device tensors: report [B,8] float64 (columns VINA_REPORT), status [B], lig_type [N] and, on request, grad
    [N,3] and atom_score [N] float64.  No host synchronisation."""
    pos, pocket_x, pocket_of, B, N, F, M, P, cap_bonds, zt, max_atoms, max_pocket = _ligand_pocket_args(
        'vina_score', pos, lig_ptr, z, mol, ('elem', 'bonds', 'order', 'bond_ptr', 'status'), pocket_x, pocket_ptr, pocket_of, max_atoms,
        max_pocket)
    lig_radius, pocket_radius = _dev_f32(lig_radius, 'lig_radius'), _dev_f32(pocket_radius, 'pocket_radius')
    pocket_type = _per_entry(pocket_type, 'vina_score: pocket_type', M, 'pocket atom')
    if lig_type_in is not None:
        lig_type_in = _per_entry(lig_type_in, 'vina_score: lig_type_in', N, 'ligand atom')
    if lig_radius.shape != (F,) or pocket_radius.shape != (M,):
        raise KpdError(f'vina_score: lig_radius {tuple(lig_radius.shape)} must be [{F}] and pocket_radius {tuple(pocket_radius.shape)} [{M}]')
    p = vina_params(**params)
    dev = pos.device
    out = dict(report=torch.empty(B, 8, dtype=torch.float64, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev),
               lig_type=torch.empty(N, dtype=torch.int32, device=dev))
    if grad:
        out['grad'] = torch.empty(N, 3, dtype=torch.float64, device=dev)
    if atom_score:
        out['atom_score'] = torch.empty(N, dtype=torch.float64, device=dev)
    check(lib().kpd_vina_score(_ptr(pos), _ptr(lig_ptr), N, B, max_atoms, _ptr(mol['elem']), F, _ptr(zt), _ptr(lig_radius), _ptr(mol['bonds']),
                               _ptr(mol['order']), _ptr(mol['bond_ptr']), cap_bonds, _ptr(mol['status']), _ptr(lig_type_in), _ptr(pocket_x),
                               _ptr(pocket_radius), _ptr(pocket_type), _ptr(pocket_ptr), M, P, max_pocket, _ptr(pocket_of), C.byref(p),
                               _ptr(out['report']), _ptr(out.get('grad')), _ptr(out.get('atom_score')), _ptr(out['lig_type']),
                               _ptr(out['status']), _stream()))
    return out


# status bits of kpd_vina_minimize (bits 0 .. 2 as for kpd_vina_score)
VINA_MIN_NO_MOLECULE, VINA_MIN_BAD_INPUT, VINA_MIN_ATOM_OUT, VINA_MIN_LINE_SEARCH = 1, 2, 4, 8
VINA_MIN_FROZEN_ROTORS, VINA_MIN_FRAGMENTS, VINA_MIN_ITER_CAP = 16, 32, 64
VINA_MIN_REPORT = ('score_before', 'score_after', 'E_before', 'E_after', 'inter_before', 'inter_after', 'intra_before', 'intra_after',
                   'rmsd', 'gnorm_before', 'gnorm_after', 'iterations', 'evaluations', 'n_rot', 'n_active', 'n_frag')
VINA_MIN_MAX_ROTORS = 64


def vina_min_params(**params) -> KpdVinaMinParams:
    """The parameters of kpd_vina_minimize: the library's defaults (kpd_vina_min_defaults: those of kpd_vina_score, w_intra 1,
    gtol 1e-3, max_step 0.2, max_iters 200) with the given fields replaced."""
    p, names = _struct_params('vina_minimize', KpdVinaMinParams, lib().kpd_vina_min_defaults, params, ints=('max_iters',))
    if not (all(abs(getattr(p, k)) < 1e12 for k in names) and 0 < p.r_c < 1e6 and p.w_rot >= 0 and p.w_intra >= 0 and p.gtol >= 0 and
            p.max_step > 0 and p.max_iters >= 0):
        raise KpdError('vina_minimize: ' + ', '.join(f'{k} {getattr(p, k)}' for k in names) +
                       ': the weights must be finite, w_rot, w_intra, gtol and max_iters >= 0, r_c and max_step > 0')
    return p


def vina_minimize(pos: torch.Tensor, lig_ptr: torch.Tensor, z, lig_radius: torch.Tensor, mol: dict, pocket_x: torch.Tensor,
                  pocket_radius: torch.Tensor, pocket_type: torch.Tensor, pocket_ptr: torch.Tensor, pocket_of: torch.Tensor,
                  lig_type_in: Optional[torch.Tensor] = None, max_atoms: int = MOL_MAX_ATOMS, max_pocket: Optional[int] = None,
                  max_rotors: int = VINA_MIN_MAX_ROTORS, **params):
    """Minimise a batch of perceived ligands in their rigid pockets under the score of `vina_score`, over rigid-body and torsional
    degrees of freedom, on the GPU in one launch (kpd_vina_minimize; include/kpd.h states the torsion tree, the chart, the
    intramolecular term and the minimiser: this library's own, NOT gnina's or Vina's numbers).  The arguments are those of
    `vina_score`, with `mol` also holding 'frag'; max_rotors (0 .. 64): the rotors beyond it are frozen, 0 = rigid bodies only.
    Returns (pos_out [N,3] fp32, report [B,16] float64 with the columns VINA_MIN_REPORT, status [B] int32).  No host
    synchronisation."""
    pos, pocket_x, pocket_of, B, N, F, M, P, cap_bonds, zt, max_atoms, max_pocket = _ligand_pocket_args(
        'vina_minimize', pos, lig_ptr, z, mol, ('elem', 'frag', 'bonds', 'order', 'bond_ptr', 'status'), pocket_x, pocket_ptr, pocket_of,
        max_atoms, max_pocket)
    lig_radius, pocket_radius = _dev_f32(lig_radius, 'lig_radius'), _dev_f32(pocket_radius, 'pocket_radius')
    pocket_type = _per_entry(pocket_type, 'vina_minimize: pocket_type', M, 'pocket atom')
    if lig_type_in is not None:
        lig_type_in = _per_entry(lig_type_in, 'vina_minimize: lig_type_in', N, 'ligand atom')
    max_rotors = int(max_rotors)
    if lig_radius.shape != (F,) or pocket_radius.shape != (M,) or not 0 <= max_rotors <= VINA_MIN_MAX_ROTORS:
        raise KpdError(f'vina_minimize: lig_radius {tuple(lig_radius.shape)} must be [{F}], pocket_radius {tuple(pocket_radius.shape)} '
                       f'[{M}] and max_rotors {max_rotors} be 0 .. {VINA_MIN_MAX_ROTORS}')
    p = vina_min_params(**params)
    dev = pos.device
    pos_out = torch.empty_like(pos)
    report = torch.empty(B, 16, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().kpd_vina_minimize(_ptr(pos), _ptr(lig_ptr), N, B, max_atoms, _ptr(mol['elem']), F, _ptr(zt), _ptr(lig_radius),
                                  _ptr(mol['frag']), _ptr(mol['bonds']), _ptr(mol['order']), _ptr(mol['bond_ptr']), cap_bonds,
                                  _ptr(mol['status']), _ptr(lig_type_in), _ptr(pocket_x), _ptr(pocket_radius), _ptr(pocket_type),
                                  _ptr(pocket_ptr), M, P, max_pocket, _ptr(pocket_of), max_rotors, C.byref(p), _ptr(pos_out),
                                  _ptr(report), _ptr(status), _stream()))
    return pos_out, report, status


# status bits of kpd_vina_dock (bits 0, 1, 2, 4, 5 as for kpd_vina_minimize)
VINA_DOCK_NO_MOLECULE, VINA_DOCK_BAD_INPUT, VINA_DOCK_ATOM_OUT, VINA_DOCK_FROZEN_ROTORS, VINA_DOCK_FRAGMENTS = 1, 2, 4, 16, 32
VINA_DOCK_BAD_BOX, VINA_DOCK_START_OUTSIDE, VINA_DOCK_FEW_MODES = 128, 256, 512
VINA_DOCK_LEFT_OUT = VINA_DOCK_NO_MOLECULE | VINA_DOCK_BAD_INPUT | VINA_DOCK_FRAGMENTS | VINA_DOCK_BAD_BOX
VINA_DOCK_REPORT = ('score', 'E', 'inter', 'intra', 'rmsd_input', 'rmsd_best', 'chain', 'gnorm')
VINA_DOCK_CHAIN_REPORT = ('E', 'inter', 'intra', 'best_step', 'accepted', 'box_rejected', 'evaluations', 'found', 'gnorm', 'score')
VINA_DOCK_MAX_CHAINS = 64


def vina_dock_params(**params) -> KpdVinaDockParams:
    """The parameters of kpd_vina_dock: the library's defaults (kpd_vina_dock_defaults: those of kpd_vina_minimize, temperature
    1.2, amplitude 2, min_rmsd 1, step_iters 20; max_iters is the refinement's) with the given fields replaced."""
    p, names = _struct_params('vina_dock', KpdVinaDockParams, lib().kpd_vina_dock_defaults, params, ints=('max_iters', 'step_iters'))
    if not (all(abs(getattr(p, k)) < 1e12 for k in names) and 0 < p.r_c < 1e6 and p.w_rot >= 0 and p.w_intra >= 0 and p.gtol >= 0 and
            p.max_step > 0 and p.max_iters >= 0 and p.step_iters >= 0 and p.temperature > 0 and p.amplitude > 0 and p.min_rmsd > 0):
        raise KpdError('vina_dock: ' + ', '.join(f'{k} {getattr(p, k)}' for k in names) + ': the weights must be finite, w_rot, w_intra, '
                       'gtol, max_iters and step_iters >= 0, r_c, max_step, temperature, amplitude and min_rmsd > 0')
    return p


def vina_dock(pos: torch.Tensor, lig_ptr: torch.Tensor, z, lig_radius: torch.Tensor, mol: dict, pocket_x: torch.Tensor,
              pocket_radius: torch.Tensor, pocket_type: torch.Tensor, pocket_ptr: torch.Tensor, pocket_of: torch.Tensor,
              box_lo: torch.Tensor, box_hi: torch.Tensor, n_chains: int = 8, n_steps: int = 50, n_modes: Optional[int] = None,
              seed: int = 0, lig_id: Optional[torch.Tensor] = None, lig_type_in: Optional[torch.Tensor] = None,
              max_atoms: int = MOL_MAX_ATOMS, max_pocket: Optional[int] = None, max_rotors: int = VINA_MIN_MAX_ROTORS, **params):
    """Search poses of a batch of perceived ligands in their rigid pockets under the score of `vina_score`: n_chains Monte-Carlo
    chains per ligand (perturb, minimise, Metropolis) inside the box [box_lo, box_hi] ([B,3] fp32), then ranking and clustering
    into n_modes poses (`min(9, n_chains)` by default), on the GPU in two launches (kpd_vina_dock; include/kpd.h DEFINES the
    search: this library's own, NOT gnina's or Vina's docking or numbers).  The other arguments are those of `vina_minimize`;
    lig_id [B] int32 names every ligand's random stream (its index by default).  Returns a dict of device tensors: pos [n_modes,N,3]
    fp32 (rows of a mode that does not exist are the input rows), n_found [B], report [B,n_modes,8] float64 (columns
    VINA_DOCK_REPORT), chain_pos [n_chains,N,3], chain_report [B,n_chains,10] (columns VINA_DOCK_CHAIN_REPORT), status [B].  No host
    synchronisation."""
    pos, pocket_x, pocket_of, B, N, F, M, P, cap_bonds, zt, max_atoms, max_pocket = _ligand_pocket_args(
        'vina_dock', pos, lig_ptr, z, mol, ('elem', 'frag', 'bonds', 'order', 'bond_ptr', 'status'), pocket_x, pocket_ptr, pocket_of,
        max_atoms, max_pocket)
    lig_radius, pocket_radius = _dev_f32(lig_radius, 'lig_radius'), _dev_f32(pocket_radius, 'pocket_radius')
    box_lo, box_hi = _dev_f32(box_lo, 'box_lo'), _dev_f32(box_hi, 'box_hi')
    pocket_type = _per_entry(pocket_type, 'vina_dock: pocket_type', M, 'pocket atom')
    if lig_type_in is not None:
        lig_type_in = _per_entry(lig_type_in, 'vina_dock: lig_type_in', N, 'ligand atom')
    if lig_id is not None:
        lig_id = _per_entry(lig_id, 'vina_dock: lig_id', B, 'ligand', contiguous=True)
    max_rotors, n_chains, n_steps, seed = int(max_rotors), int(n_chains), int(n_steps), int(seed)
    n_modes = min(9, n_chains) if n_modes is None else int(n_modes)
    if (lig_radius.shape != (F,) or pocket_radius.shape != (M,) or not 0 <= max_rotors <= VINA_MIN_MAX_ROTORS or
            box_lo.shape != (B, 3) or box_hi.shape != (B, 3)):
        raise KpdError(f'vina_dock: lig_radius {tuple(lig_radius.shape)} must be [{F}], pocket_radius {tuple(pocket_radius.shape)} '
                       f'[{M}], max_rotors {max_rotors} be 0 .. {VINA_MIN_MAX_ROTORS}, box_lo {tuple(box_lo.shape)} and box_hi '
                       f'{tuple(box_hi.shape)} be [{B},3]')
    if not (1 <= n_chains <= VINA_DOCK_MAX_CHAINS and 1 <= n_modes <= n_chains and n_steps >= 0 and 0 <= seed < 1 << 64):
        raise KpdError(f'vina_dock: n_chains {n_chains} must be 1 .. {VINA_DOCK_MAX_CHAINS}, n_modes {n_modes} 1 .. n_chains, n_steps '
                       f'{n_steps} >= 0, seed {seed} in [0, 2^64)')
    p = vina_dock_params(**params)
    dev = pos.device
    out = dict(pos=torch.empty(n_modes, N, 3, dtype=torch.float32, device=dev), n_found=torch.empty(B, dtype=torch.int32, device=dev),
               report=torch.empty(B, n_modes, len(VINA_DOCK_REPORT), dtype=torch.float64, device=dev),
               chain_pos=torch.empty(n_chains, N, 3, dtype=torch.float32, device=dev),
               chain_report=torch.empty(B, n_chains, len(VINA_DOCK_CHAIN_REPORT), dtype=torch.float64, device=dev),
               status=torch.empty(B, dtype=torch.int32, device=dev))
    check(lib().kpd_vina_dock(_ptr(pos), _ptr(lig_ptr), N, B, max_atoms, _ptr(mol['elem']), F, _ptr(zt), _ptr(lig_radius),
                              _ptr(mol['frag']), _ptr(mol['bonds']), _ptr(mol['order']), _ptr(mol['bond_ptr']), cap_bonds,
                              _ptr(mol['status']), _ptr(lig_type_in), _ptr(pocket_x), _ptr(pocket_radius), _ptr(pocket_type),
                              _ptr(pocket_ptr), M, P, max_pocket, _ptr(pocket_of), max_rotors, _ptr(box_lo), _ptr(box_hi), _ptr(lig_id),
                              seed, n_chains, n_steps, n_modes, C.byref(p), _ptr(out['pos']), _ptr(out['n_found']), _ptr(out['report']),
                              _ptr(out['chain_pos']), _ptr(out['chain_report']), _ptr(out['status']), _stream()))
    return out


def sample_update(pb: PreparedBatch, atom_nf, lig_x, lig_h, kp_x, eps_x, eps_h, noise_x, noise_h, coef):
    """In-place reverse-diffusion update + ligand-COM removal (kpd_sample_update)."""
    for t in (lig_x, lig_h, kp_x):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise KpdError('sample_update state tensors must be contiguous fp32 GPU tensors (updated in place)')
    args = [_dev_f32(a, 'arg') for a in (eps_x, eps_h, noise_x, noise_h, coef)]
    check(lib().kpd_sample_update(pb.B, _ptr(pb.lig_ptr), _ptr(pb.kp_ptr), int(atom_nf), _ptr(lig_x), _ptr(lig_h),
                                  _ptr(kp_x), *[a.data_ptr() for a in args], pb.max_lig, _stream()))


def _update_args(name, pb: PreparedBatch, atom_nf, lig_x, lig_h, kp_x, per_x, per_h, coef, width):
    """The checks of `sample_update`, and the sizes: the kernels index every per-atom array by the batch's own offsets."""
    for t in (lig_x, lig_h, kp_x):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise KpdError(f'{name} state tensors must be contiguous fp32 GPU tensors (updated in place)')
    F = int(atom_nf)
    if F < 1 or lig_x.shape != (pb.n_lig, 3) or lig_h.shape != (pb.n_lig, F) or kp_x.shape != (pb.n_kp, 3):
        raise KpdError(f'{name}: lig_x {tuple(lig_x.shape)}, lig_h {tuple(lig_h.shape)}, kp_x {tuple(kp_x.shape)} do not fit a batch of '
                       f'{pb.n_lig} ligand atoms x {F} features and {pb.n_kp} keypoints')
    per_x, per_h, coef = [_dev_f32(a, 'arg') for a in per_x], [_dev_f32(a, 'arg') for a in per_h], _dev_f32(coef, 'coef')
    if any(a.shape != lig_x.shape for a in per_x) or any(a.shape != lig_h.shape for a in per_h) or coef.shape != (pb.B, width):
        raise KpdError(f'{name}: every per-atom argument must have the shape of lig_x / lig_h, coef must be [{pb.B}, {width}]')
    return per_x, per_h, coef


def sample_update_inpaint(pb: PreparedBatch, atom_nf, lig_x, lig_h, kp_x, eps_x, eps_h, noise_x, noise_h, coef6, fixed, known_x,
                          known_h, kp_com0, known_noise_x, known_noise_h):
    """In-place reverse-diffusion update around fixed atoms + ligand-COM removal (kpd_sample_update_inpaint; include/kpd.h
    states the algorithm).  fixed [n_lig] uint8 / bool, known_x in the input frame, known_h normalised, kp_com0 [B,3]."""
    (eps_x, noise_x, known_x, known_noise_x), (eps_h, noise_h, known_h, known_noise_h), coef6 = _update_args(
        'sample_update_inpaint', pb, atom_nf, lig_x, lig_h, kp_x, (eps_x, noise_x, known_x, known_noise_x),
        (eps_h, noise_h, known_h, known_noise_h), coef6, 6)
    if not (fixed.is_cuda and fixed.dtype in (torch.bool, torch.uint8) and fixed.shape == (pb.n_lig,)):
        raise KpdError('fixed must be a bool or uint8 GPU tensor with one entry per ligand atom')
    fixed = fixed.contiguous().view(torch.uint8) if fixed.dtype == torch.bool else fixed.contiguous()
    kp_com0 = _dev_f32(kp_com0, 'kp_com0')
    if kp_com0.shape != (pb.B, 3):
        raise KpdError(f'kp_com0 must be [{pb.B}, 3] (got {tuple(kp_com0.shape)})')
    check(lib().kpd_sample_update_inpaint(pb.B, _ptr(pb.lig_ptr), _ptr(pb.kp_ptr), int(atom_nf), _ptr(lig_x), _ptr(lig_h), _ptr(kp_x),
                                          _ptr(eps_x), _ptr(eps_h), _ptr(noise_x), _ptr(noise_h), _ptr(coef6), _ptr(fixed),
                                          _ptr(known_x), _ptr(known_h), _ptr(kp_com0), _ptr(known_noise_x), _ptr(known_noise_h),
                                          pb.max_lig, _stream()))


def sample_renoise(pb: PreparedBatch, atom_nf, lig_x, lig_h, kp_x, noise_x, noise_h, coef6):
    """In-place z_t = alpha_t|s z_s + sigma_t|s noise + ligand-COM removal (kpd_sample_renoise): back from s to t between two
    repetitions of a resampled inpainting step."""
    (noise_x,), (noise_h,), coef6 = _update_args('sample_renoise', pb, atom_nf, lig_x, lig_h, kp_x, (noise_x,), (noise_h,), coef6, 6)
    check(lib().kpd_sample_renoise(pb.B, _ptr(pb.lig_ptr), _ptr(pb.kp_ptr), int(atom_nf), _ptr(lig_x), _ptr(lig_h), _ptr(kp_x),
                                   _ptr(noise_x), _ptr(noise_h), _ptr(coef6), pb.max_lig, _stream()))


def guided_coefficients(gamma: torch.Tensor, s: torch.Tensor, t: torch.Tensor, scale: float, t_max: float) -> torch.Tensor:
    """[B,9] coefficients of a guided step (kpd_guided_coefficients): the six of `inpaint_coefficients`, bit for bit, then alpha_t,
    sigma_t and the guidance weight w = scale alpha_s sigma^2_t|s / sigma_t^2 (0 above t_max)."""
    gamma, s, t = _dev_f32(gamma, 'gamma'), _dev_f32(s, 's'), _dev_f32(t, 't')
    if s.shape != t.shape or s.dim() != 1:
        raise KpdError(f'guided_coefficients: s {tuple(s.shape)} and t {tuple(t.shape)} must be equal 1-D tensors')
    if not (float(scale) >= 0.0 and 0.0 < float(t_max) <= 1.0):
        raise KpdError(f'guided_coefficients: scale must be >= 0 and t_max in (0, 1] (got scale = {scale!r}, t_max = {t_max!r})')
    coef = torch.empty(s.shape[0], 9, device=s.device)
    check(lib().kpd_guided_coefficients(gamma.data_ptr(), int(gamma.shape[0]), s.data_ptr(), t.data_ptr(), int(s.shape[0]),
                                        float(scale), float(t_max), coef.data_ptr(), _stream()))
    return coef


def _wall_args(name, wall_x, wall_ptr, B):
    """Shape, dtype and device of a wall: wall_x [n_wall,3] fp32, wall_ptr [B+1] int32, both on the GPU.  The VALUES of wall_ptr
    are not read here (that would synchronise every step, and cannot be done while a graph is captured): `check_wall` does it,
    once per tensor (`_wall_values_once`)."""
    if not (isinstance(wall_x, torch.Tensor) and isinstance(wall_ptr, torch.Tensor) and wall_x.is_cuda and wall_ptr.is_cuda):
        raise KpdError(f'{name}: wall_x and wall_ptr must be GPU tensors (there is no CPU implementation)')
    if wall_x.dtype != torch.float32 or wall_x.dim() != 2 or wall_x.shape[1] != 3 or not wall_x.is_contiguous():
        raise KpdError(f'{name}: wall_x must be a contiguous fp32 [n_wall, 3] tensor (got {wall_x.dtype} {tuple(wall_x.shape)})')
    if wall_ptr.dtype != torch.int32 or wall_ptr.shape != (B + 1,) or not wall_ptr.is_contiguous():
        raise KpdError(f'{name}: wall_ptr must be a contiguous int32 [{B + 1}] tensor, one offset per complex and the total '
                       f'(got {wall_ptr.dtype} {tuple(wall_ptr.shape)}): the wall does not fit the batch')


def check_wall(wall_x: torch.Tensor, wall_ptr: torch.Tensor, B: int, name: str = 'wall'):
    """The values of wall_ptr [B+1]: 0 first, ascending, n_wall last -- the kernels read the rows it names.  One host read; call it
    once per batch (`GuidanceContext` does), not per step."""
    if not (isinstance(wall_ptr, torch.Tensor) and wall_ptr.dim() == 1 and wall_ptr.shape[0] == B + 1 and
            not wall_ptr.dtype.is_floating_point):
        raise KpdError(f'{name}: wall_ptr must be an integer [{B + 1}] tensor (the wall does not fit the batch of {B} complexes)')
    if not (isinstance(wall_x, torch.Tensor) and wall_x.dim() == 2 and wall_x.shape[1] == 3):
        raise KpdError(f'{name}: wall_x must be [n_wall, 3] (got {tuple(getattr(wall_x, "shape", ()))})')
    p = wall_ptr.detach().cpu().long()
    if int(p[0]) != 0 or int(p[-1]) != wall_x.shape[0] or bool((p[1:] < p[:-1]).any()):
        raise KpdError(f'{name}: wall_ptr must ascend from 0 to n_wall = {wall_x.shape[0]} (got {p.tolist()[:8]}{"..." if B > 7 else ""})')


_walls_seen = {}          # (wall_ptr storage, version, n_wall) -> the tensor (held, so its address cannot be recycled)


def _wall_values_once(wall_x, wall_ptr, B, name):
    """`check_wall` the first time this wall_ptr tensor is seen, nothing afterwards: the values are read on the host once per
    batch, not per step (a step inside a graph capture never reads them: the capture's warm-up steps did)."""
    key = (wall_ptr.data_ptr(), wall_ptr._version, int(wall_x.shape[0]), B)
    if key not in _walls_seen:
        check_wall(wall_x, wall_ptr, B, name)
        if len(_walls_seen) >= 16:
            _walls_seen.pop(next(iter(_walls_seen)))
        _walls_seen[key] = wall_ptr


def sample_update_guided(pb: PreparedBatch, atom_nf, lig_x, lig_h, kp_x, eps_x, eps_h, noise_x, noise_h, coef9, wall_x, wall_ptr,
                         kp_com0, threshold, fixed=None, known_x=None, known_h=None, known_noise_x=None, known_noise_h=None):
    """In-place guided reverse-diffusion update + ligand-COM removal (kpd_sample_update_guided; include/kpd.h, "Clash guidance",
    states the algorithm).  wall_x [n_wall,3] in the input frame, wall_ptr [B+1] int32 (its values are checked the first time the tensor is seen),
    kp_com0 [B,3]; `fixed` and the four known-part tensors: all None, or the inpainting arguments of `sample_update_inpaint`."""
    masked = fixed is not None
    inp = (known_x, known_h, known_noise_x, known_noise_h)
    if any((a is not None) != masked for a in inp):
        raise KpdError('sample_update_guided: fixed, known_x, known_h, known_noise_x and known_noise_h go together (all or none)')
    per_x = (eps_x, noise_x) + ((known_x, known_noise_x) if masked else ())
    per_h = (eps_h, noise_h) + ((known_h, known_noise_h) if masked else ())
    per_x, per_h, coef9 = _update_args('sample_update_guided', pb, atom_nf, lig_x, lig_h, kp_x, per_x, per_h, coef9, 9)
    if masked:
        if not (fixed.is_cuda and fixed.dtype in (torch.bool, torch.uint8) and fixed.shape == (pb.n_lig,)):
            raise KpdError('fixed must be a bool or uint8 GPU tensor with one entry per ligand atom')
        fixed = fixed.contiguous().view(torch.uint8) if fixed.dtype == torch.bool else fixed.contiguous()
    else:
        per_x, per_h = per_x + [None, None], per_h + [None, None]
    _wall_args('sample_update_guided', wall_x, wall_ptr, pb.B)
    _wall_values_once(wall_x, wall_ptr, pb.B, 'sample_update_guided')
    kp_com0 = _dev_f32(kp_com0, 'kp_com0')
    if kp_com0.shape != (pb.B, 3):
        raise KpdError(f'kp_com0 must be [{pb.B}, 3] (got {tuple(kp_com0.shape)})')
    if not float(threshold) > 0.0:
        raise KpdError(f'sample_update_guided: threshold must be positive (got {threshold!r})')
    check(lib().kpd_sample_update_guided(pb.B, _ptr(pb.lig_ptr), _ptr(pb.kp_ptr), int(atom_nf), _ptr(lig_x), _ptr(lig_h), _ptr(kp_x),
                                         _ptr(per_x[0]), _ptr(per_h[0]), _ptr(per_x[1]), _ptr(per_h[1]), _ptr(coef9), _ptr(fixed),
                                         _ptr(per_x[2]), _ptr(per_h[2]), _ptr(kp_com0), _ptr(per_x[3]), _ptr(per_h[3]),
                                         _ptr(wall_ptr), _ptr(wall_x), float(threshold), pb.max_lig, _stream()))


def clash_score(lig_x: torch.Tensor, lig_ptr: torch.Tensor, wall_x: torch.Tensor, wall_ptr: torch.Tensor, threshold: float) -> torch.Tensor:
    """[B,3] = per complex {1/2 sum (threshold - d)+^2, pairs with d < threshold, smallest such d or +inf} between the ligand rows
    [lig_ptr[b], lig_ptr[b+1]) of lig_x and the wall rows of wall_x, both in one frame (kpd_clash_score): the report to rank or
    filter samples by.  fp32 GPU positions, int32 GPU offsets [B+1]."""
    if not (isinstance(lig_ptr, torch.Tensor) and lig_ptr.dim() == 1 and lig_ptr.shape[0] >= 2):
        raise KpdError('clash_score: lig_ptr must be a 1-D tensor of B + 1 offsets')
    B = lig_ptr.shape[0] - 1
    _wall_args('clash_score', wall_x, wall_ptr, B)
    _wall_args('clash_score (ligand side)', lig_x, lig_ptr, B)
    check_wall(wall_x, wall_ptr, B, 'clash_score')
    check_wall(lig_x, lig_ptr, B, 'clash_score (ligand side)')
    if not float(threshold) > 0.0:
        raise KpdError(f'clash_score: threshold must be positive (got {threshold!r})')
    out = torch.empty(B, 3, device=lig_x.device, dtype=torch.float32)
    check(lib().kpd_clash_score(B, _ptr(lig_ptr), _ptr(lig_x), _ptr(wall_ptr), _ptr(wall_x), float(threshold), _ptr(out), _stream()))
    return out


STRUCT_TILE = 4096            # KPD_STRUCT_TILE of include/kpd.h: bytes of text per workgroup of the line scan (the tests sit on its edges)
PDB_HETATM, PDB_HYDROGEN, PDB_WATER, PDB_ALTLOC, PDB_STD_AA, PDB_CALPHA, PDB_GUESSED, PDB_BAD = 1, 2, 4, 8, 16, 32, 64, 128   # flags
PDB_EMPTY, PDB_CAPACITY, PDB_BAD_RECORD, PDB_MODELS, PDB_BAD_SEGMENT, PDB_LINES = 1, 2, 4, 8, 16, 32                            # status
_PDB_FIELDS = (('pos', torch.float32, 3), ('occ_b', torch.float32, 2), ('sym', torch.int32, 0), ('elem', torch.int32, 0),
               ('name', torch.int32, 0), ('resname', torch.int32, 0), ('res_class', torch.int32, 0), ('resseq', torch.int32, 0),
               ('tags', torch.int32, 0), ('line_off', torch.int64, 0), ('res_idx', torch.int32, 0), ('flags', torch.int32, 0))


def _text_args(where: str, text, file_ptr):
    if not (isinstance(text, torch.Tensor) and text.is_cuda and text.dtype == torch.uint8 and text.dim() == 1):
        raise KpdError(f'{where}: text must be a 1-D uint8 GPU tensor (got {getattr(text, "device", type(text))}); there is no CPU parser')
    if not (isinstance(file_ptr, torch.Tensor) and file_ptr.is_cuda and file_ptr.dtype == torch.int64 and file_ptr.dim() == 1 and
            file_ptr.numel() >= 1 and file_ptr.is_contiguous()):
        raise KpdError(f'{where}: file_ptr must be a contiguous int64 GPU tensor of B + 1 offsets')
    if not text.is_contiguous():
        raise KpdError(f'{where}: text must be contiguous (a slice text[k:] is; a strided view is not)')
    return int(text.numel()), int(file_ptr.numel()) - 1


def pdb_parse(text: torch.Tensor, file_ptr: torch.Tensor, elements, resnames=(), cap_lines: Optional[int] = None,
              cap_atoms: Optional[int] = None):
    """ATOM / HETATM records of a batch of PDB files on the GPU (kpd_pdb_parse; include/kpd.h states every column and rounding).
    text [n_bytes] uint8 and file_ptr [B+1] int64 GPU tensors (file b = text[file_ptr[b]:file_ptr[b+1]]; no alignment needed),
    elements: F symbols in Title case ('C', 'Cl'), resnames: R residue names of exactly three characters.  Without capacities
    the call sizes its tables from the text's length and repeats itself while the sizes a call reports are larger (unusual text only); with
    them it is one call, and what does not fit is reported, not written.  Returns a dict: the per-atom device tensors pos, occ_b,
    sym, elem, name, resname, res_class, resseq, tags, line_off, res_idx, flags (cut to the atoms written), and the host lists
    atom_ptr (B + 1; the last is the size needed), n_res, status (B each) and n_lines.  One host read per call."""
    n_bytes, B = _text_args('pdb_parse', text, file_ptr)
    dev = text.device
    symbols = _packed_symbols(elements, dev, longest=2)
    for r in resnames:
        if len(r.encode('ascii')) != 3:
            raise KpdError(f'residue name {r!r} must be exactly three ASCII characters (columns 18-20 as they are)')
    rn = _packed_symbols(resnames, dev, longest=3) if len(resnames) else torch.zeros(0, dtype=torch.int32, device=dev)
    cl = n_bytes // 32 + B + 16 if cap_lines is None else int(cap_lines)
    ca = n_bytes // 60 + B + 16 if cap_atoms is None else int(cap_atoms)
    while True:
        out = {name: torch.empty((ca, w) if w else (ca,), dtype=dt, device=dev) for name, dt, w in _PDB_FIELDS}
        meta = torch.empty(3 * B + 2, dtype=torch.int32, device=dev)     # atom_ptr [B + 1], n_res [B], status [B], n_lines [1]
        nb = int(lib().kpd_pdb_scratch_bytes(n_bytes, B, cl))
        if nb < 0:
            raise KpdError(f'pdb_parse: {n_bytes} bytes in {B} files: at most 2^31 - 2 together per call')
        scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
        base = meta.data_ptr()
        check(lib().kpd_pdb_parse(_ptr(text), n_bytes, _ptr(file_ptr), B, _ptr(symbols), len(elements), _ptr(rn), len(resnames), cl, ca,
                                  *[_ptr(out[name]) for name, _, _ in _PDB_FIELDS], base, base + 4 * (B + 1), base + 4 * (2 * B + 1),
                                  base + 4 * (3 * B + 1), _ptr(scratch), _stream()))
        host = meta.cpu().tolist()
        atom_ptr, n_lines = host[:B + 1], host[-1]
        if (cap_lines is None and n_lines > cl) or (cap_atoms is None and atom_ptr[-1] > ca):
            cl = max(cl, n_lines) if cap_lines is None else cl          # with too few lines no atom was counted: the atoms may take a third call
            ca = max(ca, atom_ptr[-1]) if cap_atoms is None else ca
            continue
        break
    n = min(atom_ptr[-1], ca)
    res = {name: t[:n] for name, t in out.items()}
    res.update(atom_ptr=atom_ptr, n_res=host[B + 1:2 * B + 1], status=host[2 * B + 1:3 * B + 1], n_lines=n_lines)
    return res


# status bits of kpd_sdf_parse beside MOL_*: why a record reads as it does, or was left out (MOL_BAD_SEGMENT)
SDF_AROMATIC, SDF_CHARGES, SDF_V3000, SDF_UNPARSABLE, SDF_TRUNCATED, SDF_LIMITS = 16, 32, 64, 128, 256, 512


def sdf_parse(text: torch.Tensor, file_ptr: torch.Tensor, elements, z, allowed, remove_h: bool = True, cap_lines: Optional[int] = None,
              cap_mols: Optional[int] = None, cap_atoms: Optional[int] = None, cap_bonds: Optional[int] = None):
    """MOL V2000 records of a batch of SDF files on the GPU, in the layout `mol_perceive` returns (kpd_sdf_parse; include/kpd.h
    states the format and every reason a record is left out).  text / file_ptr as for `pdb_parse`; elements, z, allowed: the F
    symbols, atomic numbers and largest valences of the ligand classes.  Capacities as for `pdb_parse`: sized from the text, and
    repeated while a call reports larger sizes.  Returns a dict: device tensors lig_ptr [M+1], pos, sym, elem, valence, frag, bonds
    [cap_bonds,2], order, bond_ptr [M+1], summary [M,4], status [M], title_off [M,2], and host lists mol_ptr (B + 1), file_status
    (B), sizes (atoms per record), n_bonds and n_lines.  One host read per call."""
    n_bytes, B = _text_args('sdf_parse', text, file_ptr)
    F = len(elements)
    if F < 1 or len(z) != F or len(allowed) != F:
        raise KpdError(f'sdf_parse: {F} element symbols, {len(z)} atomic numbers, {len(allowed)} valences')
    dev = text.device
    symbols = _packed_symbols(elements, dev, longest=3)
    zt, at = torch.tensor(list(z), dtype=torch.int32, device=dev), torch.tensor(list(allowed), dtype=torch.int32, device=dev)
    given = dict(lines=cap_lines, mols=cap_mols, atoms=cap_atoms, bonds=cap_bonds)
    cap = dict(lines=n_bytes // 24 + B + 16, mols=n_bytes // 1024 + B + 16, atoms=n_bytes // 60 + 16, bonds=n_bytes // 13 // 4 + 16)
    cap.update({k: int(v) for k, v in given.items() if v is not None})
    while True:
        cm, ca, cb = cap['mols'], cap['atoms'], cap['bonds']
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        out = dict(pos=torch.empty(ca, 3, dtype=torch.float32, device=dev), sym=i32(ca), elem=i32(ca), valence=i32(ca), frag=i32(ca),
                   bonds=i32(cb, 2), order=i32(cb), summary=i32(cm, 4), status=i32(cm), title_off=torch.empty(cm, 2, dtype=torch.int64, device=dev))
        meta = torch.empty(2 * B + 2 + 2 * (cm + 1), dtype=torch.int32, device=dev)    # mol_ptr [B+1], file_status [B], n_lines, lig_ptr, bond_ptr [cm+1]
        nb = int(lib().kpd_sdf_parse_scratch_bytes(n_bytes, B, cap['lines'], cm))
        if nb < 0:
            raise KpdError(f'sdf_parse: {n_bytes} bytes in {B} files: at most 2^31 - 2 together per call')
        scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
        base = meta.data_ptr()
        p_fs, p_nl = base + 4 * (B + 1), base + 4 * (2 * B + 1)
        p_lig = base + 4 * (2 * B + 2)
        p_bp = p_lig + 4 * (cm + 1)
        check(lib().kpd_sdf_parse(_ptr(text), n_bytes, _ptr(file_ptr), B, _ptr(symbols), F, _ptr(zt), _ptr(at), 1 if remove_h else 0, cap['lines'],
                                  cm, ca, cb, base, p_fs, p_lig, _ptr(out['pos']), _ptr(out['sym']), _ptr(out['elem']), _ptr(out['valence']),
                                  _ptr(out['frag']), _ptr(out['bonds']), _ptr(out['order']), p_bp, _ptr(out['summary']), _ptr(out['title_off']),
                                  _ptr(out['status']), p_nl, _ptr(scratch), _stream()))
        host = meta.cpu().tolist()
        mol_ptr, file_status, n_lines = host[:B + 1], host[B + 1:2 * B + 1], host[2 * B + 1]
        lig_ptr, bond_ptr = host[2 * B + 2:2 * B + 3 + cm], host[2 * B + 3 + cm:]
        need = dict(lines=n_lines, mols=mol_ptr[-1], atoms=lig_ptr[-1], bonds=bond_ptr[-1])
        short = [k for k in cap if need[k] > cap[k] and given[k] is None]
        if short:                                           # lines, then records, then atoms and bonds: each is counted once the one before fits
            for k in short:
                cap[k] = need[k]
            continue
        break
    M = min(mol_ptr[-1], cm)
    n_at, n_bo = min(lig_ptr[M], ca), bond_ptr[M]
    off = 2 * B + 2
    res = dict(lig_ptr=meta[off:off + M + 1], bond_ptr=meta[off + cm + 1:off + cm + 2 + M], pos=out['pos'][:n_at], sym=out['sym'][:n_at],
               elem=out['elem'][:n_at], valence=out['valence'][:n_at], frag=out['frag'][:n_at], bonds=out['bonds'], order=out['order'],
               summary=out['summary'][:M], status=out['status'][:M], title_off=out['title_off'][:M], mol_ptr=mol_ptr, file_status=file_status,
               sizes=[lig_ptr[m + 1] - lig_ptr[m] for m in range(M)], n_bonds=n_bo, n_atoms=lig_ptr[M], n_lines=n_lines)
    return res
