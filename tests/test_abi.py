"""C ABI: the shared library loads without a GPU and exports exactly what include/kpd.h declares."""
import ctypes
import os
import re

from keypoint_diffusion_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'kpd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(kpd_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(hip.LIB_PATH), 'build the HIP extension first (__graft_entry__.build())'
    lib = ctypes.CDLL(hip.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/kpd.h but not exported'
    assert sorted(hip.EXPORTS) == syms, 'hip.EXPORTS out of sync with include/kpd.h'


def header_code():
    """include/kpd.h without comments and preprocessor lines."""
    text = open(os.path.join(ROOT, 'include', 'kpd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return re.sub(r'^\s*#.*$|//.*$', '', text, flags=re.M)


SCALARS = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float,
           'double': ctypes.c_double}
RESULTS = {'kpd_status': ctypes.c_int, 'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'void': None, 'const char *': ctypes.c_char_p}


def c_kind(base, declarator):
    """'pointer' for `T *x` / `T x[n]`, else the ctypes twin of the scalar type `base` (an unknown type raises)."""
    if '*' in declarator or '[' in declarator:
        return 'pointer'
    return SCALARS[' '.join(w for w in base.split() if w != 'const')]


def ctypes_kind(t):
    return 'pointer' if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer) else t


def declared_prototypes():
    """name -> (result type as written, [kind of every parameter]) for every `return-type kpd_name(params);` of the header."""
    out = {}
    for result, name, params in re.findall(r'([A-Za-z_][\w\s\*]*?)\b(kpd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', header_code()):
        kinds = []
        for p in ([] if params.strip() == 'void' else params.split(',')):
            base, declarator = re.fullmatch(r'\s*((?:const\s+)?\w+)\s*(.*?)\s*', p, flags=re.S).groups()
            kinds.append(c_kind(base, declarator))
        assert name not in out, name
        out[name] = (' '.join(result.split()), kinds)
    return out


def declared_structs():
    """name -> [(field, kind)] for every `typedef struct ... { ... } kpd_name;` of the header."""
    out = {}
    for body, name in re.findall(r'typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(kpd_\w+)\s*;', header_code()):
        fields = []
        for statement in filter(None, (s.strip() for s in body.split(';'))):
            base, rest = re.fullmatch(r'((?:const\s+)?\w+)\s*(.*)', statement, flags=re.S).groups()
            for d in rest.split(','):
                fields.append((re.sub(r'[\s\*]|\[.*\]', '', d), c_kind(base, d)))
        out[name] = fields
    return out


def test_prototype_table_agrees_with_the_header():
    """Every function the header declares has an entry of hip.PROTOTYPES with as many parameters, of the same kind in every
    position, and the same kind of result.  Needs no built library."""
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols() == sorted(hip.PROTOTYPES) and len(protos) >= 117
    for name, (result, kinds) in protos.items():
        restype, argtypes = hip.PROTOTYPES[name]
        assert restype is RESULTS[result], f'{name}: returns {result} in the header, {restype} in hip.PROTOTYPES'
        got = [ctypes_kind(t) for t in argtypes]
        assert len(got) == len(kinds), f'{name}: {len(kinds)} parameters in the header, {len(got)} in hip.PROTOTYPES'
        for k, (a, b) in enumerate(zip(got, kinds)):
            assert a == b, f'{name}: parameter {k} is {b} in the header, {a} in hip.PROTOTYPES'


def test_structures_agree_with_the_header():
    """Every ctypes.Structure of hip (KpdFooBar) has the fields of the header's kpd_foo_bar: names and kinds, in order."""
    structs = declared_structs()
    classes = [c for c in vars(hip).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]
    assert len(classes) >= 14
    for cls in classes:
        name = re.sub(r'(?<!^)(?=[A-Z])', '_', cls.__name__).lower()
        assert name in structs, f'{cls.__name__}: no typedef struct {name} in include/kpd.h'
        assert [(f, ctypes_kind(t)) for f, t in cls._fields_] == structs[name], name


def test_version_and_error_string_without_gpu():
    lib = hip.lib()
    assert lib.kpd_version() >= 100
    assert isinstance(lib.kpd_last_error(), bytes)


def test_product_build_has_no_ablation_or_ab_switches():
    """The shipped library is the only build: kpd_build_flags() == 0 and the names of the retired A/B, ablation and LDS-padding
    switches of earlier rounds are not in the binary.  What the library does read: KPD_GEMM (the opt-in f16x2 mode), KPD_TRAIN_STORE (recompute instead of keeping activations), KPD_POISON (NaN-poisoned
    workspaces for the read-before-write tests) -- bench.py refuses to run with any of them set."""
    assert hip.lib().kpd_build_flags() == 0
    blob = open(hip.LIB_PATH, 'rb').read()
    names = set(re.findall(rb'KPD_[A-Z0-9_]{3,}', blob))
    assert names <= {b'KPD_GEMM', b'KPD_TRAIN_STORE', b'KPD_POISON'}, sorted(names)
    for gone in (b'KPD_EDGE_ABLATE', b'KPD_EDGE_SPLIT', b'KPD_EDGE_LDS_PAD', b'KPD_NODE_LDS_PAD', b'KPD_SGEMM_', b'KPD_TRAIN_FUSED', b'KPD_H_PARTS'):
        assert gone not in blob, gone


def test_product_has_no_cpu_fallback():
    """The product path must fail loudly off-GPU rather than compute on the CPU."""
    import pytest
    import torch
    from keypoint_diffusion_amd.dynamics import LigRecDynamics
    from . import util
    g = util.fixed_encode(util.make_batch([20], [5]))
    m = LigRecDynamics(10, 10, graph_cutoffs=util.CUTOFFS_ALL_ATOM, **util.EGNN_C2).eval()
    if torch.cuda.is_available():
        pytest.skip('GPU present: covered by the gpu tests')
    with torch.no_grad(), pytest.raises((hip.KpdError, RuntimeError, AssertionError)):
        m(g, torch.tensor([0.5]), None)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'keypoint-diffusion_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                src = open(os.path.join(dirpath, f)).read()
                assert 'import oracle' not in src and 'from oracle' not in src, f
