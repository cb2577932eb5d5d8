"""ctypes loader for libefgh_hip.so (the C-ABI declared in include/efgh_hip.h).

The header is the only statement of a signature: lib() reads it once and gives every efgh_* entry point its restype and argtypes,
so call sites pass plain Python values and ctypes converts (or refuses) them by the header's types.

There is no CPU fallback: if the library is missing, or a call fails, this raises."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get('EFGH_LIB') or os.path.join(_HERE, 'lib', 'libefgh_hip.so')      # EFGH_LIB: A/B runs of two builds
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'efgh_hip.h')
_lib = None
ABI_VERSION = 4          # EFGH_ABI_VERSION of include/efgh_hip.h this binding was written against

c_void_p, c_int, c_int32, c_int64, c_float = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
                                              ctypes.c_int64, ctypes.c_float)


class EfghError(RuntimeError):
    pass


class GemmDesc(ctypes.Structure):
    """mirror of efgh_gemm_desc (include/efgh_hip.h)"""
    _fields_ = [
        ('A', c_void_p), ('lda', c_int64), ('C', c_int32), ('T', c_int32), ('mode', c_int32),
        ('B', c_int32), ('Hin', c_int32), ('Win', c_int32), ('Hv', c_int32), ('Wv', c_int32),
        ('sh', c_int32), ('sw', c_int32),
        ('dh', ctypes.c_int8 * 16), ('dw', ctypes.c_int8 * 16),
        ('Ho', c_int32), ('Wo', c_int32), ('osh', c_int32), ('osw', c_int32), ('oh0', c_int32),
        ('ow0', c_int32),
        ('table', c_void_p), ('W', c_void_p), ('N', c_int32), ('M', c_int64), ('M_dev', c_void_p),
        ('bias', c_void_p), ('scale', c_void_p), ('shift', c_void_p),
        ('residual', c_void_p), ('ldr', c_int64),
        ('act', c_int32), ('slope', c_float), ('out', c_void_p), ('ldo', c_int64),
        ('stats', c_void_p),
        ('nbatch', c_int32), ('batch_stride_a', c_int64), ('batch_stride_w', c_int64), ('batch_stride_out', c_int64),
        ('batch_stride_table', c_int32), ('table_alias_mask', c_int32),
        ('stats_mode', c_int32), ('bn_raw', c_void_p), ('bn_ldraw', c_int64), ('bn_y', c_void_p), ('bn_ldy', c_int64),
        ('bn_pscale', c_void_p), ('bn_pshift', c_void_p), ('bn_mean', c_void_p), ('bn_invstd', c_void_p),
        ('bn_act', c_int32), ('bn_slope', c_float),
    ]


class WgradOutDesc(ctypes.Structure):
    """mirror of efgh_wgrad_out_desc (include/efgh_hip.h): where a weight gradient belongs in the caller's own layout"""
    _fields_ = [('W', c_void_p), ('N', c_int32), ('T', c_int32), ('C', c_int32), ('Cp', c_int32),
                ('sn', c_int64), ('sc', c_int64), ('st', c_int64), ('taps', c_int32 * 16), ('accumulate', c_int32)]


GUARD_MAX_SEGMENTS = 8   # EFGH_GUARD_MAX_SEGMENTS
GUARD_RUN = 4096         # EFGH_GUARD_RUN


class GuardState(ctypes.Structure):
    """mirror of efgh_guard_state (include/efgh_hip.h): the device-resident result of efgh_grad_guard_measure"""
    _fields_ = [('sumsq', ctypes.c_double * GUARD_MAX_SEGMENTS), ('sumsq_total', ctypes.c_double), ('norm', ctypes.c_double),
                ('nonfinite', c_int64 * GUARD_MAX_SEGMENTS), ('nonfinite_total', c_int64),
                ('applied', c_int64), ('skipped', c_int64),
                ('coef', c_float), ('scale', c_float), ('bc1', c_float), ('bc2_sqrt', c_float),
                ('skip', c_int32), ('nseg', c_int32)]


class TxnState(ctypes.Structure):
    """mirror of efgh_txn_state (include/efgh_hip.h): the device-resident record of the transactional BatchNorm state"""
    _fields_ = [('forward_nonfinite', c_int64), ('rolled_back', c_int64), ('vetoed_total', c_int64),
                ('first_bad', c_int32), ('vetoed', c_int32)]


ADAM_MAX_GROUPS = 16     # EFGH_ADAM_MAX_GROUPS
ADAM_MAX_SEGMENTS = 4096 # EFGH_ADAM_MAX_SEGMENTS


class AdamGroups(ctypes.Structure):
    """mirror of efgh_adam_groups (include/efgh_hip.h): the per-group values of efgh_adam_step_groups, a HOST struct"""
    _fields_ = [('n_groups', c_int32), ('step', c_int32), ('beta1', c_float), ('beta2', c_float), ('eps', c_float),
                ('grad_scale', c_float), ('lr', c_float * ADAM_MAX_GROUPS), ('weight_decay', c_float * ADAM_MAX_GROUPS),
                ('decay', c_float * ADAM_MAX_GROUPS), ('decoupled', c_int32 * ADAM_MAX_GROUPS)]


class PackJob(ctypes.Structure):
    """mirror of efgh_pack_job (include/efgh_hip.h): one record of the DEVICE array of efgh_pack_weight_batched(_tiled)"""
    _fields_ = [('W', c_void_p), ('Wp', c_void_p), ('N', c_int32), ('T', c_int32), ('C', c_int32), ('Np', c_int32),
                ('Cp', c_int32), ('pad_', c_int32), ('sn', c_int64), ('sc', c_int64), ('st', c_int64), ('taps', c_int32 * 16)]


class WinoPackJob(ctypes.Structure):
    """mirror of efgh_wino_pack_job (include/efgh_hip.h): one record of the DEVICE array of efgh_wino_pack_batched"""
    _fields_ = [('Wp', c_void_p), ('U', c_void_p), ('N', c_int32), ('C', c_int32), ('kind', c_int32), ('pad_', c_int32),
                ('first_block', c_int64)]


class PoseLossDesc(ctypes.Structure):
    """mirror of efgh_pose_loss_desc (include/efgh_hip.h)"""
    _fields_ = [(n, c_void_p) for n in ('e_gn_abs', 'e_gn_sgn', 'h_hrzn_abs', 'h_hrzn_sgn', 'f_score', 'g_trs', 'e_l', 'f_l')] + \
               [(n, c_int64) for n in ('ld_e_gn_sgn', 'ld_h_hrzn_sgn', 'ld_f_score')] + \
               [(n, c_void_p) for n in ('rand_init_l', 'rand_init_c', 'sensor2_T_sensor1')] + \
               [(n, c_int32) for n in ('rand_init_l_dim', 'rand_init_c_dim', 'B', 'W', 'fov_pos_num')] + \
               [(n, c_float) for n in ('fov_neg_ratio', 'lambda_e_gn', 'lambda_h_hrzn', 'lambda_fov', 'lambda_g_trs',
                                       'lambda_g_depth', 'lambda_g_mask')]


STRUCTS = {'efgh_gemm_desc': GemmDesc, 'efgh_pack_job': PackJob, 'efgh_wgrad_out_desc': WgradOutDesc,
           'efgh_wino_pack_job': WinoPackJob, 'efgh_guard_state': GuardState, 'efgh_adam_groups': AdamGroups,
           'efgh_txn_state': TxnState, 'efgh_pose_loss_desc': PoseLossDesc}      # every struct typedef of the header
DEVICE_STRUCTS = ('efgh_pack_job', 'efgh_wino_pack_job', 'efgh_guard_state', 'efgh_txn_state')      # those that live in DEVICE memory


def _struct_ptr(mirror):
    native = ctypes.POINTER(mirror)

    class StructPtr(native):
        """POINTER(mirror) as a parameter type that also takes a raw address: the guard / txn state and the job arrays live in
        DEVICE memory, where a tensor's data_ptr() is all there is.  Another struct's byref, a float or a scalar wrapper is
        refused.  The host structs (descriptors, Adam's groups) get ctypes' own POINTER(mirror), which refuses an address too"""
        @classmethod
        def from_param(cls, v):
            return c_void_p.from_param(v) if isinstance(v, (int, c_void_p)) else native.from_param(v)
    return StructPtr


_SCALARS = {'int': c_int, 'int32_t': c_int32, 'int64_t': c_int64, 'float': c_float, 'double': ctypes.c_double}
_STRUCT_PTRS = {name: _struct_ptr(mirror) if name in DEVICE_STRUCTS else ctypes.POINTER(mirror) for name, mirror in STRUCTS.items()}
_POINTEES = set(_SCALARS) | set(STRUCTS) | {'void', 'char', 'uint8_t', 'uint32_t'}
_PROTOTYPE = re.compile(r'([\w\s*]+?)\b(efgh_\w+)\s*\(([^()]*)\)')


def _ctype(decl, proto, is_return):
    """one return or parameter declaration of the header -> its ctypes type, by the type map and nothing else: the scalars of
    _SCALARS; a pointer to a header struct -> POINTER(mirror); `const char *` returned -> c_char_p; any other pointer to one of
    _POINTEES -> c_void_p.  Anything else is an error, never a guess"""
    tokens = [t for t in re.findall(r'\w+|\S', decl) if t != 'const']
    if not is_return:                    # the parameter's name: required, or `const float *` would bind as a float by value
        if not tokens or not tokens[-1].isidentifier() or tokens[-1] in _POINTEES:
            raise EfghError(f'include/efgh_hip.h: `{decl.strip()}` of `{proto}` has no parameter name')
        tokens = tokens[:-1]
    if len(tokens) == 2 and tokens[1] == '*' and tokens[0] in _POINTEES:
        if is_return and tokens[0] == 'char':
            return ctypes.c_char_p
        return _STRUCT_PTRS.get(tokens[0], c_void_p)
    if len(tokens) == 1 and tokens[0] in _SCALARS:
        return _SCALARS[tokens[0]]
    raise EfghError(f'include/efgh_hip.h: `{decl.strip()}` of `{proto}` is outside the binding\'s type map')


def signatures(header_text):
    """{name: (restype, [argtypes])} of every efgh_* prototype of a C99 header text.  Not a C parser: comments, preprocessor lines,
    the extern "C" bracket and the struct typedefs are cut out, and every statement that is left must be a prototype"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', header_text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', ' ', text, flags=re.M)
    text = re.sub(r'typedef\s+struct\b[^{}]*\{[^{}]*\}\s*\w+\s*;', ' ', text)
    sigs = {}
    for stmt in text.rstrip().rstrip('}').split(';'):
        proto = ' '.join(stmt.split())
        if not proto:
            continue
        m = _PROTOTYPE.fullmatch(proto)
        if m is None or m.group(2) in sigs:
            raise EfghError(f'include/efgh_hip.h: `{proto}` is not a prototype the binding can read (or is declared twice)')
        ret, name, params = m.groups()
        params = [] if params.strip() == 'void' else params.split(',')
        sigs[name] = (_ctype(ret, proto, True), [_ctype(p, proto, False) for p in params])
    return sigs


WROTE_OUT = 1            # EFGH_WROTE_OUT


def check_wrote(rc):
    """return code of a weight-gradient entry point -> True when the launch wrote the caller's layout itself (EFGH_WROTE_OUT)"""
    if rc == WROTE_OUT:
        return True
    check(rc)
    return False


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise EfghError(f'{SO_PATH} is missing: run `python -c "import __graft_entry__ as g; '
                            f'g.build()"` (hipcc, gfx950). There is no CPU fallback.')
        import torch  # noqa: F401  (load torch's HIP runtime first so both share one runtime)
        if not os.path.exists(HEADER):
            raise EfghError(f'{HEADER} is missing: the binding takes every signature from it')
        with open(HEADER) as f:
            sigs = signatures(f.read())
        dll = ctypes.CDLL(SO_PATH)
        _bind(dll, {name: sigs[name] for name in ('efgh_version', 'efgh_last_error')})      # what the ABI check itself calls
        if dll.efgh_version() != ABI_VERSION:
            raise EfghError(f'{SO_PATH} has ABI version {dll.efgh_version()}, this package binds version {ABI_VERSION} of '
                            f'include/efgh_hip.h: rebuild it (`python -m efgh_amd.build`)')
        _bind(dll, sigs)
        _lib = dll
    return _lib


def _bind(dll, sigs):
    for name, (restype, argtypes) in sigs.items():
        if not hasattr(dll, name):
            raise EfghError(f'{SO_PATH} has no {name}, which include/efgh_hip.h declares: rebuild it (`python -m efgh_amd.build`)')
        fn = getattr(dll, name)
        fn.restype, fn.argtypes = restype, argtypes


def check(rc):
    if rc != 0:
        raise EfghError(f'libefgh_hip: rc={rc}: {lib().efgh_last_error().decode()}')


def ptr(t):
    """device pointer of a torch tensor (None -> NULL), as the plain value a pointer parameter converts"""
    return None if t is None else t.data_ptr()


_raw_stream = None


def stream_ptr():
    """the current HIP stream of the current device as a raw pointer.  `torch.cuda.current_stream().cuda_stream` builds a Python
    Stream object per call (device-index resolution, `os.environ` look-ups: 2 us x ~600 launches of a batch-1 forward = 15 % of
    its host time, tools/host_profile.py); the private raw getter is the same value without the object"""
    global _raw_stream
    import torch
    if _raw_stream is None:
        get, dev = getattr(torch._C, '_cuda_getCurrentRawStream', None), getattr(torch._C, '_cuda_getDevice', None)
        if get is not None and dev is not None:
            _raw_stream = lambda: get(dev())
        else:                                   # (a torch without the private getters)
            _raw_stream = lambda: torch.cuda.current_stream().cuda_stream
    return _raw_stream()


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise EfghError('efgh_amd runs on the GPU through libefgh_hip.so only (got a CPU tensor); '
                            'there is no CPU fallback')


def require_f32(*tensors):
    """the kernels read raw float32 memory: anything else would be misread silently (the reference's loop casts its inputs
    with .float(), iterater.py:29-32)"""
    import torch
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise EfghError('efgh_amd expects float32 tensors, got %s (cast with .float() as iterater.py:29-32 does)' % t.dtype)
