"""The binding takes every signature from include/efgh_hip.h (efgh_amd/_C.py): every prototype is bound, by the type map and
nothing else; the conversions stop a wrong width or kind before C; and every efgh_* call written in the package has the header's
number of arguments and no hand-made scalar wrapper.  No GPU."""
import ast
import ctypes
import glob
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAPPERS = ('c_int32', 'c_int64', 'c_int', 'c_float', 'c_double')


@pytest.fixture(scope='module')
def header():
    hdr = open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read()
    return re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)


@pytest.fixture(scope='module')
def arity(header):
    """name -> parameter count, read off the header with nothing of the binder's: the text between a prototype's parentheses"""
    protos = re.findall(r'\b(efgh_\w+)\s*\(([^()]*)\)\s*;', header)
    assert len(protos) == len(set(n for n, _ in protos))
    return {n: 0 if p.strip() == 'void' else p.count(',') + 1 for n, p in protos}


def _same(got, want):
    """a struct pointer is POINTER(mirror) or the binding's subclass of it (which also takes a device address)"""
    return got is want or (isinstance(want, type) and issubclass(want, ctypes._Pointer) and issubclass(got, want))


def test_every_prototype_is_bound(arity, header):
    from efgh_amd import _C
    lib = _C.lib()
    sigs = _C.signatures(open(_C.HEADER).read())
    assert sorted(sigs) == sorted(arity) and len(arity) == len(re.findall(r'\befgh_\w+\s*\([^()]*\)\s*;', header)) > 100
    for name, n in arity.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
        assert fn.restype is sigs[name][0] and list(fn.argtypes) == sigs[name][1], name
    returns = {}
    for name in arity:
        returns.setdefault(getattr(lib, name).restype, []).append(name)
    assert set(returns) == {c_int, c_int32, c_int64, c_char_p} and returns[c_char_p] == ['efgh_last_error']
    # the size queries: a 32-bit restype would truncate a workspace size
    assert sorted(returns[c_int64]) == sorted(re.findall(r'\bint64_t\s+(efgh_\w+)\s*\(', header))
    assert sorted(returns[c_int]) == sorted(re.findall(r'\bint(?:32_t)?\s+(efgh_\w+)\s*\(', header))      # (c_int32 is c_int here)


def test_signatures_written_out_by_hand():
    """the table against six signatures typed in here from the header, not against the parser that made it.  Between them: every
    scalar of the map, an int64_t return, struct pointers, `const int64_t *` host arrays and the `char *` parameter"""
    from efgh_amd import _C
    p = c_void_p
    want = {
        'efgh_grad_guard_measure': (c_int, [p, c_int64, p, c_int32, c_double, c_float, c_int32, c_float, c_float, c_int32, p,
                                            POINTER(_C.GuardState), c_int32, p]),
        'efgh_adam_step_groups': (c_int, [p, p, p, p, c_int64, p, p, c_int32, p, p, POINTER(_C.AdamGroups),
                                          POINTER(_C.GuardState), c_int32, p]),
        'efgh_gather_gemm': (c_int, [POINTER(_C.GemmDesc), p]),
        'efgh_lattice_level_build': (c_int, [p, c_int64, p, c_int32, p, c_int32, c_int32, c_float, c_float, p, p, p, p, c_int32,
                                             p, p, p, p, p, c_int64, p]),
        'efgh_lattice_part_workspace_bytes': (c_int64, [c_int32] * 5),
        'efgh_wino2d_wfinish': (c_int, [p, p, c_int32, c_int32, POINTER(_C.WgradOutDesc), p]),
        'efgh_debug_occupancy': (c_int, [p, c_int32]),
        'efgh_lattice_part_max_entries': (c_int32, [c_int32]),
        'efgh_last_error': (c_char_p, []),
        'efgh_version': (c_int, []),
    }
    lib = _C.lib()
    for name, (restype, argtypes) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert len(fn.argtypes) == len(argtypes) and all(_same(g, w) for g, w in zip(fn.argtypes, argtypes)), name


@pytest.mark.parametrize('text, where', [
    ('int efgh_ok(int32_t n);\nint efgh_bad_param(int32_t n, unsigned int flags, void *stream);', 'efgh_bad_param'),
    ('int efgh_bad_size(size_t n);', 'efgh_bad_size'),
    ('int efgh_bad_array(int32_t taps[16]);', 'efgh_bad_array'),
    ('int efgh_bad_pointee(const efgh_no_such_desc *d);', 'efgh_bad_pointee'),
    ('int efgh_bad_unnamed(int32_t);', 'efgh_bad_unnamed'),
    ('int efgh_bad_unnamed_pointer(const float *, void *stream);', 'efgh_bad_unnamed_pointer'),
    ('int efgh_bad_unnamed_void(void *);', 'efgh_bad_unnamed_void'),
    ('int efgh_bad_double_pointer(float **rows);', 'efgh_bad_double_pointer'),
    ('void efgh_bad_return(int32_t n);', 'efgh_bad_return'),
    ('uint32_t efgh_bad_return2(void);', 'efgh_bad_return2'),
    ('static inline int efgh_bad_body(void) { return 0; }', 'efgh_bad_body'),
])
def test_a_type_outside_the_map_is_an_error(text, where):
    from efgh_amd import _C
    with pytest.raises(_C.EfghError, match=where):
        _C.signatures('/* a header */\n#include <stdint.h>\nint efgh_first(const float *x, int64_t n, void *stream);\n' + text)


def test_synthetic_header_binds_by_the_map():
    from efgh_amd import _C
    sigs = _C.signatures('#ifdef __cplusplus\nextern "C" {\n#endif\n// a line comment; with a semicolon\n'
                         'typedef struct efgh_x { int32_t a; /* int b; */ } efgh_x;\n'
                         'const char *efgh_a(void);\nint64_t efgh_b(const efgh_gemm_desc *d,\n   double v /* may be 0 */, char *out);\n'
                         '#ifdef __cplusplus\n}\n#endif\n')
    assert list(sigs) == ['efgh_a', 'efgh_b'] and sigs['efgh_a'] == (c_char_p, [])
    assert sigs['efgh_b'][0] is c_int64 and issubclass(sigs['efgh_b'][1][0], POINTER(_C.GemmDesc))
    assert sigs['efgh_b'][1][1:] == [c_double, c_void_p]


def test_conversions_stop_mistakes_before_c():
    from efgh_amd import _C
    lib = _C.lib()
    assert lib.efgh_lattice_hash_capacity(131072) == 1 << 20
    with pytest.raises(ctypes.ArgumentError):
        lib.efgh_lattice_hash_capacity(131072.0)                 # a float for an int32_t
    with pytest.raises(ctypes.ArgumentError):
        lib.efgh_grad_guard_workspace(c_int32(1))                # a 32-bit wrapper for an int64_t
    assert lib.efgh_grad_guard_workspace(c_int64(1)) == lib.efgh_grad_guard_workspace(1) > 0
    assert lib.efgh_gather_gemm(None, None) == -1                # None reaches C as NULL
    assert b'invalid argument' in lib.efgh_last_error()
    # a pointer to a host struct takes its own mirror by reference and nothing else, not even an address
    assert lib.efgh_gather_gemm(ctypes.byref(_C.GemmDesc()), None) == -1
    for bad in (ctypes.byref(_C.WgradOutDesc()), 1.0, c_int32(0), 4096, c_void_p(4096)):
        with pytest.raises(ctypes.ArgumentError):
            lib.efgh_gather_gemm(bad, None)
    # the structs that live in device memory also come as a tensor's data_ptr(); still no float, wrapper or other struct
    for name, mirror in _C.STRUCTS.items():
        host = name not in _C.DEVICE_STRUCTS
        assert (_C._STRUCT_PTRS[name] is POINTER(mirror)) == host
    state = lib.efgh_adam_step_guarded.argtypes[10]
    assert issubclass(state, POINTER(_C.GuardState))
    for ok in (4096, c_void_p(4096), None, ctypes.byref(_C.GuardState())):
        state.from_param(ok)
    for bad in (ctypes.byref(_C.TxnState()), 1.0, c_int32(0)):
        with pytest.raises(TypeError):
            state.from_param(bad)
    with pytest.raises(TypeError):
        lib.efgh_gather_gemm(None)                               # too few arguments


# ------------------------------------------------------------------------------------------------ the call sites of the package
# calls with a starred argument: (file, entry point) -> the arguments written out beside the star; their totals are fixed where
# the star's tuple is built (lattice._launch_build's head, PoseLossFn.backward's seven gradients, the sweep set's lead arguments)
STARRED = {('lattice.py', 'efgh_lattice_part_build'): 12, ('lattice.py', 'efgh_lattice_level_build'): 13,
           ('losses/efghloss.py', 'efgh_pose_loss_bwd'): 6, ('data/prepare.py', 'efgh_prep_sweeps_materialize'): 4}


def _names(func):
    """the entry point(s) a call's function expression names: X.efgh_NAME, or (X.efgh_A if p else Y.efgh_B)"""
    if isinstance(func, ast.Attribute) and func.attr.startswith('efgh_'):
        return [func.attr]
    if isinstance(func, ast.IfExp):
        a, b = _names(func.body), _names(func.orelse)
        return a + b if a and b else []
    return []


def _calls():
    pkg = os.path.join(ROOT, 'efgh_amd')
    for path in sorted(glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True)):
        tree = ast.parse(open(path).read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call):
                for name in _names(node.func):
                    yield os.path.relpath(path, pkg), name, node


def test_call_sites_have_the_headers_arity(arity):
    seen, starred = 0, {}
    for rel, name, node in _calls():
        assert name in arity, (rel, node.lineno, name)
        assert not node.keywords, (rel, node.lineno, name)
        if any(isinstance(a, ast.Starred) for a in node.args):
            starred[(rel, name)] = len(node.args) - 1
            assert len(node.args) - 1 < arity[name]
            continue
        assert len(node.args) == arity[name], '%s:%d %s takes %d arguments' % (rel, node.lineno, name, arity[name])
        seen += 1
    assert starred == STARRED
    assert seen > 150        # (the walk sees the package: 165 calls written out in full)


# The calls the walk above cannot resolve: the entry point is fetched by getattr from a name held in a variable.  Every such site of the
# package is on this list, with the entry points it can reach and the arguments that reach C: (file, the getattr's name variable) ->
# {entry point: arguments written at the site (+ those of the tuples spliced in)}.
#   ops.gather_wgrad: the six families of ops._WGRAD_ENTRY, (desc, G, ldg, dWp, workspace, out desc, stream) and (desc)
#   prepare._Rows.call: getattr(_L(), name)(*lead, *args, _st()); lead is 1 / 3 arguments for a resident tensor (filter and gather /
#   thin), the 7 of SweepSet._args for a sweep set; args are the call's own: filter 6 + the box (1 resident, 3 sweep set), thin 7,
#   gather 8 (+ the kept-row count for a sweep set)
SWEEP_LEAD = 7
INDIRECT = {
    ('ops.py', 'entry'): {n: 7 for n in ('efgh_c4n4_wgrad', 'efgh_thin_wgrad', 'efgh_sc_wgrad', 'efgh_c4_wgrad', 'efgh_gather_wgrad')},
    ('ops.py', 'workspace'): {n + '_workspace': 1 for n in ('efgh_c4n4_wgrad', 'efgh_thin_wgrad', 'efgh_sc_wgrad', 'efgh_c4_wgrad',
                                                            'efgh_gather_wgrad')},
    ('data/prepare.py', 'name'): {
        'efgh_prep_radius_filter': 1 + 6 + 1 + 1, 'efgh_prep_sweeps_filter': SWEEP_LEAD + 6 + 3 + 1,
        'efgh_prep_voxel_keep': 3 + 7 + 1, 'efgh_prep_sweeps_voxel_keep': SWEEP_LEAD + 7 + 1,
        'efgh_prep_gather_transform': 1 + 8 + 1, 'efgh_prep_sweeps_gather_transform': SWEEP_LEAD + 1 + 8 + 1},
}
# what the sums above take from the source: the arguments written at each _Rows.call site, the stars beside them, the lead tuples
ROWS_CALLS = {'filter': (6, 1), 'thin': (7, 0), 'gather': (8, 1)}


def _getattr_calls():
    """(file, name variable, call node) of every call of the package whose function is getattr(X, <variable>)"""
    pkg = os.path.join(ROOT, 'efgh_amd')
    for path in sorted(glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True)):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            f = node.func if isinstance(node, ast.Call) else None
            if isinstance(f, ast.Call) and isinstance(f.func, ast.Name) and f.func.id == 'getattr' and len(f.args) == 2 \
                    and not isinstance(f.args[1], ast.Constant):
                yield os.path.relpath(path, pkg), ast.unparse(f.args[1]), node


def test_calls_through_getattr_are_listed_with_the_headers_arity(arity):
    sites = {(rel, var): node for rel, var, node in _getattr_calls()}
    assert set(sites) == set(INDIRECT)                          # a new indirect call site fails here until it is listed
    for names in INDIRECT.values():
        for name, n in names.items():
            assert arity[name] == n, (name, n, arity[name])
    # the list against the source it describes
    from efgh_amd import ops
    assert {e for e, _ in ops._WGRAD_ENTRY.values()} == set(INDIRECT[('ops.py', 'entry')])
    assert {w for _, w in ops._WGRAD_ENTRY.values()} == set(INDIRECT[('ops.py', 'workspace')])
    assert len(sites[('ops.py', 'entry')].args) == 7 and len(sites[('ops.py', 'workspace')].args) == 1
    tree = ast.parse(open(os.path.join(ROOT, 'efgh_amd', 'data', 'prepare.py')).read())
    rows_calls, leads = {}, {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'call' and node.args \
                and isinstance(node.args[0], ast.Attribute) and node.args[0].attr in ROWS_CALLS:
            rest = node.args[1:]
            rows_calls[node.args[0].attr] = (sum(not isinstance(a, ast.Starred) for a in rest), sum(isinstance(a, ast.Starred) for a in rest))
        if isinstance(node, ast.Tuple) and len(node.elts) == 2 and isinstance(node.elts[0], ast.Constant) \
                and str(node.elts[0].value).startswith('efgh_prep_') and isinstance(node.elts[1], ast.Tuple):
            leads[node.elts[0].value] = len(node.elts[1].elts)
        if isinstance(node, ast.FunctionDef) and node.name == '_args':          # SweepSet._args: return pts, (the lead arguments)
            ret = [n for n in ast.walk(node) if isinstance(n, ast.Return)][-1].value
            leads['sweep set'] = len(ret.elts[1].elts)
    assert rows_calls == ROWS_CALLS
    assert leads == {'efgh_prep_radius_filter': 1, 'efgh_prep_gather_transform': 1, 'efgh_prep_voxel_keep': 3, 'sweep set': SWEEP_LEAD}
    assert [len(a.args) for a in [sites[('data/prepare.py', 'name')]]] == [3]      # (*lead, *args, _st())
    # no hand-made scalar wrapper at these sites either
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'call']
    for node in list(sites.values()) + calls + [n for n in ast.walk(tree) if isinstance(n, ast.Tuple)]:
        for a in (node.args if isinstance(node, ast.Call) else node.elts):
            f = a.func if isinstance(a, ast.Call) else None
            assert (f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None) not in WRAPPERS, ast.unparse(node)


def test_entry_points_named_in_strings_exist(arity):
    """the calls made through getattr (ops' weight-gradient families, the prep steps of a point source) name their entry point in
    a string: every such name is the header's (their argument counts: the test above)"""
    from efgh_amd import _C
    pkg = os.path.join(ROOT, 'efgh_amd')
    named = set()
    for path in sorted(glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True)):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r'efgh_[a-z0-9_]+', node.value) \
                    and node.value not in _C.STRUCTS:          # (the struct typedefs' names, keys of _C.STRUCTS)
                named.add(node.value)
                prefix = node.value.endswith('_') and any(n.startswith(node.value) for n in arity)      # 'efgh_prep_sweeps_' + step
                assert node.value in arity or prefix, (os.path.relpath(path, pkg), node.lineno, node.value)
    assert 'efgh_prep_voxel_keep' in named and 'efgh_version' in named


def test_no_scalar_wrapper_left_in_a_call():
    for rel, name, node in _calls():
        for a in node.args:
            a = a.value if isinstance(a, ast.Starred) else a
            f = a.func if isinstance(a, ast.Call) else None
            wrapper = f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None
            assert wrapper not in WRAPPERS, '%s:%d %s(... %s(...) ...)' % (rel, node.lineno, name, wrapper)
