"""CPU-side checks of the split-bf16 plane GEMMs (fp32 'high' matmul precision): the two C-ABI entry points, the one resolver of
the mode (ops.planes_split_active) against both of torch's APIs and the ops.PLANES_SPLIT override, and the launcher's
--fp32-precision flag in one process and in the children of a --gpus N run."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X6 = ('efgh_plane_gemm_x6', 'efgh_plane_wgrad_x6_batched')


@pytest.fixture(scope='module')
def so_path():
    from efgh_amd import build
    return build.build()


def _decl(hdr, name):
    m = re.search(r'\bint ' + name + r'\(([^;]*)\);', hdr)
    assert m, name
    return ' '.join(m.group(1).split())


def test_header_declares_and_library_exports_the_x6_entry_points(so_path):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'efgh_hip.h')).read(), flags=re.S)
    assert _decl(hdr, 'efgh_plane_gemm_x6') == _decl(hdr, 'efgh_plane_gemm')
    assert _decl(hdr, 'efgh_plane_wgrad_x6_batched') == _decl(hdr, 'efgh_plane_wgrad_batched')
    assert int(re.search(r'#define\s+EFGH_ABI_VERSION\s+(\d+)', hdr).group(1)) == 4
    lib = ctypes.CDLL(so_path)
    for n in X6:
        assert hasattr(lib, n), n
    # argument validation before any device work, as the exact forms
    lib.efgh_last_error.restype = ctypes.c_char_p
    assert lib.efgh_plane_gemm_x6(None, ctypes.c_int32(0), None) == -1
    assert b'invalid argument' in lib.efgh_last_error()
    assert lib.efgh_plane_wgrad_x6_batched(None, None, ctypes.c_int64(128), ctypes.c_int64(0), None, ctypes.c_int64(0), None,
                                           ctypes.c_int32(0), None) == -1


@pytest.fixture
def torch_precision():
    """restores torch's switch with the API that set it (the legacy call and the fp32_precision properties)"""
    m = torch.backends.cuda.matmul
    saved = (torch.backends.fp32_precision, m.fp32_precision)
    yield
    torch.backends.fp32_precision = saved[0]
    m.fp32_precision = saved[1]


def test_planes_split_follows_torch_and_the_override(torch_precision):
    from efgh_amd import ops
    m = torch.backends.cuda.matmul
    assert ops.PLANES_SPLIT is None                           # default: follow torch
    try:
        torch.backends.fp32_precision = 'ieee'
        m.fp32_precision = 'ieee'
        assert ops.planes_split_active() is False
        torch.set_float32_matmul_precision('high')            # legacy API
        assert ops.planes_split_active() is True
        torch.set_float32_matmul_precision('medium')
        assert ops.planes_split_active() is True
        torch.set_float32_matmul_precision('highest')
        assert ops.planes_split_active() is False
        m.fp32_precision = 'tf32'                              # new API, matmul backend
        assert ops.planes_split_active() is True
        m.fp32_precision = 'ieee'
        assert ops.planes_split_active() is False
        m.fp32_precision = 'none'                              # 'none' inherits the generic switch
        torch.backends.fp32_precision = 'tf32'
        assert ops.planes_split_active() is True
        torch.backends.fp32_precision = 'ieee'
        assert ops.planes_split_active() is False
        # (both APIs used: the resolver must not call torch.get_float32_matmul_precision, which raises then)
        torch.set_float32_matmul_precision('high')
        m.fp32_precision = 'tf32'
        assert ops.planes_split_active() is True
        ops.PLANES_SPLIT = False
        assert ops.planes_split_active() is False
        m.fp32_precision = 'ieee'
        ops.PLANES_SPLIT = True
        assert ops.planes_split_active() is True
    finally:
        ops.PLANES_SPLIT = None


def test_planes_split_tls_overrides_the_live_switch(torch_precision):
    """inside a layer (GemmLayerFn) the mode resolved by its forward holds, whatever torch's switch says meanwhile"""
    from efgh_amd import ops
    torch.backends.cuda.matmul.fp32_precision = 'ieee'
    assert ops.TLS.planes_split is None and ops._planes_split_now() is False
    ops.TLS.planes_split = True
    try:
        assert ops._planes_split_now() is True
    finally:
        ops.TLS.planes_split = None


def test_launcher_parses_fp32_precision():
    from efgh_amd import run
    assert run.parse(['s.py', 'a'])[5] is None
    assert run.parse(['--fp32-precision', 'high', 's.py', 'a'])[3:] == ('s.py', ['a'], 'high')
    assert run.parse(['--gpus', '2', '--fp32-precision=highest', 's.py'])[2:] == (2, 's.py', [], 'highest')
    assert run.parse(['s.py', '--fp32-precision', 'high'])[4:] == (['--fp32-precision', 'high'], None)      # the script's own argument
    with pytest.raises(SystemExit):
        run.parse(['--fp32-precision', 'tf32', 's.py'])


_SCRIPT = ('import json, os, sys, torch\n'
           'json.dump({"p": torch.backends.cuda.matmul.fp32_precision, "argv": sys.argv[1:]},\n'
           '          open(sys.argv[1] + ".r" + os.environ.get("RANK", "x"), "w"))\n')


def _run(tmp_path, launcher_args):
    (tmp_path / 'main.py').write_text(_SCRIPT)
    out = str(tmp_path / 'out')
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES='', EFGH_DIST_BACKEND='gloo')
    env.pop('CUDA_VISIBLE_DEVICES', None)
    env.pop('RANK', None)
    subprocess.check_call([sys.executable, '-m', 'efgh_amd.run'] + launcher_args + [str(tmp_path / 'main.py'), out], env=env,
                          cwd=str(tmp_path), timeout=300)
    return out


def test_launcher_sets_fp32_precision_in_process(tmp_path):
    out = _run(tmp_path, ['--fp32-precision', 'high'])
    r = json.load(open(out + '.rx'))
    assert r['p'] == 'tf32' and r['argv'] == [out]
    out = _run(tmp_path, [])
    assert json.load(open(out + '.rx'))['p'] != 'tf32'          # without the flag: torch's default


def test_launcher_passes_fp32_precision_to_the_children(tmp_path):
    out = _run(tmp_path, ['--gpus', '2', '--fp32-precision', 'high'])
    for r in range(2):
        got = json.load(open(out + '.r%d' % r))
        assert got['p'] == 'tf32' and got['argv'] == [out]


def test_spawn_hands_the_flag_to_every_child(monkeypatch):
    from efgh_amd import run
    seen = []

    class P:
        def __init__(self, cmd, env=None):
            seen.append(cmd)

        def poll(self):
            return 0
    monkeypatch.setattr(subprocess, 'Popen', P)
    monkeypatch.setenv('HIP_VISIBLE_DEVICES', '0,1')
    argv = ['--gpus', '2', '--fp32-precision', 'high', 'main.py', 'cfg.yaml']
    assert run.spawn(2, argv) == 0
    assert len(seen) == 2
    for cmd in seen:
        assert cmd[cmd.index('--fp32-precision') + 1] == 'high'
