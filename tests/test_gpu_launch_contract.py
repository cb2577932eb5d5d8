"""Every gather-GEMM launch of real training steps and eval forwards, checked against the float64 contract of tests/gemm_contract.py.

ops.gather_gemm and ops.gather_wgrad - the two entry points every convolution, linear layer and BCL blur of the model goes through -
are wrapped for the duration of a run; ops._L is replaced by a proxy that records which C entry points each launch called.  Each
launch is compared at its real shape, with its real data, strides and offsets, whichever kernel served it: the written region within
tau[family] * S, every element of the destination outside the declared write set bit-unchanged, the statistics epilogue and the
returned BatchNorm-backward partials.  The runs: (a) the golden size, (b) config R, (c) config R with every activation materialised,
then again on the split-bf16 planes, (d) config S at batch 2 and its eval forward, (e) the E net at BCL radius 2.
The operands of the launches recorded as `unchecked (pre_v / pre_gy)` - Vd and Gy of efgh_wino2d_bwd_transforms(_pooled) - are held
element by element by tests/w2_contract.py (tests/test_gpu_w2_contract.py)."""
import threading
import time

import pytest
import torch

import gemm_contract as GC
from efgh_amd import synthetic as syn

pytestmark = pytest.mark.gpu

# entry points the runs together must reach
REQUIRED = [
    'efgh_gather_gemm', 'efgh_thin_gemm', 'efgh_c4_conv3x3', 'efgh_c4_conv3x3_pooled', 'efgh_sc_conv3x3', 'efgh_wino_conv3x3',
    'efgh_wino_conv3x3_hpool',
    'efgh_wino2d_input', 'efgh_wino2d_input_act', 'efgh_wino2d_output', 'efgh_wino2d_output_pooled',
    'efgh_plane_gemm', 'efgh_plane_gemm_x6', 'efgh_fold_planes', 'efgh_blur_r_gemm',
    'efgh_gather_wgrad', 'efgh_thin_wgrad', 'efgh_c4n4_wgrad', 'efgh_c4_wgrad', 'efgh_sc_wgrad', 'efgh_wino_wgrad',
    'efgh_plane_wgrad_batched', 'efgh_plane_wgrad_x6_batched', 'efgh_wino2d_wfinish', 'efgh_blur_r_wgrad',
]
# those no model run reaches, with the reason and the unit test that covers them
NOT_REACHED = {}
# size and query functions: not launches
_QUERIES = ('_supported', '_workspace', '_tiles', '_stats_rows', '_grid_m', '_groups', 'efgh_last_error', 'efgh_version')

RESULTS = {}             # run name -> list of launch records


def _shares(a, b):
    return a is not None and b is not None and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


class _Proxy:
    """ops._L() stand-in: forwards every attribute of the library, logging the efgh_* entry points to the open launch frames"""

    def __init__(self, lib, rec):
        self._lib, self._rec = lib, rec

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name.startswith('efgh_') and not any(q in name for q in _QUERIES):
            for fr in getattr(self._rec.tls, 'stack', ()):
                fr.append(name)
        return f


class Recorder:
    """wraps ops.gather_gemm / ops.gather_wgrad and ops._L for the life of the monkeypatch it is given; one record per launch"""

    def __init__(self, monkeypatch):
        from efgh_amd import ops
        self.tls = threading.local()
        self.launches = []
        self.lock = threading.Lock()
        self.t_check = 0.0
        self.real_gemm, self.real_wgrad = ops.gather_gemm, ops.gather_wgrad
        proxy = _Proxy(ops._L(), self)
        monkeypatch.setattr(ops, '_L', lambda: proxy)
        monkeypatch.setattr(ops, 'gather_gemm', self.gemm)
        monkeypatch.setattr(ops, 'gather_wgrad', self.wgrad)

    def _call(self, fn, args, kwargs):
        st = self.tls.__dict__.setdefault('stack', [])
        fr = []
        st.append(fr)
        try:
            return fn(*args, **kwargs), fr
        finally:
            st.pop()

    def _record(self, kind, L, calls, chk, unchecked=None, inplace=False):
        geom = L.get('geom')
        feats = {'in-place residual': inplace, 'channel slice of out': kind == 'gemm' and (L['out_off'] > 0 or L['ldo'] > L['N']),
                 'transposed-conv class': geom is not None and len(geom) > 11 and geom[11] == 2,
                 'pooled epilogue': bool(L.get('pool')), 'statistics epilogue': L.get('stats') is not None,
                 'BatchNorm-backward sums': bool(chk and chk.get('bn')), 'lazy operand': L.get('lazy') is not None,
                 'caller-layout weight gradient': kind == 'wgrad' and bool(chk and chk.get('done'))}
        rec = dict(kind=kind, calls=tuple(sorted(set(calls))), family=GC.family_of(calls), mode=L['mode'], M=L['M'], N=L['N'],
                   T=L['T'], C=L['C'], geom=None if geom is None else tuple(geom[:7]) + tuple(geom[9:]), unchecked=unchecked,
                   feats={k for k, v in feats.items() if v}, **(chk or {}))
        with self.lock:
            self.launches.append(rec)

    def gemm(self, *args, **kwargs):
        L = GC.bind(self.real_gemm, args, kwargs)
        if L['pre_v'] is not None or L['A'] is None:
            r, calls = self._call(self.real_gemm, args, kwargs)
            self._record('gemm', L, calls, None, unchecked='pre_v')
            return r
        torch.cuda.synchronize()
        out = L['out']
        before = GC.flat(out).clone()
        A = GC.flat(L['A']).clone() if _shares(L['A'], out) else None
        res = GC.flat(L['residual']).clone() if _shares(L['residual'], out) else None      # in-place accumulation
        r, calls = self._call(self.real_gemm, args, kwargs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tau = GC.TAU[GC.family_of(calls)]
        chk = GC.check_forward(L, GC.flat(out), before, tau, A=A, residual=res)
        chk['ratio'] /= tau
        chk['bn'] = GC.check_bn_bwd(L, GC.flat(out), r) if r is not None else None
        torch.cuda.synchronize()
        self.t_check += time.perf_counter() - t0
        self._record('gemm', L, calls, chk, inplace=res is not None)
        return r

    def wgrad(self, *args, **kwargs):
        L = GC.bind(self.real_wgrad, args, kwargs)
        if L['pre_gy'] is not None or L['G'] is None:
            r, calls = self._call(self.real_wgrad, args, kwargs)
            self._record('wgrad', L, calls, None, unchecked='pre_gy')
            return r
        torch.cuda.synchronize()
        up = L['unpack']
        dW_before = GC.flat(up[0]).clone() if up is not None else None
        done, calls = self._call(self.real_wgrad, args, kwargs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fam = GC.family_of(calls)
        tau = GC.TAU[fam]
        chk = GC.check_wgrad(L, done, tau, dW_before, rows=fam == 'wino1d')
        chk['ratio'] /= tau
        chk['stats'] = chk['bn'] = None
        chk['done'] = bool(done)
        torch.cuda.synchronize()
        self.t_check += time.perf_counter() - t0
        self._record('wgrad', L, calls, chk)
        return done

    def finish(self, name, t_run, materialised=False):
        """assert over the run's launches, keep them for the summary"""
        lst = self.launches
        assert lst, name
        checked = [r for r in lst if r['unchecked'] is None]
        bad = [r for r in checked if r['bad'] or r['wild'] or (r['stats'] and r['stats'][1]) or (r['bn'] and r['bn'][1])]
        unchecked = [r for r in lst if r['unchecked'] is not None]
        worst = max(checked, key=lambda r: r['ratio'])
        print(f'\n[{name}] {len(lst)} launches, {len(unchecked)} unchecked (pre_v / pre_gy), worst {worst["ratio"]:.3f} x tau '
              f'({worst["kind"]} {"+".join(worst["calls"])} M={worst["M"]} N={worst["N"]} T={worst["T"]} C={worst["C"]}); '
              f'run {t_run:.1f} s of which checks {self.t_check:.1f} s; statistics worst '
              f'{max([r["stats"][0] for r in checked if r["stats"]] or [0]):.3f}, BatchNorm-backward sums worst '
              f'{max([r["bn"][0] for r in checked if r["bn"]] or [0]):.3f} x tau')
        RESULTS[name] = lst
        assert not bad, [(r['kind'], r['calls'], r['mode'], r['M'], r['N'], r['T'], r['C'], r['geom'], r['ratio'], r['bad'], r['wild'],
                          r['stats'], r['bn']) for r in bad[:10]]
        assert all(r['unchecked'] in ('pre_v', 'pre_gy') for r in unchecked)
        if materialised:
            assert not unchecked, len(unchecked)


def _inputs(raw, npts, batch):
    b = syn.make_batch(raw, npts, batch)
    inp = [torch.from_numpy(b[k]).cuda() for k in ('pc', 'img', 'calib', 'A')]
    gt = {k: torch.from_numpy(v) for k, v in b['gt'].items()}
    return inp, gt


def _model(manifest, raw, args_over=None):
    from efgh_amd.nets import EFGHBackbone
    args = dict(syn.default_args(raw, 'cuda'), **(args_over or {}))
    torch.manual_seed(0)
    m = EFGHBackbone(args)
    if manifest is not None:
        m.load_state_dict(syn.synthetic_state_dict(manifest['state_dict'], 1), strict=True)
    return m.cuda(), args


def _train_step(m, args, inp, gt):
    from efgh_amd.losses import EFGHCriterion
    m.train()
    m.zero_grad(set_to_none=True)
    pred = m(*inp)
    L, _ = EFGHCriterion(args).compute_loss(inp[0], inp[1], inp[2], inp[3], gt, pred)
    L['total'].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(L['total'])


def _eval_forward(m, inp):
    m.eval()
    with torch.no_grad():
        m(*inp)
    torch.cuda.synchronize()


def _run(name, monkeypatch, body, materialised=False):
    t0 = time.perf_counter()
    with monkeypatch.context() as mp:
        rec = Recorder(mp)
        body()
    rec.finish(name, time.perf_counter() - t0, materialised=materialised)
    torch.cuda.empty_cache()


def test_run_a_golden_size(manifest, monkeypatch):
    """RAW (128, 256), 2048 points: a training step and an eval forward, default switches"""
    m, args = _model(manifest, (128, 256))
    inp, gt = _inputs((128, 256), 2048, 1)
    _run('a golden train', monkeypatch, lambda: _train_step(m, args, inp, gt))
    _run('a golden eval', monkeypatch, lambda: _eval_forward(m, inp))


def test_run_b_config_r(manifest, monkeypatch):
    """config R (900 x 1600, 65536 points, batch 1): a training step, default switches"""
    m, args = _model(manifest, (900, 1600))
    inp, gt = _inputs((900, 1600), 65536, 1)
    _run('b config R train', monkeypatch, lambda: _train_step(m, args, inp, gt))


def test_run_c_config_r_materialised_and_split(manifest, monkeypatch):
    """config R with LAZY_ACT / W2_BWD_FUSED / W2_BWD_FUSED_POOL off (every operand materialised: nothing left unchecked), then
    once more with the plane GEMMs on the split-bf16 form"""
    from efgh_amd import ops
    m, args = _model(manifest, (900, 1600))
    inp, gt = _inputs((900, 1600), 65536, 1)
    for k in ('LAZY_ACT', 'W2_BWD_FUSED', 'W2_BWD_FUSED_POOL'):
        monkeypatch.setattr(ops, k, False)
    _run('c config R materialised', monkeypatch, lambda: _train_step(m, args, inp, gt), materialised=True)
    monkeypatch.setattr(ops, 'PLANES_SPLIT', True)
    h0 = list(ops.PLANE_SPLIT_HITS)
    _run('c config R split planes', monkeypatch, lambda: _train_step(m, args, inp, gt), materialised=True)
    assert ops.PLANE_SPLIT_HITS[0] > h0[0] and ops.PLANE_SPLIT_HITS[1] > h0[1]


def test_run_d_config_s(manifest, monkeypatch):
    """config S (768 x 2560, 131072 points): a training step at batch 2, and an eval forward at batch 1 (pooled epilogues)"""
    m, args = _model(manifest, (768, 2560))
    inp, gt = _inputs((768, 2560), 131072, 2)
    _run('d config S train b2', monkeypatch, lambda: _train_step(m, args, inp, gt))
    inp1, _ = _inputs((768, 2560), 131072, 1)
    _run('d config S eval b1', monkeypatch, lambda: _eval_forward(m, inp1))


def test_run_e_bcl_radius_2(monkeypatch):
    """the E net with scale_map radius 2 on one level (tests/test_gpu_bcl_radius.py): the radius-r blur and its weight gradient"""
    scales = (1.0, 0.75, 0.5, 0.25, 0.125)
    m, args = _model(None, (128, 256), dict(scale_map=[[s, r] for s, r in zip(scales, (2, 1, 1, 1, 1))]))
    inp, gt = _inputs((128, 256), 2048, 1)
    _run('e radius 2 train', monkeypatch, lambda: _train_step(m, args, inp, gt))


def test_entry_point_coverage_and_summary():
    """the runs together reach every entry point of REQUIRED (or NOT_REACHED names why not); one line per kernel family"""
    runs = ('a golden train', 'a golden eval', 'b config R train', 'c config R materialised', 'c config R split planes',
            'd config S train b2', 'd config S eval b1', 'e radius 2 train')
    missing_runs = [r for r in runs if r not in RESULTS]
    assert not missing_runs, f'run the whole module: {missing_runs} did not run'
    allr = [r for lst in RESULTS.values() for r in lst]
    reached = set(c for r in allr for c in r['calls'])
    fams = {}
    for r in allr:
        f = fams.setdefault((r['kind'], '+'.join(r['calls'])), dict(n=0, shapes=set(), worst=0.0, unchecked=0, fam=r['family'], K=0))
        f['n'] += 1
        f['shapes'].add((r['mode'], r['M'], r['N'], r['T'], r['C'], r['geom']))
        f['K'] = max(f['K'], r['T'] * r['C'])
        if r['unchecked'] is None:
            f['worst'] = max(f['worst'], r['ratio'])
        else:
            f['unchecked'] += 1
    print()
    for (kind, calls), f in sorted(fams.items()):
        print(f'{kind:5s} {f["fam"]:12s} {calls:70s} launches {f["n"]:5d}  shapes {len(f["shapes"]):4d}  max K {f["K"]:5d}  '
              f'worst {f["worst"]:.3f} x tau  unchecked {f["unchecked"]}')
    for fam in GC.TAU:
        ks = [r for r in allr if r['family'] == fam and r['unchecked'] is None]
        if ks:
            w = max(ks, key=lambda r: r['ratio'])
            print(f'tau[{fam}] = {GC.TAU[fam]:.1e}: observed max |got - ref| / S = {w["ratio"] * GC.TAU[fam]:.2e} '
                  f'({len(ks)} launches, largest K {max(r["T"] * r["C"] for r in ks)})')
    feats = {}
    for r in allr:
        for f in r['feats']:
            feats[f] = feats.get(f, 0) + 1
    print('launches with', ', '.join(f'{k}: {v}' for k, v in sorted(feats.items())))
    # the production combinations no unit test names: each met at least once
    assert set(feats) >= {'in-place residual', 'channel slice of out', 'transposed-conv class', 'pooled epilogue', 'statistics epilogue',
                          'BatchNorm-backward sums', 'lazy operand', 'caller-layout weight gradient'}, feats
    for key in ('stats', 'bn_sums'):
        v = [r['stats' if key == 'stats' else 'bn'][0] for r in allr if r.get('stats' if key == 'stats' else 'bn')]
        if v:
            print(f'tau[{key}] = {GC.TAU[key]:.1e}: observed max relative error {max(v) * GC.TAU[key]:.2e} ({len(v)} launches)')
    missing = [e for e in REQUIRED if e not in reached and e not in NOT_REACHED]
    assert not missing, missing
