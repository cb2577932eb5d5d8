"""Thinning on a voxel grid (efgh_prep_voxel_keep / efgh_prep_sweeps_voxel_keep, include/efgh_hip.h), restated in numpy.

The contract.  The candidates are rows j = 0 .. n-1 in kept order: what the ego box and the radius filter leave
(tests/sweeps_contract.py `chain`), or the lidar-line list, or 0 .. n-1.  Row j stands at q: the float64 position of
sweeps_contract.positions for a sweep set (the own sweep untouched), (double)p for a plain float32 array; always before the
RELLIS flip and before rand_init_l.  Per axis t = floor(q / v), float64, IEEE division.  A row is representable when its
three t are finite and |t| < 2^20; its key is (tx + 2^20) | (ty + 2^20) << 21 | (tz + 2^20) << 42.  Row j is kept when it is
not representable, or when no row j' < j has its key.  Output: the kept rows' source indices, ascending in j.

Nothing here is taken from an implementation's output.  numpy is the yardstick: `keep` is checked against
np.unique(..., return_index=True) in tests/test_voxel_host.py.

The hash table the kernels use is part of the interface only so that directed fixtures can be built: cap = the smallest power of
two >= 2 n (at least 2), home slot = mix64(key) & (cap - 1), linear probing +1 with wrap.  `collision_fixture` and
`wrap_fixture` pick voxels by that rule; the kept rows never depend on it.

The margin.  The transformed position of a neighbouring sweep is fixed by no single evaluation (tests/sweeps_contract.py: two
evaluations differ by at most GAMMA . sum|terms|, about 1e-13 at the magnitudes used here), so a fixture with a non-identity
transform must keep every q / v further than MARGIN = 1e-9 from an integer: then every evaluation gives the same voxel and no
row has to be left out of a comparison.  `margin` measures it, for every row and axis.
"""
import numpy as np

from tests import sweeps_contract as SC

LIM = 1 << 20
MARGIN = 1e-9
_M64 = (1 << 64) - 1
FAULTS = ('trunc', 'last_seen', 'f32_division', 'merge_unrepresentable', 'unstable')


def mix64(x):
    x &= _M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x


def capacity(n):
    cap = 2
    while cap < 2 * n:
        cap <<= 1
    return cap


def home(key, cap):
    return mix64(int(key)) & (cap - 1)


def pack(tx, ty, tz):
    return (int(tx) + LIM) | (int(ty) + LIM) << 21 | (int(tz) + LIM) << 42


def indices(q, v, fault=None):
    """t = floor(q / v) per axis, float64 [n, 3]"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if fault == 'f32_division':
            return np.floor((q.astype(np.float32) / np.float32(v)).astype(np.float64))
        if fault == 'trunc':
            return np.trunc(q / float(v))
        return np.floor(q / float(v))


def keys(q, v, fault=None):
    """-> (key [n] as python ints in an object array, representable [n] bool); the key of an unrepresentable row is None"""
    t = indices(q, v, fault)
    with np.errstate(invalid='ignore'):
        rep = np.isfinite(t).all(axis=1) & (np.abs(t) < LIM).all(axis=1)        # tested in float64, before any integer cast
    out = np.empty(t.shape[0], object)
    for j in range(t.shape[0]):
        out[j] = pack(*t[j]) if rep[j] else None
    return out, rep


def keep(q, v, fault=None):
    """the kept candidates j, ascending: the unrepresentable rows and the first row of every key"""
    key, rep = keys(q, v, fault)
    owner = {}
    alone = []
    for j in range(key.size):
        k = key[j]
        if not rep[j]:
            if fault != 'merge_unrepresentable':
                alone.append(j)
                continue
            k = 'unrepresentable'
        if k not in owner or fault == 'last_seen':
            owner[k] = j
    if fault == 'unstable':                                 # grouped by voxel, not by row
        return np.array(alone + [owner[k] for k in sorted(owner, key=str)], np.int64)
    return np.array(sorted(alone + list(owner.values())), np.int64)


def margin(q, v):
    """the smallest distance of q / v from an integer over every finite entry (inf when there is none)"""
    r = np.asarray(q, np.float64) / float(v)
    r = r[np.isfinite(r)]
    return float(np.abs(r - np.rint(r)).min()) if r.size else float('inf')


def radius_margin(c):
    """the smallest distance of a transformed x or y from +-radius (the radius test is the other place where the evaluation of q
    could decide; inf without a radius or without a neighbouring sweep)"""
    if c['radius'] is None or len(c['sweeps']) < 2:
        return float('inf')
    q = SC.positions(c['sweeps'], c['transforms'], c['own_order'], c['ego_box'])[0][c['sweeps'][0].shape[0]:]
    return float(np.abs(np.abs(q[:, :2]) - c['radius']).min()) if q.size else float('inf')


# ---- cases: a dict per case, the arguments of SweepSet / preproc_pcd and of `expected` ------------------------------------
def case(sweeps, v, transforms=(), exact=False, **kw):
    c = {'sweeps': [np.ascontiguousarray(s, np.float32) for s in sweeps], 'transforms': [np.asarray(T, np.float64) for T in transforms],
         'v': float(v), 'exact': exact, 'ego_box': None, 'lidar_line': None, 'radius': None, 'flip_xy': False, 'own_order': None}
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def candidates(c):
    """-> (cand: the candidate rows of the concatenation in kept order, q [n_total, 3] float64)"""
    n_total = sum(s.shape[0] for s in c['sweeps'])
    r = SC.chain(c['sweeps'], c['transforms'], np.eye(4), n_total, c['own_order'], c['ego_box'], c['lidar_line'], c['radius'],
                 c['flip_xy'])
    q = SC.positions(c['sweeps'], c['transforms'], c['own_order'], c['ego_box'])[0]
    return r['keep'].astype(np.int64), q


def expected(c, fault=None):
    """the kept rows of the concatenation, int32, in order"""
    cand, q = candidates(c)
    return cand[keep(q[cand], c['v'], fault)].astype(np.int32)


def centre(t, v):
    """the centre of voxel t: exact in float32 for v = 0.25 and |t| < 2^20"""
    return (np.asarray(t, np.float64) + 0.5) * v


def _rows(tlist, v, cols=4):
    p = np.zeros((len(tlist), cols), np.float32)
    p[:, :3] = centre(np.array(tlist, np.float64).reshape(-1, 3), v)
    if cols == 4:
        p[:, 3] = 0.5
    return p


def chain_keys(n_rows, slot, length, start=0):
    """`length` distinct voxels (tx, 0, 0), tx >= start, whose home slot in the table of n_rows candidates is `slot`"""
    cap, out, tx = capacity(n_rows), [], start
    while len(out) < length:
        if home(pack(tx, 0, 0), cap) == slot:
            out.append((tx, 0, 0))
        tx += 1
        assert tx < LIM
    return out


def collision_fixture(v=0.25):
    """14 rows, cap 32: four voxels on home slot 5 and three on slot 6 (which the first chain runs over), each voxel seen twice, the
    second time in the opposite order"""
    n = 14
    a, b = chain_keys(n, 5, 4), chain_keys(n, 6, 3)
    order = a + b
    return case([_rows(order + order[::-1], v)], v, exact=True), {'n': n, 'cap': capacity(n), 'chains': {5: a, 6: b}}


def wrap_fixture(v=0.25):
    """10 rows, cap 32: three voxels on home slot 31 (the chain continues at slots 0 and 1), one on slot 0 and one on slot 1 (pushed
    behind it), each seen twice"""
    n = 10
    a, b, c = chain_keys(n, 31, 3), chain_keys(n, 0, 1), chain_keys(n, 1, 1)
    order = a + b + c
    return case([_rows(order + order[::-1], v)], v, exact=True), {'n': n, 'cap': capacity(n), 'chains': {31: a, 0: b, 1: c}}


def f32_division_fixture():
    """v = 0.1: x = float32(k / 10) whose float32 quotient by float32(0.1) lands in another voxel than the float64 quotient by 0.1,
    each between a row half a voxel below and one half a voxel above (so the wrong voxel changes which rows merge)"""
    rows = []
    for k in range(1, 400):
        x = np.float32(k / 10.0)
        t64 = np.floor(np.float64(x) / 0.1)
        t32 = np.floor(np.float64(x / np.float32(0.1)))
        r = np.float64(x) / 0.1
        if t64 != t32 and abs(r - np.rint(r)) > 1e-8:
            for xx in (np.float32((t64 + 0.5) * 0.1), x, np.float32((t64 + 1.5) * 0.1), np.float32((t64 - 0.5) * 0.1)):
                rows.append((xx, 0.05, 0.05, 0.5))
        if len(rows) >= 12:
            break
    assert len(rows) >= 4
    return case([np.array(rows, np.float32)], 0.1)


def faces_fixture():
    """identity, v = 0.25: every operation exact.  Coordinates on voxel faces, +-0, the last representable index and the first
    unrepresentable one on either side, NaN and inf in z"""
    v, top = 0.25, float(LIM) * 0.25
    xs = [-0.5, -0.0, 0.0, 0.25, 0.5, 0.75, -0.25, -0.75, -1.0, 0.125, -0.125, 0.375, -0.375,
          top - 0.25, top - 0.125, top, top + 0.25, -(top - 0.25), -top, -top - 0.25, -top + 0.125]
    rows = [(x, 0.0, 0.0, 0.5) for x in xs] + [(0.0, x, -0.0, 0.5) for x in xs] + [(-0.0, 0.0, x, 0.5) for x in xs]
    rows += [(1.0, 1.0, np.nan, 0.5), (1.0, 1.0, np.nan, 0.5), (1.0, 1.0, np.inf, 0.5), (1.0, 1.0, -np.inf, 0.5),
             (1.0, 1.0, np.inf, 0.5), (1.0, 1.0, 1.0, 0.5), (1.125, 1.125, 1.125, 0.5), (top, top, top, 0.5), (top, top, top, 0.5)]
    rows = rows + rows[::-1]                                # every row a second time: only the unrepresentable ones stay twice
    return case([np.array(rows, np.float32)], v, exact=True)


def random_cloud(n, seed, cols=4, half=(2.0, 2.0, 0.5)):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, cols), np.float32)
    p[:, :3] = rng.uniform(-1, 1, (n, 3)) * np.array(half)
    if cols == 4:
        p[:, 3] = 0.5
    return p


def rigid(i):
    a = 0.02 * i
    M = np.eye(4)
    M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    M[:3, 3] = (0.31 * i, -0.07 * i, 0.013 * i)
    return M


def sweep_set(lengths, seed, cols=4, half=(2.0, 2.0, 0.5)):
    """sweeps that re-observe one scene: sweep k holds points of the common box, moved into its own frame by inv(M_k)"""
    sweeps, Ms = [], []
    for k, n in enumerate(lengths):
        p = random_cloud(n, seed + k, cols, half)
        if k:
            M = rigid(k)
            Ms.append(M)
            R, t = M[:3, :3], M[:3, 3]
            p[:, :3] = ((p[:, :3].astype(np.float64) - t) @ R).astype(np.float32)    # R^T (x - t), row-wise
        sweeps.append(p)
    return sweeps, Ms


def distinct_voxels_fixture(n=4000, distinct=3000, seed=11, v=0.25):
    """`distinct` voxels drawn without repetition, the remaining rows repeat earlier ones: n = 4000 rows live in a table of 8192"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(64 ** 3, distinct, replace=False)
    t = np.stack([cells % 64, (cells // 64) % 64, cells // 4096], axis=1) - 32
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
    rng.shuffle(pick)
    return case([_rows(t[pick].tolist(), v)], v, exact=True)


def cases():
    """name -> case: everything tests/test_voxel_host.py examines and tests/test_gpu_voxel.py runs"""
    v = 0.25
    out = {}
    out['n1'] = case([_rows([(3, -2, 1)], v)], v, exact=True)
    out['two_in_one'] = case([np.array([(0.3, 0.3, 0.3, 0.5), (0.26, 0.49, 0.37, 0.5)], np.float32)], v)
    out['131_in_one'] = case([random_cloud(131, 1, half=(0.1, 0.1, 0.1)) + np.float32(0.125)], v)
    # rows 0..254 in voxels of their own, row 255 (the last of block 0) opens a voxel that rows 256..299 fall into
    t = [(j, 0, 0) for j in range(255)] + [(-7, 3, 2)] * 45
    out['first_is_last_of_block'] = case([_rows(t, v)], v, exact=True)
    for n in (255, 256, 257, 511, 513):
        out['n%d' % n] = case([random_cloud(n, n)], 0.2)
        out['n%d/stride3' % n] = case([random_cloud(n, n, cols=3)], 0.2)
    out['faces'] = faces_fixture()
    out['collisions'] = collision_fixture()[0]
    out['wrap'] = wrap_fixture()[0]
    out['f32_division'] = f32_division_fixture()
    out['distinct3000'] = distinct_voxels_fixture()
    own = random_cloud(300, 21)
    out['k3_identical'] = case([own, own, own], 0.2, [np.eye(4), np.eye(4)])
    sw, Ms = sweep_set([60] * 21, 40)
    out['k21'] = case(sw, 0.2, Ms)
    sw, Ms = sweep_set([257, 0, 63, 64, 65, 1, 700], 60)
    out['lengths'] = case(sw, 0.2, Ms)
    out['lengths/stride3'] = case([s[:, :3] for s in sw], 0.2, Ms)
    out['lengths/rellis'] = case(sw, 0.2, Ms, flip_xy=True, radius=1.7)
    sw, Ms = sweep_set([300, 200, 0, 260], 80, cols=3, half=(4.0, 4.0, 0.5))
    out['ego_radius_voxel'] = case(sw, 0.2, Ms, ego_box=(0.8, 2.7), radius=3.1)
    sw, Ms = sweep_set([640, 320, 333], 90)
    out['lidar_line'] = case(sw, 0.2, Ms, lidar_line=16, radius=1.9)
    out['own_order'] = case(sw, 0.2, Ms, own_order=np.random.default_rng(5).permutation(640), radius=1.9)
    return out
