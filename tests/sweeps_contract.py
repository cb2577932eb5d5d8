"""The multi-sweep chain of the reference's loaders, restated in float64 numpy with an error bound per output element.

What is restated (every step elementwise, no BLAS, so that this file fixes ONE evaluation):
  ego box        nusc_loader.py:88-93     per sweep, on the raw float32 point, strict on both sides; numpy compares a float32
                                          array with a Python float in float32
  transform      kitti_odom_loader.py:184-186, rellis3d_loader.py:239-241, nusc_utils.py:65-69 (transform_pc_np)
                                          q = M_k . (p, 1) in float64; the own sweep is not transformed
  concatenate    kitti_odom_loader.py:221-223 (own, previous, next), nusc_loader.py:137-144 (own, next, previous): float64
  RELLIS flip    rellis3d_loader.py:310-316     x, y negated (exact)
  line reduction loader_utils.py:165-177        rows i*line_num + j, j in [int(-line_num/2), int(line_num/2)), python indexing
  radius filter  loader_utils.py:182-187        -r <= x < r and -r <= y < r, stable
  sub-sample     loader_utils.py:189-196        the given index list, or zero padding up to num_points
  mis-calibration loader_utils.py:198-200       rand_init_l @ (q, 1) in float64

The bound.  numpy's (4x4)@(4xN) goes through BLAS, which fixes neither the order in which the four terms of an element are
summed nor whether a product is fused into the sum.  Whatever the order, each term passes through at most four roundings
(its product, three additions), so one evaluation is within 4u . sum|terms| of the exact value, u = 2^-53 (the second-order
part of gamma_4 = 4u/(1-4u) is below 1e-31 relative and ignored); two evaluations - the reference's and any other - are
within GAMMA . sum|terms| of each other, GAMMA = 8u.  For the second stage the first stage's bound b1 propagates through
|rand_init_l| and the stage's own terms add theirs:
    b1[r]  = GAMMA . (|M_r0 x| + |M_r1 y| + |M_r2 z| + |M_r3|)          (0 for the own sweep: nothing is computed)
    b2[r]  = sum_c |T_rc| . b1[c]  +  GAMMA . (|T_r0 qx| + |T_r1 qy| + |T_r2 qz| + |T_r3|)
No tolerance here is taken from any implementation's output.
"""
import numpy as np

U = 2.0 ** -53
GAMMA = 8.0 * U


def _affine(M, x, y, z):
    """rows 0..2 of M . (x, y, z, 1) summed left to right, and the sum of the absolute terms"""
    val = np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=-1)
    mag = np.stack([np.abs(M[r, 0] * x) + np.abs(M[r, 1] * y) + np.abs(M[r, 2] * z) + np.abs(M[r, 3]) for r in range(3)],
                   axis=-1)
    return val, mag


def positions(sweeps, transforms, own_order=None, ego_box=None):
    """-> q [n_total, 3] float64 of the concatenation (own sweep first, BEFORE the ego box), b1 [n_total, 3], and the bool
    mask of the rows the ego box leaves"""
    qs, bs, ms = [], [], []
    for k, sw in enumerate(sweeps):
        p = np.asarray(sw, np.float32)[:, :3]
        if k == 0 and own_order is not None:
            p = p[np.asarray(own_order)]
        mask = np.ones(p.shape[0], bool)
        if ego_box is not None:
            bx, by = np.float32(ego_box[0]), np.float32(ego_box[1])
            inside = ((p[:, 0] < bx) & (p[:, 0] > -bx)) & ((p[:, 1] < by) & (p[:, 1] > -by))
            mask = ~inside
        x, y, z = (p[:, c].astype(np.float64) for c in range(3))
        if k == 0:
            q, b = np.stack([x, y, z], axis=-1), np.zeros((p.shape[0], 3))
        else:
            with np.errstate(invalid='ignore', over='ignore'):
                q, mag = _affine(np.asarray(transforms[k - 1], np.float64), x, y, z)
            b = GAMMA * mag
        qs.append(q), bs.append(b), ms.append(mask)
    return np.concatenate(qs), np.concatenate(bs), np.concatenate(ms)


def lidar_line_rows(n_points, reduce_to):
    """loader_utils.py:165-177 as a row list (python's negative indices wrapped)"""
    rate = 64 / reduce_to
    line_num = int(n_points / 64)
    rows = []
    for i in range(64):
        if i % rate == 0:
            for j in range(int(-line_num / 2), int(line_num / 2)):
                r = i * line_num + j
                rows.append(r + n_points if r < 0 else r)
    return np.array(rows, np.int64)


def chain(sweeps, transforms, rand_init_l, num_points, own_order=None, ego_box=None, lidar_line=None, radius=50.,
          flip_xy=False, sampled_indices=None):
    """-> dict: keep (rows of the pre-ego concatenation that survive, in order), out64 [3, num_points], bound [3, num_points],
    acc / acc_bound (the accumulated cloud the loader returns: q of the rows the ego box leaves, and its single-stage bound)"""
    q, b1, ego = positions(sweeps, transforms, own_order, ego_box)
    cand = np.nonzero(ego)[0]                                  # the loader's concatenated cloud, as rows of ours
    acc, acc_bound = q[cand], b1[cand]
    if lidar_line is not None:
        cand = cand[lidar_line_rows(cand.size, lidar_line)]
    s = -1.0 if flip_xy else 1.0
    if radius is not None:
        x, y = q[cand, 0] * s, q[cand, 1] * s
        # one sweep alone stays float32 in the loader, and numpy compares it with float32(radius)
        r = float(np.float32(radius)) if len(sweeps) == 1 else float(radius)
        with np.errstate(invalid='ignore'):
            cand = cand[(x >= -r) & (x < r) & (y >= -r) & (y < r)]
    keep = cand
    if num_points < keep.size:
        pick = keep[np.asarray(sampled_indices)]
        assert pick.size == num_points
    else:
        pick = keep
    T = np.asarray(rand_init_l, np.float64)
    x = np.zeros(num_points)
    y, z, bq = np.zeros(num_points), np.zeros(num_points), np.zeros((num_points, 3))
    x[:pick.size], y[:pick.size], z[:pick.size] = q[pick, 0] * s, q[pick, 1] * s, q[pick, 2]
    bq[:pick.size] = b1[pick]
    out, mag = _affine(T, x, y, z)
    bound = np.stack([sum(np.abs(T[r, c]) * bq[:, c] for c in range(3)) for r in range(3)], axis=-1) + GAMMA * mag
    return {'keep': keep.astype(np.int32), 'out64': out.T, 'bound': bound.T, 'acc': acc, 'acc_bound': acc_bound}


def within(got, ref, bound):
    """|got - ref| <= bound elementwise; where ref is not finite, got has to be the same non-finite value"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    with np.errstate(invalid='ignore'):
        ok = np.where(fin, np.abs(got - ref) <= bound, (got == ref) | (np.isnan(got) & np.isnan(ref)))
    return bool(ok.all())


# ---- the recorded cases of tests/golden/sweeps.npz (make_golden_sweeps.py) as arguments of `chain` / SweepSet ------------
def load_cases(golden_dir):
    import os
    G = np.load(os.path.join(str(golden_dir), 'sweeps.npz'))
    cases = {}
    for name in ('odomA', 'odomB', 'odomC', 'rellisA', 'rawA', 'nuscA', 'nuscB'):
        own, num, skip, ll, npts, seed, n_frames = [int(v) for v in G[name + '.meta']]
        nusc = name.startswith('nusc')
        if name == 'rawA':
            sweeps, Ms = [G['rawA.pcd']], []
        else:
            frames = [int(f) for f in G[name + '.frames']]
            sweeps = [G['%s.sweep%d' % ('nusc' if nusc else name, f)] for f in frames]
            Ms = list(G[name + '.M'])
        ri = tuple(float(v) for v in G[name + '.rand_init'])
        cases[name] = {
            'name': name, 'sweeps': sweeps, 'transforms': Ms, 'own': own, 'num': num, 'skip': skip,
            'own_order': G[name + '.order'] if name + '.order' in G.files else None,
            'ego_box': (0.8, 2.7) if nusc else None, 'lidar_line': None if ll < 0 else ll, 'num_points': npts,
            'flip_xy': name.startswith('rellis'), 'rand_init': ri,
            'sampled': G[name + '.sampled'] if name + '.sampled' in G.files else None,
            'keep': G[name + '.keep'], 'out_pc': G[name + '.out.pc'],
            'acc': G[name + '.acc'] if name + '.acc' in G.files else None,
        }
    return G, cases


def chain_of(case, rand_init_l):
    return chain(case['sweeps'], case['transforms'], rand_init_l, case['num_points'], case['own_order'], case['ego_box'],
                 case['lidar_line'], 50., case['flip_xy'], case['sampled'])
