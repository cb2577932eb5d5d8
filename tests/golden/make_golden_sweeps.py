"""Generate tests/golden/sweeps.npz from the UNMODIFIED reference loaders (run in the build container only):
multi-sweep accumulation (`KITTI_ODOM.get_accumulated_pc`, kitti_odom_loader.py:160-225; `RELLIS_3D.get_accumulated_pc`,
rellis3d_loader.py:218-280; `NUSC.accumulate_lidar_points`, nusc_loader.py:83-146) and the four Process callables on top
of it, over tiny directory trees (`poses`, `.bin` sweeps) written into a temporary directory.

Fixtures are data only: the sweeps, poses and calibrations that went in, and what the reference returned.  On top of
ref_harness.py this installs three stand-ins for third-party pieces the build container lacks: a `nusc.get` over dicts,
`LidarPointCloud.from_file` over `.bin` files and `Quaternion.rotation_matrix`; and it wraps the readers (`pcd_read`,
`from_file`) to log which files a walk touched, which is how the index and token lists are recorded.

How the reference's KEPT INDICES are recorded although it returns no indices: its own `preproc_pcd` is run a second time on
the cloud with z replaced by (row + 1) and `rand_init_l` = I, so row 2 of what it returns is the list of surviving rows, in
order, after its lidar-line reduction and radius filter.  The ego box of nuScenes is recorded the same way, through
`get_lidar_pc_intensity_by_token` on a copy of each sweep with z = row + 1.

Conditions this generator asserts (tests/test_sweeps_host.py re-checks them): no point of a TRANSFORMED sweep lies within
1e-6 of +-radius in x or y, so that no rounding of the float64 transform can decide the radius filter; the boundary
behaviour is pinned by directed points in the OWN sweep, whose positions are exact.

    python tests/golden/make_golden_sweeps.py
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402
from make_golden_prep import synth_image  # noqa: E402

RADIUS = 50.0
F32 = np.float32


def quant(a):
    """coordinates on a 1/256 grid: exact in float32, and the fixture compresses"""
    return (np.round(np.asarray(a, np.float64) * 256.0) / 256.0).astype(F32)


def synth_sweep(n, seed, spread=58.0, centre=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    p = np.empty((n, 4), F32)
    p[:, 0] = quant(rng.uniform(-spread, spread, n) + centre[0])
    p[:, 1] = quant(rng.uniform(-spread, spread, n) + centre[1])
    p[:, 2] = quant(rng.uniform(-3, 5, n))
    p[:, 3] = 0.5                                  # the intensity column is never read
    return p


def nb(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


def radius_directed():
    """the half-open radius test at its boundary, in x and in y, plus a NaN and a -0.0 row"""
    r = F32(RADIUS)
    xs = [r, -r, nb(r, False), nb(r, True), nb(-r, False), nb(-r, True)]
    rows = [(x, 1.0, 0.5, 0.0) for x in xs] + [(2.0, x, 0.25, 0.0) for x in xs]
    rows += [(np.nan, 3.0, 1.0, 0.0), (-0.0, -0.0, -0.0, 0.0)]
    return np.array(rows, F32)


def ego_directed():
    """the strict ego box (0.8, 2.7) at its boundary: float32(0.8), float32(2.7), their neighbours and negatives"""
    bx, by = F32(0.8), F32(2.7)
    rows = []
    for s in (1, -1):
        for x in (bx, nb(bx, False), nb(bx, True)):
            rows.append((s * x, 0.5, 0.0, 0.0))          # |y| inside: x decides
        for y in (by, nb(by, False), nb(by, True)):
            rows.append((0.25, s * y, 0.0, 0.0))         # |x| inside: y decides
    rows += [(0.0, 0.0, 1.0, 0.0), (0.79, 2.69, 1.0, 0.0), (-0.79, -2.69, 1.0, 0.0), (0.5, 3.0, 1.0, 0.0), (1.0, 0.5, 1.0, 0.0)]
    return np.array(rows, F32)


def pose_of(i, step=(0.9, 0.07, 0.01), yaw=0.012):
    c, s = np.cos(yaw * i), np.sin(yaw * i)
    P = np.eye(4)
    P[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    P[:3, 3] = [step[0] * i, step[1] * i * i * 0.1, step[2] * i]
    return P


def write_poses(path, n):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        for i in range(n):
            f.write(' '.join(repr(float(v)) for v in pose_of(i)[:3].reshape(-1)) + '\n')


def draw(seed, n_keep, num_points):
    """the index list `np.random.choice` of the reference's preproc_pcd draws after np.random.seed(seed)"""
    np.random.seed(seed)
    return np.random.choice(range(n_keep), size=num_points, replace=False, p=None).astype(np.int32)


class Log(object):
    def __init__(self, fn):
        self.fn, self.seen = fn, []

    def __call__(self, path, *a, **k):
        self.seen.append(os.path.basename(path))
        return self.fn(path, *a, **k)


def main():
    ref_harness._install_stubs()
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    kitti = importlib.import_module('data_loader.kitti_odom_loader')
    rellis = importlib.import_module('data_loader.rellis3d_loader')
    raw = importlib.import_module('data_loader.kitti_raw_loader')
    nusc = importlib.import_module('data_loader.nusc_loader')
    nusc_utils = importlib.import_module('data_loader.nusc_utils')
    lu = importlib.import_module('data_loader.loader_utils')
    for m in (kitti, rellis, raw, nusc, lu):
        assert m.__file__.startswith(ref_harness.REF_ROOT), m.__file__

    out = {}
    P2 = np.array([[700., 0, 80, 40], [0, 700, 24, 2], [0, 0, 1, 0.003], [0, 0, 0, 1]])
    Tr = np.array([[0.01, -0.999, -0.02, 0.05], [0.02, 0.02, -0.999, -0.07], [0.999, 0.01, 0.02, -0.3], [0, 0, 0, 1.]])
    calibs = {'P2': P2, 'Tr': Tr, 'Tr_inv': np.linalg.inv(Tr)}
    pose_ji = np.eye(4)
    pose_ji[:3, 3] = (0.4, -0.1, 0.02)
    out['P2'], out['Tr'], out['pose_ji'] = P2, Tr, pose_ji
    identity_gts = {'rand_init_l': np.eye(4)}

    def kept_rows(cloud, lidar_line, flip=False):
        """rows of `cloud` the reference's preproc_pcd keeps, in its order (see the module docstring)"""
        c = np.array(cloud, np.float64)
        if flip:
            c[:, :2] = -c[:, :2]
        c[:, 2] = np.arange(1, c.shape[0] + 1)
        pc = lu.preproc_pcd(c, identity_gts, c.shape[0] + 1, lidar_line)
        z = pc[2]
        return (z[z > 0] - 1).astype(np.int32)

    def check_margin(name, cloud, n_own):
        far = np.abs(np.abs(cloud[n_own:, :2]) - RADIUS)
        assert far.size == 0 or far.min() > 1e-6, (name, far.min())

    def record_process(name, proc, call, acc, lidar_line, num_points, seed, flip=False, full=True):
        """run the reference's Process callable on its own accumulated cloud; record outputs, kept rows and the draw"""
        keep = kept_rows(acc, lidar_line, flip)
        np.random.seed(seed)
        pc, im, calib, A, gts, tag = call(proc)
        out[name + '.keep'] = keep
        if num_points < keep.size:
            out[name + '.sampled'] = draw(seed, keep.size, num_points)
        out[name + '.out.pc'] = np.asarray(pc)
        if not full:                                                   # the point side only (odomB, odomC)
            return keep
        out[name + '.out.img'] = np.asarray(im)
        out[name + '.out.calib'] = np.asarray(calib)
        out[name + '.out.A'] = np.asarray(A)
        for k, v in gts.items():
            out[name + '.gt.' + k] = np.asarray(v)
        return keep

    with tempfile.TemporaryDirectory() as tmp:
        # ---------------------------------------------------------------- KITTI odometry ----------------------
        # name, lengths per frame, own frame, num, skip, lidar_line, num_points, rand_init, seed
        odom_cases = [
            ('odomA', [64, 63, 0, 257, 65, 1, 700], 3, 3, 1, None, 1280, (0.05, -0.03, 0.2, 0.3, -0.2, 0.1, 0.07), 11),
            ('odomB', [20 + (i * 7) % 9 for i in range(21)], 10, 10, 1, None, 256, (-0.1, 0.02, -0.4, 0.0, 0.5, -0.3, -0.31), 12),
            ('odomC', [128, 128, 128], 1, 1, 1, 32, 96, (0.02, 0.01, -0.05, 0.1, 0.0, -0.1, 0.0), 13),
        ]
        for ci, (name, lengths, own, num, skip, ll, npts, ri, seed) in enumerate(odom_cases):
            seq = '%02d' % ci
            root = os.path.join(tmp, name)
            vdir = os.path.join(root, 'dataset', 'sequences', seq, 'velodyne')
            os.makedirs(vdir)
            write_poses(os.path.join(root, 'dataset', 'poses', seq + '.txt'), len(lengths))
            sweeps = []
            for f, n in enumerate(lengths):
                p = synth_sweep(n, 100 * ci + f)
                if name == 'odomA' and f == 1:
                    p = synth_sweep(n, 100 * ci + f, spread=8.0, centre=(75.0, -70.0))      # the radius removes this sweep entirely
                if name == 'odomA' and f == own:
                    d = radius_directed()
                    p[:d.shape[0]] = d
                p.tofile(os.path.join(vdir, '%06d.bin' % f))
                sweeps.append(p)
            ds = object.__new__(kitti.KITTI_ODOM)
            ds.data_path = os.path.join(root, 'dataset')
            ds.accumulation_frame_num, ds.accumulation_frame_skip = num, skip
            np.random.seed(seed)
            order = np.random.permutation(lengths[own])
            np.random.seed(seed)
            acc = ds.get_accumulated_pc(os.path.join(vdir, '%06d.bin' % own), seq, own, calibs)
            assert acc.dtype == np.float64 and np.array_equal(acc[:lengths[own]], sweeps[own][order, :3], equal_nan=True)
            # the frames the walk touched, and the transforms as the loader evaluates them (kitti_odom_loader.py:165,182,185):
            # checked to reproduce the loader's own cloud bit for bit before they are recorded
            logged = Log(kitti.pcd_read)
            kitti.pcd_read = logged
            np.random.seed(seed)
            ds.get_accumulated_pc(os.path.join(vdir, '%06d.bin' % own), seq, own, calibs)
            kitti.pcd_read = logged.fn
            frames = [int(b[:6]) for b in logged.seen]
            assert frames[0] == own
            poses = [lu.pose_read(line) for line in open(os.path.join(root, 'dataset', 'poses', seq + '.txt'))]
            P_io = np.linalg.inv(poses[own])
            Ms, at = [], lengths[own]
            for f in frames[1:]:
                M = calibs['Tr_inv'] @ (P_io @ poses[f]) @ calibs['Tr']
                pj = sweeps[f].T
                pj = np.concatenate((pj[:3, :], np.ones((1, pj.shape[1]), dtype=pj.dtype)), axis=0)
                assert np.array_equal((M @ pj)[:3].T, acc[at:at + lengths[f]]), (name, f)
                at += lengths[f]
                Ms.append(M)
            assert at == acc.shape[0]
            check_margin(name, acc, lengths[own])
            out[name + '.frames'] = np.array(frames, np.int32)
            out[name + '.poses'] = np.array(poses)
            out[name + '.M'] = np.array(Ms).reshape(-1, 4, 4)
            out[name + '.order'] = order.astype(np.int32)
            for f in sorted(set(frames)):
                out['%s.sweep%d' % (name, f)] = sweeps[f]
            out[name + '.meta'] = np.array([own, num, skip, -1 if ll is None else ll, npts, seed, len(lengths)], np.int64)
            out[name + '.rand_init'] = np.array(ri, np.float64)
            if name == 'odomA':
                out[name + '.acc'] = acc
            img = synth_image(16, 28, 40 + ci)
            if name == 'odomA':
                out[name + '.img'] = img
            args = {'raw_cam_img_size': [12, 24], 'lidar_line': ll, 'num_points': npts, 'test': True}
            record_process(name, kitti.ProcessKITTIODOM(args),
                           lambda proc: proc(acc, img, calibs, pose_ji, name, rand_init=ri), acc, ll, npts, seed,
                           full=name == 'odomA')

        # walks at both ends of a sequence, with a skip, and with num = 0 (the odomB tree: 21 frames)
        root = os.path.join(tmp, 'odomB')
        ds = object.__new__(kitti.KITTI_ODOM)
        ds.data_path = os.path.join(root, 'dataset')
        walks = []
        for own, num, skip in ((0, 2, 1), (20, 2, 1), (1, 3, 2), (19, 2, 2), (10, 0, 1), (10, 12, 1), (3, 2, 3)):
            ds.accumulation_frame_num, ds.accumulation_frame_skip = num, skip
            logged = Log(kitti.pcd_read)
            kitti.pcd_read = logged
            ds.get_accumulated_pc(os.path.join(root, 'dataset', 'sequences', '01', 'velodyne', '%06d.bin' % own), '01', own, calibs)
            kitti.pcd_read = logged.fn
            frames = [int(b[:6]) for b in logged.seen][1:]
            prev = [f for f in frames if f < own]
            walks.append([own, 21, num, skip, len(prev), len(frames) - len(prev)] + frames + [-1] * (24 - len(frames)))
        out['odom.walks'] = np.array(walks, np.int32)      # own, n_frames, num, skip, n_prev, n_next, prev..., next..., -1 pad

        # ---------------------------------------------------------------- RELLIS ------------------------------
        name, lengths, own, num, skip, npts, ri, seed = 'rellisA', [90, 100, 110], 1, 1, 1, 384, (0.3, 0.1, -0.25, -0.4, 0.2, 0.0, -0.2), 21
        root = os.path.join(tmp, name)
        vdir = os.path.join(root, 'Rellis-3D', '00004', 'os1_cloud_node_kitti_bin')
        os.makedirs(vdir)
        write_poses(os.path.join(root, 'Rellis-3D', '00004', 'poses.txt'), len(lengths))
        sweeps = [synth_sweep(n, 300 + f) for f, n in enumerate(lengths)]
        for f, p in enumerate(sweeps):
            p.tofile(os.path.join(vdir, '%06d.bin' % f))
        ds = object.__new__(rellis.RELLIS_3D)
        ds.data_path = root
        ds.accumulation_frame_num, ds.accumulation_frame_skip = num, skip
        np.random.seed(seed)
        order = np.random.permutation(lengths[own])
        np.random.seed(seed)
        acc = ds.get_accumulated_pc(os.path.join(vdir, '%06d.bin' % own), 4, own)
        poses = [lu.pose_read(line) for line in open(os.path.join(root, 'Rellis-3D', '00004', 'poses.txt'))]
        P_io = np.linalg.inv(poses[own])
        Ms, at, frames = [], lengths[own], [own, 0, 2]
        assert np.array_equal(acc[:at], sweeps[own][order, :3])
        for f in frames[1:]:
            M = P_io @ poses[f]
            pj = sweeps[f].T
            pj = np.concatenate((pj[:3, :], np.ones((1, pj.shape[1]), dtype=pj.dtype)), axis=0)
            assert np.array_equal((M @ pj)[:3].T, acc[at:at + lengths[f]]), (name, f)
            at += lengths[f]
            Ms.append(M)
        check_margin(name, acc, lengths[own])
        out[name + '.frames'] = np.array(frames, np.int32)
        out[name + '.poses'] = np.array(poses)
        out[name + '.M'] = np.array(Ms)
        out[name + '.order'] = order.astype(np.int32)
        for f in frames:
            out['%s.sweep%d' % (name, f)] = sweeps[f]
        out[name + '.meta'] = np.array([own, num, skip, -1, npts, seed, len(lengths)], np.int64)
        out[name + '.rand_init'] = np.array(ri, np.float64)
        out[name + '.acc'] = acc
        img = synth_image(18, 30, 50)
        out[name + '.img'] = img
        args = {'raw_cam_img_size': [14, 26], 'lidar_line': None, 'num_points': npts, 'test': True}
        record_process(name, rellis.ProcessRELLIS(args),
                       lambda proc: proc(acc, img, {'P': P2, 'Tr': Tr}, pose_ji, name, rand_init=ri), acc, None, npts, seed, flip=True)

        # ---------------------------------------------------------------- KITTI raw ---------------------------
        name, npts, ri, seed = 'rawA', 192, (0.04, 0.02, -0.1, 0.2, -0.1, 0.05, -0.05), 31
        pcd = synth_sweep(300, 400)
        pcd[:14] = radius_directed()
        pts3 = np.ascontiguousarray(pcd[:, :3])                       # what file_reader hands over (kitti_raw_loader.py:225)
        T2 = (P2 @ Tr)[:3]
        T3 = T2 + np.array([[0, 0, 0, -37.5], [0, 0, 0, 0.1], [0, 0, 0, 0.002]])
        cal = types.SimpleNamespace(T_cam2_velo=T2, T_cam3_velo=T3)
        out[name + '.pcd'], out[name + '.T_cam2_velo'], out[name + '.T_cam3_velo'] = pts3, T2, T3
        out[name + '.meta'] = np.array([0, 0, 1, -1, npts, seed, 1], np.int64)
        out[name + '.rand_init'] = np.array(ri, np.float64)
        img = synth_image(16, 28, 60)
        out[name + '.img'] = img
        args = {'raw_cam_img_size': [12, 24], 'lidar_line': None, 'num_points': npts, 'test': True}
        record_process(name, raw.ProcessKITTIRAW(args),
                       lambda proc: proc(pts3, img, cal, 'image_03', name, rand_init=ri), pts3, None, npts, seed)

        # ---------------------------------------------------------------- nuScenes ----------------------------
        class Quaternion(object):                                      # pyquaternion's (w, x, y, z) -> rotation matrix
            def __init__(self, q):
                self.q = np.asarray(q, np.float64) / np.linalg.norm(q)

            @property
            def rotation_matrix(self):
                w, x, y, z = self.q
                return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

        class LidarPointCloud(object):
            def __init__(self, points):
                self.points = points

            @classmethod
            def from_file(cls, path):
                return cls(np.ascontiguousarray(np.fromfile(path, dtype=F32).reshape(-1, 4).T))

        class Nusc(object):
            def __init__(self, dataroot, tables):
                self.dataroot, self.tables = dataroot, tables

            def get(self, table, token):
                return self.tables[table][token]

        nusc_utils.Quaternion = Quaternion
        nroot = os.path.join(tmp, 'nusc')
        os.makedirs(os.path.join(nroot, 'sweeps'))
        n_rec = 9
        nlen = [60, 55, 70, 48, 40, 66, 52, 58, 45]
        tables = {'sample_data': {}, 'ego_pose': {}, 'calibrated_sensor': {}}
        tables['calibrated_sensor']['cs'] = {'rotation': [0.7071, -0.005, 0.012, -0.7070], 'translation': [0.94, 0.0, 1.84]}
        nsweeps = []
        for i in range(n_rec):
            p = synth_sweep(nlen[i], 500 + i, spread=40.0)
            if i == 4:
                d = ego_directed()
                p[:d.shape[0]] = d
            if i == 6:
                p = synth_sweep(nlen[i], 500 + i, spread=0.7)          # the ego box removes this sweep entirely
            p.tofile(os.path.join(nroot, 'sweeps', 't%d.bin' % i))
            q = p.copy()
            q[:, 2] = np.arange(1, nlen[i] + 1)
            q.tofile(os.path.join(nroot, 'sweeps', 'i%d.bin' % i))    # z = row + 1: records what the ego box keeps
            nsweeps.append(p)
            yaw = 0.4 + 0.01 * i
            for pre in 't', 'i':
                tables['sample_data'][pre + str(i)] = {
                    'token': pre + str(i), 'filename': 'sweeps/%s%d.bin' % (pre, i), 'ego_pose_token': 'e%d' % i,
                    'calibrated_sensor_token': 'cs', 'next': pre + str(i + 1) if i + 1 < n_rec else '',
                    'prev': pre + str(i - 1) if i > 0 else ''}
            tables['ego_pose']['e%d' % i] = {'rotation': [np.cos(yaw / 2), 0.002, -0.001, np.sin(yaw / 2)],
                                              'translation': [600.0 + 0.5 * i, 1500.0 + 0.21 * i, 0.0]}
        nusc.LidarPointCloud = LidarPointCloud
        ds = object.__new__(nusc.NUSC)
        ds.nusc = Nusc(nroot, tables)
        ego_keep = []
        for i in range(n_rec):
            pc_i, _ = ds.get_lidar_pc_intensity_by_token('i%d' % i)
            ego_keep.append(pc_i[2].astype(np.int32) - 1)

        def nusc_case(name, own, num, skip, npts, ri, seed):
            ds.accumulation_frame_num, ds.accumulation_frame_skip = num, skip
            logged = Log(LidarPointCloud.from_file)
            nusc.LidarPointCloud = types.SimpleNamespace(from_file=logged)
            rec = tables['sample_data']['t%d' % own]
            acc = ds.accumulate_lidar_points(rec)
            nusc.LidarPointCloud = LidarPointCloud
            frames = [int(b[1:-4]) for b in logged.seen]
            assert frames[0] == own and acc.shape[0] == 3
            # the matrices as nusc_loader.py:95,113-114,131-134 evaluates them, checked against the loader's own cloud bit for bit
            P_o = [nusc_utils.get_sample_data_ego_pose_P(ds.nusc, tables['sample_data']['t%d' % f]) for f in range(n_rec)]
            P_io = np.linalg.inv(P_o[own])
            P_vl = nusc_utils.get_calibration_P(ds.nusc, rec)
            P_lv = np.linalg.inv(P_vl)
            Ms, at = [], ego_keep[own].size
            assert np.array_equal(acc[:, :at].T, nsweeps[own][ego_keep[own], :3])
            acc_dtype = acc.dtype
            for f in frames[1:]:
                M = np.dot(np.dot(P_lv, np.dot(P_io, P_o[f])), P_vl)
                kept = nsweeps[f][ego_keep[f], :3].T
                assert np.array_equal(nusc_utils.transform_pc_np(M, kept), acc[:, at:at + kept.shape[1]]), (name, f)
                at += kept.shape[1]
                Ms.append(M)
            assert at == acc.shape[1]
            pcd = acc[:3, :].T                                         # file_reader, nusc_loader.py:156
            if len(frames) > 1:
                assert acc_dtype == np.float64
                check_margin(name, pcd, ego_keep[own].size)
            concat_of = np.concatenate([ego_keep[f] + sum(nlen[g] for g in frames[:j]) for j, f in enumerate(frames)])
            out[name + '.frames'] = np.array(frames, np.int32)
            out[name + '.P_o'] = np.array(P_o)
            out[name + '.P_vehicle_lidar'] = P_vl
            out[name + '.M'] = np.array(Ms).reshape(-1, 4, 4)
            out[name + '.ego_keep'] = concat_of.astype(np.int32)      # rows of the concatenation that survive the ego box
            for f in sorted(set(frames)):
                out['nusc.sweep%d' % f] = np.ascontiguousarray(nsweeps[f][:, :3])
            out[name + '.meta'] = np.array([own, num, skip, -1, npts, seed, n_rec], np.int64)
            out[name + '.rand_init'] = np.array(ri, np.float64)
            out[name + '.acc'] = pcd
            img = synth_image(16, 28, 70 + own)
            out[name + '.img'] = img
            K = np.array([[630., 0, 24], [0, 630, 12], [0, 0, 1]])
            cal = {'T_cam_velo': K @ np.linalg.inv(Tr)[:3, :], 'posej_T_posei': pose_ji}
            out[name + '.T_cam_velo'] = cal['T_cam_velo']
            args = {'raw_cam_img_size': [12, 24], 'num_points': npts, 'test': True}
            keep = record_process(name, nusc.ProcessNUSC(args),
                                  lambda proc: proc(pcd, img, cal, name, rand_init=ri), pcd, None, npts, seed)
            out[name + '.keep'] = concat_of[keep].astype(np.int32)    # as rows of the concatenation BEFORE the ego box

        nusc_case('nuscA', 4, 3, 1, 512, (0.05, 0.02, 0.1, -0.2, 0.1, 0.05, 0.04), 41)        # K = 7, zero-pad tail
        nusc_case('nuscB', 4, 0, 1, 32, (-0.03, 0.05, -0.2, 0.1, 0.2, -0.1, -0.06), 42)       # own sweep only, sampled
        nwalks = []
        for own, num, skip in ((3, 2, 2), (6, 3, 1), (1, 2, 1), (0, 2, 3), (8, 1, 1), (4, 0, 1)):
            ds.accumulation_frame_num, ds.accumulation_frame_skip = num, skip
            logged = Log(LidarPointCloud.from_file)
            nusc.LidarPointCloud = types.SimpleNamespace(from_file=logged)
            ds.accumulate_lidar_points(tables['sample_data']['t%d' % own])
            nusc.LidarPointCloud = LidarPointCloud
            frames = [int(b[1:-4]) for b in logged.seen][1:]
            nxt = [f for f in frames if f > own]
            nwalks.append([own, n_rec, num, skip, len(nxt), len(frames) - len(nxt)] + frames + [-1] * (8 - len(frames)))
        out['nusc.walks'] = np.array(nwalks, np.int32)     # own, n_records, num, skip, n_next, n_prev, next..., prev..., -1 pad

    path = os.path.join(HERE, 'sweeps.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
