"""On-disk formats the reference's loaders / drivers use, host side only.

* KITTI-style velodyne `.bin`: float32 x 4 per point                (loader_utils.py:59-61)
* KITTI odometry `poses.txt` lines (12 floats) and `calib.txt`        (loader_utils.py:12-52)
* RELLIS `camera_info.txt` (fx fy cx cy) and lidar->camera yaml       (loader_utils.py:206-229)
* random-initialisation CSV  name,roll,pitch,yaw,tx,ty,tz,cam_roll   (rellis3d_loader.py:44-48)
* prediction CSV  fname,<12 floats of sensor2_T_sensor1[:3,:]>,      (test.py:46-53)
* binary PLY point clouds (not in the reference): what common.fuse writes, and only that
"""
import csv
import re

import numpy as np


def read_velodyne_bin(path):
    """-> (N,4) float32 (x,y,z,reflectance)"""
    return np.fromfile(path, dtype=np.float32).reshape((-1, 4))


def write_velodyne_bin(path, pts):
    np.asarray(pts, dtype=np.float32).reshape((-1, 4)).tofile(path)


def parse_pose_line(line):
    """one line of KITTI poses.txt -> 4x4"""
    v = np.array([float(p) for p in line.split()], dtype=float).reshape((3, 4))
    out = np.eye(4)
    out[:3, :] = v
    return out


def read_kitti_calib(path):
    data = {}
    with open(path) as f:
        for line in f:
            if ':' not in line:
                continue
            key, value = line.split(':', 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    P2, Tr = np.eye(4), np.eye(4)
    P2[:3, :] = data['P2'].reshape(3, 4)
    Tr[:3, :] = data['Tr'].reshape(3, 4)
    return {'Tr': Tr, 'Tr_inv': np.linalg.inv(Tr), 'P2': P2, 'P2_inv': np.linalg.inv(P2)}


def read_rellis_camera_info(path):
    d = np.loadtxt(path)
    K = np.zeros((3, 3))
    K[0, 0], K[1, 1], K[2, 2], K[0, 2], K[1, 2] = d[0], d[1], 1, d[2], d[3]
    return K


def quat_xyzw_to_matrix(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def read_rellis_lidar2cam(path):
    import yaml
    with open(path) as f:
        d = yaml.safe_load(f)['os1_cloud_node-pylon_camera_node']
    RT = np.eye(4)
    RT[:3, :3] = quat_xyzw_to_matrix(np.array([d['q']['x'], d['q']['y'], d['q']['z'], d['q']['w']], dtype=float))
    RT[:3, 3] = [d['t']['x'], d['t']['y'], d['t']['z']]
    return np.linalg.inv(RT)


def read_rand_init_csv(path):
    """-> {name: [roll, pitch, yaw, tx, ty, tz, cam_roll]} (radians / metres)"""
    out = {}
    with open(path) as f:
        for line in csv.reader(f):
            if line:
                out[line[0]] = [float(v) for v in line[1:]]
    return out


def append_prediction_csv(path, fname, sensor2_T_sensor1):
    """one row per sample, exactly as test.py:46-53 writes it (trailing comma included)"""
    v = np.asarray(sensor2_T_sensor1, dtype=np.float32)[:3, :].flatten()
    with open(path, 'a') as f:
        f.write(fname + ',' + ''.join(str(x) + ',' for x in v) + '\n')


def read_prediction_csv(path):
    out = {}
    with open(path) as f:
        for line in csv.reader(f):
            if line:
                out[line[0]] = np.array([float(v) for v in line[1:13]], dtype=np.float32).reshape(3, 4)
    return out


_PLY_TYPES = {'float': np.dtype('<f4'), 'uchar': np.dtype('u1')}
_PLY_FIXED = ('x', 'y', 'z', 'red', 'green', 'blue')


def write_ply(path, xyz, rgb=None, **columns):
    """(n,3) points -> `binary_little_endian 1.0` PLY with `float x y z`, `uchar red green blue` when rgb (n,3) is given, and one
    property per named (n,) column: `uchar` for a uint8 array, `float` for anything else.  n may be 0."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape((-1, 3))
    n = xyz.shape[0]
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if rgb is not None:
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.shape != (n, 3):
            raise ValueError('write_ply: rgb must be uint8 (%d, 3), got %s %s' % (n, rgb.dtype, rgb.shape))
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    cols = {}
    for name, col in columns.items():
        col = np.asarray(col)
        if not re.fullmatch(r'[A-Za-z_]\w*', name) or name in _PLY_FIXED:
            raise ValueError('write_ply: %r is not a usable property name' % name)
        if col.shape != (n,):
            raise ValueError('write_ply: column %r has shape %s, expected (%d,)' % (name, col.shape, n))
        cols[name] = col if col.dtype == np.uint8 else col.astype(np.float32)
        fields.append((name, 'u1' if col.dtype == np.uint8 else '<f4'))
    rows = np.empty(n, dtype=np.dtype(fields))
    rows['x'], rows['y'], rows['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        rows['red'], rows['green'], rows['blue'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    for name, col in cols.items():
        rows[name] = col
    kinds = {np.dtype(t): k for k, t in _PLY_TYPES.items()}
    header = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % n]
    header += ['property %s %s' % (kinds[np.dtype(t)], name) for name, t in fields] + ['end_header']
    with open(path, 'wb') as f:
        f.write(('\n'.join(header) + '\n').encode('ascii'))
        f.write(rows.tobytes())


def read_ply(path):
    """what `write_ply` writes -> {'xyz': (n,3) float32, 'rgb': (n,3) uint8 or None, <column name>: (n,) float32 / uint8 ...}"""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError('read_ply: %s is not a PLY file' % path)
    lines = data[:end].decode('ascii').split('\n')
    if lines[1] != 'format binary_little_endian 1.0':
        raise ValueError('read_ply: only binary_little_endian 1.0 is read, got %r' % lines[1])
    n, fields = None, []
    for line in lines[2:]:
        tok = line.split()
        if not tok or tok[0] == 'comment':
            continue
        if tok[0] == 'element' and len(tok) == 3 and tok[1] == 'vertex' and n is None:
            n = int(tok[2])
        elif tok[0] == 'property' and len(tok) == 3 and tok[1] in _PLY_TYPES and n is not None:
            fields.append((tok[2], _PLY_TYPES[tok[1]]))
        else:
            raise ValueError('read_ply: cannot read the header line %r (only vertex elements with float / uchar properties)' % line)
    names = [k for k, _ in fields]
    if n is None or names[:3] != ['x', 'y', 'z']:
        raise ValueError('read_ply: no vertex element that starts with x y z')
    dt = np.dtype(fields)
    body = data[end + len(b'end_header\n'):]
    if len(body) != n * dt.itemsize:
        raise ValueError('read_ply: %d bytes of vertex data, the header announces %d' % (len(body), n * dt.itemsize))
    rows = np.frombuffer(body, dtype=dt, count=n)
    out = {'xyz': np.stack([rows['x'], rows['y'], rows['z']], 1).astype(np.float32).reshape((n, 3)), 'rgb': None}
    if all(c in names for c in ('red', 'green', 'blue')):
        out['rgb'] = np.stack([rows['red'], rows['green'], rows['blue']], 1).reshape((n, 3))
    for name in names:
        if name not in _PLY_FIXED:
            out[name] = rows[name].copy()
    return out
