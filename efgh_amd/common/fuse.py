"""Fusing a registered LiDAR / camera pair on the device: which image pixel every point falls on, what colour it has there, and
whether the camera sees it or a nearer surface hides it (csrc/fuse.hip).  Not in the reference, whose
test.py stops at the twelve numbers of the pose; off unless called.

    fused = fuse(pcd, image, pred)                     # pred['cam_T_velo'], or any (B,3,4) matrix to pixel coordinates
    fused.state                                        # uint8 (B,N): 0 not in front, 1 out of frame, 2 occluded, 3 visible
    fused.rgb[fused.visible]                           # colours of the points the camera sees
    fused.save_ply('frame.ply', pcd)

Pixel convention: u = x / w, v = y / w in float64, the point is on pixel (row (int)v, column (int)u) and pixel centres sit at +0.5.
The image must be the one the matrix projects into: `pred['cam_T_velo']` (and `calib`, the initial pose) map to the camera image at
`raw_cam_img_size`, as the depth overlays of `summary.image_draw` use them.

The defaults are the exact z-buffer: a point is visible iff no point with a smaller float32 depth shares its pixel.  `radius` > 0
lets every point cover its (2 radius + 1)^2 window, which closes the gaps between the returns of a foreground surface - and makes
an oblique plane hide itself, because a neighbour's window reaches over pixels whose own point is a little farther away.  A radius
therefore needs a tolerance (`rel_tol`, `abs_tol`: visible iff d <= zmin (1 + rel_tol) + abs_tol); which one suits a sensor and a
scene is the caller's choice, none is built in."""
import numpy as np
import torch

from .. import _C

WANT = ('rgb', 'state', 'uv', 'depth', 'index')
MAX_RADIUS = 8
BEHIND, OUT_OF_FRAME, OCCLUDED, VISIBLE = 0, 1, 2, 3


class Fused:
    """device tensors of one `fuse` call; what was not in `want` is None.
    state uint8 (B,N) | rgb uint8 (B,N,3) | uv float32 (B,N,2), NaN for state 0 | depth float32 (B,H,W), 0 where no point fell |
    index int32 (B,H,W): the winning point of a pixel, -1 where none.  `index` is the way to carry a per-point quantity into the
    image: `torch.where(index >= 0, intensity[b][index.clamp(min=0)], fill)`."""
    __slots__ = WANT

    def __init__(self, **kw):
        for k in WANT:
            setattr(self, k, kw.get(k))

    @property
    def visible(self):
        if self.state is None:
            raise _C.EfghError("Fused.visible needs 'state' among `want`")
        return self.state == VISIBLE

    def save_ply(self, path, pc, sample=0, only_visible=True, extra=None):
        """one sample as a binary PLY (io.formats.write_ply): float x y z of `pc` (B, C >= 3, N), uchar red green blue, uchar
        `state` unless only the visible points are kept, and the columns of `extra` ({name: per-point (N,) values of that sample,
        uint8 -> uchar, anything else -> float}).  Returns the number of rows written."""
        from ..io.formats import write_ply
        if self.state is None or self.rgb is None:
            raise _C.EfghError("Fused.save_ply needs 'state' and 'rgb' among `want`")
        b = int(sample)
        state = self.state[b].cpu().numpy()
        keep = state == VISIBLE if only_visible else np.ones(state.shape, dtype=bool)
        xyz = pc[b, :3].detach().float().cpu().numpy().T
        if xyz.shape[0] != state.shape[0]:
            raise _C.EfghError('pc: %d points, the fused sample has %d' % (xyz.shape[0], state.shape[0]))
        cols = {} if only_visible else {'state': state[keep]}
        for name, col in (extra or {}).items():
            col = col.detach().cpu().numpy() if torch.is_tensor(col) else np.asarray(col)
            if col.shape != state.shape:
                raise _C.EfghError('extra[%r]: shape %s, expected %s' % (name, col.shape, state.shape))
            cols[name] = col[keep]
        write_ply(path, xyz[keep], self.rgb[b].cpu().numpy()[keep], **cols)
        return int(keep.sum())


def _fail(what, who='fuse'):
    raise _C.EfghError(who + ': ' + what)


def _cloud_dims(pc, who='fuse'):
    """(B, N) of a cloud argument float32 (B, C >= 3, N)"""
    if not torch.is_tensor(pc):
        _fail('pc: expected a tensor, got %s' % type(pc).__name__, who)
    if pc.dtype != torch.float32:
        _fail('pc: dtype %s, expected float32' % pc.dtype, who)
    if pc.dim() != 3 or pc.shape[1] < 3 or pc.shape[2] < 1 or pc.shape[0] < 1:
        _fail('pc: expected (B, C >= 3, N >= 1), got %s' % (tuple(pc.shape),), who)
    B, _, N = pc.shape
    if B > 65535 or N >= 2 ** 31:
        _fail('pc: B = %d (at most 65535) or N = %d (below 2^31) is too large' % (B, N), who)
    return B, N


def _image_u8(img, B, who='fuse'):
    """an image argument in one of the accepted forms -> (img with a batch axis, H, W), without touching the argument"""
    if not torch.is_tensor(img):
        _fail('img: expected a tensor, got %s' % type(img).__name__, who)
    if img.dtype == torch.uint8:
        if img.dim() == 3:
            img = img[None]
        if img.dim() != 4 or img.shape[3] != 3:
            _fail('img: a uint8 image is (B,H,W,3) or (H,W,3), got %s' % (tuple(img.shape),), who)
    elif img.is_floating_point():
        if img.dim() != 4 or img.shape[1] != 3:
            _fail('img: a float image is the model\'s (B,3,H,W) holding 0..255, got %s' % (tuple(img.shape),), who)
    else:
        _fail('img: dtype %s, expected uint8 or a float type' % img.dtype, who)
    if img.shape[0] != B:
        _fail('img: batch size %d, the cloud has %d' % (img.shape[0], B), who)
    H, W = (img.shape[1], img.shape[2]) if img.dtype == torch.uint8 else (img.shape[2], img.shape[3])
    if H < 1 or W < 1 or H * W >= 2 ** 31 - 1:
        _fail('img: H = %d, W = %d: both positive and H*W < 2^31' % (H, W), who)
    return img, H, W


def _finite_nonneg(name, v, who='fuse'):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) < float('inf'):
        _fail('%s: %r, expected a finite number >= 0' % (name, v), who)


def _on_the_clouds_device(pc, named, who='fuse', what='the fusion'):
    """the last check: every tensor on the GPU, and on the cloud's"""
    for name, t in (('pc', pc),) + tuple(named):
        if not t.is_cuda:
            _fail('%s: a CPU tensor; %s runs on the GPU through libefgh_hip.so only' % (name, what), who)
        if t.device != pc.device:
            _fail('%s: on %s, the cloud is on %s' % (name, t.device, pc.device), who)


def _u8_hwc(img):
    """contiguous uint8 (B,H,W,3) of a checked image; a float image as summary._u8_hwc converts it: truncation as astype('uint8')
    for in-range values"""
    if img.dtype != torch.uint8:
        img = img.detach().to(torch.int64).to(torch.uint8).permute(0, 2, 3, 1)
    return img.contiguous()


def fuse(pc, img, cam_T_velo, radius=0, rel_tol=0.0, abs_tol=0.0, min_depth=0.0, bilinear=True, want=WANT):
    """pc float32 (B, C >= 3, N) | img uint8 (B,H,W,3) / (H,W,3) or float (B,3,H,W) holding 0..255 | cam_T_velo (B,3,4) of either
    float width, or a `pred` dict -> Fused.  Inputs are never written, outputs are new tensors, nothing is read back to the host."""
    if isinstance(cam_T_velo, dict):
        if 'cam_T_velo' not in cam_T_velo:
            _fail("cam_T_velo: the dict has no 'cam_T_velo'")
        cam_T_velo = cam_T_velo['cam_T_velo']
    want = (want,) if isinstance(want, str) else tuple(want)
    for k in want:
        if k not in WANT:
            _fail('want: %r is none of %s' % (k, ', '.join(WANT)))
    if not want:
        _fail('want: nothing asked for')
    B, N = _cloud_dims(pc)
    T = cam_T_velo
    if not torch.is_tensor(T):
        _fail('cam_T_velo: expected a tensor or a dict, got %s' % type(T).__name__)
    if T.dtype not in (torch.float32, torch.float64):
        _fail('cam_T_velo: dtype %s, expected float32 or float64' % T.dtype)
    if tuple(T.shape) != (B, 3, 4):
        _fail('cam_T_velo: expected (%d, 3, 4), got %s' % (B, tuple(T.shape)))
    img, H, W = _image_u8(img, B)
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= MAX_RADIUS:
        _fail('radius: %r, supported are the integers 0 .. %d' % (radius, MAX_RADIUS))
    for name, v in (('rel_tol', rel_tol), ('abs_tol', abs_tol), ('min_depth', min_depth)):
        _finite_nonneg(name, v)
    _on_the_clouds_device(pc, (('img', img), ('cam_T_velo', T)))

    dev = pc.device
    L, st = _C.lib(), _C.stream_ptr
    with torch.cuda.device(dev):
        if pc.stride(2) != 1:
            pc = pc.contiguous()
        P = T.detach().to(torch.float64).contiguous()            # float32 -> float64 is exact
        args = (_C.ptr(pc), pc.stride(0), pc.stride(1), B, N, _C.ptr(P))
        zbuf = torch.empty(L.efgh_fuse_workspace_bytes(B, H, W) // 8, dtype=torch.int64, device=dev)
        _C.check(L.efgh_fuse_zbuffer(args[0], args[1], args[2], B, N, args[5], H, W, int(radius), float(min_depth), _C.ptr(zbuf), st()))
        out = {}
        if any(k in want for k in ('rgb', 'state', 'uv')):
            img = _u8_hwc(img)
            state = torch.empty((B, N), dtype=torch.uint8, device=dev)
            rgb = torch.empty((B, N, 3), dtype=torch.uint8, device=dev)
            uv = torch.empty((B, N, 2), dtype=torch.float32, device=dev) if 'uv' in want else None
            _C.check(L.efgh_fuse_resolve(args[0], args[1], args[2], B, N, args[5], _C.ptr(img), H, W, 1 if bilinear else 0,
                                         float(min_depth), float(rel_tol), float(abs_tol), _C.ptr(zbuf), _C.ptr(state), _C.ptr(rgb),
                                         _C.ptr(uv), st()))
            out.update(state=state, rgb=rgb, uv=uv)
        if 'depth' in want or 'index' in want:
            depth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if 'depth' in want else None
            index = torch.empty((B, H, W), dtype=torch.int32, device=dev) if 'index' in want else None
            _C.check(L.efgh_fuse_maps(_C.ptr(zbuf), B, H * W, _C.ptr(depth), _C.ptr(index), st()))
            out.update(depth=depth, index=index)
    return Fused(**{k: v for k, v in out.items() if k in want})
