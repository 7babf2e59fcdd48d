"""Feature-TSDF fusion of SplatLoc's pre_process/gen_3d_fusion_feature.py (utils/fusion_utils.py, TSDFVolumeTorch) on the device.

The volume update and the surface extraction are the HIP of csrc/fusion.hip behind the C ABI (include/splatraster.h,
splatraster_fusion_*).  `TSDFVolume` has the reference class's constructor, `integrate`, `get_volume`, `sdf_trunc` and
`voxel_size`; `integrate_frames` takes stacked frames in batches of up to 8 per launch; `feature_cloud` gives the decoder's input
(vertices and their feature rows); `get_mesh`, `meshwrite` and `save_mesh` give the reference's triangle mesh and its mesh.ply
(csrc/fusion_mesh.hip).  There is no CPU fallback: without the device the calls raise, and host tensors are
refused for the volume.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _native
from .ply import header_bytes
from ._host import _ptr, _stream

MAX_FRAMES = _native.FUSION_MAX_FRAMES
MAX_FEAT_DIM = _native.FUSION_MAX_FEAT_DIM
MAX_VOXELS = 1 << 30
_STATE_KEYS = ("tsdf", "weight", "color", "feat")


def check_feat_dim(feat_dim) -> int:
    c = int(feat_dim)
    if c != feat_dim or c < 4 or c > MAX_FEAT_DIM or c % 4:
        raise ValueError(f"feat_dim must be a multiple of 4 in [4, {MAX_FEAT_DIM}], got {feat_dim}")
    return c


def _dims(voxel_dim):
    """the reference's `voxel_dim.long()`: truncation towards zero"""
    d = torch.as_tensor(voxel_dim).detach().cpu().reshape(-1)
    if d.numel() != 3:
        raise ValueError(f"voxel_dim must have 3 entries, got {d.numel()}")
    d = [int(v) for v in d.long()]
    if min(d) < 1:
        raise ValueError(f"voxel_dim must be positive, got {d}")
    if d[0] * d[1] * d[2] > MAX_VOXELS:
        raise ValueError(f"voxel_dim {d}: more than 2^30 voxels")
    return d


def volume_bytes(voxel_dim, feat_dim) -> tuple:
    """(bytes of the four volumes, bytes of the surface workspace) from the library's host-only sizing function"""
    d = _dims(voxel_dim)
    c = check_feat_dim(feat_dim)
    vb, sb = C.c_size_t(0), C.c_size_t(0)
    _native.check(_native.load().splatraster_fusion_bytes(d[0], d[1], d[2], c, C.byref(vb), C.byref(sb)), "splatraster_fusion_bytes")
    return int(vb.value), int(sb.value)


def check_memory(need: int, free: int, what: str = "the TSDF volume") -> None:
    """the constructor's guard: a clear error before anything is allocated.  It covers the four volumes; the surface workspace is
    checked when surface() allocates it, and the per-batch device copies of host images (at most 8 frames) are not counted."""
    if need > free:
        raise RuntimeError(f"{what} needs {need} bytes ({need / 2 ** 30:.2f} GiB) of device memory, "
                           f"{free} bytes ({free / 2 ** 30:.2f} GiB) are free")


def axis_tables(voxel_dim, origin, voxel_size) -> list:
    """The voxel centres along each axis as the reference computes them (fusion_utils.py:217-221): a python float times a long
    tensor (f32), plus the origin in its own dtype (f64 from gen_3d_fusion_feature.py), then .float().  The reference does this for
    every voxel; the value depends on the voxel's index along the axis only, so three tables hold them all.  CPU tensors."""
    d = _dims(voxel_dim)
    o = torch.as_tensor(origin).detach().cpu().reshape(-1)
    if o.numel() != 3:
        raise ValueError(f"origin must have 3 entries, got {o.numel()}")
    vs = float(voxel_size)
    # o[a:a + 1], not o[a]: a 0-dim f64 tensor would not promote the f32 product, the reference's [3] origin does
    return [(o[a:a + 1] + (vs * torch.arange(0, d[a]))).float().contiguous() for a in range(3)]


def grid_from_bounds(bounds, voxel_size: float = 0.02):
    """(voxel_dim, origin) of run_feature_fusion (gen_3d_fusion_feature.py:54-60) for scene bounds [3, 2]: float64 tensors, the
    dimension still fractional as there (the constructor truncates it)."""
    b = np.asarray(bounds, dtype=np.float64)
    if b.shape != (3, 2):
        raise ValueError(f"bounds must be [3, 2], got {list(b.shape)}")
    voxel_dim = (b[:, 1] - b[:, 0]) / voxel_size
    world_dims = (voxel_dim - 1) * voxel_size
    origin = b[:, 0] - (world_dims - b[:, 1] + b[:, 0]) / 2
    return torch.from_numpy(voxel_dim), torch.from_numpy(origin)


def volume_from_bounds(bounds, voxel_size: float = 0.02, feat_dim: int = 256, margin=2, device=None) -> "TSDFVolume":
    """the volume run_feature_fusion builds for a scene's bounds (gen_3d_fusion_feature.py:54-60, 70: margin 2 there)"""
    voxel_dim, origin = grid_from_bounds(bounds, voxel_size)
    return TSDFVolume(voxel_dim=voxel_dim, origin=origin, voxel_size=voxel_size, feat_dim=feat_dim, margin=margin, device=device)


def _device(device) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("TSDF fusion runs on the GPU: no HIP device is available (there is no CPU fallback)")
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError(f"TSDF fusion runs on the GPU, got device {dev}: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _free_bytes(dev) -> int:
    """what an allocation on `dev` can get: the driver's free memory plus the blocks torch's caching allocator holds unused (a
    volume freed a moment ago sits there, and mem_get_info does not count it)"""
    free, _ = torch.cuda.mem_get_info(dev)
    return int(free) + int(torch.cuda.memory_reserved(dev)) - int(torch.cuda.memory_allocated(dev))


def meshwrite(filename, verts, faces, norms, colors):
    """The reference's meshwrite (fusion_utils.py:35-76), byte for byte: an ASCII PLY of vertices "x y z nx ny nz r g b" (%f and
    %d) and faces "3 a b c"."""
    verts, norms = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(norms, np.float64).reshape(-1, 3)
    colors, faces = np.asarray(colors).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    if not (verts.shape[0] == norms.shape[0] == colors.shape[0]):
        raise ValueError(f"meshwrite: {verts.shape[0]} vertices, {norms.shape[0]} normals, {colors.shape[0]} colours")
    props = [f"property float {n}" for n in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {n}" for n in ("red", "green", "blue")]
    header = ["ply", "format ascii 1.0", f"element vertex {verts.shape[0]}", *props, f"element face {faces.shape[0]}",
              "property list uchar int vertex_index", "end_header"]
    # %d truncates a float towards zero, as astype(int64) does
    c = np.char.mod("%d", colors.astype(np.int64))
    cols = [np.char.mod("%f", a[:, k]) for a in (verts, norms) for k in range(3)] + [c[:, k] for k in range(3)]
    with open(filename, "w") as f:
        f.write("\n".join(header) + "\n")
        _write_rows(f, cols)
        fc = np.char.mod("%d", faces.astype(np.int64))
        _write_rows(f, [np.full(faces.shape[0], "3")] + [fc[:, k] for k in range(3)])


def _write_rows(f, cols):
    """one line per row: the columns (arrays of strings) joined by blanks"""
    if cols[0].shape[0] == 0:
        return
    line = cols[0]
    for c in cols[1:]:
        line = np.char.add(np.char.add(line, " "), c)
    f.write("\n".join(line.tolist()) + "\n")


class TSDFVolume:
    """`TSDFVolumeTorch(voxel_dim, origin, voxel_size, feat_dim, margin=3)` with the volumes on a ROCm device."""

    def __init__(self, voxel_dim, origin, voxel_size, feat_dim, margin=3, device=None):
        self._vol_dim = _dims(voxel_dim)
        self._feat_dim = check_feat_dim(feat_dim)
        self._voxel_size = float(voxel_size)
        if not (self._voxel_size > 0.0 and np.isfinite(self._voxel_size)):
            raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
        self._sdf_trunc = margin * self._voxel_size
        if not (self._sdf_trunc > 0.0 and np.isfinite(self._sdf_trunc)):
            raise ValueError(f"margin * voxel_size must be positive and finite, got {self._sdf_trunc}")
        self._vol_origin = torch.as_tensor(origin).detach().cpu().reshape(-1).clone()
        tables = axis_tables(self._vol_dim, self._vol_origin, self._voxel_size)
        self.bytes, self.surface_bytes = volume_bytes(self._vol_dim, self._feat_dim)
        self.device = _device(device)
        check_memory(self.bytes, _free_bytes(self.device),
                     f"a {self._vol_dim[0]} x {self._vol_dim[1]} x {self._vol_dim[2]} volume with {self._feat_dim} feature channels")
        self._axis = [t.to(self.device) for t in tables]
        self._tsdf_vol = torch.empty(self._vol_dim, dtype=torch.float32, device=self.device)
        self._weight_vol = torch.empty(self._vol_dim, dtype=torch.float32, device=self.device)
        self._color_vol = torch.empty((*self._vol_dim, 3), dtype=torch.float32, device=self.device)
        self._feat_vol = torch.empty((*self._vol_dim, self._feat_dim), dtype=torch.float32, device=self.device)
        self.reset()

    # ---- the reference's interface --------------------------------------------------------------------------------------------
    def reset(self):
        self._tsdf_vol.fill_(1.0)
        self._weight_vol.zero_()
        self._color_vol.zero_()
        self._feat_vol.zero_()

    def integrate(self, depth_im, color_im, feat_im, cam_intr, cam_pose, obs_weight=1.0):
        """One RGB-D frame with its dense feature map: depth [H,W], colour [H,W,3] (0..255), features [H,W,C], intrinsics [3,3],
        camera-to-world pose [4,4]."""
        depth_im, color_im, feat_im = (torch.as_tensor(t) for t in (depth_im, color_im, feat_im))
        if depth_im.dim() != 2:
            raise ValueError(f"depth_im must be [H, W], got {list(depth_im.shape)}")
        self.integrate_frames(depth_im[None], color_im[None], feat_im[None], cam_intr, torch.as_tensor(cam_pose)[None], obs_weight)

    def integrate_frames(self, depth_ims, color_ims, feat_ims, cam_intr, cam_poses, obs_weight=1.0):
        """Stacked frames, integrated in order, up to 8 per launch: depth [F,H,W], colour [F,H,W,3], features [F,H,W,C], poses
        [F,4,4]; intrinsics [3,3] for all frames or [F,3,3].  Bit-identical to F calls of integrate()."""
        dev = self.device
        depth = torch.as_tensor(depth_ims)
        if depth.dim() != 3:
            raise ValueError(f"depth images must be [F, H, W], got {list(depth.shape)}")
        F, H, W = (int(s) for s in depth.shape)
        color, feat = torch.as_tensor(color_ims), torch.as_tensor(feat_ims)
        if tuple(color.shape) != (F, H, W, 3):
            raise ValueError(f"colour images must be [{F}, {H}, {W}, 3], got {list(color.shape)}")
        if tuple(feat.shape) != (F, H, W, self._feat_dim):
            raise ValueError(f"feature images must be [{F}, {H}, {W}, {self._feat_dim}], got {list(feat.shape)}")
        if H < 1 or W < 1 or H > 32768 or W > 32768:
            raise ValueError(f"images of {H} x {W}: each side must be in [1, 32768]")
        poses = torch.as_tensor(cam_poses).detach().float().cpu()
        if tuple(poses.shape) != (F, 4, 4):
            raise ValueError(f"poses must be [{F}, 4, 4], got {list(poses.shape)}")
        K = torch.as_tensor(cam_intr).detach().float().cpu()
        if tuple(K.shape) == (3, 3):
            K = K[None].expand(F, 3, 3)
        if tuple(K.shape) != (F, 3, 3):
            raise ValueError(f"intrinsics must be [3, 3] or [{F}, 3, 3], got {list(K.shape)}")
        if F == 0:
            return
        # fusion_utils.py:130: the inverse of the f32 pose, on the CPU
        w2c = torch.stack([torch.inverse(poses[f]).float() for f in range(F)])[:, :3, :].reshape(F, 12).contiguous()
        intr = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], dim=1).contiguous()
        obs = float(obs_weight)
        lib = _native.load()
        vol = self._native()
        for s in range(0, F, MAX_FRAMES):
            e = min(F, s + MAX_FRAMES)
            d = depth[s:e].detach().to(device=dev, dtype=torch.float32).contiguous()
            c = color[s:e].detach().to(device=dev, dtype=torch.float32).contiguous()
            f = feat[s:e].detach().to(device=dev, dtype=torch.float32).contiguous()
            w, k = w2c[s:e].contiguous(), intr[s:e].contiguous()
            with torch.cuda.device(dev):
                st = lib.splatraster_fusion_integrate(
                    C.byref(vol), e - s, H, W, _ptr(d), _ptr(c), _ptr(f), C.cast(w.numpy().ctypes.data, C.c_void_p),
                    C.cast(k.numpy().ctypes.data, C.c_void_p), obs, self._sdf_trunc, _stream(dev))
            _native.check(st, "splatraster_fusion_integrate")

    def get_volume(self):
        return self._tsdf_vol, self._color_vol, self._weight_vol, self._feat_vol

    @property
    def sdf_trunc(self):
        return self._sdf_trunc

    @property
    def voxel_size(self):
        return self._voxel_size

    @property
    def feat_dim(self):
        return self._feat_dim

    @property
    def voxel_dim(self):
        return tuple(self._vol_dim)

    @property
    def origin(self):
        return self._vol_origin

    def state(self) -> dict:
        """the dictionary the reference's save() hands to torch.save (device tensors, not copies)"""
        return {"tsdf": self._tsdf_vol, "weight": self._weight_vol, "color": self._color_vol, "feat": self._feat_vol}

    def load_state(self, state: dict) -> None:
        mine = self.state()
        for k in _STATE_KEYS:
            if k not in state:
                raise ValueError(f"load_state: key {k!r} is missing")
            t = torch.as_tensor(state[k])
            if tuple(t.shape) != tuple(mine[k].shape):
                raise ValueError(f"load_state: {k} has shape {list(t.shape)}, the volume's is {list(mine[k].shape)}")
        for k in _STATE_KEYS:
            mine[k].copy_(torch.as_tensor(state[k]).to(device=self.device, dtype=torch.float32))

    # ---- the surface ------------------------------------------------------------------------------------------------------------
    def _native(self) -> _native.FusionVolume:
        v = _native.FusionVolume()
        for a in range(3):
            v.dim[a] = self._vol_dim[a]
            v.axis[a] = self._axis[a].data_ptr()
        v.feat_dim = self._feat_dim
        v.tsdf, v.weight = self._tsdf_vol.data_ptr(), self._weight_vol.data_ptr()
        v.color, v.feat = self._color_vol.data_ptr(), self._feat_vol.data_ptr()
        return v

    def surface(self, level=None) -> dict:
        """Vertices of the level set of the TSDF, one per crossing grid edge in ascending (voxel, axis) order (the rule is the
        project's own: INTEGRATION.md §20).  level None: 0.5 * (min + max) of the TSDF.  Device tensors: `verts` [M,3] f32 in
        voxel units, `points` [M,3] f64 in world units, `index` [M] i64 (voxel of each vertex, rounded half to even), `colors`
        [M,3] u8, `feats` [M,C] f32, `level` (0-dim f32)."""
        return self._surface(level)[0]

    def _surface(self, level):
        """(surface()'s dictionary, the surface workspace the counts and the level live in)"""
        dev = self.device
        check_memory(self.surface_bytes, _free_bytes(dev), "the surface workspace")
        ws = torch.empty(self.surface_bytes, dtype=torch.uint8, device=dev)
        lib, vol = _native.load(), self._native()
        M = C.c_int64(0)
        with torch.cuda.device(dev):
            st = lib.splatraster_fusion_surface_count(C.byref(vol), int(level is not None), 0.0 if level is None else float(level),
                                                      _ptr(ws), C.byref(M), _stream(dev))
        _native.check(st, "splatraster_fusion_surface_count")
        m = int(M.value)
        out = {"verts": torch.empty((m, 3), dtype=torch.float32, device=dev),
               "points": torch.empty((m, 3), dtype=torch.float64, device=dev),
               "index": torch.empty((m,), dtype=torch.int64, device=dev),
               "colors": torch.empty((m, 3), dtype=torch.uint8, device=dev),
               "feats": torch.empty((m, self._feat_dim), dtype=torch.float32, device=dev)}
        origin = (C.c_double * 3)(*[float(v) for v in self._vol_origin.double()])
        with torch.cuda.device(dev):
            st = lib.splatraster_fusion_surface_extract(
                C.byref(vol), _ptr(ws), self._voxel_size, C.cast(origin, C.c_void_p), m,
                *[_ptr(out[k]) if m else None for k in ("verts", "points", "index", "colors", "feats")], _stream(dev))
        _native.check(st, "splatraster_fusion_surface_extract")
        out["level"] = ws[:4].view(torch.float32)[0].clone()
        return out, ws

    def mesh(self, level=None) -> dict:
        """surface()'s dictionary plus the triangles over its vertices and the vertex normals (the rule is the project's own:
        INTEGRATION.md §20): `faces` [F,3] i32 (rows of `verts`; cells in ascending order; the geometric normal of a face points
        towards increasing TSDF) and `normals` [M,3] f32 (the normalised TSDF gradient at the vertex, zero where it vanishes)."""
        dev = self.device
        d = self._vol_dim
        lib, vol = _native.load(), self._native()
        nbytes = C.c_size_t(0)
        _native.check(lib.splatraster_fusion_mesh_bytes(d[0], d[1], d[2], C.byref(nbytes)), "splatraster_fusion_mesh_bytes")
        out, ws = self._surface(level)
        check_memory(int(nbytes.value), _free_bytes(dev), "the mesh workspace")
        mws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        F = C.c_int64(0)
        with torch.cuda.device(dev):
            st = lib.splatraster_fusion_mesh_count(C.byref(vol), _ptr(ws), _ptr(mws), C.byref(F), _stream(dev))
        _native.check(st, "splatraster_fusion_mesh_count")
        m, f = int(out["verts"].shape[0]), int(F.value)
        out["faces"] = torch.empty((f, 3), dtype=torch.int32, device=dev)
        out["normals"] = torch.empty((m, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = lib.splatraster_fusion_mesh_extract(C.byref(vol), _ptr(ws), _ptr(mws), m, f, _ptr(out["faces"]) if f else None,
                                                     _ptr(out["normals"]) if m else None, _stream(dev))
        _native.check(st, "splatraster_fusion_mesh_extract")
        return out

    def get_mesh(self, level=None):
        """The reference's get_mesh (fusion_utils.py:271-289): (verts [M,3] f64 in world units, faces [F,3] i32, norms [M,3] f32,
        colors [M,3] u8, feats [M,C] f32) as numpy arrays."""
        s = self.mesh(level)
        return tuple(s[k].cpu().numpy() for k in ("points", "faces", "normals", "colors", "feats"))

    def save_mesh(self, ply_path, npy_path=None, level=None):
        """mesh.ply with faces, as the reference's meshwrite writes it, and (npy_path given) the vertices' feature rows:
        gen_3d_fusion_feature.py:91-94 in one call.  Returns (vertices, faces)."""
        verts, faces, norms, colors, feats = self.get_mesh(level)
        for p in (ply_path, npy_path):
            if p is not None:
                os.makedirs(os.path.dirname(os.fspath(p)) or ".", exist_ok=True)
        meshwrite(ply_path, verts, faces, norms, colors)
        if npy_path is not None:
            np.save(npy_path, feats)
        return int(verts.shape[0]), int(faces.shape[0])

    def feature_cloud(self, level=None):
        """(points [M,3] f64, colors [M,3] u8, feats [M,C] f32) on the device: what get_mesh returns as verts, colors and feats,
        and what decoder.train_decoder takes as points and features."""
        s = self.surface(level)
        return s["points"], s["colors"], s["feats"]

    def save_feature_cloud(self, ply_path, npy_path, level=None):
        """mesh.ply (a point cloud: x, y, z, zero normals, red, green, blue as float properties; no faces) and feat_cloud.npy, the
        two files the reference's Autoencoder_dataset reads.  Returns the number of points."""
        points, colors, feats = self.feature_cloud(level)
        table = np.concatenate([points.cpu().numpy().astype(np.float32), np.zeros((points.shape[0], 3), np.float32),
                                colors.cpu().numpy().astype(np.float32)], axis=1)
        for p in (ply_path, npy_path):
            os.makedirs(os.path.dirname(os.fspath(p)) or ".", exist_ok=True)
        with open(ply_path, "wb") as f:
            f.write(header_bytes(["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"], table.shape[0]))
            f.write(np.ascontiguousarray(table).tobytes())
        np.save(npy_path, feats.cpu().numpy())
        return int(table.shape[0])
