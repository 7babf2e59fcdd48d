"""Test-side restatements for the feature-TSDF fusion (splatloc_amd/fusion.py, csrc/fusion.hip), beside decoder_reference.py:

    integrate_f64   the reference's integrate (utils/fusion_utils.py:112-181) for a list of voxel centres, in float64 numpy with
                    elementwise operations only (no BLAS), with the per-frame quantities whose rounding decides a voxel's fate
    integrate_f32   the kernel's operation sequence in np.float32, one rounding per operation: on the exact scenes (EDGE_SCENES) it
                    equals the reference's own f32 volumes bit for bit, ties included (tests/golden/make_golden_fusion_edges.py)
    tie_counts      how many voxel-frames of a scene sit exactly on each of the rounding rules' edges
    surface_numpy   the project's own vertex rule in numpy
    scene / images  the synthetic box room of tests/golden/make_golden_fusion.py: the camera parameters and the analytic depth are
                    built here; colour and feature images come from seeds with elementwise numpy only, bit-identical everywhere

Nothing here imports the product."""
import numpy as np

WINDOW_PX = 1e-3     # >= 100 x the f32 rounding of a pixel coordinate below 128 (2^-17 = 7.6e-6)
WINDOW_M = 1e-5      # >= 100 x the f32 rounding of a depth below 1 m (2^-24 = 6e-8)
WINDOW_TIE = 1e-3    # colour elements whose pre-rounding value lies this close to a tie

SCENES = {
    # name: voxel_dim, voxel_size, margin, feat_dim, bounds of the grid (gen_3d_fusion_feature.py's arithmetic gives the origin)
    "c256": dict(bounds=[[-0.5, 0.5], [-0.4, 0.4], [-0.3, 0.3]], voxel_size=0.02, margin=3, feat_dim=256, seed=11),
    "c8": dict(bounds=[[-0.44, 0.44], [-0.36, 0.36], [-0.3, 0.3]], voxel_size=0.02, margin=2, feat_dim=8, seed=23),
}
H, W, FOCAL, FRAMES = 60, 80, 70.0, 8
WALL = 0.07   # the room's walls lie this far inside the grid's bounds


def intrinsics():
    return np.array([[FOCAL, 0.0, (W - 1) / 2], [0.0, FOCAL, (H - 1) / 2], [0.0, 0.0, 1.0]], np.float32)


def poses(name):
    """FRAMES camera-to-world matrices (f64): positions in the middle of the room, looking at random points of the walls"""
    cfg = SCENES[name]
    rng = np.random.default_rng(cfg["seed"])
    b = np.asarray(cfg["bounds"], np.float64)
    half = (b[:, 1] - b[:, 0]) / 2 - WALL
    out = []
    for _ in range(FRAMES):
        eye = (rng.random(3) - 0.5) * half
        target = (rng.random(3) - 0.5) * 4 * half
        c2w = look_at(eye, target)
        out.append(c2w)
    return np.stack(out)


def room_depth(bounds, wall, c2w, K, h, w):
    """z-depth [F, h, w] (f32) of the axis-aligned room whose walls lie `wall` inside `bounds` (outside when negative), seen from
    inside through the cameras c2w [F,4,4] with intrinsics K"""
    b = np.asarray(bounds, np.float64)
    lo, hi = b[:, 0] + wall, b[:, 1] - wall
    K = np.asarray(K, np.float64)
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rays = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)
    out = []
    for f in range(c2w.shape[0]):
        d = rays @ c2w[f, :3, :3].T
        eye = c2w[f, :3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(d > 0, (hi - eye) / d, np.where(d < 0, (lo - eye) / d, np.inf))
        out.append(s.min(axis=-1))
    return np.stack(out).astype(np.float32)


def analytic_depth(name, c2w):
    """z-depth [FRAMES, H, W] (f32) of a scene's room; frame 2 has a block of zero depth"""
    depth = room_depth(SCENES[name]["bounds"], WALL, c2w, intrinsics(), H, W)
    depth[2, 10:25, 30:50] = 0.0
    return depth


def look_at(eye, target):
    """camera-to-world [4,4] f64: x right, y down, z forward"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.sqrt((fwd * fwd).sum())
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.sqrt((right * right).sum())
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return c2w


def images(name):
    """(colour [FRAMES,H,W,3] in [0, 255), not integers: the reference feeds rgb * 255 of a float image; features [FRAMES,H,W,C] in
    [-0.4, 0.6)), both f32"""
    cfg = SCENES[name]
    rng = np.random.default_rng(1000 + cfg["seed"])
    color = rng.random((FRAMES, H, W, 3), dtype=np.float32) * np.float32(255)
    feat = rng.random((FRAMES, H, W, cfg["feat_dim"]), dtype=np.float32) - np.float32(0.4)
    return color, feat


def grid(name):
    """(voxel_dim float64 [3], origin float64 [3]) by run_feature_fusion's arithmetic (gen_3d_fusion_feature.py:54-60)"""
    cfg = SCENES[name]
    b = np.asarray(cfg["bounds"], np.float64)
    voxel_size = cfg["voxel_size"]
    voxel_dim = (b[:, 1] - b[:, 0]) / voxel_size
    world_dims = (voxel_dim - 1) * voxel_size
    origin = b[:, 0] - (world_dims - b[:, 1] + b[:, 0]) / 2
    return voxel_dim, origin


def centres(axes):
    """[N, 3] voxel centres in the volume's linear order from the three per-axis tables"""
    x, y, z = np.meshgrid(*[np.asarray(a) for a in axes], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def integrate_f64(p, state, depth, color_im, feat_im, K, w2c, obs_weight, sdf_trunc, diag=None, windows=(WINDOW_PX, WINDOW_M)):
    """One frame.  p [N,3] voxel centres; state = dict(tsdf [N], weight [N], color [N,3], feat [N,C]) of float64 arrays, updated in
    place; depth [H,W], color_im [H,W,3], feat_im [H,W,C], K [3,3], w2c [4,4] (or [3,4]) in any float dtype, taken to float64 as
    they are; obs_weight and sdf_trunc are rounded to f32 first, as torch does with a python scalar beside an f32 tensor.
    diag (optional dict) receives `undecided` [N] (a rounding-sized change of z, a pixel coordinate or depth_diff could change the
    voxel's fate: `windows` in pixels and metres), `valid` [N], `zbar` [N] (sum of the magnitudes entering z) and `tie` [N,3]."""
    p = np.asarray(p, np.float64)
    m = np.asarray(w2c, np.float64)
    K = np.asarray(K, np.float64)
    depth = np.asarray(depth, np.float64)
    h, w = depth.shape
    obs = np.float64(np.float32(obs_weight))
    trunc = np.float64(np.float32(sdf_trunc))
    cam = [m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1] + m[r, 2] * p[:, 2] + m[r, 3] for r in range(3)]
    z = cam[2]
    front = z > 0
    zs = np.where(front, z, 1.0)
    fx_ = cam[0] * K[0, 0] / zs + K[0, 2]
    fy_ = cam[1] * K[1, 1] / zs + K[1, 2]
    px, py = np.rint(fx_), np.rint(fy_)
    inside = front & (px >= 0) & (px < w) & (py >= 0) & (py < h)
    ix = np.where(inside, px, 0).astype(np.int64)
    iy = np.where(inside, py, 0).astype(np.int64)
    d = depth[iy, ix]
    diff = d - z
    valid = inside & (d > 0) & (diff >= -trunc)
    if diag is not None:
        near_half = lambda v: np.abs(v - np.floor(v) - 0.5) < windows[0]   # noqa: E731
        # a pixel coordinate only matters in front of the camera and near the image (one pixel of slack on every side)
        near_image = front & (fx_ > -1.5) & (fx_ < w + 0.5) & (fy_ > -1.5) & (fy_ < h + 0.5)
        und = np.abs(z) < windows[1]
        und |= near_image & (near_half(fx_) | near_half(fy_))
        und |= inside & (d > 0) & (np.abs(diff + trunc) < windows[1])
        diag["undecided"] = und
        diag["valid"] = valid
        diag["zbar"] = np.abs(m[2, 0] * p[:, 0]) + np.abs(m[2, 1] * p[:, 1]) + np.abs(m[2, 2] * p[:, 2]) + np.abs(m[2, 3])
        diag["tie"] = np.zeros((p.shape[0], 3), bool)
    v = np.nonzero(valid)[0]
    w_old = state["weight"][v]
    w_new = w_old + obs
    dist = np.minimum(diff[v] / trunc, 1.0)
    state["tsdf"][v] = (w_old * state["tsdf"][v] + obs * dist) / w_new
    state["weight"][v] = w_new
    pre = (w_old[:, None] * state["color"][v] + obs * np.asarray(color_im)[iy[v], ix[v]].astype(np.float64)) / w_new[:, None]
    if diag is not None:
        diag["tie"][v] = np.abs(pre - np.floor(pre) - 0.5) < WINDOW_TIE
    state["color"][v] = np.clip(np.rint(pre), 0, 255)
    new = np.asarray(feat_im)[iy[v], ix[v]].astype(np.float64)
    state["feat"][v] = np.clip((w_old[:, None] * state["feat"][v] + obs * new) / w_new[:, None], 0, 255)
    return state


def fresh_state(n, feat_dim):
    """reset(): tsdf 1, the rest 0"""
    return {"tsdf": np.ones(n), "weight": np.zeros(n), "color": np.zeros((n, 3)), "feat": np.zeros((n, feat_dim))}


def surface_numpy(tsdf, color=None, feat=None, level=None, voxel_size=None, origin=None):
    """The vertex rule in numpy, in f32 as the device evaluates it.  tsdf [X,Y,Z] f32.  level None: 0.5 * (min + max) in f32.  One
    vertex per edge from a voxel to its +x, +y or +z neighbour whose end values satisfy (a < level) != (b < level), at
    i + (level - a) / (b - a) along the edge's axis, in ascending (voxel linear index, axis) order.  Returns a dict: level, verts
    [M,3] f32 (voxel units), index [M] i64 (linear index of rint(verts), half to even), edge [M,2] (voxel linear index, axis), and,
    when given, points [M,3] f64 = f64(verts * f32(voxel_size)) + origin, colors = floor(color[index]) u8, feats = feat[index].
    NaN voxels, as the device treats them: level None ignores them in the minimum and the maximum, as fminf / fmaxf do (a volume
    of NaN only: min = +inf, max = -inf, level NaN, no vertex); an edge with one NaN end crosses when its other end lies below the
    level, its vertex coordinate is NaN (kept in verts and points) and its index is the edge's own voxel."""
    t = np.ascontiguousarray(tsdf, np.float32)
    X, Y, Z = t.shape
    if level is None:
        with np.errstate(invalid="ignore"):
            lo = np.fmin.reduce(t.ravel(), initial=np.float32(np.inf))
            hi = np.fmax.reduce(t.ravel(), initial=np.float32(-np.inf))
            level = np.float32(0.5) * (lo + hi)
    level = np.float32(level)
    lin = np.arange(X * Y * Z, dtype=np.int64).reshape(X, Y, Z)
    keys, verts = [], []
    for ax in range(3):
        n = t.shape[ax]
        a = np.take(t, np.arange(0, n - 1), axis=ax)
        b = np.take(t, np.arange(1, n), axis=ax)
        base = np.take(lin, np.arange(0, n - 1), axis=ax)
        with np.errstate(invalid="ignore"):
            cross = (a < level) != (b < level)
        a, b, base = a[cross], b[cross], base[cross]
        with np.errstate(all="ignore"):
            tt = (level - a) / (b - a)
        ijk = np.stack(np.unravel_index(base, (X, Y, Z)), axis=1).astype(np.float32)
        ijk[:, ax] = ijk[:, ax] + tt.astype(np.float32)
        keys.append(base * 3 + ax)
        verts.append(ijk)
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    keys, verts = keys[order], np.concatenate(verts)[order].astype(np.float32)
    nan = np.isnan(verts)
    own = np.stack(np.unravel_index(keys // 3, (X, Y, Z)), axis=1)
    r = np.where(nan, own, np.rint(np.where(nan, 0, verts)).astype(np.int64))
    out = {"level": level, "verts": verts, "index": (r[:, 0] * Y + r[:, 1]) * Z + r[:, 2],
           "edge": np.stack([keys // 3, keys % 3], axis=1)}
    if voxel_size is not None:
        out["points"] = (verts * np.float32(voxel_size)).astype(np.float64) + np.asarray(origin, np.float64)
    if color is not None:
        out["colors"] = np.floor(np.asarray(color).reshape(-1, 3)[out["index"]]).astype(np.uint8)
    if feat is not None:
        f = np.asarray(feat)
        out["feats"] = f.reshape(-1, f.shape[-1])[out["index"]]
    return out


def fixture(name):
    """tests/golden/fusion_<name>.npz as a dict, the bit-packed masks unpacked to bool [N] and [N,3]"""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"fusion_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    n = int(np.prod(fx["dims"]))
    fx["undecided"] = np.unpackbits(fx["undecided"])[:n].astype(bool)
    fx["tie"] = np.unpackbits(fx["tie"])[:3 * n].astype(bool).reshape(n, 3)
    return fx


def sphere_sdf(dims, centre, radius):
    """distance to a sphere in voxel units, f32 [X,Y,Z]"""
    x, y, z = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij")
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(np.float32)


# ---- exact scenes: the reference's own f32 arithmetic is pinned, ties included ------------------------------------------------
# Axis-aligned cameras (rotations of 0 and +-1 entries, dyadic translations) over a dyadic grid: every product of the reference's
# matmul is exact and every partial sum representable, so any summation order gives the same f32 numbers and its TSDFVolumeTorch
# pins every voxel.  Images come from an integer hash with elementwise numpy only (no generator state): bit-identical everywhere.
EDGE_H, EDGE_W, EDGE_FRAMES = 9, 8, 8           # W even: W - 0.5 rounds out of the image; H odd: H - 0.5 rounds in
EDGE_K = (4.0, 4.0, 3.5, 2.0)                   # fx, fy, cx, cy
EDGE_DEPTHS = (0.0, -1.0, 1.0, 0.625, 0.625 - 2.0 ** -10, 1.1875, 4.0, np.inf, np.nan, 2.0, 0.5, 0.125, 1.625)
TIE_KINDS = ("px_half", "py_half", "px_low", "px_high", "py_low", "py_high", "diff_trunc", "color_half", "z_zero")

_I = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
_LOOK_PX = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]   # camera-to-world rotation: right = -y, down = -z, forward = +x
_LOOK_MY = [[-1, 0, 0], [0, 0, -1], [0, -1, 0]]  # right = -x, down = -z, forward = -y
_AXIS_FRAMES = [(_I, (0.0, 0.0, 0.0)), (_I, (0.125, 0.0, -1.0)), (_I, (-0.125, 0.375, 0.5)), (_I, (-0.25, -0.375, 1.0)),
                (_I, (0.5, -0.375, 0.0)), (_I, (0.0, 0.0, 2.0)), (_I, (0.0, -0.5, 0.0)), (_I, (0.125, 0.5, 1.0))]
_PERM_FRAMES = [(_LOOK_PX, (-1.0, -0.375, 0.25)), (_LOOK_PX, (0.0, 0.125, 0.0)), (_LOOK_PX, (-0.5, -0.25, 0.375)),
                (_LOOK_PX, (0.125, 0.0, -0.5)), (_LOOK_MY, (0.0, 1.0, 0.125)), (_LOOK_MY, (0.125, 0.0, 0.125)),
                (_LOOK_MY, (-0.25, 0.5, -0.375)), (_LOOK_MY, (0.0, 0.25, 0.5))]
_AXIS_GRID = dict(dims=(37, 21, 3), voxel_size=0.125, origin=(-2.0, -1.25, 0.875), margin=3)
_PERM_GRID = dict(dims=(10, 10, 24), voxel_size=0.125, origin=(-0.125, -1.0, -1.5), margin=3)
EDGE_SCENES = {
    # the exact scenes: identity rotation; signed permutations looking along +x (frames 0-3) and along -y (frames 4-7)
    "axis": dict(**_AXIS_GRID, feat_dim=8, obs_weight=1.0, frames=_AXIS_FRAMES, seed=1),
    "perm": dict(**_PERM_GRID, feat_dim=8, obs_weight=1.0, frames=_PERM_FRAMES, seed=2),
    # feature widths: 252 leaves lane 63 of the row's wave without channels, 4 leaves all lanes but one
    "c252": dict(**_AXIS_GRID, feat_dim=252, obs_weight=1.0, frames=_AXIS_FRAMES, seed=3),
    "c4": dict(**_AXIS_GRID, feat_dim=4, obs_weight=1.0, frames=_AXIS_FRAMES, seed=4),
    # observation weights: 0.5 and 2 keep every operation dyadic-friendly, 3 is inexact but pinned by the reference
    "w05": dict(**_AXIS_GRID, feat_dim=8, obs_weight=0.5, frames=_AXIS_FRAMES, seed=5),
    "w2": dict(**_AXIS_GRID, feat_dim=8, obs_weight=2.0, frames=_AXIS_FRAMES, seed=6),
    "w3": dict(**_AXIS_GRID, feat_dim=8, obs_weight=3.0, frames=_AXIS_FRAMES, seed=7),
}
EXACT_SCENES = ("axis", "perm")


def _hash(seed, *idx):
    """a 32-bit integer hash of broadcast index arrays, elementwise uint64 numpy"""
    mask = np.uint64(0xFFFFFFFF)
    h = np.uint64((seed * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF)
    for i in idx:
        h = ((h ^ np.asarray(i).astype(np.uint64)) * np.uint64(0x85EBCA6B)) & mask
        h = h ^ (h >> np.uint64(13))
        h = (h * np.uint64(0xC2B2AE35)) & mask
        h = h ^ (h >> np.uint64(16))
    return h


def edge_poses(frames):
    """camera-to-world [F,4,4] f32 and its analytic inverse [R^T | -R^T t] (exact: entries 0, +-1 and dyadic)"""
    c2w = np.zeros((len(frames), 4, 4), np.float32)
    w2c = np.zeros((len(frames), 4, 4), np.float32)
    for f, (rot, t) in enumerate(frames):
        rot, t = np.asarray(rot, np.float32), np.asarray(t, np.float32)
        c2w[f, :3, :3], c2w[f, :3, 3], c2w[f, 3, 3] = rot, t, 1
        w2c[f, :3, :3], w2c[f, :3, 3], w2c[f, 3, 3] = rot.T, -(rot.T * t[None, :]).sum(axis=1), 1
    return c2w, w2c + np.float32(0)      # + 0: no negative zeros, as torch.inverse returns them


def edge_images(seed, feat_dim, frames=EDGE_FRAMES, h=EDGE_H, w=EDGE_W, first=0):
    """(depth [F,h,w] from EDGE_DEPTHS, colour [F,h,w,3] integers 0..255, features [F,h,w,C] multiples of 1/8 in [-1, 1] and a few
    values of 300), f32, for the frames first .. first + frames - 1"""
    f, v, u = np.meshgrid(np.arange(first, first + frames), np.arange(h), np.arange(w), indexing="ij")
    depth = np.asarray(EDGE_DEPTHS, np.float32)[(_hash(seed, 1, f, v, u) % np.uint64(len(EDGE_DEPTHS))).astype(np.int64)]
    k = np.arange(3)
    color = (_hash(seed, 2, f[..., None], v[..., None], u[..., None], k) % np.uint64(256)).astype(np.float32)
    c = np.arange(feat_dim)
    hf = _hash(seed, 3, f[..., None], v[..., None], u[..., None], c)
    feat = ((hf % np.uint64(17)).astype(np.float32) - np.float32(8)) / np.float32(8)
    feat[(hf >> np.uint64(8)) % np.uint64(97) == 0] = 300.0
    return depth, color, feat


def edge_axes(dims, origin, voxel_size):
    """the three axis tables, f32: origin + voxel_size * i is exact on the dyadic grids used here (asserted against the
    reference's _world_c by the generator and against axis_tables by the device tests)"""
    return [(np.float64(origin[a]) + np.float64(voxel_size) * np.arange(dims[a])).astype(np.float32) for a in range(3)]


def edge_scene(name, frames=None):
    """everything a scene's integration takes: dict(dims, axes, origin, voxel_size, margin, sdf_trunc, feat_dim, obs_weight, K
    [3,3], poses, w2c, depth, color, feat).  frames: how many (default the scene's 8; beyond them the poses repeat from the start
    with fresh images)"""
    cfg = EDGE_SCENES[name]
    n = EDGE_FRAMES if frames is None else frames
    fr = [cfg["frames"][f % EDGE_FRAMES] for f in range(n)]
    c2w, w2c = edge_poses(fr)
    depth, color, feat = edge_images(cfg["seed"], cfg["feat_dim"], n)
    fx, fy, cx, cy = EDGE_K
    return dict(dims=tuple(cfg["dims"]), axes=edge_axes(cfg["dims"], cfg["origin"], cfg["voxel_size"]),
                origin=np.asarray(cfg["origin"], np.float64), voxel_size=cfg["voxel_size"], margin=cfg["margin"],
                sdf_trunc=cfg["margin"] * float(cfg["voxel_size"]), feat_dim=cfg["feat_dim"], obs_weight=cfg["obs_weight"],
                K=np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32), poses=c2w, w2c=w2c, depth=depth, color=color,
                feat=feat)


def fresh_state_f32(n, feat_dim):
    f = np.float32
    return {"tsdf": np.ones(n, f), "weight": np.zeros(n, f), "color": np.zeros((n, 3), f), "feat": np.zeros((n, feat_dim), f)}


def _clamp_0_255(v):
    """torch.clamp(v, 0, 255): NaN stays NaN"""
    return np.where(v < 0, np.float32(0), np.where(v > 255, np.float32(255), v))


def _is_half(v):
    return np.isfinite(v) & (v - np.floor(v) == 0.5)


def integrate_f32(axes, state, depth, color_im, feat_im, K, w2c, obs_weight, sdf_trunc, counts=None):
    """One frame in the kernel's operation sequence (csrc/fusion.hip: fus_project, fusion_integrate_kernel), np.float32 with one
    rounding per operation: cam = ((m0 x + m1 y) + m2 z) + m3, z > 0 tested first, pix = rint((cam * f) / z + c) half to even and
    compared as a float (-0.0 >= 0 keeps pixel 0), d > 0 (false for NaN) and d - z >= -trunc, dist = q > 1 ? 1 : q, the running
    means, colour rint then clamp, features clamp (NaN kept).  axes: three per-axis tables; state: f32 arrays [N], [N], [N,3],
    [N,C], updated in place.  counts (optional dict) accumulates the voxel-frames that sit exactly on an edge (TIE_KINDS)."""
    f32 = np.float32
    p = centres([np.asarray(a, f32) for a in axes])
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    m = np.asarray(w2c, f32)
    K = np.asarray(K, f32)
    depth, color_im, feat_im = np.asarray(depth, f32), np.asarray(color_im, f32), np.asarray(feat_im, f32)
    h, w = depth.shape
    obs, trunc = f32(obs_weight), f32(sdf_trunc)
    assert all(a.dtype == f32 for a in state.values())
    with np.errstate(all="ignore"):
        cam = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]
        cz = cam[2]
        front = cz > 0
        fx_ = (cam[0] * K[0, 0]) / cz + K[0, 2]
        fy_ = (cam[1] * K[1, 1]) / cz + K[1, 2]
        px, py = np.rint(fx_), np.rint(fy_)
        in_x, in_y = (px >= 0) & (px < f32(w)), (py >= 0) & (py < f32(h))
        inside = front & in_x & in_y
        ix = np.where(inside, px, 0).astype(np.int64)
        iy = np.where(inside, py, 0).astype(np.int64)
        d = depth[iy, ix]
        diff = d - cz
        valid = inside & (d > 0) & (diff >= -trunc)
        v = np.nonzero(valid)[0]
        q = diff[v] / trunc
        dist = np.where(q > 1, f32(1), q)
        w_old = state["weight"][v]
        wn = w_old + obs
        state["tsdf"][v] = (w_old * state["tsdf"][v] + obs * dist) / wn
        state["weight"][v] = wn
        pre = (w_old[:, None] * state["color"][v] + obs * color_im[iy[v], ix[v]]) / wn[:, None]
        state["color"][v] = _clamp_0_255(np.rint(pre))
        state["feat"][v] = _clamp_0_255((w_old[:, None] * state["feat"][v] + obs * feat_im[iy[v], ix[v]]) / wn[:, None])
        if counts is not None:
            # a pixel tie counts where the other coordinate is in the image and the tie lies within half a pixel of it: there
            # another rounding rule reads another pixel, or none
            tie_x = front & in_y & _is_half(fx_) & (fx_ >= -0.5) & (fx_ <= w - 0.5)
            tie_y = front & in_x & _is_half(fy_) & (fy_ >= -0.5) & (fy_ <= h - 0.5)
            new = {"px_half": tie_x.sum(), "py_half": tie_y.sum(), "px_low": (tie_x & (fx_ == -0.5)).sum(),
                   "px_high": (tie_x & (fx_ == w - 0.5)).sum(), "py_low": (tie_y & (fy_ == -0.5)).sum(),
                   "py_high": (tie_y & (fy_ == h - 0.5)).sum(), "diff_trunc": (inside & (d > 0) & (diff == -trunc)).sum(),
                   "color_half": _is_half(pre).sum(), "z_zero": (cz == 0).sum()}
            for k in TIE_KINDS:
                counts[k] = counts.get(k, 0) + int(new[k])
            counts["updates"] = counts.get("updates", 0) + int(v.size)
    return state


def integrate_scene_f32(sc, state=None, first=0, counts=None):
    """frames first .. of an edge_scene dict through integrate_f32, from `state` (default: a fresh volume)"""
    n = int(np.prod(sc["dims"]))
    state = fresh_state_f32(n, sc["feat_dim"]) if state is None else state
    for f in range(first, sc["depth"].shape[0]):
        integrate_f32(sc["axes"], state, sc["depth"][f], sc["color"][f], sc["feat"][f], sc["K"], sc["w2c"][f], sc["obs_weight"],
                      sc["sdf_trunc"], counts)
    return state


def tie_counts(name):
    """{kind: voxel-frames exactly on that edge} for a scene's 8 frames, plus `updates` (voxel-frames integrated)"""
    counts = {}
    integrate_scene_f32(edge_scene(name), counts=counts)
    return counts


def edges_fixture():
    """tests/golden/fusion_edges.npz as a dict"""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_edges.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- exact surfaces: dyadic volumes on which (level - a) / (b - a) is exact, so verts and points are pinned bit for bit -----------
_DYADIC = (-3.0, -1.0, 0.0, 1.0, 3.0)      # offsets from the level in units of `scale`: every quotient is 0, 1/4, 1/2, 3/4 or 1


def dyadic_volume(dims, seed, level=0.0, scale=1.0, nan_share=0, neg_zero=False, zeros=True):
    """[X,Y,Z] f32 of level + scale * {-3, -1, 0, 1, 3} chosen by the integer hash; one voxel in `nan_share` is NaN (0: none);
    neg_zero turns every other voxel that equals a level of 0 into -0.0; zeros=False leaves the level's own value out"""
    i, j, k = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    h = _hash(seed, 4, i, j, k)
    offs = np.asarray(_DYADIC if zeros else (-3.0, -1.0, 1.0, 3.0), np.float32)
    t = (np.float32(level) + np.float32(scale) * offs[(h % np.uint64(len(offs))).astype(np.int64)]).astype(np.float32)
    if neg_zero:
        t[(t == 0) & ((h >> np.uint64(9)) % np.uint64(2) == 0)] = np.float32(-0.0)
    if nan_share:
        t[(h >> np.uint64(11)) % np.uint64(nan_share) == 0] = np.nan
    return t


def checkerboard(dims):
    i, j, k = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    return np.where((i + j + k) % 2 == 0, np.float32(-1), np.float32(1)).astype(np.float32)


def surface_payload(dims, seed, feat_dim=4):
    """(color [X,Y,Z,3] with fractional parts 0, .25, .5 and .99 up to 254.99, feat [X,Y,Z,C] multiples of 1/8), f32"""
    i, j, k = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    c = np.arange(3)
    h = _hash(seed, 5, i[..., None], j[..., None], k[..., None], c)
    frac = np.asarray((0.0, 0.25, 0.5, 0.99), np.float32)[((h >> np.uint64(8)) % np.uint64(4)).astype(np.int64)]
    color = (h % np.uint64(255)).astype(np.float32) + frac
    hf = _hash(seed, 6, i[..., None], j[..., None], k[..., None], np.arange(feat_dim))
    feat = ((hf % np.uint64(65)).astype(np.float32) - np.float32(32)) / np.float32(8)
    return color, feat


def crossing_count(t, level):
    """edges whose ends lie on different sides of the level (a < level) != (b < level), counted by slicing"""
    with np.errstate(invalid="ignore"):
        below = t < np.float32(level)
    return int((below[1:] != below[:-1]).sum() + (below[:, 1:] != below[:, :-1]).sum() + (below[:, :, 1:] != below[:, :, :-1]).sum())


def surface_cases():
    """{name: dict(tsdf, level (None: mid-range), count (expected vertices), ties (least number of vertices at exactly i + 0.5),
    nans (least number of NaN vertices), seed)}: the exact volumes of tests/test_gpu_fusion_edges.py, checked on the host by
    tests/test_host_fusion_edges.py"""
    cases = {}

    def add(name, tsdf, level, count=None, ties=1, nans=0, seed=0):
        cases[name] = dict(tsdf=tsdf, level=level, ties=ties, nans=nans, seed=seed,
                           count=crossing_count(tsdf, level) if count is None else count)

    add("dyadic_level_0", dyadic_volume((6, 7, 9), 11, neg_zero=True), 0.0, ties=30, seed=11)
    add("dyadic_level_half", dyadic_volume((7, 6, 5), 12, level=0.5, scale=0.5), 0.5, ties=20, seed=12)
    add("dyadic_mid_range", dyadic_volume((5, 8, 6), 13, level=0.25, scale=0.125, zeros=False), None,
        count=crossing_count(dyadic_volume((5, 8, 6), 13, level=0.25, scale=0.125, zeros=False), 0.25), ties=20, seed=13)
    nan0 = dyadic_volume((6, 7, 9), 14, nan_share=7)
    add("nan_level_0", nan0, 0.0, ties=20, nans=10, seed=14)
    nan1 = dyadic_volume((6, 7, 9), 15, nan_share=5, zeros=False)
    add("nan_mid_range", nan1, None, count=crossing_count(nan1, 0.0), ties=20, nans=10, seed=15)
    add("all_nan", np.full((4, 5, 6), np.nan, np.float32), None, count=0, ties=0, seed=16)
    add("one_voxel", np.full((1, 1, 1), -1.0, np.float32), None, count=0, ties=0, seed=17)
    for name, dims in (("column_z", (1, 1, 70)), ("column_x", (70, 1, 1)), ("column_y", (1, 70, 1))):
        add(name, checkerboard(dims), 0.0, count=69, ties=69, seed=18)
        add(name + "_mid_range", checkerboard(dims), None, count=69, ties=69, seed=18)
    for name, dims in (("n_2047", (23, 89, 1)), ("n_2048", (8, 16, 16)), ("n_2049", (683, 1, 3))):
        add(name, dyadic_volume(dims, 19, neg_zero=True), 0.0, ties=100, seed=19)
    X, Y, Z = 31, 32, 30
    add("checkerboard", checkerboard((X, Y, Z)), 0.0, count=(X - 1) * Y * Z + X * (Y - 1) * Z + X * Y * (Z - 1),
        ties=(X - 1) * Y * Z + X * (Y - 1) * Z + X * Y * (Z - 1), seed=20)
    return cases
