"""Test-side restatement of the surface mesh (splatloc_amd/fusion.py: mesh / get_mesh; csrc/fusion_mesh.hip) in
numpy, beside fusion_reference.py:

    mc_table        the 256-case triangulation table, derived from the face-walk rule (never typed in)
    mesh_numpy      faces over surface_numpy's vertices and the vertex normals in np.float32, one rounding per operation
    cases           one seeded builder per test volume
    directed_edges / euler / used_vertices   the invariants of a closed, consistently oriented mesh

Conventions.  Corner c of a cell lies at (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's lowest voxel; bit c of a cell's case
is set when tsdf(corner c) < level.  Edge e = axis * 4 + k runs along `axis` from the corner whose offset along the lower of the
two other axes is k & 1 and along the higher one (k >> 1) & 1.  Nothing here imports the product."""
import zlib

import numpy as np

from tests import fusion_reference as R

TABLE_ROW = 16          # byte 0: triangles, bytes 1..15: edge ids, 0xFF where unused
COUNT_CRC = 0x952dd28b  # zlib.crc32 of the 256 count bytes
EDGE_CRC = 0xd468feb8   # zlib.crc32 of the 2460 edge-id bytes in case and triangle order
HISTOGRAM = [2, 16, 50, 80, 76, 32]   # cases with 0..5 triangles


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_start(e):
    """offset of the corner edge e starts at"""
    axis, k = e // 4, e % 4
    lo, hi = [a for a in range(3) if a != axis]
    o = [0, 0, 0]
    o[lo], o[hi] = k & 1, (k >> 1) & 1
    return tuple(o)


def edge_corners(e):
    s = list(edge_start(e))
    t = list(s)
    t[e // 4] = 1
    return s[0] | s[1] << 1 | s[2] << 2, t[0] | t[1] << 1 | t[2] << 2


def edge_between(c0, c1):
    for e in range(12):
        if set(edge_corners(e)) == {c0, c1}:
            return e
    raise ValueError((c0, c1))


def edge_faces(e):
    """the two cube faces (axis, side) edge e lies in"""
    s = edge_start(e)
    return {(a, s[a]) for a in range(3) if a != e // 4}


def face_walk(axis, side):
    """the four corners of the face `axis` = side, counter-clockwise as seen from outside the cube"""
    u, v = (axis + 1) % 3, (axis + 2) % 3      # u x v = +axis
    walk = []
    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
        o = [0, 0, 0]
        o[axis], o[u], o[v] = side, du, dv
        walk.append(o[0] | o[1] << 1 | o[2] << 2)
    return walk if side else walk[::-1]


def case_segments(case, flip=False):
    """{from edge: to edge}: one directed segment per maximal run of below corners on every face's walk, from the edge where the
    walk enters the run to the edge where it leaves it.  flip: the wrong model that joins, not separates, two diagonal below corners
    (runs of not-below corners instead, direction kept)"""
    nxt = {}
    for axis in range(3):
        for side in (0, 1):
            w = face_walk(axis, side)
            below = [bool(case >> c & 1) for c in w]
            if flip and below in ([True, False, True, False], [False, True, False, True]):
                # cut off the not-below corner i + 1 instead: from the edge where the walk enters the next run to the edge
                # where it left the previous one (the below side stays on the same hand)
                for i in range(4):
                    if below[i]:
                        nxt[edge_between(w[(i + 1) % 4], w[(i + 2) % 4])] = edge_between(w[i], w[(i + 1) % 4])
                continue
            for i in range(4):
                if below[i] and not below[i - 1]:
                    j = i
                    while below[(j + 1) % 4]:
                        j += 1
                    nxt[edge_between(w[i - 1], w[i])] = edge_between(w[j % 4], w[(j + 1) % 4])
    return nxt


def case_loops(case, flip=False):
    """the directed loops of a case, each from its smallest edge id, in ascending order of that id"""
    nxt = case_segments(case, flip)
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    return loops


def fan_start(loop):
    """the first rotation whose fan diagonals never join two edges of one cube face"""
    n = len(loop)
    for s in range(n):
        if all(not (edge_faces(loop[s]) & edge_faces(loop[(s + i) % n])) for i in range(2, n - 1)):
            return s
    raise ValueError(loop)


def case_triangles(case, rotate=True, flip=False, reverse=False):
    tris = []
    for loop in case_loops(case, flip):
        s = fan_start(loop) if rotate else 0
        r = loop[s:] + loop[:s]
        for i in range(1, len(r) - 1):
            tris.append((r[0], r[i + 1], r[i]) if reverse else (r[0], r[i], r[i + 1]))
    return tris


_TABLES = {}


def mc_table(rotate=True, flip=False, reverse=False):
    """[256, 16] u8.  rotate=False, flip=True and reverse=True are the wrong models of tests/test_host_fusion_mesh.py"""
    key = (rotate, flip, reverse)
    if key not in _TABLES:
        t = np.full((256, TABLE_ROW), 0xFF, np.uint8)
        for case in range(256):
            tris = case_triangles(case, rotate, flip, reverse)
            assert len(tris) <= 5
            t[case, 0] = len(tris)
            t[case, 1:1 + 3 * len(tris)] = np.asarray(tris, np.uint8).reshape(-1)
        t.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


def table_crcs(table):
    table = np.asarray(table, np.uint8).reshape(256, TABLE_ROW)
    ids = b"".join(table[c, 1:1 + 3 * int(table[c, 0])].tobytes() for c in range(256))
    return zlib.crc32(table[:, 0].tobytes()), zlib.crc32(ids), len(ids)


def cell_cases(tsdf, level):
    """[X-1, Y-1, Z-1] u8 (empty when an axis has one voxel)"""
    t = np.asarray(tsdf, np.float32)
    with np.errstate(invalid="ignore"):
        below = t < np.float32(level)
    X, Y, Z = t.shape
    case = np.zeros((max(X - 1, 0), max(Y - 1, 0), max(Z - 1, 0)), np.uint8)
    if case.size:
        for c in range(8):
            dx, dy, dz = corner_offset(c)
            case |= (below[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.uint8) << c).astype(np.uint8)
    return case


def gradient_f32(t):
    """[3, X, Y, Z] f32: 0.5f * (t[i+1] - t[i-1]) inside, the one-sided difference at the two ends, 0 on an axis of one voxel"""
    t = np.asarray(t, np.float32)
    g = np.zeros((3,) + t.shape, np.float32)
    with np.errstate(all="ignore"):
        for ax in range(3):
            n = t.shape[ax]
            if n < 2:
                continue
            m = np.moveaxis(t, ax, 0)
            d = np.moveaxis(g[ax], ax, 0)
            d[1:-1] = np.float32(0.5) * (m[2:] - m[:-2])
            d[0] = m[1] - m[0]
            d[-1] = m[-1] - m[-2]
    return g


def mesh_numpy(tsdf, level=None, table=None, surface=None, table_odd=None):
    """surface_numpy's dict plus faces [F,3] i32 (cells in ascending linear order, each cell's triangles in table order; a
    triangle's vertices are those of its three edges) and normals [M,3] f32.  table_odd: another table for the cells whose
    x + y + z is odd (a wrong model)."""
    t = np.ascontiguousarray(tsdf, np.float32)
    X, Y, Z = t.shape
    s = dict(R.surface_numpy(t, level=level) if surface is None else surface)
    lvl = np.float32(s["level"])
    table = mc_table() if table is None else np.asarray(table)
    M = s["verts"].shape[0]
    vid = np.full((3, X, Y, Z), -1, np.int64)
    vid.reshape(3, -1)[s["edge"][:, 1], s["edge"][:, 0]] = np.arange(M)
    case = cell_cases(t, lvl)
    faces = np.zeros((0, 3), np.int32)
    if case.size:
        flat_case = case.reshape(-1)
        live = np.nonzero((flat_case != 0) & (flat_case != 255))[0]       # cells with a crossing, ascending
        rows = table[flat_case[live]]                                     # [live, 16]
        cx, cy, cz = np.unravel_index(live, case.shape)
        if table_odd is not None:
            rows = np.where(((cx + cy + cz) % 2 == 1)[:, None], np.asarray(table_odd)[flat_case[live]], rows)
        starts = np.asarray([edge_start(k) for k in range(12)], np.int64)
        tri = np.full((live.size, 5, 3), -1, np.int64)
        for slot in range(15):
            e = rows[:, 1 + slot].astype(np.int64)
            ok = e != 0xFF
            ee = np.where(ok, e, 0)
            st = starts[ee]
            v = vid[ee // 4, cx + st[:, 0], cy + st[:, 1], cz + st[:, 2]]
            assert (v[ok] >= 0).all()
            tri[:, slot // 3, slot % 3] = np.where(ok, v, -1)
        keep = np.arange(5)[None, :] < rows[:, :1].astype(np.int64)
        faces = tri[keep].astype(np.int32).reshape(-1, 3)
    g = gradient_f32(t).reshape(3, -1)
    flat = t.reshape(-1)
    n, ax = s["edge"][:, 0], s["edge"][:, 1]
    nb = n + np.asarray([Y * Z, Z, 1], np.int64)[ax]
    with np.errstate(all="ignore"):
        a, b = flat[n], flat[nb] if M else flat[n]
        q = (lvl - a) / (b - a)
        gv = [g[k][n] + q * (g[k][nb] - g[k][n]) for k in range(3)]
        ln = np.sqrt((gv[0] * gv[0] + gv[1] * gv[1]) + gv[2] * gv[2])
        ok = (ln > 0) & np.isfinite(ln)
        normals = np.stack([np.where(ok, gv[k] / ln, np.float32(0)) for k in range(3)], axis=1).astype(np.float32)
    assert ln.dtype == np.float32
    s["faces"], s["normals"], s["case"] = faces, normals.reshape(M, 3), case
    return s


# ---- invariants --------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    """(unique directed edges [E,2], how often each appears [E])"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if not e.size:
        return e.reshape(0, 2), np.zeros(0, np.int64)
    return np.unique(e, axis=0, return_counts=True)


def closed_and_oriented(faces):
    """every directed edge once, and its reverse once"""
    e, n = directed_edges(faces)
    if not (n == 1).all():
        return False
    have = set(map(tuple, e.tolist()))
    return all((b, a) in have for a, b in have)


def duplicate_edges(faces):
    return int((directed_edges(faces)[1] > 1).sum())


def unpaired_edges(faces):
    e, _ = directed_edges(faces)
    have = set(map(tuple, e.tolist()))
    return sum((b, a) not in have for a, b in have)


def euler(n_vertices, faces):
    e, _ = directed_edges(faces)
    undirected = {(min(a, b), max(a, b)) for a, b in e.tolist()}
    return int(n_vertices) - len(undirected) + int(np.asarray(faces).reshape(-1, 3).shape[0])


def used_vertices(n_vertices, faces):
    used = np.zeros(int(n_vertices), bool)
    used[np.asarray(faces, np.int64).reshape(-1)] = True
    return used


def face_normals(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


# ---- builders ------------------------------------------------------------------------------------------------------------------
def sphere():
    return R.sphere_sdf((12, 12, 12), (5.3, 5.6, 5.45), 3.7)


def two_spheres():
    a = R.sphere_sdf((14, 12, 20), (6.3, 5.6, 5.45), 3.2)
    b = R.sphere_sdf((14, 12, 20), (6.6, 5.4, 13.7), 3.4)
    return np.minimum(a, b)


def torus():
    x, y, z = np.meshgrid(*[np.arange(16, dtype=np.float64)] * 3, indexing="ij")
    c = (7.4, 7.55, 7.6)
    ring = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - 4.6
    return (np.sqrt(ring ** 2 + (z - c[2]) ** 2) - 1.7).astype(np.float32)


def padded(block, value=1.0):
    return np.pad(np.asarray(block, np.float32), 1, constant_values=np.float32(value))


def random_pm1(seed, negate=False):
    """a 7 x 6 x 5 volume of +-1 from the seed, padded with +1 (negate: the whole volume negated, padding -1)"""
    rng = np.random.default_rng(seed)
    t = padded(rng.integers(0, 2, (7, 6, 5)).astype(np.float32) * np.float32(2) - np.float32(1))
    return -t if negate else t


def padded_checkerboard():
    return padded(R.checkerboard((6, 6, 6)))


def all_cases():
    """every case as a 2 x 2 x 2 block padded to 4 x 4 x 4 with +1, the 256 blocks stacked along z: [4, 4, 1024]"""
    blocks = []
    for case in range(256):
        b = np.ones((2, 2, 2), np.float32)
        for c in range(8):
            if case >> c & 1:
                b[corner_offset(c)] = -1
        blocks.append(padded(b))
    return np.concatenate(blocks, axis=2)


def cases():
    """{name: dict(tsdf, level, closed (the mesh is a closed surface), euler (None: not stated))}"""
    out = {}

    def add(name, tsdf, level=0.0, closed=True, euler=None):
        out[name] = dict(tsdf=np.ascontiguousarray(tsdf, np.float32), level=level, closed=closed, euler=euler)

    add("sphere", sphere(), euler=2)
    add("two_spheres", two_spheres(), euler=4)
    add("torus", torus(), euler=0)
    for seed in (1, 2, 3):
        add(f"random_{seed}", random_pm1(seed))
        add(f"random_{seed}_negated", random_pm1(seed, negate=True))
    add("padded_checkerboard", padded_checkerboard())
    add("all_cases", all_cases())
    add("dyadic", R.dyadic_volume((6, 7, 9), 11, neg_zero=True), closed=False)
    add("dyadic_mid_range", R.dyadic_volume((5, 8, 6), 13, level=0.25, scale=0.125, zeros=False), level=None, closed=False)
    add("dyadic_nan", R.dyadic_volume((6, 7, 9), 14, nan_share=7), closed=False)
    return out


def ambiguous_faces(case):
    """cell faces whose four corners alternate below / not below"""
    n = 0
    for axis in range(3):
        for side in (0, 1):
            b = [case >> c & 1 for c in face_walk(axis, side)]
            n += b in ([1, 0, 1, 0], [0, 1, 0, 1])
    return n


def write_case():
    """(verts f64 [20,3], faces i32 [F,3], norms f32 [20,3], colors u8 [20,3]) for the PLY writer: coordinates from a seed, and rows
    that exercise %f: halves of the sixth decimal (binary neighbours of x.xxxxxx5 round either way), values that round up into
    the next integer, magnitudes below 5e-7 of either sign (printed 0.000000 and -0.000000), negative zero, and 1e6-sized values"""
    rng = np.random.default_rng(20)
    verts = (rng.random((20, 3)) - 0.5) * 8.0
    verts[0] = [0.00000051, -0.00000051, 2.5000005]
    verts[1] = [-0.0, 0.0, -0.00000049]
    verts[2] = [0.9999995, 1.9999996, -2.9999999]
    verts[3] = [1234567.125, -7654321.5, 0.1234565]
    verts[4] = [0.3000015, 0.0625005, -0.0078125]
    norms = (rng.random((20, 3)) - 0.5).astype(np.float32)
    norms /= np.sqrt((norms * norms).sum(axis=1, keepdims=True))
    norms[0] = [0.0, -0.0, 1.0]
    norms[1] = [0.0, 0.0, 0.0]
    colors = rng.integers(0, 256, (20, 3)).astype(np.uint8)
    colors[0], colors[1] = [0, 255, 7], [255, 0, 128]
    faces = rng.integers(0, 20, (31, 3)).astype(np.int32)
    return verts, faces, norms.astype(np.float32), colors
