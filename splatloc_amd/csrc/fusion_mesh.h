// fusion_mesh.h — the marching-cubes triangulation table of the surface mesh, derived at compile time (the
// same derivation in numpy: tests/mesh_reference.py).  Nothing in it is typed in.
//
// Corner c of a cell lies at (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's lowest voxel; bit c of a case is set when
// tsdf(corner c) < level.  Edge e = axis * 4 + k runs along `axis` from the corner whose offset along the lower of the two other
// axes is k & 1 and along the higher one (k >> 1) & 1.  Every cube face is walked through its four corners counter-clockwise as
// seen from outside; each maximal run of below corners gives one directed segment from the edge where the walk enters the run to
// the edge where it leaves it (two diagonal below corners are cut off separately, from either cell of the face alike).  The
// segments form disjoint directed loops.  Loops are taken in ascending order of their smallest edge, each from that edge, rotated
// to the first start whose fan diagonals never join two edges of one cube face (such a diagonal would lie in the face and the
// neighbouring cell could produce the same mesh edge again), and fanned from there.  The geometric normal (p1 - p0) x (p2 - p0)
// of every triangle points from below to not below.
//
// Row of a case: byte 0 the triangle count (at most 5), bytes 1..15 edge ids, 0xFF where unused.
#pragma once
#include <stdint.h>

namespace sr {

constexpr int MC_ROW = 16;
constexpr int MC_MAX_TRIANGLES = 5;

struct alignas(16) McTable {
    uint8_t b[256][MC_ROW];
};

// edge between two corners that differ in one bit
constexpr int mc_edge_between(int c0, int c1)
{
    const int d = c0 ^ c1;
    const int axis = d == 1 ? 0 : (d == 2 ? 1 : 2);
    const int s = c0 < c1 ? c0 : c1;
    const int k = axis == 0 ? (s >> 1) : (axis == 1 ? ((s & 1) | ((s >> 2) << 1)) : (s & 3));
    return axis * 4 + k;
}

// corner an edge starts at
constexpr int mc_edge_start(int e)
{
    const int axis = e >> 2, k = e & 3;
    return axis == 0 ? (k << 1) : (axis == 1 ? ((k & 1) | ((k >> 1) << 2)) : k);
}

// the two cube faces an edge lies in, as bits (axis * 2 + side)
constexpr int mc_edge_faces(int e)
{
    const int axis = e >> 2, s = mc_edge_start(e);
    int m = 0;
    for (int a = 0; a < 3; ++a)
        if (a != axis) m |= 1 << (a * 2 + ((s >> a) & 1));
    return m;
}

// corner i of the walk around the face `axis` = side, counter-clockwise from outside
constexpr int mc_face_corner(int axis, int side, int i)
{
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;   // u x v = +axis
    const int j = side ? i : 3 - i;
    const int du = (j == 1 || j == 2) ? 1 : 0, dv = j >= 2 ? 1 : 0;
    return (side << axis) | (du << u) | (dv << v);
}

constexpr McTable make_mc_table()
{
    McTable t{};
    for (int cs = 0; cs < 256; ++cs) {
        for (int k = 0; k < MC_ROW; ++k) t.b[cs][k] = 0xFF;
        int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
        for (int face = 0; face < 6; ++face) {
            int w[4] = {0, 0, 0, 0};
            bool below[4] = {false, false, false, false};
            for (int i = 0; i < 4; ++i) {
                w[i] = mc_face_corner(face >> 1, face & 1, i);
                below[i] = (cs >> w[i]) & 1;
            }
            for (int i = 0; i < 4; ++i) {
                if (!below[i] || below[(i + 3) & 3]) continue;
                int j = i;
                while (below[(j + 1) & 3]) ++j;   // ends: corner i - 1 is not below
                next[mc_edge_between(w[(i + 3) & 3], w[i])] = mc_edge_between(w[j & 3], w[(j + 1) & 3]);
            }
        }
        int count = 0, seen = 0;
        for (int e0 = 0; e0 < 12; ++e0) {
            if (next[e0] < 0 || ((seen >> e0) & 1)) continue;
            int loop[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, faces[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            int n = 0;
            for (int e = e0; n == 0 || e != e0; e = next[e]) {
                loop[n] = e;
                faces[n] = mc_edge_faces(e);
                seen |= 1 << e;
                ++n;
            }
            int s = 0;
            for (; s < n; ++s) {
                bool ok = true;
                for (int i = 2; i <= n - 2; ++i) ok = ok && !(faces[s] & faces[(s + i) % n]);
                if (ok) break;
            }
            // every loop has such a start; a table without one fails the static_asserts of fusion_mesh.hip
            for (int i = 1; i + 1 < n && s < n && count < MC_MAX_TRIANGLES; ++i) {
                t.b[cs][1 + 3 * count] = (uint8_t)loop[s];
                t.b[cs][2 + 3 * count] = (uint8_t)loop[(s + i) % n];
                t.b[cs][3 + 3 * count] = (uint8_t)loop[(s + i + 1) % n];
                ++count;
            }
        }
        t.b[cs][0] = (uint8_t)count;
    }
    return t;
}

constexpr int mc_total_triangles(const McTable& t)
{
    int n = 0;
    for (int cs = 0; cs < 256; ++cs) n += t.b[cs][0];
    return n;
}

}  // namespace sr
