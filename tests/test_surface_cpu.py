"""hpsdf_extract_surface without a device: the case table (exhaustively), the numpy restatement of the lattice -> mesh step on analytic
lattices, save_obj against the native OBJ reader, and the C++ drop-in's ExtractSurface / SurfaceMesh::WriteObj compiling with g++."""
import os
import subprocess

import numpy as np
import pytest

import surface_reference as S
from conftest import ROOT

MAX_TRIS = 5  # HPSDF_SURFACE_MAX_TRIS


@pytest.fixture(scope="module")
def table(H):
    return H.surface_case_table()


def crossing_edges(case):
    return {e for e, (a, b) in enumerate(S.EDGE_ENDS) if ((case >> a) & 1) != ((case >> b) & 1)}


def triangles(table, case):
    row = [int(x) for x in table[case]]
    n = row.index(-1) // 3 if -1 in row else 5
    assert all(x == -1 for x in row[3 * n:]), "row %d: entries after the terminator" % case
    return [tuple(row[3 * t:3 * t + 3]) for t in range(n)]


def test_table_cases_reference_exactly_their_crossing_edges(table):
    assert table.shape == (256, 16) and table.dtype == np.int8
    assert triangles(table, 0) == [] and triangles(table, 255) == []
    most = 0
    for case in range(256):
        tris = triangles(table, case)
        used = {e for t in tris for e in t}
        assert used == crossing_edges(case), case
        for t in tris:
            assert len(set(t)) == 3, (case, t)  # no degenerate triangle
        most = max(most, len(tris))
    assert most <= MAX_TRIS
    assert most == MAX_TRIS  # the header's figure is the rule's, not a loose bound


def corner_pos(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def edge_on_face(e, axis, side):
    a, b = S.EDGE_ENDS[e]
    return ((a >> axis) & 1) == side and ((b >> axis) & 1) == side


def face_segments(table, case, axis, side):
    """Directed triangle edges used once within the case and lying on the face (the loops' boundary there)."""
    from collections import Counter
    cnt = Counter()
    for t in triangles(table, case):
        for k in range(3):
            cnt[(t[k], t[(k + 1) % 3])] += 1
    segs = set()
    for (u, w), c in cnt.items():
        if c == 1 and (w, u) not in cnt and edge_on_face(u, axis, side) and edge_on_face(w, axis, side):
            segs.add((u, w))
    return segs


def shift_edge(e, axis):
    """The cube-local edge of the neighbour across face (axis, side 1) that is edge e of this cube (on that face)."""
    a, b = S.EDGE_ENDS[e]
    a2, b2 = a & ~(1 << axis), b & ~(1 << axis)
    for f, (p, q) in enumerate(S.EDGE_ENDS):
        if (p, q) == (a2, b2):
            return f
    raise AssertionError


def test_faces_agree_across_cases_and_with_the_neighbour(table):
    """Watertightness by exhaustion: for every face and every sign pattern on it, every case with that pattern draws the same
    segments there, and the neighbouring cube's opposite face draws them reversed."""
    for axis in range(3):
        for side in range(2):
            corners = [c for c in range(8) if ((c >> axis) & 1) == side]
            seen = {}
            for case in range(256):
                pattern = tuple((case >> c) & 1 for c in corners)
                segs = face_segments(table, case, axis, side)
                if pattern in seen:
                    assert segs == seen[pattern], (axis, side, pattern, case)
                else:
                    seen[pattern] = segs
                # crossing edges of the face each carry one segment end
                face_cross = {e for e in crossing_edges(case) if edge_on_face(e, axis, side)}
                assert {u for s in segs for u in s} == face_cross, (axis, side, case)
            assert len(seen) == 16
            if side == 1:  # neighbour across this face: its side-0 face sees the same four lattice points
                for case in range(256):
                    nb = 0
                    for c in range(8):
                        if (c >> axis) & 1 and (case >> c) & 1:
                            nb |= 1 << (c & ~(1 << axis))
                    mine = {(shift_edge(u, axis), shift_edge(w, axis)) for u, w in face_segments(table, case, axis, 1)}
                    theirs = face_segments(table, nb, axis, 0)
                    assert mine == {(w, u) for u, w in theirs}, (axis, case)


def sphere_lattice(n, r=0.37, c=(0.013, -0.021, 0.008)):
    lo, hi = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    P = S.lattice_points(lo, hi, (n, n, n))
    v = np.linalg.norm(P - np.array(c), axis=1) - r
    return lo, hi, v.reshape(n + 1, n + 1, n + 1), r, np.array(c)


@pytest.mark.parametrize("n", [16, 24, 37])
def test_restatement_sphere_is_closed_with_the_right_volume(table, n):
    lo, hi, v, r, c = sphere_lattice(n)
    verts, tris = S.extract(v, lo, hi, (n, n, n), 0.0, table)
    assert len(tris) > 0 and S.unmatched_edges(tris) == []
    assert S.euler_characteristic(verts, tris) == 2 and S.components(tris) == 1
    h = 1.0 / n
    # vertices: the exact SDF is convex along an edge, so a chord's root is at most h^2 / (8 (r - h)) off the sphere
    d = np.abs(np.linalg.norm(verts - c, axis=1) - r)
    assert d.max() <= h * h / (8 * (r - h)) + 1e-12
    # volume: inscribed within that bound, triangles sag at most (sqrt(3) h)^2 / (8 (r - h))
    vol, exact = S.signed_volume(verts, tris), 4.0 / 3.0 * np.pi * r ** 3
    assert vol > 0
    assert abs(vol - exact) <= 4 * np.pi * r * r * (h * h / (8 * (r - h)) + 3 * h * h / (8 * (r - h)))


def test_restatement_torus_has_euler_characteristic_zero(table):
    n = 40
    lo, hi = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    P = S.lattice_points(lo, hi, (n, n, n))
    q = np.sqrt(P[:, 0] ** 2 + P[:, 2] ** 2) - 0.28
    v = (np.sqrt(q * q + P[:, 1] ** 2) - 0.1).reshape(n + 1, n + 1, n + 1)
    verts, tris = S.extract(v, lo, hi, (n, n, n), 0.0, table)
    assert S.unmatched_edges(tris) == []
    assert S.euler_characteristic(verts, tris) == 0 and S.components(tris) == 1
    assert S.signed_volume(verts, tris) > 0


def test_restatement_random_field_is_open_only_at_the_lattice_boundary(table):
    rng = np.random.default_rng(7)
    n = (11, 9, 13)
    lo, hi = (-0.4, -0.3, -0.2), (0.3, 0.35, 0.4)
    v = rng.standard_normal((n[2] + 1, n[1] + 1, n[0] + 1))
    verts, tris = S.extract(v, lo, hi, n, 0.1, table)
    bad = S.unmatched_edges(tris)
    assert bad, "a random field crosses the box's faces"
    _, coords = S.lattice(lo, hi, n)
    for u, w in bad:
        pu, pw = verts[u], verts[w]
        # both ends on one face of the box
        on = [any(pu[a] == coords[a][k] and pw[a] == coords[a][k] for k in (0, -1)) for a in range(3)]
        assert any(on), (u, w, pu, pw)


def test_restatement_ordering_and_arithmetic(table):
    """Vertices in increasing edge id with the stated arithmetic; triangles in cube order."""
    lo, hi, v, r, c = sphere_lattice(8)
    verts, tris = S.extract(v, lo, hi, (8, 8, 8), 0.0, table)
    h, coords = S.lattice(lo, hi, (8, 8, 8))
    flat = v.ravel()
    k = 0
    for L in range(9 ** 3):
        i, j, kk = L % 9, (L // 9) % 9, L // 81
        for a, (idx, s) in enumerate(((i, 1), (j, 9), (kk, 81))):
            if idx == 8 or (flat[L] < 0) == (flat[L + s] < 0):
                continue
            t = (0.0 - flat[L]) / (flat[L + s] - flat[L])
            p = [coords[0][i], coords[1][j], coords[2][kk]]
            xa, xb = coords[a][idx], coords[a][idx + 1]
            p[a] = xa + t * (xb - xa)
            assert np.array_equal(np.array(p).view(np.uint64), verts[k].view(np.uint64))
            k += 1
    assert k == len(verts)


def test_save_obj_round_trips_through_the_native_reader(H, table, tmp_path):
    lo, hi, v, r, c = sphere_lattice(20)
    verts, tris = S.extract(v, lo, hi, (20, 20, 20), 0.0, table)
    verts = verts + 1e-3 * np.pi  # bits beyond float32
    p = str(tmp_path / "s.obj")
    H.save_obj(p, verts, tris)
    v2, t2 = H.load_obj(p)
    assert np.array_equal(v2.view(np.uint32), verts.astype(np.float32).view(np.uint32))
    assert np.array_equal(t2, tris)


CXX = r'''
#include "HP/Octree.h"
#include "Meshing/ObjParser.h"
#include <cstdio>
int main(int argc, char** argv) {
    try {
        SDF::Config cfg;
        cfg.targetErrorThreshold = 1e-4;
        cfg.continuity.enforce = false;
        SDF::Octree oct;
        oct.Create(cfg, SDF::DeviceField::Sphere(0.02, -0.01, 0.03, 0.3));
        const SDF::SurfaceMesh m = oct.ExtractSurface(oct.GetRootAABB(), Eigen::Vector3i(40, 36, 44));
        if (m.triangles.empty() || m.vertices.size() % 3 || m.triangles.size() % 3) { printf("empty\n"); return 2; }
        if (!m.WriteObj(argv[1])) { printf("WriteObj\n"); return 3; }
        Meshing::ObjParser parser;
        if (!parser.Load(argv[1])) { printf("ObjParser::Load\n"); return 4; }
        if (parser.GetVertices().size() * 3 != m.vertices.size() || parser.GetTriIndices().size() != m.triangles.size()) { printf("counts\n"); return 5; }
        for (size_t i = 0; i < m.triangles.size(); ++i)
            if (parser.GetTriIndices()[i] != m.triangles[i]) { printf("indices\n"); return 6; }
        printf("ok %zu %zu\n", m.vertices.size() / 3, m.triangles.size() / 3);
        return 0;
    } catch (const SDF::Error& e) {
        printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
'''


def build_surface_prog(H, tmp):
    src, exe = os.path.join(tmp, "surface.cpp"), os.path.join(tmp, "surface")
    open(src, "w").write(CXX)
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir,
           "-lhpsdf", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def test_cxx_extract_surface_compiles_with_the_eigen_shim(H, tmp_path):
    build_surface_prog(H, str(tmp_path))
