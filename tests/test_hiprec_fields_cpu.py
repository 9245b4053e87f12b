"""Fits and builds on fields that are data -- a mesh -- and on fields under the tree-CSG wrapper, against the extended-precision
reference (tests/hiprec.py section 1, "Data" and "Tree CSG") on the CPU: the oracle's fits within the derived bounds, mutants of
the sampling and of the wrapper that the bounds reject, and the oracle's Create and the product's host scheduler against the
replay of the build (tests/hiprec_build.py).  tests/test_gpu_hiprec_fields.py runs the same cases on the device and shares the
caches below."""
import numpy as np
import pytest

import hiprec as R
import hiprec_build as B
from helpers import icosphere, true_distance_f64
from test_hiprec_cpu import ROOTS, query_blocks

DEGREES = (2, 3, 5, 8, 11)
DEPTHS = (0, 1, 4, 8, 10)
COUNTS = (1, 15, 16, 17, 33)
# Every mesh is placed off the coordinate planes: cells that mirror each other in a plane of symmetry of the mesh would have
# equal errors, and a build would tie at the K-th place.
SHIFT = (0.031, -0.017, 0.012)
FIELDS = ("octa", "ico", "union", "subtract", "intersect")
# Roots for the mesh fields: the unit root, and one whose (-, -, -) corner -- where hpsdf_fit_cells' lattice starts, so where the
# cells of depth 4, 8 and 10 lie -- is at the mesh's surface.
NEAR = {"octa": ((-0.07, -0.1, -0.055), (0.43, 0.4, 0.445)), "ico": ((-0.142, -0.19, -0.161), (0.483, 0.435, 0.464))}
_CACHE = {}


def octahedron(shift=SHIFT):
    """The 8-triangle octahedron of tests/test_gpu_mesh_structure.py (semi-axes 0.3, 0.25, 0.2), shifted."""
    verts = np.float32([[0.3, 0, 0], [-0.3, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.2], [0, 0, -0.2]]) + np.float32(shift)
    return verts, np.uint64([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def mesh_of(name):
    return octahedron() if name == "octa" else icosphere(1, 0.3, SHIFT)


class Recorder:
    """The oracle's mesh scan, remembering which simplices answered (vertex 0, edge 1, face 2)."""

    def __init__(self, mesh):
        self.mesh, self.simplices, self.calls = mesh, set(), 0

    def signed_distance(self, pts):
        out, tri, simp = self.mesh.signed_distance(pts)
        self.simplices |= set((np.unique(simp) // 4).tolist())
        self.calls += len(out)
        return out, tri, simp


def oracle_mesh(O, name):
    if ("mesh", name) not in _CACHE:
        _CACHE["mesh", name] = Recorder(O.MeshField(*mesh_of(name)))
    return _CACHE["mesh", name]


def old_block(name):
    """name: (root, block) -> one of test_hiprec_cpu.query_blocks' synthetic blocks (degrees 0..12, depths up to 10)."""
    if "blocks" not in _CACHE:
        made = query_blocks(np.random.default_rng(41))
        _CACHE["blocks"] = {("unit" if i < 3 else "cube", n): b for i, (n, b) in enumerate(made)}
    return _CACHE["blocks"][name]


# field -> (old block, op, inner): the inner field is the corner_fields' crease of the case's depth (its features lie in the
# first cells of the lattice) or the shifted octahedron.
CSG = {"union": (("unit", "chain"), R.OP_UNION, "crease"), "subtract": (("cube", "syn0-7"), R.OP_SUBTRACT, "octa"),
       "intersect": (("unit", "syn8-12"), R.OP_INTERSECT, "crease")}


def case_root(field, p, depth):
    if field in CSG:
        return ROOTS[CSG[field][0][0]]
    return ROOTS["unit"] if (p + depth) % 2 else NEAR[field]


def reference_field(O, field, root, depth, mutant=None):
    """The field of a case for hiprec: a DataField over the oracle's scan, or a CsgField."""
    if field not in CSG:
        return R.mesh_field(oracle_mesh(O, field), mutant)
    blk, op, inner = CSG[field]
    inner = R.mesh_field(oracle_mesh(O, "octa")) if inner == "octa" else R.corner_fields(*root, depth)[inner]
    return R.CsgField(old_block(blk), op, inner, mutant)


def oracle_field(O, field, root, depth):
    if field not in CSG:
        return oracle_mesh(O, field).mesh
    blk, op, inner = CSG[field]
    inner = oracle_mesh(O, "octa").mesh if inner == "octa" else O.AnalyticField(R.corner_fields(*root, depth)[inner])
    return O.TreeCsgField(O.Tree.from_block(old_block(blk)), inner, op)


def product_field(H, ctx, field, root, depth):
    """-> (Field, what must outlive it)."""
    if field not in CSG:
        return H.Field.mesh(ctx, *mesh_of(field)), ()
    blk, op, inner = CSG[field]
    inner = H.Field.mesh(ctx, *mesh_of("octa")) if inner == "octa" else H.Field.analytic(R.corner_fields(*root, depth)[inner])
    tree = H.DeviceTree(ctx, old_block(blk))
    return H.Field.tree_csg(tree, op, inner), (tree, inner)


def fit_cases():
    """Every degree meets every depth and every field (a Latin square), counts rotating as test_gpu_hiprec._cases does."""
    return [(p, d, FIELDS[(pi + di) % 5], COUNTS[(pi + 2 * di) % 5]) for pi, p in enumerate(DEGREES) for di, d in enumerate(DEPTHS)]


def distinct_cells(depth, n):
    """The lattice wraps after 8^depth cells: the reference is computed once per distinct cell."""
    return min(n, 8 ** depth)


def reference(O, field, p, depth, n, left=False, mutant=None):
    """fit_reference for the first n distinct cells of the case's lattice -> (ref, bmin, bmax, root), cached."""
    key = ("ref", field, p, depth, n, left, mutant)
    if key not in _CACHE:
        root = case_root(field, p, depth)
        bmin, bmax = R.lattice_cells(depth, n)
        spec = reference_field(O, field, root, depth, mutant)
        step = max(1, 2 ** 21 // (4 * p + 1) ** 3)
        parts = [R.fit_reference(spec, *root, bmin[i:i + step], bmax[i:i + step], p, depth, left) for i in range(0, n, step)]
        _CACHE[key] = ({k: np.concatenate([q[k] for q in parts]) for k in parts[0]}, bmin, bmax, root)
    return _CACHE[key]


def oracle_fits(O, field, root, depth, bmin, bmax, p, cells):
    cfg, of = O.default_config(1e-5, *root), oracle_field(O, field, root, depth)
    got = [O.fit_polynomial(of, cfg, bmin[i], bmax[i], p, depth) for i in cells]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])


# ---------------------------------------------------------------------------------------------------------------- the oracle's batch entry
def test_batched_mesh_entry_is_the_per_point_entry(O):
    """ora_mesh_signed_distance_batch gives the per-point entry's distances, triangles and simplices, bit for bit."""
    m = O.MeshField(*mesh_of("ico"))
    pts = np.random.default_rng(3).random((4000, 3)) - 0.5
    for a, b in zip(m.signed_distance(pts), m.signed_distance_per_point(pts)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_batched_query_reference_is_the_per_point_one():
    """hiprec.fapprox_batch (what a CsgField evaluates the old tree with) against fapprox_reference: the same long-double values
    bit for bit, the bounds to the last places of their float64 sums."""
    rng = np.random.default_rng(5)
    for name, blk in query_blocks(rng):
        pts = R.points_in_leaves(blk, rng, 200)
        a, b = R.fapprox_reference(blk, pts), R.fapprox_batch(blk, pts)
        assert np.array_equal(a["leaf"], b["leaf"]) and np.array_equal(a["f"], b["f"]), name
        assert np.allclose(a["f_bound"], b["f_bound"], rtol=1e-12, atol=0), name


# ---------------------------------------------------------------------------------------------------------------- fits
@pytest.mark.parametrize("case", fit_cases(), ids=lambda c: "p%d-d%d-%s-n%d" % c)
def test_oracle_fits_within_the_bounds(O, case):
    """ora_fit_polynomial on a mesh field and on the three CSG fields -- the exact mode's bits -- within fit_reference's bounds,
    coefficients and errors, with the bound unchanged (eF = 0 for the data, the old tree's Query bound under the wrapper)."""
    p, depth, field, _ = case
    n = distinct_cells(depth, 2)
    ref, bmin, bmax, root = reference(O, field, p, depth, n)
    c, e = oracle_fits(O, field, root, depth, bmin, bmax, p, range(n))
    rc, re = R.fit_ratio(ref, c, e)
    print("\n%s p%d d%d: coefficients %.3g, errors %.3g of the bound" % (field, p, depth, rc, re))
    _CACHE["worst fit"] = max(_CACHE.get("worst fit", 0.0), rc, re)
    assert rc <= 1 and re <= 1, (case, rc, re)


def test_mesh_samples_meet_vertices_edges_and_faces(O):
    """Among the samples of the icosphere's fits the closest simplex is a vertex, an edge and a face -- each pseudo-normal rule
    of the scan feeds the fits above."""
    rec = oracle_mesh(O, "ico")
    for p, depth, field, _ in fit_cases():
        if field == "ico":
            reference(O, field, p, depth, distinct_cells(depth, 2))
    assert rec.calls > 0 and rec.simplices == {0, 1, 2}, rec.simplices


def _centre_sample(root, bmin, bmax, p):
    """The centre node of the rule of order 4p + 1 (x = 0) in cell 0: its world position as the fit forms it."""
    x, _ = R.rule(4 * p + 1)
    assert int((x == 0.0).sum()) == 1
    scale = (bmax[0] - bmin[0]).astype(np.float64) * 0.5
    centre = ((bmin[0] + bmax[0]) / np.float32(2.0)).astype(np.float64)
    rmin, rmax = np.asarray(root[0], np.float32), np.asarray(root[1], np.float32)
    return (0.0 * scale + centre) * (rmax - rmin).astype(np.float64) + ((rmin + rmax) / np.float32(2.0)).astype(np.float64)


@pytest.mark.parametrize("field,p", [("union", 5), ("subtract", 8), ("intersect", 11)])
def test_centre_sample_lies_on_an_old_leafs_face(O, field, p):
    """The depth-0 cases fit a cell shallower than every old leaf under it.  The rule has 4p + 1 nodes, an odd number: its centre
    sample lies on a face of an old leaf (a corner here), the reference's descent sends it to the upper child (>=, :681-683), and
    the oracle's Query there is that leaf's series -- not the lower neighbour's, which differs by far more than the bound."""
    assert (p, 0, field) in {c[:3] for c in fit_cases()}
    root = case_root(field, p, 0)
    bmin, bmax = R.lattice_cells(0, 1)
    pt = _centre_sample(root, bmin, bmax, p)[None, :]
    blk = R.Block(old_block(CSG[field][0]))
    q = blk.to_unit(pt)
    up, low = R.fapprox_batch(blk, pt), R.fapprox_batch(blk, pt, tie_low=True)
    leaf = int(up["leaf"][0])
    assert blk.depth[leaf] > 0 and (q[0] == blk.bmin[leaf].astype(np.float64)).all(), (q, blk.bmin[leaf])
    assert int(low["leaf"][0]) != leaf and (q[0] == blk.bmax[int(low["leaf"][0])].astype(np.float64)).all()
    got = O.Tree.from_block(old_block(CSG[field][0])).query(pt)[0]
    assert abs(R.LD(got) - up["f"][0]) <= up["f_bound"][0]
    assert abs(R.LD(got) - low["f"][0]) > up["f_bound"][0] + low["f_bound"][0]


# ---------------------------------------------------------------------------------------------------------------- mutants
def _uncast_octahedron(O):
    """The mutant that does not cast: the distance at the float64 position itself (exact float64 geometry, the oracle's sign)."""
    verts, tris = octahedron()
    scan = oracle_mesh(O, "octa").mesh

    def values(pts):
        sign = np.sign(scan.signed_distance(np.ascontiguousarray(pts, np.float32))[0].astype(np.float64))
        return sign * np.array([true_distance_f64(verts, tris, q) for q in pts])
    return R.DataField(values)


# mutant -> (field, degree, depth): the smallest case that shows it.  The two that concern an old leaf's face and the old tree's
# own argument need a cell that old leaves of degree >= 1 lie under: depth 0.
MUTANT_CASES = {"ulp": ("octa", 2, 4), "nocast": ("octa", 2, 4), "subtract_swapped": ("subtract", 2, 1), "union_max": ("union", 2, 1),
                "tree_f32": ("subtract", 2, 0), "tie_low": ("subtract", 2, 0)}


@pytest.mark.parametrize("mutant", list(MUTANT_CASES))
def test_bounds_reject_the_mutants(O, mutant):
    """Each mutant of the reference -- the positions one float32 ulp off before the cast; not cast at all; subtract taken as
    max(old, -F); union taken as max; the old tree evaluated at the float32-cast point; at a centre-node tie the neighbouring old
    leaf taken -- puts the oracle's fit outside the bounds, by the margin printed.  A bound loose enough to admit one of them
    would fail here."""
    field, p, depth = MUTANT_CASES[mutant]
    root = NEAR["octa"] if field == "octa" else case_root(field, p, depth)      # (octa: cell 0 of the depth-4 lattice at the surface)
    bmin, bmax = R.lattice_cells(depth, 1)
    spec = _uncast_octahedron(O) if mutant == "nocast" else reference_field(O, field, root, depth, mutant)
    true = R.fit_reference(reference_field(O, field, root, depth), *root, bmin, bmax, p, depth)
    mut = R.fit_reference(spec, *root, bmin, bmax, p, depth)
    c, e = oracle_fits(O, field, root, depth, bmin, bmax, p, [0])
    assert max(R.fit_ratio(true, c, e)) <= 1
    rc, re = R.fit_ratio(mut, c, e)
    print("\n%s on %s p%d d%d: the oracle's fit is %.3g (coefficients) and %.3g (errors) bounds from the mutant reference" % (mutant, field, p, depth, rc, re))
    _CACHE["mutant", mutant] = (rc, re)
    assert rc > 1 and re > 1, (mutant, rc, re)


# ---------------------------------------------------------------------------------------------------------------- builds
# (a) "octa": the shifted octahedron, K = 256.  The target is the loosest of 3e-8, 4e-8, ... (steps of 1e-8) at which the replay's
#     history holds at least 16 fits of degree >= 4: 7e-8, 10 rounds, exactly 16.  At 8e-8 the build stops a round earlier with 10
#     (test_octahedron_target_is_the_loosest_with_16_fits_of_degree_4).
# (b) "union": the tree-CSG union of the oracle's sphere tree at 1e-5 (4096 leaves of degree 2 at depth 4) with a sphere of radius
#     0.15, target 2e-7, K = 64: 9 rounds, leaves down to depth 6.  Found on the way, from the reference and the oracle alone:
#     with the old sphere at (0.25, 0, 0) the cells that mirror each other in y = 0 and z = 0 have equal errors wherever the inner
#     sphere does not reach, and EVERY round past round 0 ties at the K-th place -- no position of the inner sphere can undo that, so
#     the old sphere gets the meshes' SHIFT like everything else here; with the inner sphere at (0.3, 0.3, 0.3), on the diagonal,
#     cells that swap two axes tie once more (round 1), so it is moved by INNER_OFFSET.  After both: zero undecided.
OLD_SPHERE = ((0.25 + SHIFT[0], SHIFT[1], SHIFT[2]), 0.5)
INNER_OFFSET = (0.0, 0.013, -0.021)
INNER_SPHERE = [(R.PRIM_SPHERE, R.OP_UNION, [0.3 + INNER_OFFSET[0], 0.3 + INNER_OFFSET[1], 0.3 + INNER_OFFSET[2], 0.15])]
BUILD_CASES = {"octa": (7e-8, 256), "union": (2e-7, 64)}
BUILD_ROOT = ROOTS["unit"]
SEEN = {}


def old_sphere_block(O):
    if "old sphere" not in _CACHE:
        _CACHE["old sphere"] = O.Tree.create(O.default_config(1e-5), O.sphere_field(*OLD_SPHERE), 1024).to_block()
    return _CACHE["old sphere"]


def build_spec(O, name):
    """The field of a build case for hiprec."""
    if name == "octa":
        return R.mesh_field(oracle_mesh(O, "octa"))
    return R.CsgField(old_sphere_block(O), R.OP_UNION, INNER_SPHERE)


def build_oracle_field(O, name):
    if name == "octa":
        return oracle_mesh(O, "octa").mesh
    return O.TreeCsgField(O.Tree.from_block(old_sphere_block(O)), O.AnalyticField(INNER_SPHERE), O.OP_UNION)


def build_product_field(H, ctx, O, name):
    """-> (Field, what must outlive it)."""
    if name == "octa":
        return H.Field.mesh(ctx, *octahedron()), ()
    tree, inner = H.DeviceTree(ctx, old_sphere_block(O)), H.Field.analytic(INNER_SPHERE)
    return H.Field.tree_csg(tree, R.OP_UNION, inner), (tree, inner)


def fits_of(O, name):
    """One cache of long-double fits per case, shared by every test of this module and of the GPU module."""
    if ("fits", name) not in _CACHE:
        _CACHE["fits", name] = B.Fits(build_spec(O, name), BUILD_ROOT)
    return _CACHE["fits", name]


def oracle_create(O, name):
    if ("create", name) not in _CACHE:
        target, K = BUILD_CASES[name]
        t = O.Tree.create(O.default_config(target, *BUILD_ROOT), build_oracle_field(O, name), K)
        _CACHE["create", name] = (t.to_block(), t.stats)
    return _CACHE["create", name]


def free_replay(O, name, rounds):
    if ("free", name, rounds) not in _CACHE:
        target, K = BUILD_CASES[name]
        _CACHE["free", name, rounds] = B.replay_free(build_spec(O, name), BUILD_ROOT, target, K, rounds, fits=fits_of(O, name))
    return _CACHE["free", name, rounds]


def degree4_fits(history):
    """The fits of degree >= 4 that formed rows of the leaves: a from-scratch fit and every P-append count one each."""
    return sum((p0 >= 4) + sum(q >= 4 for q in app) for p0, app in history.values())


def guided(H, O, name):
    """test_hiprec_build_cpu.run_guided's loop for a field of this module: the product's host scheduler, the oracle's job numerics,
    every round under check_round -> (block, stats, Guided.finish's observations, the float64 total after each round)."""
    if ("guided", name) not in _CACHE:
        target, K = BUILD_CASES[name]
        cfg, ocfg, f = H.make_config(target, *BUILD_ROOT), O.default_config(target, *BUILD_ROOT), build_oracle_field(O, name)
        b = H.Build(cfg, K, 0, 1)
        g = B.Guided(build_spec(O, name), BUILD_ROOT, target, K, fits=fits_of(O, name))
        totals = []
        while True:
            n = b.select()
            if n == 0:
                break
            jobs = b.jobs(n)
            headers = np.zeros((n, 9))
            for j in range(n):
                jb = jobs[j]
                res, pc, hc = O.job(f, ocfg, tuple(jb.aabb_min), tuple(jb.aabb_max), jb.depth, jb.degree, jb.err,
                                    None if jb.coarse else np.zeros(O.NCOEF[jb.degree]))
                headers[j, 0] = res.p_err
                headers[j, 1:] = list(res.h_err)
                b.inject(j, pc, hc.reshape(-1))
            g.check_round(B.job_list(jobs), headers)
            b.apply(headers)
            totals.append(float(g.tot.f64))
        _, counts = b.layout()
        blk = b.assemble([b.pack_host(None, counts[0])])
        st = b.stats()
        _CACHE["guided", name] = (blk, st, g.finish(blk, st), totals)
    return _CACHE["guided", name]


@pytest.mark.parametrize("name", list(BUILD_CASES))
def test_oracle_create_equals_the_free_replay(O, name):
    """Tree.create of the oracle on a mesh and on a tree-CSG union, one shot, against replay_free grown from long-double errors of
    the data / wrapped field alone: the tree node by node, rounds / jobs / P / H / dropped, every leaf's rows against the fits that
    formed them, zero undecided decisions and selections, the stop consistent with the true total."""
    target, K = BUILD_CASES[name]
    blk, st = oracle_create(O, name)
    rep = free_replay(O, name, st["rounds"])
    print("\n%s: rounds %d, jobs %d, P %d, H %d, max degree %d, max depth %d, min margin %.3g bounds, fits %d"
          % (name, st["rounds"], st["jobs"], st["p_refines"], st["h_refines"], rep["degree"][rep["degree"] < 13].max(), rep["depth"].max(),
             rep["min_margin"], rep["fits"].computed))
    assert rep["undecided_decisions"] == 0 and rep["undecided_selections"] == 0, (rep["undecided_decisions"], rep["undecided_selections"])
    B.same_tree(blk, rep)
    for k in ("rounds", "jobs", "p_refines", "h_refines", "dropped"):
        assert st[k] == rep["counts"][k], k
    assert rep["stop_consistent"], (float(rep["true_total"]), rep["true_bound"], rep["B"], target)
    assert st["rounds"] > 2 and st["h_refines"] > 0
    rows = B.check_leaf_rows(blk, build_spec(O, name), rep["history"], fits=fits_of(O, name))
    print("%s: leaf rows %.3g of the bound, longest chain of P-appends %d" % (name, rows["worst"], rows["chain"]))
    SEEN[name + "/rows"] = rows["worst"]
    assert rows["worst"] <= 1


@pytest.mark.parametrize("name", list(BUILD_CASES))
def test_host_scheduler_under_check_round(H, O, name):
    """The product's host scheduler with the oracle's job numerics on the same two fields, every round under check_round, then
    the assembled block: the oracle's bytes, total_error bit for bit from the restated float64 statements and within B of the true
    total, every leaf's rows; no tie at the K-th place and no undecided decision in any round."""
    blk, st, seen, _ = guided(H, O, name)
    print("\n%s: rounds %d, job errors %.3g of the bound, smallest decision margin %.3g bounds, undecided %d, ties at the K-th place %d, "
          "total drift %.3g of B (B %.3g)" % (name, st["rounds"], seen["job_error"], seen["min_margin"], seen["undecided"],
                                            seen["selection_ties"], seen["drift_over_B"], seen["B"]))
    rows = B.check_leaf_rows(blk, build_spec(O, name), seen["history"], fits=fits_of(O, name))
    SEEN[name + "/job"] = seen["job_error"]
    assert rows["worst"] <= 1 and seen["job_error"] <= 1
    assert seen["selection_ties"] == 0 and seen["undecided"] == 0
    assert blk == oracle_create(O, name)[0]
    assert oracle_create(O, name)[1]["total_error"] == st["total_error"]


def test_octahedron_target_is_the_loosest_with_16_fits_of_degree_4(H, O):
    """Case (a)'s target: at 7e-8 the replay's history holds at least 16 fits of degree >= 4; at 8e-8, the next looser step, the
    build stops after round 9 (the restated float64 total is below 8e-8 there and not before) and the replay of those 9 rounds --
    the same selections, decisions and fits -- holds fewer."""
    target, K = BUILD_CASES["octa"]
    assert target == 7e-8 and K == 256
    _, st, _, totals = guided(H, O, "octa")
    rep = free_replay(O, "octa", st["rounds"])
    assert degree4_fits(rep["history"]) >= 16, degree4_fits(rep["history"])
    looser = 8e-8
    stop = [r + 1 for r, t in enumerate(totals) if t < looser][0]
    assert stop == st["rounds"] - 1, (stop, totals)
    assert degree4_fits(free_replay(O, "octa", stop)["history"]) < 16
