"""MI355X-native hp-adaptive SDF octree: Python host mirror of the C ABI (include/hpsdf.h).

The directory name is the one the build contract prescribes and is not a Python
identifier; load it with ``hpsdf_loader.load()`` (repo root) or importlib.  All numerics
run in ``lib/libhpsdf.so`` (HIP, gfx950).  There is no CPU fallback: without the built
library ``lib()`` raises, and without a GPU every compute entry point returns
HPSDF_ERR_NO_DEVICE, which surfaces here as ``HpsdfError``.

Reference API mirrored (file:line in the reference checkout):
  Config            Include/HP/Config.h:12-43, Source/HP/Config.cpp:5-32
  Octree.Create     Include/HP/Octree.h:50      Source/HP/Octree.cpp:312-352
  Octree.Query      Include/HP/Octree.h:71      Source/HP/Octree.cpp:662-702
  To/FromMemoryBlock Include/HP/Octree.h:65-68  Source/HP/Octree.cpp:403-456
  Union/Subtract/IntersectSDF Include/HP/Octree.h:53-59, Octree.cpp:355-400
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (HPSDF_LIBRARY=hooks: lib/libhpsdf_hooks.so, the same library with the tests' fault-injection hook compiled in -- tests/ only;
#  HPSDF_LIBRARY=lab: lib/libhpsdf_lab.so, made on demand by `build.py --lab` for tools/query_general_floor.py -- its Query lab kernels
#  return values that are not the tree's)
#  (any other name: lib/libhpsdf_<name>.so, a measurement variant made by `build.py --variant=<name>:<flags>`)
_WHICH = os.environ.get("HPSDF_LIBRARY", "")
LIB_PATH = os.path.join(_HERE, "lib", "libhpsdf_%s.so" % _WHICH if _WHICH else "libhpsdf.so")
_LIB = None

OK = 0
ERR_INVALID_ARGUMENT = 1
ERR_NO_DEVICE = 2
ERR_HIP = 3
ERR_BAD_BLOCK = 4
ERR_UNSUPPORTED = 5
ERR_STATE = 6
ERR_OUT_OF_MEMORY = 7
ERR_OPEN_MESH = 8
ERR_BUILD_LIMIT = 9
ABI_VERSION = 4  # HPSDF_ABI_VERSION this binding was written against (lib() refuses a library built with another)
PRIM_SPHERE, PRIM_BOX, PRIM_TORUS_Y, PRIM_PLANE = 0, 1, 2, 3
OP_UNION, OP_INTERSECT, OP_SUBTRACT = 0, 1, 2
JOB_HEADER_DOUBLES = 9
DEFAULT_JOBS_PER_ROUND = 1024
NCOEF = [1, 4, 10, 20, 35, 56, 83, 120, 165, 220, 286, 364, 455]
DBL_MAX = float(np.finfo(np.float64).max)


class HpsdfError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("hpsdf status %d: %s" % (status, msg))
        self.status = status


class PodConfig(C.Structure):
    """hpsdf_config == SDF::Config, 80 bytes."""
    _fields_ = [
        ("weighting_type", C.c_uint8), ("pad0", C.c_uint8 * 7),
        ("weighting_strength", C.c_double),
        ("continuity_enforce", C.c_uint8), ("pad1", C.c_uint8 * 7),
        ("continuity_strength", C.c_double),
        ("enable_logging", C.c_uint8), ("pad2", C.c_uint8 * 7),
        ("target_error_threshold", C.c_double),
        ("thread_count", C.c_uint64),
        ("root_min", C.c_float * 3),
        ("root_max", C.c_float * 3),
    ]


class Prim(C.Structure):
    _fields_ = [("kind", C.c_int32), ("op", C.c_int32), ("p", C.c_double * 8)]


class BuildOpts(C.Structure):
    _fields_ = [("max_jobs_per_round", C.c_uint64), ("rank", C.c_int32), ("world", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class Job(C.Structure):
    _fields_ = [("node_idx", C.c_uint64), ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("err", C.c_double), ("degree", C.c_uint8), ("depth", C.c_uint8), ("coarse", C.c_uint8),
                ("pad", C.c_uint8 * 5)]


class BuildStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rounds", "jobs", "p_refines", "h_refines", "dropped", "fits", "samples",
                                           "n_nodes", "n_leaves", "n_coeffs")] + [("total_error", C.c_double), ("fit_mode", C.c_uint64),
                                                                                    ("split_fits", C.c_uint64), ("device_frontier", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ContinuityStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_pairs", "n_pairs_analytic", "n_pairs_numeric", "nnz", "iterations")] + \
               [(n, C.c_double) for n in ("residual", "jump_before", "jump_after", "assemble_ms", "solve_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


CALLBACK = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_uint64, C.c_void_p)

# every symbol include/hpsdf.h declares (tests/test_capi_symbols.py checks the list against the header)
_SIGNATURES = {
    "hpsdf_config_default": (C.c_int, [C.POINTER(PodConfig)]),
    "hpsdf_last_error": (C.c_char_p, []),
    "hpsdf_version": (C.c_char_p, []),
    "hpsdf_tables_get": (C.c_int, [C.c_void_p] * 7),
    "hpsdf_ctx_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "hpsdf_ctx_destroy": (C.c_int, [C.c_void_p]),
    "hpsdf_ctx_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hpsdf_ctx_synchronize": (C.c_int, [C.c_void_p]),
    "hpsdf_ctx_set_fast_fit": (C.c_int, [C.c_void_p, C.c_int]),
    "hpsdf_ctx_set_fit_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "hpsdf_ctx_get_fit_mode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "hpsdf_ctx_set_split_min_degree": (C.c_int, [C.c_void_p, C.c_int]),
    "hpsdf_ctx_set_block_allocator": (None, [C.c_void_p] * 4),
    "hpsdf_field_release_host_copies": (C.c_int, [C.c_void_p]),
    "hpsdf_set_mesh_face_rule": (None, [C.c_int]),
    "hpsdf_get_mesh_face_rule": (C.c_int, []),
    "hpsdf_set_reduction_order": (None, [C.c_int]),
    "hpsdf_get_reduction_order": (C.c_int, []),
    "hpsdf_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "hpsdf_abi_version": (C.c_int, []),
    "hpsdf_ctx_set_reduction_order": (C.c_int, [C.c_void_p, C.c_int]),
    "hpsdf_ctx_get_reduction_order": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "hpsdf_ctx_set_mesh_face_rule": (C.c_int, [C.c_void_p, C.c_int]),
    "hpsdf_ctx_get_mesh_face_rule": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "hpsdf_ctx_set_build_limits": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "hpsdf_ctx_get_build_limits": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hpsdf_field_create_analytic": (C.c_int, [C.POINTER(Prim), C.c_int, C.POINTER(C.c_void_p)]),
    "hpsdf_field_create_callback": (C.c_int, [CALLBACK, C.c_void_p, C.POINTER(C.c_void_p)]),
    "hpsdf_field_create_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                          C.POINTER(C.c_void_p)]),
    "hpsdf_obj_load": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint64),
                                 C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]),
    "hpsdf_field_create_tree_csg": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "hpsdf_field_destroy": (C.c_int, [C.c_void_p]),
    "hpsdf_field_mesh_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "hpsdf_field_mesh_arrays": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "hpsdf_field_eval_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hpsdf_field_eval_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hpsdf_field_eval_naive_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hpsdf_field_eval_wave_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hpsdf_field_eval_lane_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hpsdf_selftest_acosf": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p]),
    "hpsdf_selftest_running_total": (C.c_int, [C.c_void_p, C.c_double, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_tree_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "hpsdf_tree_destroy": (C.c_int, [C.c_void_p]),
    "hpsdf_tree_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hpsdf_query_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hpsdf_query_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hpsdf_query_gradient_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "hpsdf_query_gradient_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "hpsdf_query_true_gradient_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]),
    "hpsdf_query_true_gradient_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]),
    "hpsdf_query_true_gradient_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]),
    "hpsdf_query_hessian_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "hpsdf_query_hessian_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "hpsdf_query_hessian_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "hpsdf_project_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_project_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_project_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_surface_project_vertices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_double), C.c_double, C.c_double,
                                                 C.c_uint32, C.POINTER(C.c_uint64)]),
    "hpsdf_cast_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "hpsdf_cast_rays_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                       C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "hpsdf_cast_rays_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                        C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "hpsdf_query_bounds_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "hpsdf_query_bounds_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "hpsdf_query_bounds_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "hpsdf_query_bounds_grid_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                                 C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_query_bounds_grid_host": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                               C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_query_bounds_grid_block": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                                C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_integrate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_integrate_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_integrate_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_integrate_pair_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                              C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_integrate_pair_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_integrate_pair_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_double, C.c_double, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_clearance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_clearance_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_clearance_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_double, C.c_uint32, C.c_double, C.c_uint32,
                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_clearance_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_uint32, C.c_double,
                                               C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "hpsdf_clearance_batch_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_uint32, C.c_double,
                                             C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "hpsdf_clearance_batch_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_uint32,
                                              C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "hpsdf_simplify":(C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]),
    "hpsdf_simplify_block": (C.c_int, [C.c_void_p, C.c_size_t, C.c_double, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]),
    "hpsdf_simplify_transfer": (C.c_int, [C.c_void_p]),
    "hpsdf_query_ray_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_void_p]),
    "hpsdf_query_ray_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_void_p]),
    "hpsdf_function_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       C.c_uint64, C.c_void_p, C.c_void_p]),
    "hpsdf_surface_case_table": (C.c_int, [C.c_void_p]),
    "hpsdf_extract_surface": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                        C.c_double, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_uint64),
                                        C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64), C.c_void_p]),
    "hpsdf_surface_last_timings": (C.c_int, [C.POINTER(C.c_double)]),
    "hpsdf_extract_surface_sparse": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                               C.c_double, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_uint64),
                                               C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64), C.c_void_p]),
    "hpsdf_extract_surface_dual": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                             C.c_double, C.c_double, C.c_uint32, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_uint64),
                                             C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint8)), C.c_void_p]),
    "hpsdf_extract_surface_dual_block": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                                   C.c_double, C.c_double, C.c_uint32, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_uint64),
                                                   C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint8)), C.c_void_p]),
    "hpsdf_surface_dual_last_timings": (C.c_int, [C.POINTER(C.c_double)]),
    "hpsdf_surface_classify_host": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                              C.c_double, C.c_uint64, C.c_uint64, C.c_void_p]),
    "hpsdf_surface_classify_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                                C.c_double, C.c_uint64, C.c_uint64, C.c_void_p]),
    "hpsdf_build_begin": (C.c_int, [C.POINTER(PodConfig), C.POINTER(BuildOpts), C.POINTER(C.c_void_p)]),
    "hpsdf_build_destroy": (C.c_int, [C.c_void_p]),
    "hpsdf_build_round_select": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "hpsdf_build_round_jobs": (C.c_int, [C.c_void_p, C.POINTER(Job)]),
    "hpsdf_build_round_slice": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hpsdf_build_round_max_slice": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "hpsdf_build_round_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_build_round_results_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "hpsdf_build_round_results_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_build_round_apply": (C.c_int, [C.c_void_p, C.c_void_p]),
    "hpsdf_build_round_inject": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "hpsdf_build_rows_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "hpsdf_build_rows_pack_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_build_rows_unpack_host": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "hpsdf_build_node_rows_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "hpsdf_build_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hpsdf_build_pack_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "hpsdf_build_pack_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hpsdf_build_assemble": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_size_t)]),
    "hpsdf_build_get_stats": (C.c_int, [C.c_void_p, C.POINTER(BuildStats)]),
    "hpsdf_continuity_post_process": (C.c_int, [C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_uint64,
                                                C.POINTER(ContinuityStats)]),
    "hpsdf_continuity_post_process_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_uint64,
                                                       C.POINTER(ContinuityStats)]),
    "hpsdf_continuity_matrix": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.POINTER(C.c_uint64)),
                                          C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_double)),
                                          C.POINTER(ContinuityStats)]),
    "hpsdf_continuity_matrix_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint64)),
                                          C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_double)),
                                          C.POINTER(ContinuityStats)]),
    "hpsdf_continuity_last_stats": (C.c_int, [C.POINTER(ContinuityStats)]),
    "hpsdf_create": (C.c_int, [C.c_void_p, C.POINTER(PodConfig), C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p),
                               C.POINTER(C.c_size_t), C.POINTER(BuildStats)]),
    "hpsdf_create_distributed": (C.c_int, [C.c_void_p, C.POINTER(PodConfig), C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(BuildStats)]),
    "hpsdf_fit_cells": (C.c_int, [C.c_void_p, C.POINTER(PodConfig), C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]),
    "hpsdf_bench_fit": (C.c_int, [C.c_void_p, C.POINTER(PodConfig), C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                  C.POINTER(C.c_double)]),
}


def lib():
    """The HIP extension.  Raises if it has not been built: there is no fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libhpsdf.so is not built (run __graft_entry__.build() or "
                              "python hp-adaptive-signed-distance-field-octree_amd/build.py); "
                              "there is no CPU fallback for the hot path")
        try:
            # torch-rocm bundles its own HIP/HSA runtime under the same SONAME; loading it first makes
            # this library bind to that one copy (two HSA runtimes in one process cannot both see the GPU)
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.hpsdf_abi_version() != ABI_VERSION:  # (structs are handed over by size: a library of another ABI would write past them)
            raise ImportError("libhpsdf.so has ABI version %d, this binding was written against %d: rebuild the library" % (L.hpsdf_abi_version(), ABI_VERSION))
        L._libc = C.CDLL(None)
        L._libc.free.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def check(rc):
    if rc != OK:
        raise HpsdfError(rc, lib().hpsdf_last_error().decode("utf-8", "replace"))


def tables():
    L = lib()
    out = {"roots": np.zeros(2080), "weights": np.zeros(2080), "normalised_lengths": np.zeros((13, 11)),
           "recurrence": np.zeros((13, 2)), "coeff_count": np.zeros(13, np.uint64),
           "basis_index": np.zeros((455, 3), np.uint64), "sum_to_n": np.zeros(50, np.uint64)}
    check(L.hpsdf_tables_get(*[out[k].ctypes.data_as(C.c_void_p) for k in
                               ("roots", "weights", "normalised_lengths", "recurrence", "coeff_count", "basis_index",
                                "sum_to_n")]))
    return out


# ------------------------------------------------------------------------------------------------
class Config:
    """SDF::Config with the reference's field names and defaults (Config.cpp:5-14)."""

    def __init__(self):
        pod = PodConfig()
        check(lib().hpsdf_config_default(C.byref(pod)))
        self.nearnessWeighting_type = 0
        self.nearnessWeighting_strength = 0.0
        self.continuity_enforce = bool(pod.continuity_enforce)
        self.continuity_strength = pod.continuity_strength
        self.enableLogging = False
        self.targetErrorThreshold = pod.target_error_threshold
        self.threadCount = int(pod.thread_count)
        self.root_min = (-0.5, -0.5, -0.5)
        self.root_max = (0.5, 0.5, 0.5)

    def to_pod(self):
        pod = PodConfig()
        pod.weighting_type = self.nearnessWeighting_type
        pod.weighting_strength = self.nearnessWeighting_strength
        pod.continuity_enforce = 1 if self.continuity_enforce else 0
        pod.continuity_strength = self.continuity_strength
        pod.enable_logging = 1 if self.enableLogging else 0
        pod.target_error_threshold = self.targetErrorThreshold
        pod.thread_count = self.threadCount
        for a in range(3):
            pod.root_min[a] = self.root_min[a]
            pod.root_max[a] = self.root_max[a]
        return pod

    @staticmethod
    def from_pod(pod):
        c = Config.__new__(Config)
        c.nearnessWeighting_type = pod.weighting_type
        c.nearnessWeighting_strength = pod.weighting_strength
        c.continuity_enforce = bool(pod.continuity_enforce)
        c.continuity_strength = pod.continuity_strength
        c.enableLogging = bool(pod.enable_logging)
        c.targetErrorThreshold = pod.target_error_threshold
        c.threadCount = int(pod.thread_count)
        c.root_min = tuple(pod.root_min)
        c.root_max = tuple(pod.root_max)
        return c


FIT_EXACT, FIT_SPLIT, FIT_FAST = 0, 1, 2


def set_reduction_order(left_assoc):
    """Eigen's 3-vector reductions (prod / norm / normalize) as (a . b) . c (True) instead of a . (b . c) (False, the default): which one
    the reference computes depends on how its Eigen was built (include/hpsdf.h).  Process-wide; set it between calls, not during."""
    lib().hpsdf_set_reduction_order(1 if left_assoc else 0)


def reduction_order():
    return int(lib().hpsdf_get_reduction_order())


def set_mesh_face_rule(reference):
    """Mesh fields: True = the reference's closest-point routine to the letter (its face-case point whatever the weights,
    Utility.cpp:5-97); False (default) = a face-case point that has left its triangle is replaced by the boundary's closest point, so
    that every evaluation path gives one answer (include/hpsdf.h).  Process-wide; set it between calls, not during."""
    lib().hpsdf_set_mesh_face_rule(1 if reference else 0)


def mesh_face_rule():
    return int(lib().hpsdf_get_mesh_face_rule())


def make_config(target=1e-10, root_min=(-0.5, -0.5, -0.5), root_max=(0.5, 0.5, 0.5), threads=1, continuity=False):
    c = Config()
    c.targetErrorThreshold = target
    c.root_min, c.root_max = tuple(root_min), tuple(root_max)
    c.threadCount = threads
    c.continuity_enforce = continuity
    return c


BLOCK_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)
BLOCK_RELEASE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
_bytes_new = C.pythonapi.PyBytes_FromStringAndSize  # (NULL, n): an uninitialised bytes object of n bytes, ours alone until returned
_bytes_new.restype, _bytes_new.argtypes = C.py_object, [C.c_void_p, C.c_ssize_t]
_bytes_ptr = C.pythonapi.PyBytes_AsString
_bytes_ptr.restype, _bytes_ptr.argtypes = C.c_void_p, [C.py_object]


class Context:
    """One GPU + one HIP stream.  stream: raw hipStream_t (int) or None for a library-owned one."""

    def __init__(self, device=0, stream=None):
        self.handle = C.c_void_p()
        check(lib().hpsdf_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self.handle)))
        self.device = device
        # Create writes its block straight into a bytes object (hpsdf_ctx_set_block_allocator): no second copy of the block
        self._blocks = {}

        def _alloc(size, _user, held=self._blocks):
            try:
                obj = _bytes_new(None, size)
                ptr = _bytes_ptr(obj)
                held[ptr] = obj
                return ptr
            except BaseException:  # noqa: BLE001 -- must not propagate through the C frames: NULL fails the build
                return None

        def _release(ptr, _user, held=self._blocks):
            held.pop(ptr, None)

        self._alloc_cb, self._release_cb = BLOCK_ALLOC(_alloc), BLOCK_RELEASE(_release)
        lib().hpsdf_ctx_set_block_allocator(self.handle, C.cast(self._alloc_cb, C.c_void_p), C.cast(self._release_cb, C.c_void_p), None)

    def _take_block(self, blk, size):
        """The bytes object behind a block pointer Create returned (or a copy of a malloc'd block)."""
        obj = self._blocks.pop(blk.value, None)
        if obj is not None and len(obj) == size:
            return obj
        data = C.string_at(blk, size)
        if obj is None:
            lib()._libc.free(blk)
        return data

    def set_stream(self, stream):
        """Moves the context to another stream (raw hipStream_t; None: the null stream).  What the context queues afterwards runs behind
        everything queued on the old stream so far, without a host wait; a library-owned old stream is synchronised and destroyed
        (include/hpsdf.h, "The stream contract")."""
        check(lib().hpsdf_ctx_set_stream(self.handle, C.c_void_p(stream) if stream else None))

    def set_reduction_order(self, left_assoc):
        """This context's own reduction order (True / False), or None to follow the process-wide setting again (hpsdf.h)."""
        check(lib().hpsdf_ctx_set_reduction_order(self.handle, -1 if left_assoc is None else (1 if left_assoc else 0)))

    def reduction_order(self):
        v = C.c_int()
        check(lib().hpsdf_ctx_get_reduction_order(self.handle, C.byref(v)))
        return v.value

    def set_mesh_face_rule(self, reference):
        """This context's own mesh face rule (True = the reference's), or None to follow the process-wide rule again."""
        check(lib().hpsdf_ctx_set_mesh_face_rule(self.handle, -1 if reference is None else (1 if reference else 0)))

    def mesh_face_rule(self):
        v = C.c_int()
        check(lib().hpsdf_ctx_get_mesh_face_rule(self.handle, C.byref(v)))
        return v.value

    def set_build_limits(self, max_nodes=0, max_bytes=0):
        """Bounds on a Create (hpsdf_ctx_set_build_limits): 0 = the default (no bound on nodes; bytes: 1/64 of the free device
        memory, at least 1 GiB), None = no limit.  A build that crosses one raises HpsdfError with status ERR_BUILD_LIMIT."""
        none = (1 << 64) - 1
        check(lib().hpsdf_ctx_set_build_limits(self.handle, none if max_nodes is None else int(max_nodes), none if max_bytes is None else int(max_bytes)))

    def build_limits(self):
        a, b = C.c_uint64(), C.c_uint64()
        check(lib().hpsdf_ctx_get_build_limits(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_fast_fit(self, on=True):
        """Every row of every fit of degree >= 4 on the matrix cores (FIT_FAST; errors then only agree to ~1e-15)."""
        check(lib().hpsdf_ctx_set_fast_fit(self.handle, 1 if on else 0))

    def set_fit_mode(self, mode):
        """FIT_EXACT (0): every row bit-exact, the canonical bytes; FIT_SPLIT (1, default): top-degree rows of from-scratch fits of
        degree >= split_min_degree (default 6) exact, the rows below them by sum factorisation from the same samples -- errors and topology
        canonical; FIT_FAST (2): every row of every fit of degree >= 4 on the matrix cores."""
        check(lib().hpsdf_ctx_set_fit_mode(self.handle, int(mode)))

    def set_split_min_degree(self, degree):
        """FIT_SPLIT splits from-scratch fits from this degree on (2..12, 12 = never; default 6: it pays from degree 5)."""
        check(lib().hpsdf_ctx_set_split_min_degree(self.handle, int(degree)))

    def fit_mode(self):
        m = C.c_int(0)
        check(lib().hpsdf_ctx_get_fit_mode(self.handle, C.byref(m)))
        return m.value

    def synchronize(self):
        check(lib().hpsdf_ctx_synchronize(self.handle))

    def close(self):
        if self.handle:
            lib().hpsdf_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# one 64-byte BVH node / slab record (csrc/device_types.hpp: BvhNode, NodeSlab), as Field.mesh_arrays returns them
BVH_DTYPE = np.dtype([("lo0", np.float32, 3), ("hi0", np.float32, 3), ("lo1", np.float32, 3), ("hi1", np.float32, 3),
                      ("c0", np.int32), ("c1", np.int32), ("pad", np.uint32, 2)])
SLAB_DTYPE = np.dtype([("g0", np.float32, 4), ("n0", np.float32, 4), ("g1", np.float32, 4), ("n1", np.float32, 4)])


class Field:
    def __init__(self, handle, keep=(), kind=None):
        self.handle = handle
        self._keep = keep
        self.kind = kind  # "analytic" | "callback" | "mesh" | "tree_csg"

    @staticmethod
    def analytic(spec):
        """spec: list of (kind, op, params)."""
        arr = (Prim * len(spec))()
        for i, (kind, op, params) in enumerate(spec):
            arr[i].kind, arr[i].op = kind, op
            for j, v in enumerate(params):
                arr[i].p[j] = float(v)
        h = C.c_void_p()
        check(lib().hpsdf_field_create_analytic(arr, len(spec), C.byref(h)))
        return Field(h, kind="analytic")

    @staticmethod
    def sphere(centre=(0.25, 0.0, 0.0), radius=0.5):
        return Field.analytic([(PRIM_SPHERE, OP_UNION, list(centre) + [radius])])

    @staticmethod
    def union3():
        """BASELINE config[1]: union of sphere, box, torus."""
        return Field.analytic([
            (PRIM_SPHERE, OP_UNION, [-0.2, -0.15, 0.1, 0.18]),
            (PRIM_BOX, OP_UNION, [0.15, 0.2, -0.1, 0.12, 0.10, 0.15]),
            (PRIM_TORUS_Y, OP_UNION, [0.0, -0.2, -0.2, 0.15, 0.05]),
        ])

    @staticmethod
    def callback(fn):
        """fn(pt: (x,y,z), thread_idx) -> float, called from host threads."""
        def tramp(p, t, _u):
            return float(fn((p[0], p[1], p[2]), t))
        cb = CALLBACK(tramp)
        h = C.c_void_p()
        check(lib().hpsdf_field_create_callback(cb, None, C.byref(h)))
        return Field(h, keep=(cb, fn), kind="callback")

    @staticmethod
    def mesh(ctx, verts, tris):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tris, np.uint64).reshape(-1, 3)
        h = C.c_void_p()
        check(lib().hpsdf_field_create_mesh(ctx.handle, v.ctypes.data_as(C.c_void_p), len(v),
                                            t.ctypes.data_as(C.c_void_p), len(t), C.byref(h)))
        return Field(h, keep=(ctx,), kind="mesh")

    @staticmethod
    def tree_csg(tree, op, inner):
        h = C.c_void_p()
        check(lib().hpsdf_field_create_tree_csg(tree.handle, op, inner.handle, C.byref(h)))
        return Field(h, keep=(tree, inner), kind="tree_csg")

    def eval(self, ctx, pts):
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        check(lib().hpsdf_field_eval_host(ctx.handle, self.handle, pts.ctypes.data_as(C.c_void_p), len(pts),
                                          out.ctypes.data_as(C.c_void_p)))
        return out

    def eval_naive(self, ctx, pts):
        """Mesh fields: Mesh::SignedDistanceAtPt(pt) without the BVH -- the O(n) scan, on the GPU."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        check(lib().hpsdf_field_eval_naive_host(ctx.handle, self.handle, pts.ctypes.data_as(C.c_void_p), len(pts),
                                                out.ctypes.data_as(C.c_void_p)))
        return out

    def eval_wave(self, ctx, pts):
        """Mesh fields: the BVH query as Create's sampler runs it (64 consecutive points share one traversal)."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        check(lib().hpsdf_field_eval_wave_host(ctx.handle, self.handle, pts.ctypes.data_as(C.c_void_p), len(pts),
                                               out.ctypes.data_as(C.c_void_p)))
        return out

    def eval_lane(self, ctx, pts):
        """Mesh fields: the per-point stack traversal (what the fused mesh fit and a mesh under a tree-CSG wrapper run;
        eval() itself takes the shared traversal for plain mesh fields): same bits."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        check(lib().hpsdf_field_eval_lane_host(ctx.handle, self.handle, pts.ctypes.data_as(C.c_void_p), len(pts),
                                               out.ctypes.data_as(C.c_void_p)))
        return out

    def mesh_stats(self, reset=True):
        """BVH traversal counters (mesh fields created under HPSDF_MESH_STATS=1, diagnostic builds): wave queries, nodes
        visited, pairs through the lower-bound test ("tri_tests"), pairs through the closest-point test ("tri_test_lanes")."""
        out = (C.c_uint64 * 8)()
        check(lib().hpsdf_field_mesh_stats(self.handle, out, 1 if reset else 0))
        return dict(zip(("wave_queries", "node_visits", "tri_tests", "tri_test_lanes", "leaf_pairs", "bound_batches", "closest_batches",
                         "seed_exact"), (int(v) for v in out)))

    def mesh_arrays(self, ctx=None):
        """Mesh fields, diagnostics: host copies of what the field keeps on its device (read-only), as a dict of numpy arrays --
        verts (nVerts, 3) f32, tris (nTris, 3) u32, triPos and triPre (nTris, 12) f32, halfEdges (3 nTris) u32, bvh (BVH_DTYPE) and slabs
        (SLAB_DTYPE, or None for a field without them) -- with nVerts, nTris, nBvhNodes, leafLog2.  The field knows its device: ctx is
        accepted for symmetry with the eval calls."""
        info = (C.c_uint64 * 5)()
        check(lib().hpsdf_field_mesh_arrays(self.handle, info, None, None))
        nv, nt, nn, leaf_log2, has_slabs = (int(v) for v in info)
        arrs = [np.empty((nv, 3), np.float32), np.empty((nt, 3), np.uint32), np.empty((nt, 12), np.float32), np.empty((nt, 12), np.float32),
                np.empty(3 * nt, np.uint32), np.empty(nn, BVH_DTYPE), np.empty(nn if has_slabs else 0, SLAB_DTYPE)]
        bufs = (C.c_void_p * 7)(*[a.ctypes.data if a.size else None for a in arrs])
        caps = (C.c_uint64 * 7)(*[a.nbytes for a in arrs])
        check(lib().hpsdf_field_mesh_arrays(self.handle, info, bufs, caps))
        out = dict(zip(("verts", "tris", "triPos", "triPre", "halfEdges", "bvh", "slabs"), arrs))
        if not has_slabs:
            out["slabs"] = None
        out.update(nVerts=nv, nTris=nt, nBvhNodes=nn, leafLog2=leaf_log2)
        return out

    def release_host_copies(self):
        """Drops the host-side copies of a mesh field's arrays that calls of one or two points are answered from (they come back with
        the next such call)."""
        check(lib().hpsdf_field_release_host_copies(self.handle))

    def close(self):
        if self.handle:
            lib().hpsdf_field_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTree:
    """A serialised octree resident in HBM (FromMemoryBlock on the device side)."""

    def __init__(self, ctx, block):
        self.ctx = ctx
        self.block = bytes(block)
        self.handle = C.c_void_p()
        check(lib().hpsdf_tree_upload(ctx.handle, self.block, len(self.block), C.byref(self.handle)))

    def info(self):
        nn, nc, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        md, mdep = C.c_int(), C.c_int()
        check(lib().hpsdf_tree_info(self.handle, C.byref(nn), C.byref(nc), C.byref(nl), C.byref(md), C.byref(mdep)))
        return {"n_nodes": nn.value, "n_coeffs": nc.value, "n_leaves": nl.value, "max_degree": md.value,
                "max_depth": mdep.value}

    def query(self, pts):
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        check(lib().hpsdf_query_host(self.ctx.handle, self.handle, pts.ctypes.data_as(C.c_void_p), len(pts),
                                     out.ctypes.data_as(C.c_void_p)))
        return out

    def query_with_gradient(self, pts, grad_init=None):
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        grad = np.zeros((len(pts), 3)) if grad_init is None else np.array(grad_init, np.float64).reshape(-1, 3).copy()
        check(lib().hpsdf_query_gradient_host(self.ctx.handle, self.handle, pts.ctypes.data_as(C.c_void_p), len(pts),
                                              out.ctypes.data_as(C.c_void_p), grad.ctypes.data_as(C.c_void_p)))
        return out, grad

    def query_gradient(self, pts, unit=False):
        """QueryGradient (include/hpsdf.h): Query's values and the gradient of the polynomial they come from -- not
        query_with_gradient's shortcut -> (values f64 [n], grad f64 [n,3]); unit: rows normalised.  Outside the root: DBL_MAX, NaN rows."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out, grad = np.empty(len(pts)), np.empty((len(pts), 3))
        check(lib().hpsdf_query_true_gradient_host(self.ctx.handle, self.handle, pts.ctypes.data_as(C.c_void_p), len(pts),
                                                   GRADIENT_UNIT if unit else 0, out.ctypes.data_as(C.c_void_p), grad.ctypes.data_as(C.c_void_p)))
        return out, grad

    def query_gradient_device(self, d_xyz_ptr, n, d_out_ptr, d_grad_ptr, unit=False):
        """Raw device pointers (ints; d_out_ptr may be 0: gradients only); asynchronous on the context stream."""
        check(lib().hpsdf_query_true_gradient_device(self.ctx.handle, self.handle, C.c_void_p(d_xyz_ptr), n, GRADIENT_UNIT if unit else 0,
                                                     C.c_void_p(d_out_ptr) if d_out_ptr else None, C.c_void_p(d_grad_ptr)))

    def query_hessian(self, pts, unit=False, curvature=False):
        """QueryHessian (include/hpsdf.h): Query's values, QueryGradient's gradients and the second derivative of the polynomial they come
        from -> (values f64 [n], grad f64 [n,3], hess f64 [n,6]: xx, yy, zz, xy, xz, yz), and with curvature curv f64 [n,2]: the level
        set's (mean, gauss).  unit: the gradient rows normalised.  Outside the root: DBL_MAX, NaN rows."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = len(pts)
        out, grad, hess = np.empty(n), np.empty((n, 3)), np.empty((n, 6))
        curv = np.empty((n, 2)) if curvature else None
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(lib().hpsdf_query_hessian_host(self.ctx.handle, self.handle, vp(pts), n, GRADIENT_UNIT if unit else 0, vp(out), vp(grad),
                                             vp(hess), vp(curv)))
        return (out, grad, hess, curv) if curvature else (out, grad, hess)

    def query_curvature(self, pts):
        """The level set's (mean, gauss) curvature at the points alone (hpsdf_query_hessian_host with only curv) -> f64 [n,2]."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        curv = np.empty((len(pts), 2))
        check(lib().hpsdf_query_hessian_host(self.ctx.handle, self.handle, pts.ctypes.data_as(C.c_void_p), len(pts), 0, None, None, None,
                                             curv.ctypes.data_as(C.c_void_p)))
        return curv

    def query_hessian_device(self, d_xyz_ptr, n, d_out_ptr=0, d_grad_ptr=0, d_hess_ptr=0, d_curv_ptr=0, unit=False):
        """Raw device pointers (ints; 0 = NULL for any output, but not for d_hess_ptr and d_curv_ptr both); asynchronous on the context
        stream."""
        vp = lambda p: C.c_void_p(p) if p else None
        check(lib().hpsdf_query_hessian_device(self.ctx.handle, self.handle, vp(d_xyz_ptr), n, GRADIENT_UNIT if unit else 0, vp(d_out_ptr),
                                               vp(d_grad_ptr), vp(d_hess_ptr), vp(d_curv_ptr)))

    def project(self, pts, iso=0.0, tol=1e-9, max_iter=16, unit=False):
        """ProjectToSurface (include/hpsdf.h): Newton's iteration along the gradient onto {Query = iso}, per point until |f - iso| <= tol
        -> (points f64 [n,3], values f64 [n], grad f64 [n,3], iters u8 [n], status u8 [n]); (values, grad) is query_gradient(points, unit)
        bit for bit.  status: PROJECT_CONVERGED, PROJECT_ITER_LIMIT (max_iter steps taken: the iteration can hop between two cells for
        ever near creases), PROJECT_LEFT_ROOT (DBL_MAX, NaN row), PROJECT_FLAT (zero gradient)."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = len(pts)
        out, val, grad = np.empty((n, 3)), np.empty(n), np.empty((n, 3))
        iters, status = np.empty(n, np.uint8), np.empty(n, np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().hpsdf_project_host(self.ctx.handle, self.handle, vp(pts), n, float(iso), float(tol), _max_iter(max_iter),
                                       PROJECT_UNIT if unit else 0, vp(out), vp(val), vp(grad), vp(iters), vp(status)))
        return out, val, grad, iters, status

    def project_device(self, d_xyz_ptr, n, d_out_xyz_ptr, d_out_val_ptr=0, d_out_grad_ptr=0, d_out_iters_ptr=0, d_out_status_ptr=0, iso=0.0,
                       tol=1e-9, max_iter=16, unit=False):
        """Raw device pointers (ints; 0 = NULL for every output but d_out_xyz_ptr, which may equal d_xyz_ptr); asynchronous on the
        context stream."""
        vp = lambda p: C.c_void_p(p) if p else None
        check(lib().hpsdf_project_device(self.ctx.handle, self.handle, vp(d_xyz_ptr), n, float(iso), float(tol), _max_iter(max_iter),
                                         PROJECT_UNIT if unit else 0, vp(d_out_xyz_ptr), vp(d_out_val_ptr), vp(d_out_grad_ptr),
                                         vp(d_out_iters_ptr), vp(d_out_status_ptr)))

    def project_vertices(self, verts, h, iso=0.0, tol=1e-9, max_iter=16):
        """hpsdf_surface_project_vertices: the vertices of an extracted mesh moved onto the level set, each only if its projection
        converged and stays within half a cube (h[a] / 2 per axis) of it -> (verts f64 [V,3] (a copy), n_moved)."""
        v = np.array(verts, np.float64).reshape(-1, 3)
        h3 = (C.c_double * 3)(*[float(x) for x in h])
        moved = C.c_uint64()
        check(lib().hpsdf_surface_project_vertices(self.ctx.handle, self.handle, v.ctypes.data_as(C.c_void_p), len(v), h3, float(iso),
                                                   float(tol), _max_iter(max_iter), C.byref(moved)))
        return v, int(moved.value)

    def cast_rays(self, origins, directions, t_max, iso=0.0, tol=1e-9, max_iter=32, max_cells=4096, unit=False):
        """CastRays (include/hpsdf.h): the first crossing of each ray o + t d (t in [0, t_max], d as given) with {Query = iso}: the
        ray is walked leaf by leaf and the first sign change refined until |f - iso| <= tol -> (status u8 [n], t f64 [n], points f64
        [n,3], values f64 [n], grad f64 [n,3], evals u16 [n], cells u16 [n]); (values, grad) is query_gradient(points, unit) bit for
        bit.  status: CAST_HIT, CAST_MISS, CAST_UNCONVERGED (a sign change that sits on a jump across a cell face, or max_iter too
        small: the row is the first sample behind it), CAST_CELL_LIMIT, CAST_INVALID; t and the row are NaN for MISS, CELL_LIMIT
        and INVALID."""
        o, d, tm, n = _ray_arrays(origins, directions, t_max)
        bufs = _cast_outputs(n)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().hpsdf_cast_rays_host(self.ctx.handle, self.handle, vp(o), vp(d), vp(tm), n, float(iso), float(tol), _max_iter(max_iter),
                                         _max_iter(max_cells), CAST_UNIT if unit else 0, *[vp(b) for b in bufs]))
        return bufs

    def cast_rays_device(self, d_origins_ptr, d_dirs_ptr, d_t_max_ptr, n, d_out_status_ptr, d_out_t_ptr=0, d_out_xyz_ptr=0, d_out_val_ptr=0,
                         d_out_grad_ptr=0, d_out_evals_ptr=0, d_out_cells_ptr=0, iso=0.0, tol=1e-9, max_iter=32, max_cells=4096, unit=False):
        """Raw device pointers (ints; 0 = NULL for every output but d_out_status_ptr); asynchronous on the context stream."""
        vp = lambda p: C.c_void_p(p) if p else None
        check(lib().hpsdf_cast_rays_device(self.ctx.handle, self.handle, vp(d_origins_ptr), vp(d_dirs_ptr), vp(d_t_max_ptr), n, float(iso),
                                           float(tol), _max_iter(max_iter), _max_iter(max_cells), CAST_UNIT if unit else 0,
                                           vp(d_out_status_ptr), vp(d_out_t_ptr), vp(d_out_xyz_ptr), vp(d_out_val_ptr), vp(d_out_grad_ptr),
                                           vp(d_out_evals_ptr), vp(d_out_cells_ptr)))

    def query_bounds(self, boxes, subdiv=1, max_leaves=4096):
        """QueryBounds (include/hpsdf.h): for each box (a row of six doubles: lower corner, upper corner, world coordinates) an interval
        that holds Query(x) for every point x of the box -> (lo f64 [n], hi f64 [n], status u8 [n], leaves u32 [n]).  status:
        BOUNDS_OK; BOUNDS_LEAF_LIMIT (more than max_leaves leaves: [-inf, inf]); BOUNDS_INVALID (a corner outside the root, a NaN,
        a > b: NaNs); BOUNDS_NOT_FINITE (a leaf with a non-finite coefficient: [-inf, inf]).  subdiv 2 or 4 splits a leaf's part of
        the box that many times per axis: tighter, at 8 or 64 evaluations a leaf."""
        b = _box_array(boxes)
        bufs = _bounds_outputs(len(b))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().hpsdf_query_bounds_host(self.ctx.handle, self.handle, vp(b), len(b), _max_iter(subdiv), _max_iter(max_leaves),
                                            *[vp(x) for x in bufs]))
        return bufs

    def query_bounds_device(self, d_boxes_ptr, n, d_out_lo_ptr, d_out_hi_ptr, d_out_status_ptr, d_out_leaves_ptr=0, subdiv=1, max_leaves=4096):
        """Raw device pointers (ints; 0 = NULL for d_out_leaves_ptr only); asynchronous on the context stream."""
        vp = lambda p: C.c_void_p(p) if p else None
        check(lib().hpsdf_query_bounds_device(self.ctx.handle, self.handle, vp(d_boxes_ptr), n, _max_iter(subdiv), _max_iter(max_leaves),
                                              vp(d_out_lo_ptr), vp(d_out_hi_ptr), vp(d_out_status_ptr), vp(d_out_leaves_ptr)))

    def query_bounds_grid(self, lo, hi, n, subdiv=1, max_leaves=4096):
        """query_bounds over the cells of the lattice of n[a] cells per axis on [lo, hi] (extract_surface's lattice; no box array is
        made) -> (lo, hi, status, leaves) shaped [n2, n1, n0]."""
        lo3, hi3, n3 = _lattice_args(lo, hi, n)
        shape = (int(n[2]), int(n[1]), int(n[0]))
        bufs = _bounds_outputs(shape)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().hpsdf_query_bounds_grid_host(self.ctx.handle, self.handle, lo3, hi3, n3, _max_iter(subdiv), _max_iter(max_leaves),
                                                 *[vp(x) for x in bufs]))
        return bufs

    def query_bounds_grid_device(self, lo, hi, n, d_out_lo_ptr, d_out_hi_ptr, d_out_status_ptr, d_out_leaves_ptr=0, subdiv=1, max_leaves=4096):
        """Raw device pointers for the n0 n1 n2 rows (x fastest); asynchronous on the context stream."""
        lo3, hi3, n3 = _lattice_args(lo, hi, n)
        vp = lambda p: C.c_void_p(p) if p else None
        check(lib().hpsdf_query_bounds_grid_device(self.ctx.handle, self.handle, lo3, hi3, n3, _max_iter(subdiv), _max_iter(max_leaves),
                                                   vp(d_out_lo_ptr), vp(d_out_hi_ptr), vp(d_out_status_ptr), vp(d_out_leaves_ptr)))

    def integrate(self, iso=0.0, depth=8, samples=2, max_cells=1 << 24, cells=False, host=False):
        """Integrate (include/hpsdf.h): a guaranteed enclosure of the volume of {Query < iso} over the root and an estimate of its zeroth,
        first and second moments, by refining the leaves into dyadic cells down to absolute depth `depth` where the leaves' bound cannot
        decide the sign -> Integral (the struct's fields, centroid, inertia, and with cells=True the final cells as a structured array
        of CELL_DTYPE).  host=True computes on the calling thread from the tree's host copies: the same bytes."""
        fn = lib().hpsdf_integrate_host if host else lib().hpsdf_integrate_device
        return _integrate(lambda *rest: fn(self.ctx.handle, self.handle, *rest), iso, depth, samples, max_cells, cells)

    def integrate_pair(self, other, op, pose=None, iso_a=0.0, iso_b=0.0, depth=8, samples=2, max_cells=1 << 24, max_leaves=256, cells=False,
                       host=False):
        """IntegratePair (include/hpsdf.h): Integrate over this tree (A) with every cell also classified against `other` (B) under
        pose (12 doubles [M | t], see pose(); None: the identity) -> PairIntegral for op = PAIR_INTERSECTION, PAIR_UNION or
        PAIR_DIFFERENCE of {Query_A < iso_a} and {x : Query_B(M x + t) < iso_b}, over A's root and in A's frame.  host=True: on the
        calling thread from the trees' host copies (the same bits)."""
        fn = lib().hpsdf_integrate_pair_host if host else lib().hpsdf_integrate_pair_device
        return _integrate_pair(lambda *rest: fn(self.ctx.handle, self.handle, other.handle, *rest), op, pose, iso_a, iso_b, depth, samples,
                               max_cells, max_leaves, cells)

    def clearance(self, other, pose=None, iso_a=0.0, depth=10, tol=0.0, max_cells=1 << 24, max_leaves=256, cells=False, host=False):
        """Clearance (include/hpsdf.h): lo <= min of other's field (B) over {Query_A < iso_a} of this tree (A) under pose <= hi, by
        branch and bound over A's cells -> Clearance with the witness point that attains hi.  host=True: on the calling thread from
        the trees' host copies (the same bits)."""
        fn = lib().hpsdf_clearance_host if host else lib().hpsdf_clearance_device
        return _clearance(lambda *rest: fn(self.ctx.handle, self.handle, other.handle, *rest), pose, iso_a, depth, tol, max_cells, max_leaves, cells)

    def clearance_batch(self, other, poses, iso_a=0.0, depth=10, tol=0.0, max_cells=1 << 24, max_leaves=256, decide=None, max_total_cells=1 << 24,
                        host=False):
        """clearance for n poses ([n, 12], or a sequence of pose(...)) in one device call (include/hpsdf.h, "Clearance", "Batches") ->
        ClearanceBatch; element i is clearance(other, poses[i], ...)'s struct, byte for byte.  decide: a pose stops with
        CLEARANCE_DECIDED once lo > decide or hi < decide is proven (None: off); max_total_cells: the cells of all poses' lists of one
        pass together.  host=True: a loop on the calling thread from the trees' host copies."""
        fn = lib().hpsdf_clearance_batch_host if host else lib().hpsdf_clearance_batch_device
        return _clearance_batch(lambda *rest: fn(self.ctx.handle, self.handle, other.handle, *rest), poses, iso_a, depth, tol, max_cells, max_leaves,
                                decide, max_total_cells)

    def query_ray(self, origins, directions, t_max, t_init=None):
        """Octree::QueryRay per row -> (hit u8 [n], t f64 [n]); t rows of misses keep t_init."""
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
        n = len(o)
        tm = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float64), (n,)))
        hit = np.zeros(n, np.uint8)
        t = np.zeros(n) if t_init is None else np.array(t_init, np.float64).reshape(n).copy()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().hpsdf_query_ray_host(self.ctx.handle, self.handle, vp(o), vp(d), vp(tm), n, vp(hit), vp(t)))
        return hit, t

    def function_slice(self, c, view_min, view_max, n_samples=2048):
        """Octree::OutputFunctionSlice up to the byte image -> (rgb u8 [n,n,3], values f64 [n,n])."""
        n = int(n_samples)
        rgb = np.zeros((n, n, 3), np.uint8)
        vals = np.zeros((n, n))
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
        check(lib().hpsdf_function_slice(self.ctx.handle, self.handle, float(c), f3(view_min), f3(view_max), n,
                                         rgb.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p)))
        return rgb, vals

    def extract_surface(self, lo, hi, n, iso=0.0, values=False):
        """Marching cubes over the lattice of n[a] cubes per axis on [lo, hi] (include/hpsdf.h, hpsdf_extract_surface) ->
        (verts f64 [V,3], tris u64 [T,3]), plus the lattice values f64 [n2+1, n1+1, n0+1] when values is true."""
        lo3, hi3, n3 = _lattice_args(lo, hi, n)
        vals = np.empty((int(n[2]) + 1, int(n[1]) + 1, int(n[0]) + 1)) if values else None
        verts, tris = _take_mesh(lambda *out: lib().hpsdf_extract_surface(
            self.ctx.handle, self.handle, lo3, hi3, n3, float(iso), *out, vals.ctypes.data_as(C.c_void_p) if values else None))
        return (verts, tris, vals) if values else (verts, tris)

    def extract_surface_sparse(self, lo, hi, n, iso=0.0, stats=False):
        """extract_surface's mesh, bit for bit, evaluated only in the blocks of 8^3 cubes the tree cannot rule out (include/hpsdf.h,
        hpsdf_extract_surface_sparse): up to 2^40 lattice points, device memory proportional to the surface -> (verts f64 [V,3],
        tris u64 [T,3]), plus the call's statistics as a dict when stats is true."""
        lo3, hi3, n3 = _lattice_args(lo, hi, n)
        st = SurfaceSparseStats()
        verts, tris = _take_mesh(lambda *out: lib().hpsdf_extract_surface_sparse(
            self.ctx.handle, self.handle, lo3, hi3, n3, float(iso), *out, C.byref(st)))
        if not stats:
            return verts, tris
        return verts, tris, {k: getattr(st, k) for k, _ in SurfaceSparseStats._fields_ if k != "reserved"}

    def extract_surface_dual(self, lo, hi, n, iso=0.0, tau=0.1, values=False, info=False):
        """Dual contouring over extract_surface's lattice (include/hpsdf.h, hpsdf_extract_surface_dual): one vertex a mixed cube, placed
        by the field's tangent planes at the crossing edges (tau: the relative eigenvalue cut of the fit), two triangles an interior
        crossing edge -> (verts f64 [V,3], tris u64 [T,3]), then the info bytes u8 [V] (rank in bits 0-1, DUAL_CLAMPED) when info is
        true, then the lattice values f64 [n2+1, n1+1, n0+1] when values is true."""
        return _dual_call(lambda *a: lib().hpsdf_extract_surface_dual(self.ctx.handle, self.handle, *a), lo, hi, n, iso, tau, values, info)

    def classify_surface_blocks(self, lo, hi, n, iso=0.0, first_block=0, count=None):
        """The classification kernel's class byte per block (0 evaluate, 1 all >= iso, 2 all < iso) for blocks [first_block,
        first_block + count), default all of them, x fastest -> u8 [count]."""
        lo3, hi3, n3 = _lattice_args(lo, hi, n)
        count = surface_block_count(n) - int(first_block) if count is None else int(count)
        out = np.zeros(max(count, 0), np.uint8)
        check(lib().hpsdf_surface_classify_device(self.ctx.handle, self.handle, lo3, hi3, n3, float(iso), int(first_block), count,
                                                  out.ctypes.data_as(C.c_void_p)))
        return out

    def query_device(self, d_xyz_ptr, n, d_out_ptr):
        """Raw device pointers (ints); asynchronous on the context stream."""
        check(lib().hpsdf_query_device(self.ctx.handle, self.handle, C.c_void_p(d_xyz_ptr), n, C.c_void_p(d_out_ptr)))

    def close(self):
        if self.handle:
            lib().hpsdf_tree_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Build:
    """Stepwise Create (one canonical round at a time); see include/hpsdf.h."""

    def __init__(self, config, K=0, rank=0, world=1):
        self.pod = config.to_pod() if isinstance(config, Config) else config
        self.opts = BuildOpts(K, rank, world)
        self.handle = C.c_void_p()
        self.rank, self.world = rank, world
        check(lib().hpsdf_build_begin(C.byref(self.pod), C.byref(self.opts), C.byref(self.handle)))

    def select(self):
        n = C.c_uint64()
        check(lib().hpsdf_build_round_select(self.handle, C.byref(n)))
        return n.value

    def jobs(self, n):
        arr = (Job * n)()
        check(lib().hpsdf_build_round_jobs(self.handle, arr))
        return arr

    def slice(self, rank=None):
        f, c = C.c_uint64(), C.c_uint64()
        check(lib().hpsdf_build_round_slice(self.handle, self.rank if rank is None else rank, C.byref(f), C.byref(c)))
        return f.value, c.value

    def max_slice(self):
        n = C.c_uint64()
        check(lib().hpsdf_build_round_max_slice(self.handle, C.byref(n)))
        return n.value

    def compute(self, ctx, field):
        check(lib().hpsdf_build_round_compute(self.handle, ctx.handle if ctx is not None else None, field.handle))

    def results_device(self):
        p, n = C.c_void_p(), C.c_uint64()
        check(lib().hpsdf_build_round_results_device(self.handle, C.byref(p), C.byref(n)))
        return p.value, n.value

    def results_host(self, ctx):
        _, cnt = self.slice()
        out = np.zeros(cnt * JOB_HEADER_DOUBLES)
        check(lib().hpsdf_build_round_results_host(self.handle, ctx.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def apply(self, headers):
        h = np.ascontiguousarray(headers, np.float64)
        check(lib().hpsdf_build_round_apply(self.handle, h.ctypes.data_as(C.c_void_p)))

    def inject(self, job, p_coeffs, h_coeffs):
        p = np.ascontiguousarray(p_coeffs, np.float64) if p_coeffs is not None else None
        h = np.ascontiguousarray(h_coeffs, np.float64) if h_coeffs is not None else None
        check(lib().hpsdf_build_round_inject(self.handle, job, p.ctypes.data_as(C.c_void_p) if p is not None else None,
                                             h.ctypes.data_as(C.c_void_p) if h is not None else None))

    def rows_counts(self):
        """Weighted builds on N ranks: doubles every rank hands over after the round just applied (hpsdf.h)."""
        counts = (C.c_uint64 * self.world)()
        check(lib().hpsdf_build_rows_counts(self.handle, counts))
        return list(counts)

    def rows_pack_host(self, ctx, count):
        out = np.zeros(max(1, count))
        check(lib().hpsdf_build_rows_pack_host(self.handle, ctx.handle if ctx is not None else None, out.ctypes.data_as(C.c_void_p)))
        return out[:count]

    def rows_unpack_host(self, ctx, parts):
        keep = [np.ascontiguousarray(p, np.float64) if len(p) else np.zeros(1) for p in parts]
        arr = (C.c_void_p * len(keep))(*[k.ctypes.data_as(C.c_void_p).value for k in keep])
        check(lib().hpsdf_build_rows_unpack_host(self.handle, ctx.handle if ctx is not None else None, arr))

    def node_rows(self, ctx, node_idx):
        """The coefficient rows node ``node_idx`` holds right now (its full array in a weighted build), if on this rank."""
        n = C.c_uint64()
        check(lib().hpsdf_build_node_rows_host(self.handle, ctx.handle if ctx is not None else None, node_idx, None, C.byref(n)))
        out = np.zeros(max(1, n.value))
        check(lib().hpsdf_build_node_rows_host(self.handle, ctx.handle if ctx is not None else None, node_idx,
                                               out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out[:n.value]

    def layout(self):
        tot = C.c_uint64()
        counts = (C.c_uint64 * self.world)()
        check(lib().hpsdf_build_layout(self.handle, C.byref(tot), counts))
        return tot.value, list(counts)

    def pack_host(self, ctx, count):
        out = np.zeros(max(1, count))
        check(lib().hpsdf_build_pack_host(self.handle, ctx.handle if ctx is not None else None,
                                          out.ctypes.data_as(C.c_void_p)))
        return out[:count]

    def pack_device(self, ctx):
        p, n = C.c_void_p(), C.c_uint64()
        check(lib().hpsdf_build_pack_device(self.handle, ctx.handle, C.byref(p), C.byref(n)))
        return p.value, n.value

    def assemble(self, packs):
        keep = [np.ascontiguousarray(p, np.float64) if len(p) else np.zeros(1) for p in packs]
        arr = (C.c_void_p * len(keep))(*[k.ctypes.data_as(C.c_void_p).value for k in keep])
        blk, sz = C.c_void_p(), C.c_size_t()
        check(lib().hpsdf_build_assemble(self.handle, arr, C.byref(blk), C.byref(sz)))
        data = C.string_at(blk, sz.value)
        lib()._libc.free(blk)
        return data

    def stats(self):
        st = BuildStats()
        check(lib().hpsdf_build_get_stats(self.handle, C.byref(st)))
        return st.as_dict()

    def close(self):
        if self.handle:
            lib().hpsdf_build_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def create_block(ctx, config, field, K=0):
    """Octree::Create on one GPU -> (serialised block bytes, stats dict)."""
    pod = config.to_pod() if isinstance(config, Config) else config
    blk, sz, st = C.c_void_p(), C.c_size_t(), BuildStats()
    rc = lib().hpsdf_create(ctx.handle if ctx is not None else None, C.byref(pod), field.handle, K, C.byref(blk), C.byref(sz), C.byref(st))
    if rc and ctx is not None:
        ctx._blocks.clear()  # (a failed build gave its blocks back; nothing of it is kept)
    check(rc)
    if ctx is None:  # (not reached: Create needs a device)
        data = C.string_at(blk, sz.value)
        lib()._libc.free(blk)
    else:
        data = ctx._take_block(blk, sz.value)
    return data, st.as_dict()


ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


def create_block_distributed(ctx, config, field, K, rank, world, gather):
    """hpsdf_create_distributed: this rank's part of a Create sharded over `world` GPUs, frontier on the device.
    gather(d_buf_ptr, bytes_per_rank, stream_ptr) -> None performs the in-place all-gather (rank r's part at
    d_buf_ptr + r * bytes_per_rank); exceptions it raises fail the build.  Returns (block bytes, stats)."""
    pod = config.to_pod() if hasattr(config, "to_pod") else config
    failure = []

    def _cb(_user, d_buf, nbytes, stream):
        try:
            gather(d_buf, nbytes, stream)
            return 0
        except BaseException as e:  # noqa: BLE001 -- must not propagate through the C frames
            failure.append(e)
            return 1

    cb = ALLGATHER(_cb)
    blk, size, st = C.c_void_p(), C.c_size_t(), BuildStats()
    rc = lib().hpsdf_create_distributed(ctx.handle, C.byref(pod), field.handle, K, rank, world, C.cast(cb, C.c_void_p), None,
                                        C.byref(blk), C.byref(size), C.byref(st))
    if failure or rc:
        ctx._blocks.clear()
    if failure:
        raise failure[0]
    check(rc)
    return ctx._take_block(blk, size.value), st.as_dict()


def continuity_post_process(block, tol=0.0, max_iter=0, threads=0, ctx=None):
    """Octree::PerformContinuityPostProcess (Octree.cpp:1717-1762) on a serialised block.  ctx=None: everything on
    the host; with a Context the conjugate-gradient loop runs on its device (bit-identical result).
    Returns (new block bytes, stats dict).  tol 0 = the reference's EPSILON_F32."""
    buf = C.create_string_buffer(bytes(block), len(block))
    st = ContinuityStats()
    if ctx is None:
        check(lib().hpsdf_continuity_post_process(buf, len(block), tol, max_iter, threads, C.byref(st)))
    else:
        check(lib().hpsdf_continuity_post_process_device(ctx.handle, buf, len(block), tol, max_iter, threads, C.byref(st)))
    return buf.raw, st.as_dict()


def continuity_matrix(block, threads=0):
    """(row_ptr, col, val, stats) of the jump-energy matrix M (no regularisation), CSR."""
    b = bytes(block)
    rp, ci, v = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_double)()
    st = ContinuityStats()
    check(lib().hpsdf_continuity_matrix(b, len(b), threads, C.byref(rp), C.byref(ci), C.byref(v), C.byref(st)))
    n = int(np.frombuffer(b[:8], np.uint64)[0])
    row_ptr = np.ctypeslib.as_array(rp, shape=(n + 1,)).copy()
    nnz = int(row_ptr[-1])
    col = np.ctypeslib.as_array(ci, shape=(max(nnz, 1),))[:nnz].copy()
    val = np.ctypeslib.as_array(v, shape=(max(nnz, 1),))[:nnz].copy()
    for p in (rp, ci, v):
        lib()._libc.free(C.cast(p, C.c_void_p))
    return row_ptr, col, val, st.as_dict()


def continuity_matrix_device(ctx, block):
    """The same matrix assembled on the device (what Create uses) and copied back: (row_ptr, col, val, stats)."""
    b = bytes(block)
    rp, ci, v = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_double)()
    st = ContinuityStats()
    check(lib().hpsdf_continuity_matrix_device(ctx.handle, b, len(b), C.byref(rp), C.byref(ci), C.byref(v), C.byref(st)))
    n = int(np.frombuffer(b[:8], np.uint64)[0])
    row_ptr = np.ctypeslib.as_array(rp, shape=(n + 1,)).copy()
    nnz = int(row_ptr[-1])
    col = np.ctypeslib.as_array(ci, shape=(max(nnz, 1),))[:nnz].copy()
    val = np.ctypeslib.as_array(v, shape=(max(nnz, 1),))[:nnz].copy()
    for p in (rp, ci, v):
        lib()._libc.free(C.cast(p, C.c_void_p))
    return row_ptr, col, val, st.as_dict()


def continuity_last_stats():
    st = ContinuityStats()
    check(lib().hpsdf_continuity_last_stats(C.byref(st)))
    return st.as_dict()


def selftest_acosf(ctx, first_bits, stride, n):
    """The device's acosf (the angle weights of vertex pseudo-normals) of the floats with bit patterns first_bits + i * stride."""
    out = np.empty(n, np.float32)
    check(lib().hpsdf_selftest_acosf(ctx.handle, first_bits, stride, n, out.ctypes.data_as(C.c_void_p)))
    return out


CHAIN_OPS, CHAIN_ROUND0 = 0, 1
CHAIN_ALL_WAVES, CHAIN_THIRTEEN_WAVES = 0, 1


def selftest_running_total(ctx, total0, ops=None, errs=None, batch_err=None, population=CHAIN_ALL_WAVES):
    """Create's running total on chosen operands, by the device code Create runs: total0 + x[0] + x[1] + ... in order, as a float64.
    x = ops, or -- errs and batch_err given -- errs[9 k] - batch_err[k], formed on the device as round 0 forms it."""
    out = np.empty(1, np.float64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    if ops is not None:
        ops = np.ascontiguousarray(ops, np.float64)
        check(lib().hpsdf_selftest_running_total(ctx.handle, total0, ops.size, CHAIN_OPS, population, ptr(ops), None, None, ptr(out)))
    else:
        errs, batch_err = np.ascontiguousarray(errs, np.float64), np.ascontiguousarray(batch_err, np.float64)
        if errs.size != 9 * batch_err.size:
            raise ValueError("errs holds nine doubles a job")
        check(lib().hpsdf_selftest_running_total(ctx.handle, total0, batch_err.size, CHAIN_ROUND0, population, None, ptr(errs), ptr(batch_err), ptr(out)))
    return out[0]


def bench_fit(ctx, config, field, degree, depth, n_cells, repeats=5):
    pod = config.to_pod()
    ms = C.c_double()
    check(lib().hpsdf_bench_fit(ctx.handle, C.byref(pod), field.handle, degree, depth, n_cells, repeats, C.byref(ms)))
    return ms.value


def fit_cells(ctx, config, field, degree, depth, n_cells):
    """From-scratch fits of `degree` for the first n_cells cells of the depth-`depth` lattice (x fastest) -> (coeffs[n, ncoef], errs[n])."""
    pod = config.to_pod()
    nc = int(NCOEF[degree])
    coeffs, errs = np.empty((n_cells, nc)), np.empty(n_cells)
    check(lib().hpsdf_fit_cells(ctx.handle, C.byref(pod), field.handle, degree, depth, n_cells, coeffs.ctypes.data_as(C.c_void_p),
                                errs.ctypes.data_as(C.c_void_p)))
    return coeffs, errs


class Octree:
    """SDF::Octree mirror: Create / Query / ToMemoryBlock / FromMemoryBlock / CSG rebuilds."""

    def __init__(self, device=0, stream=None, jobs_per_round=0):
        self._device, self._stream, self.K = device, stream, jobs_per_round
        self._ctx = None
        self._tree = None
        self.block = None
        self.config = None
        self.stats = None

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = Context(self._device, self._stream)
        return self._ctx

    def Create(self, config, F):
        """F: a Field, or a Python callable f(pt, threadIdx) like the reference's std::function."""
        field = F if isinstance(F, Field) else Field.callback(F)
        block, stats = create_block(self.ctx, config, field, self.K)
        self.Clear()
        self.block, self.stats, self.config = block, stats, config
        self._tree = DeviceTree(self.ctx, block)

    def _csg(self, op, F):
        if self._tree is None:
            raise HpsdfError(6, "CSG on an empty octree")
        inner = F if isinstance(F, Field) else Field.callback(F)
        field = Field.tree_csg(self._tree, op, inner)
        old = self._tree
        block, stats = create_block(self.ctx, self.config, field, self.K)
        field.close()
        old.close()
        self.block, self.stats = block, stats
        self._tree = DeviceTree(self.ctx, block)

    def UnionSDF(self, F):
        self._csg(OP_UNION, F)

    def SubtractSDF(self, F):
        self._csg(OP_SUBTRACT, F)

    def IntersectSDF(self, F):
        self._csg(OP_INTERSECT, F)

    def Clear(self):
        if self._tree is not None:
            self._tree.close()
        self._tree, self.block = None, None

    def FromMemoryBlock(self, block):
        if not block:
            raise HpsdfError(4, "empty MemoryBlock")
        if len(block) < 16 + C.sizeof(PodConfig):
            raise HpsdfError(4, "MemoryBlock too small")
        self.Clear()
        self.block = bytes(block)
        pod = PodConfig.from_buffer_copy(self.block[-C.sizeof(PodConfig):])
        self.config = Config.from_pod(pod)
        self._tree = DeviceTree(self.ctx, self.block)

    def ToMemoryBlock(self):
        return bytes(self.block) if self.block is not None else b""

    def Query(self, pts):
        """One point (3,) -> float, or (n,3) -> ndarray; DBL_MAX outside the root."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        a = np.asarray(pts, np.float64)
        out = self._tree.query(a)
        return float(out[0]) if a.ndim == 1 else out

    def QueryWithGradient(self, pts):
        """(n,3) -> (values, unit 'gradients' as the reference's central-difference shortcut computes them)."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        return self._tree.query_with_gradient(pts)

    def QueryGradient(self, pts, unit=False):
        """The field's true gradient (DeviceTree.query_gradient): one point (3,) -> (float, (3,)), or (n,3) -> (values, grad [n,3])."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        a = np.asarray(pts, np.float64)
        out, grad = self._tree.query_gradient(a, unit)
        return (float(out[0]), grad[0]) if a.ndim == 1 else (out, grad)

    def QueryHessian(self, pts, unit=False, curvature=False):
        """The field's second derivative (DeviceTree.query_hessian): one point (3,) -> (float, grad (3,), hess (6,): xx, yy, zz, xy, xz,
        yz), or (n,3) -> (values, grad [n,3], hess [n,6]); curvature appends the level set's (mean, gauss): (2,) or [n,2]."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        a = np.asarray(pts, np.float64)
        res = self._tree.query_hessian(a, unit, curvature)
        return (float(res[0][0]),) + tuple(r[0] for r in res[1:]) if a.ndim == 1 else res

    def QueryCurvature(self, points):
        """(mean, gauss) curvature of the level set through every point: one point (3,) -> two floats, or (n,3) -> two arrays [n].  With
        the field positive outside, a sphere of radius r gives (1/r, 1/r^2).  Leaves of degree <= 2 give a crude answer (zero or a
        constant Hessian): use a refined tree."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        a = np.asarray(points, np.float64)
        curv = self._tree.query_curvature(a)
        return (float(curv[0, 0]), float(curv[0, 1])) if a.ndim == 1 else (curv[:, 0].copy(), curv[:, 1].copy())

    def ProjectToSurface(self, pts, iso=0.0, tol=1e-9, max_iter=16, unit=False):
        """The points moved onto the level set {Query = iso} along the gradient (DeviceTree.project): one point (3,) -> (point (3,),
        value, grad (3,), iters, status) with scalars, or (n,3) -> the five arrays."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        a = np.asarray(pts, np.float64)
        out, val, grad, iters, status = self._tree.project(a, iso, tol, max_iter, unit)
        return (out[0], float(val[0]), grad[0], int(iters[0]), int(status[0])) if a.ndim == 1 else (out, val, grad, iters, status)

    def CastRays(self, origins, directions, t_max, iso=0.0, tol=1e-9, max_iter=32, max_cells=4096, unit=False):
        """Where each ray first crosses the level set {Query = iso} (DeviceTree.cast_rays): one ray (3,), (3,) -> (status, t, point
        (3,), value, grad (3,), evals, cells) with scalars, or (n,3) arrays -> the seven arrays.  Unlike QueryRay -- the reference's
        sphere tracing -- the direction is used as given, t is the ray parameter, and a hit lies within tol of the level set."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        o = np.asarray(origins, np.float64)
        st, t, pts, val, grad, evals, cells = self._tree.cast_rays(o, directions, t_max, iso, tol, max_iter, max_cells, unit)
        if o.ndim == 1:
            return int(st[0]), float(t[0]), pts[0], float(val[0]), grad[0], int(evals[0]), int(cells[0])
        return st, t, pts, val, grad, evals, cells

    def QueryBounds(self, boxes, subdiv=1, max_leaves=4096):
        """An interval that holds Query over each whole box (DeviceTree.query_bounds): one box (6,) = lower corner then upper corner
        -> (lo, hi, status, leaves) with scalars, or (n,6) -> the four arrays.  lo > 0 proves the box outside the surface, hi < 0
        inside it; no sampling density can."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        b = np.asarray(boxes, np.float64)
        lo, hi, st, leaves = self._tree.query_bounds(b, subdiv, max_leaves)
        return (float(lo[0]), float(hi[0]), int(st[0]), int(leaves[0])) if b.ndim == 1 else (lo, hi, st, leaves)

    def QueryBoundsGrid(self, view_min, view_max, n, subdiv=1, max_leaves=4096):
        """QueryBounds over the cells of the lattice of n cells per axis (an int or three) on [view_min, view_max]
        (DeviceTree.query_bounds_grid) -> (lo, hi, status, leaves), each shaped [n2, n1, n0]."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        n3 = (int(n),) * 3 if np.ndim(n) == 0 else tuple(int(x) for x in n)
        return self._tree.query_bounds_grid(view_min, view_max, n3, subdiv, max_leaves)

    def Integrate(self, iso=0.0, depth=8, samples=2, max_cells=1 << 24, cells=False):
        """Volume bounds and moments of the solid {Query < iso} (DeviceTree.integrate) -> Integral: volume_lo <= volume <= volume_hi
        guaranteed, volume / m1 / m2 estimated, centroid and inertia derived."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        return self._tree.integrate(iso, depth, samples, max_cells, cells)

    def IntegratePair(self, other, op, pose=None, iso_a=0.0, iso_b=0.0, depth=8, samples=2, max_cells=1 << 24, max_leaves=256, cells=False):
        """Volume bounds and moments of the intersection, union or difference (op: PAIR_*) of this solid with other's under a pose
        (DeviceTree.integrate_pair) -> PairIntegral, in this octree's frame; .disjoint / .overlapping are proofs for the intersection."""
        if self._tree is None or other._tree is None:
            raise HpsdfError(ERR_STATE, "IntegratePair on an empty octree")
        return self._tree.integrate_pair(other._tree, op, pose, iso_a, iso_b, depth, samples, max_cells, max_leaves, cells)

    def Clearance(self, other, pose=None, iso_a=0.0, depth=10, tol=0.0, max_cells=1 << 24, max_leaves=256, cells=False):
        """The guaranteed minimum of other's field over this solid under a pose (DeviceTree.clearance) -> Clearance: .lo <= it <= .hi,
        .point (this octree's frame) and .image (other's) where .hi is attained; .gap(iso_b) for two distance fields."""
        if self._tree is None or other._tree is None:
            raise HpsdfError(ERR_STATE, "Clearance on an empty octree")
        return self._tree.clearance(other._tree, pose, iso_a, depth, tol, max_cells, max_leaves, cells)

    def ClearanceBatch(self, other, poses, iso_a=0.0, depth=10, tol=0.0, max_cells=1 << 24, max_leaves=256, decide=None, max_total_cells=1 << 24):
        """Clearance for n poses in one device call (DeviceTree.clearance_batch) -> ClearanceBatch"""
        if self._tree is None or other._tree is None:
            raise HpsdfError(ERR_STATE, "ClearanceBatch on an empty octree")
        return self._tree.clearance_batch(other._tree, poses, iso_a, depth, tol, max_cells, max_leaves, decide, max_total_cells)

    def Simplify(self, rms, merge=True, truncate=True, stats=False):
        """A NEW Octree on the same context whose field is within `rms` of this one's in the root-normalised L2 sense, leaf cell by leaf
        cell (include/hpsdf.h, "Simplify"): sibling leaves merged into their parent, top degrees dropped, from the coefficients alone.
        This tree is not modified.  stats: (octree, stats dict)."""
        if self._tree is None:
            raise HpsdfError(6, "Simplify on an empty octree")
        block, st = simplify(self.ctx, self.block, rms, merge, truncate)
        o = Octree(self._device, self._stream, self.K)
        o._ctx = self._ctx
        o.FromMemoryBlock(block)
        return (o, st) if stats else o

    def QueryRay(self, origins, directions, t_max):
        """Octree::QueryRay (Octree.h:75) for one ray -> (hit, t) or (n,3) arrays -> (hit[n], t[n])."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        o = np.asarray(origins, np.float64)
        hit, t = self._tree.query_ray(o, directions, t_max)
        return (bool(hit[0]), float(t[0])) if o.ndim == 1 else (hit, t)

    def OutputFunctionSlice(self, fname, c, view_min, view_max, n_samples=2048):
        """Octree::OutputFunctionSlice (Octree.h:83-86): writes <fname>.bmp (24-bit, bottom-up rows as
        stb_image_write lays them out) and returns the (n,n,3) RGB array."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        rgb, _ = self._tree.function_slice(c, view_min, view_max, n_samples)
        write_bmp(fname + ".bmp", rgb)
        return rgb

    def ExtractSurface(self, view_min, view_max, n, iso=0.0, sparse=False, normals=False, project=False, tol=1e-9, max_iter=16,
                       curvature=False, dual=False, tau=0.1):
        """Triangle mesh of the level set {Query = iso} over the box [view_min, view_max] with n cubes per axis (an int or three)
        -> (verts f64 [V,3], tris u64 [T,3]); DeviceTree.extract_surface states the lattice.  sparse: the same arrays through
        DeviceTree.extract_surface_sparse (lattices up to 2^40 points).  project: the vertices -- linear interpolants along lattice
        edges -- are moved onto the polynomial's level set (DeviceTree.project_vertices with tol and max_iter: a vertex moves only if
        its projection converged within half a cube of it); tris is unchanged.  normals: (verts, tris, normals f64 [V,3]) with
        normals = query_gradient(verts, unit=True)[1], the field's unit gradient at every vertex (the projected ones under project).
        curvature: a last array f64 [V,2] is appended, query_curvature(verts): the level set's (mean, gauss) at the final vertices;
        verts and tris are the same bytes with and without it.  dual: dual contouring instead of marching cubes
        (DeviceTree.extract_surface_dual with tau): one vertex a cube, creases and corners kept; normals and curvature apply to its
        vertices as to any; with sparse or project it raises ValueError."""
        if self._tree is None:
            raise HpsdfError(6, "Query on an empty octree")
        if dual and (sparse or project):
            raise ValueError("dual=True does not combine with sparse or project")
        n3 = (int(n),) * 3 if np.ndim(n) == 0 else tuple(int(x) for x in n)
        if curvature:
            res = self.ExtractSurface(view_min, view_max, n3, iso, sparse, normals, project, tol, max_iter, False, dual, tau)
            return res + (self._tree.query_curvature(res[0]),)
        if normals:
            verts, tris = self.ExtractSurface(view_min, view_max, n3, iso, sparse, False, project, tol, max_iter, False, dual, tau)
            return verts, tris, self._tree.query_gradient(verts, unit=True)[1]
        if dual:
            return self._tree.extract_surface_dual(view_min, view_max, n3, iso, tau)
        if sparse:
            verts, tris = self._tree.extract_surface_sparse(view_min, view_max, n3, iso)
        else:
            verts, tris = self._tree.extract_surface(view_min, view_max, n3, iso)
        if project:
            verts = self._tree.project_vertices(verts, surface_cube_size(view_min, view_max, n3), iso, tol, max_iter)[0]
        return verts, tris

    def GetRootAABB(self):
        return self.config.root_min, self.config.root_max

    def copy(self):
        o = Octree(self._device, self._stream, self.K)
        if self.block is not None:
            o.FromMemoryBlock(self.block)
            o.stats = self.stats
        return o


def write_bmp(path, rgb):
    """24-bit uncompressed BMP of an (h, w, 3) RGB array: 14-byte file header, 40-byte BITMAPINFOHEADER, rows
    bottom-up, BGR, padded to 4 bytes -- the layout stbi_write_bmp produces for comp = 3."""
    import struct
    h, w, _ = rgb.shape
    pad = (-3 * w) % 4
    rows = np.zeros((h, 3 * w + pad), np.uint8)
    rows[:, :3 * w] = rgb[::-1, :, ::-1].reshape(h, 3 * w)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<2sIHHI", b"BM", 14 + 40 + rows.size, 0, 0, 14 + 40))
        fh.write(struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, 0, 0, 0, 0, 0))
        fh.write(rows.tobytes())


def surface_case_table():
    """hpsdf_surface_case_table: int8 [256, 16], row c = 3 cube-local edges per triangle of case c, then -1 (host only)."""
    out = np.zeros((256, 16), np.int8)
    check(lib().hpsdf_surface_case_table(out.ctypes.data_as(C.c_void_p)))
    return out


class SurfaceSparseStats(C.Structure):  # hpsdf_surface_sparse_stats, 96 bytes
    _fields_ = [("blocks", C.c_uint64), ("active_blocks", C.c_uint64), ("leaves_visited", C.c_uint64),
                ("classify_ms", C.c_double), ("count_ms", C.c_double), ("scan_ms", C.c_double), ("emit_ms", C.c_double),
                ("sort_ms", C.c_double), ("download_ms", C.c_double), ("total_ms", C.c_double),
                ("peak_scratch_bytes", C.c_uint64), ("reserved", C.c_uint64)]


SURFACE_BLOCK = 8  # HPSDF_SURFACE_BLOCK
DUAL_SWEEPS = 5  # HPSDF_DUAL_SWEEPS
DUAL_CLAMPED = 4  # HPSDF_DUAL_CLAMPED
GRADIENT_UNIT = 1  # HPSDF_GRADIENT_UNIT
PROJECT_UNIT = 1  # HPSDF_PROJECT_UNIT
PROJECT_CONVERGED, PROJECT_ITER_LIMIT, PROJECT_LEFT_ROOT, PROJECT_FLAT = 0, 1, 2, 3  # HPSDF_PROJECT_*: out_status


CAST_UNIT = 1  # HPSDF_CAST_UNIT
CAST_HIT, CAST_MISS, CAST_UNCONVERGED, CAST_CELL_LIMIT, CAST_INVALID = 0, 1, 2, 3, 4  # HPSDF_CAST_*: out_status


def _max_iter(max_iter):
    m = int(max_iter)
    if m < 0:
        raise ValueError("max_iter must be >= 0")
    return min(m, 0xFFFFFFFF)  # (the library rejects anything above 255)


def surface_cube_size(lo, hi, n):
    """The cube size h[a] = (hi[a] - lo[a]) / n[a] of hpsdf_extract_surface's lattice, as the library derives it (doubles)."""
    return tuple((float(hi[a]) - float(lo[a])) / float(int(n[a])) for a in range(3))


def project_block(block, pts, iso=0.0, tol=1e-9, max_iter=16, unit=False):
    """hpsdf_project_block: DeviceTree.project's arrays from a serialised block on the calling thread (no device; the process-wide
    reduction order) -> (points f64 [n,3], values f64 [n], grad f64 [n,3], iters u8 [n], status u8 [n])."""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    out, val, grad = np.empty((n, 3)), np.empty(n), np.empty((n, 3))
    iters, status = np.empty(n, np.uint8), np.empty(n, np.uint8)
    buf = bytes(block)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().hpsdf_project_block(buf, len(buf), vp(pts), n, float(iso), float(tol), _max_iter(max_iter), PROJECT_UNIT if unit else 0,
                                    vp(out), vp(val), vp(grad), vp(iters), vp(status)))
    return out, val, grad, iters, status


def _ray_arrays(origins, directions, t_max):
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
    if len(d) != len(o):
        raise ValueError("origins and directions must have the same number of rows")
    return o, d, np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float64), (len(o),))), len(o)


def _cast_outputs(n):
    return (np.empty(n, np.uint8), np.empty(n), np.empty((n, 3)), np.empty(n), np.empty((n, 3)), np.empty(n, np.uint16),
            np.empty(n, np.uint16))


def cast_rays_block(block, origins, directions, t_max, iso=0.0, tol=1e-9, max_iter=32, max_cells=4096, unit=False):
    """hpsdf_cast_rays_block: DeviceTree.cast_rays' arrays from a serialised block on the calling thread (no device; the process-wide
    reduction order) -> (status u8 [n], t f64 [n], points f64 [n,3], values f64 [n], grad f64 [n,3], evals u16 [n], cells u16 [n])."""
    o, d, tm, n = _ray_arrays(origins, directions, t_max)
    bufs = _cast_outputs(n)
    buf = bytes(block)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().hpsdf_cast_rays_block(buf, len(buf), vp(o), vp(d), vp(tm), n, float(iso), float(tol), _max_iter(max_iter),
                                      _max_iter(max_cells), CAST_UNIT if unit else 0, *[vp(b) for b in bufs]))
    return bufs


BOUNDS_OK, BOUNDS_LEAF_LIMIT, BOUNDS_INVALID, BOUNDS_NOT_FINITE = 0, 1, 2, 3  # HPSDF_BOUNDS_*: out_status


def _box_array(boxes):
    b = np.ascontiguousarray(boxes, np.float64)
    if b.size % 6:
        raise ValueError("a box is six doubles: the lower corner, then the upper corner")
    return b.reshape(-1, 6)


def _bounds_outputs(shape):
    return np.empty(shape), np.empty(shape), np.empty(shape, np.uint8), np.empty(shape, np.uint32)


def query_bounds_block(block, boxes, subdiv=1, max_leaves=4096):
    """hpsdf_query_bounds_block: DeviceTree.query_bounds' arrays from a serialised block on the calling thread (no device)
    -> (lo f64 [n], hi f64 [n], status u8 [n], leaves u32 [n])."""
    b = _box_array(boxes)
    bufs = _bounds_outputs(len(b))
    buf = bytes(block)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().hpsdf_query_bounds_block(buf, len(buf), vp(b), len(b), _max_iter(subdiv), _max_iter(max_leaves), *[vp(x) for x in bufs]))
    return bufs


def query_bounds_grid_block(block, lo, hi, n, subdiv=1, max_leaves=4096):
    """hpsdf_query_bounds_grid_block: DeviceTree.query_bounds_grid's arrays [n2, n1, n0] from a serialised block (no device)."""
    lo3, hi3, n3 = _lattice_args(lo, hi, n)
    bufs = _bounds_outputs((int(n[2]), int(n[1]), int(n[0])))
    buf = bytes(block)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().hpsdf_query_bounds_grid_block(buf, len(buf), lo3, hi3, n3, _max_iter(subdiv), _max_iter(max_leaves), *[vp(x) for x in bufs]))
    return bufs


INTEGRATE_OK, INTEGRATE_CELL_LIMIT, INTEGRATE_NOT_FINITE = 0, 1, 2  # HPSDF_INTEGRATE_*: Integral.status
CELL_DTYPE = np.dtype([("node", "<u4"), ("depth", "u1"), ("cls", "u1"), ("i", "<u2"), ("j", "<u2"), ("k", "<u2")])  # hpsdf_integrate_cell


class hpsdf_integral(C.Structure):
    _fields_ = [("unit_volume_lo", C.c_double), ("unit_volume_hi", C.c_double), ("unit_volume", C.c_double),
                ("volume_lo", C.c_double), ("volume_hi", C.c_double), ("volume", C.c_double),
                ("m1", C.c_double * 3), ("m2", C.c_double * 6), ("unit_m1", C.c_double * 3), ("unit_m2", C.c_double * 6),
                ("cells_inside", C.c_uint64), ("cells_outside", C.c_uint64), ("cells_undecided", C.c_uint64), ("evaluations", C.c_uint64),
                ("status", C.c_uint32), ("levels", C.c_uint32)]


class Integral:
    """hpsdf_integral's fields (arrays as numpy), `raw` (the struct's bytes), `cells` (a CELL_DTYPE array, or None when not asked for),
    and derived: centroid = m1 / volume; inertia: the 3 x 3 inertia tensor about the centroid at unit density,
    trace(C) I - C with C_jk = m2_jk - volume centroid_j centroid_k."""

    def __init__(self, st, cells):
        self.raw = bytes(st)
        for name, _ in st._fields_:
            v = getattr(st, name)
            setattr(self, name, np.array(v[:]) if hasattr(v, "__len__") else v)
        self.cells = cells
        with np.errstate(divide="ignore", invalid="ignore"):
            self.centroid = self.m1 / self.volume
            xx, yy, zz, xy, xz, yz = self.m2
            second = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]) - self.volume * np.outer(self.centroid, self.centroid)
            self.inertia = np.trace(second) * np.eye(3) - second

    def __repr__(self):
        return "Integral(status=%d, levels=%d, volume in [%r, %r], estimate %r)" % (self.status, self.levels, self.volume_lo, self.volume_hi, self.volume)


def _integrate(call, iso, depth, samples, max_cells, cells):
    """call(iso, depth, samples, max_cells, out, out_cells, out_n_cells) -> Integral; the malloc'd cell array copied and freed."""
    st = hpsdf_integral()
    ptr, count = C.c_void_p(), C.c_uint64()
    check(call(float(iso), _max_iter(depth), _max_iter(samples), _max_iter(max_cells), C.byref(st),
               C.byref(ptr) if cells else None, C.byref(count) if cells else None))
    arr = None
    if cells:
        arr = np.zeros(count.value, CELL_DTYPE)
        if count.value:
            C.memmove(arr.ctypes.data, ptr, count.value * CELL_DTYPE.itemsize)
        lib()._libc.free(ptr)
    return Integral(st, arr)


def integrate_block(block, iso=0.0, depth=8, samples=2, max_cells=1 << 24, cells=False):
    """hpsdf_integrate_block: DeviceTree.integrate's result from a serialised block on the calling thread (no device)."""
    buf = bytes(block)
    return _integrate(lambda *rest: lib().hpsdf_integrate_block(buf, len(buf), *rest), iso, depth, samples, max_cells, cells)


PAIR_INTERSECTION, PAIR_UNION, PAIR_DIFFERENCE = 0, 1, 2  # HPSDF_PAIR_*: the operation of IntegratePair


def pose(R=None, t=None):
    """The 12 doubles [M | t] of IntegratePair's pose, row-major, from a 3 x 3 matrix R (None: the identity) and a translation t (None:
    zero): a point x of A's frame is R x + t in B's.  pose(None) is the identity."""
    out = np.zeros((3, 4))
    out[:, :3] = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    if t is not None:
        out[:, 3] = np.asarray(t, np.float64).reshape(3)
    return np.ascontiguousarray(out.reshape(12))


class PairIntegral(Integral):
    """Integral of an IntegratePair call, with the two proofs the enclosure gives for the intersection: disjoint (volume_hi == 0: no
    point of A's root is in both solids) and overlapping (volume_lo > 0: the solids interfere)."""

    @property
    def disjoint(self):
        return self.status != INTEGRATE_NOT_FINITE and self.unit_volume_hi == 0.0

    @property
    def overlapping(self):
        return self.status != INTEGRATE_NOT_FINITE and self.unit_volume_lo > 0.0


def _integrate_pair(call, op, pose_, iso_a, iso_b, depth, samples, max_cells, max_leaves, cells):
    """call(op, pose, iso_a, iso_b, depth, samples, max_cells, max_leaves, out, out_cells, out_n_cells) -> PairIntegral"""
    P = pose() if pose_ is None else np.ascontiguousarray(np.asarray(pose_, np.float64).reshape(12))
    r = _integrate(lambda iso, *rest: call(_max_iter(op), P.ctypes.data_as(C.c_void_p), iso, float(iso_b), *rest[:3], _max_iter(max_leaves), *rest[3:]),
                   iso_a, depth, samples, max_cells, cells)
    r.__class__ = PairIntegral
    return r


def integrate_pair_block(block_a, block_b, op, pose=None, iso_a=0.0, iso_b=0.0, depth=8, samples=2, max_cells=1 << 24, max_leaves=256, cells=False):
    """hpsdf_integrate_pair_block: DeviceTree.integrate_pair's result from two serialised blocks on the calling thread (no device)."""
    a, b = bytes(block_a), bytes(block_b)
    return _integrate_pair(lambda *rest: lib().hpsdf_integrate_pair_block(a, len(a), b, len(b), *rest), op, pose, iso_a, iso_b, depth, samples,
                           max_cells, max_leaves, cells)


CLEARANCE_CONVERGED, CLEARANCE_DEPTH, CLEARANCE_CELL_LIMIT, CLEARANCE_EMPTY, CLEARANCE_NOT_FINITE = 0, 1, 2, 3, 4  # HPSDF_CLEARANCE_*


class hpsdf_clearance(C.Structure):
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("point", C.c_double * 3), ("image", C.c_double * 3), ("value_a", C.c_double),
                ("cells_visited", C.c_uint64), ("cells_outside_a", C.c_uint64), ("cells_pruned", C.c_uint64), ("cells_open", C.c_uint64),
                ("status", C.c_uint32), ("levels", C.c_uint32)]


class Clearance:
    """hpsdf_clearance's fields (arrays as numpy), `raw` (the struct's bytes) and `cells` (the final cells as a CELL_DTYPE array, or
    None when not asked for).  lo <= min of B's field over A's solid <= hi; hi is B's value at `image`, the image of `point`."""

    def __init__(self, st, cells):
        self.raw = bytes(st)
        for name, _ in st._fields_:
            v = getattr(st, name)
            setattr(self, name, np.array(v[:]) if hasattr(v, "__len__") else v)
        self.cells = cells

    def gap(self, iso_b=0.0):
        """(lo - iso_b, hi - iso_b): for a distance field B the enclosure of the signed clearance of solid A from solid B -- both
        positive: provably that far apart inside B's root; both negative: A reaches that deep into B."""
        return self.lo - iso_b, self.hi - iso_b

    def __repr__(self):
        return "Clearance(status=%d, levels=%d, min in [%r, %r], open cells %d)" % (self.status, self.levels, self.lo, self.hi, self.cells_open)


def _clearance(call, pose_, iso_a, depth, tol, max_cells, max_leaves, cells):
    """call(pose, iso_a, depth, tol, max_cells, max_leaves, out, out_cells, out_n_cells) -> Clearance; the malloc'd cell array copied and freed."""
    P = pose() if pose_ is None else np.ascontiguousarray(np.asarray(pose_, np.float64).reshape(12))
    st = hpsdf_clearance()
    ptr, count = C.c_void_p(), C.c_uint64()
    check(call(P.ctypes.data_as(C.c_void_p), float(iso_a), _max_iter(depth), float(tol), _max_iter(max_cells), _max_iter(max_leaves), C.byref(st),
               C.byref(ptr) if cells else None, C.byref(count) if cells else None))
    arr = None
    if cells:
        arr = np.zeros(count.value, CELL_DTYPE)
        if count.value:
            C.memmove(arr.ctypes.data, ptr, count.value * CELL_DTYPE.itemsize)
        lib()._libc.free(ptr)
    return Clearance(st, arr)


def clearance_block(block_a, block_b, pose=None, iso_a=0.0, depth=10, tol=0.0, max_cells=1 << 24, max_leaves=256, cells=False):
    """hpsdf_clearance_block: DeviceTree.clearance's result from two serialised blocks on the calling thread (no device)."""
    a, b = bytes(block_a), bytes(block_b)
    return _clearance(lambda *rest: lib().hpsdf_clearance_block(a, len(a), b, len(b), *rest), pose, iso_a, depth, tol, max_cells, max_leaves, cells)


CLEARANCE_DECIDED = 5  # HPSDF_CLEARANCE_DECIDED: the batch entries' `decide` only
CLEARANCE_DTYPE = np.dtype([("lo", "<f8"), ("hi", "<f8"), ("point", "<f8", (3,)), ("image", "<f8", (3,)), ("value_a", "<f8"),
                            ("cells_visited", "<u8"), ("cells_outside_a", "<u8"), ("cells_pruned", "<u8"), ("cells_open", "<u8"),
                            ("status", "<u4"), ("levels", "<u4")])
assert CLEARANCE_DTYPE.itemsize == C.sizeof(hpsdf_clearance) == 112


class ClearanceBatch:
    """n hpsdf_clearance structs of one batch call: `array` (a CLEARANCE_DTYPE array; every field is also an attribute, an array over
    the poses), `raw` (the n x 112 bytes); len() and [i] -> the Clearance of pose i (no cells: batches return none)."""

    def __init__(self, array):
        self.array = array
        self.raw = array.tobytes()
        for name in CLEARANCE_DTYPE.names:
            setattr(self, name, array[name])

    def __len__(self):
        return len(self.array)

    def __getitem__(self, i):
        return Clearance(hpsdf_clearance.from_buffer_copy(self.array[i].tobytes()), None)

    def gap(self, iso_b=0.0):
        """(lo - iso_b, hi - iso_b) for every pose: Clearance.gap, as two arrays"""
        return self.lo - iso_b, self.hi - iso_b

    def __repr__(self):
        return "ClearanceBatch(%d poses, statuses %s)" % (len(self), sorted(set(self.status.tolist())))


def _clearance_batch(call, poses, iso_a, depth, tol, max_cells, max_leaves, decide, max_total_cells):
    """call(poses, n, iso_a, depth, tol, decide, max_cells, max_leaves, max_total_cells, out) -> ClearanceBatch; poses: [n, 12] or a
    sequence of pose(...)"""
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))
    out = np.zeros(len(P), CLEARANCE_DTYPE)
    check(call(P.ctypes.data_as(C.c_void_p), len(P), float(iso_a), _max_iter(depth), float(tol), float("nan") if decide is None else float(decide),
               _max_iter(max_cells), _max_iter(max_leaves), _max_iter(max_total_cells), out.ctypes.data_as(C.c_void_p)))
    return ClearanceBatch(out)


def clearance_batch_block(block_a, block_b, poses, iso_a=0.0, depth=10, tol=0.0, max_cells=1 << 24, max_leaves=256, decide=None,
                          max_total_cells=1 << 24):
    """hpsdf_clearance_batch_block: DeviceTree.clearance_batch's result from two serialised blocks on the calling thread (no device)."""
    a, b = bytes(block_a), bytes(block_b)
    return _clearance_batch(lambda *rest: lib().hpsdf_clearance_batch_block(a, len(a), b, len(b), *rest), poses, iso_a, depth, tol, max_cells,
                            max_leaves, decide, max_total_cells)


SIMPLIFY_MERGE, SIMPLIFY_TRUNCATE = 1, 2  # HPSDF_SIMPLIFY_*


class SimplifyStats(C.Structure):  # hpsdf_simplify_stats, 88 bytes
    _fields_ = [(n, C.c_uint64) for n in ("nodes_in", "coeffs_in", "leaves_in", "nodes_out", "coeffs_out", "leaves_out", "merges",
                                          "truncations", "levels")] + [("error_bound", C.c_double), ("max_cell_rms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _simplify_flags(merge, truncate):
    return (SIMPLIFY_MERGE if merge else 0) | (SIMPLIFY_TRUNCATE if truncate else 0)


def simplify_block(block, rms, merge=True, truncate=True, flags=None):
    """hpsdf_simplify_block: a coarser tree within `rms` of the block's, cell by cell (include/hpsdf.h, "Simplify"), on the calling
    thread with no device -> (block bytes, stats dict).  flags overrides merge / truncate with raw HPSDF_SIMPLIFY_* bits."""
    buf = bytes(block)
    blk, sz, st = C.c_void_p(), C.c_size_t(), SimplifyStats()
    check(lib().hpsdf_simplify_block(buf, len(buf), float(rms), _simplify_flags(merge, truncate) if flags is None else int(flags),
                                     C.byref(blk), C.byref(sz), C.byref(st)))
    data = C.string_at(blk, sz.value)
    lib()._libc.free(blk)
    return data, st.as_dict()


def simplify(ctx, block, rms, merge=True, truncate=True, flags=None):
    """hpsdf_simplify: simplify_block's bytes and stats, computed on ctx's device."""
    buf = bytes(block)
    blk, sz, st = C.c_void_p(), C.c_size_t(), SimplifyStats()
    rc = lib().hpsdf_simplify(ctx.handle, buf, len(buf), float(rms), _simplify_flags(merge, truncate) if flags is None else int(flags),
                              C.byref(blk), C.byref(sz), C.byref(st))
    if rc:
        ctx._blocks.clear()
    check(rc)
    return ctx._take_block(blk, sz.value), st.as_dict()


def simplify_transfer():
    """hpsdf_simplify_transfer: Simplify's transfer matrices -> f64 [2, 13, 13] (lower half, upper half of an axis)."""
    out = np.zeros((2, 13, 13))
    check(lib().hpsdf_simplify_transfer(out.ctypes.data_as(C.c_void_p)))
    return out


def cells_to_boxes(block_or_tree, cells):
    """The world boxes of Integrate's cells -> f64 [n, 6], QueryBounds' row format (lower corner, upper corner): per axis
    rootCentre + p * size with p = -0.5 + i * 2^-depth and -0.5 + (i + 1) * 2^-depth (exact), size = 1 / rootInvSizes.
    block_or_tree: a serialised block, or a DeviceTree or an Octree (the block it keeps)."""
    raw = bytes(block_or_tree) if isinstance(block_or_tree, (bytes, bytearray, memoryview)) else bytes(block_or_tree.block)
    cfg = PodConfig.from_buffer_copy(raw[-C.sizeof(PodConfig):])
    rmin, rmax = np.array(cfg.root_min[:], np.float32), np.array(cfg.root_max[:], np.float32)
    centre = ((rmin + rmax) / np.float32(2.0)).astype(np.float64)
    size = 1.0 / (np.float32(1.0) / (rmax - rmin)).astype(np.float64)
    s = 1.0 / (1 << cells["depth"].astype(np.int64)).astype(np.float64)
    ijk = np.stack([cells["i"], cells["j"], cells["k"]], 1).astype(np.float64)
    lo = -0.5 + ijk * s[:, None]
    hi = lo + s[:, None]
    return np.ascontiguousarray(np.concatenate([centre + lo * size, centre + hi * size], 1))


def query_hessian_block(block, pts, unit=False, curvature=False):
    """hpsdf_query_hessian_block: DeviceTree.query_hessian's arrays from a serialised block on the calling thread (no device; the
    process-wide reduction order) -> (values f64 [n], grad f64 [n,3], hess f64 [n,6]) and, with curvature, curv f64 [n,2]."""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    out, grad, hess = np.empty(n), np.empty((n, 3)), np.empty((n, 6))
    curv = np.empty((n, 2)) if curvature else None
    buf = bytes(block)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    check(lib().hpsdf_query_hessian_block(buf, len(buf), vp(pts), n, GRADIENT_UNIT if unit else 0, vp(out), vp(grad), vp(hess), vp(curv)))
    return (out, grad, hess, curv) if curvature else (out, grad, hess)


def query_gradient_block(block, pts, unit=False):
    """hpsdf_query_true_gradient_block: DeviceTree.query_gradient's arrays from a serialised block on the calling thread (no device;
    the process-wide reduction order) -> (values f64 [n], grad f64 [n,3])."""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    out, grad = np.empty(len(pts)), np.empty((len(pts), 3))
    buf = bytes(block)
    check(lib().hpsdf_query_true_gradient_block(buf, len(buf), pts.ctypes.data_as(C.c_void_p), len(pts), GRADIENT_UNIT if unit else 0,
                                                out.ctypes.data_as(C.c_void_p), grad.ctypes.data_as(C.c_void_p)))
    return out, grad


def _lattice_args(lo, hi, n):
    return ((C.c_double * 3)(*[float(x) for x in lo]), (C.c_double * 3)(*[float(x) for x in hi]), (C.c_uint32 * 3)(*[int(x) for x in n]))


def _take_mesh(call):
    """call(verts, n_verts, tris, n_tris): an extraction's malloc'd result -> (verts f64 [V,3], tris u64 [T,3]), the C arrays freed."""
    v, t = C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)()
    nv, nt = C.c_uint64(), C.c_uint64()
    check(call(C.byref(v), C.byref(nv), C.byref(t), C.byref(nt)))
    verts, tris = np.zeros((0, 3)), np.zeros((0, 3), np.uint64)
    if nt.value:
        verts = np.ctypeslib.as_array(v, shape=(nv.value, 3)).copy()
        tris = np.ctypeslib.as_array(t, shape=(nt.value, 3)).copy()
    lib()._libc.free(C.cast(v, C.c_void_p))
    lib()._libc.free(C.cast(t, C.c_void_p))
    return verts, tris


def _dual_call(call, lo, hi, n, iso, tau, values, info):
    """call(lo, hi, n, iso, tau, flags, verts, n_verts, tris, n_tris, vert_info, values): a dual extraction's malloc'd result as arrays,
    the C arrays freed.  The vertices come back whenever there are any, with or without triangles."""
    lo3, hi3, n3 = _lattice_args(lo, hi, n)
    vals = np.empty((int(n[2]) + 1, int(n[1]) + 1, int(n[0]) + 1)) if values else None
    v, t, b = C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
    nv, nt = C.c_uint64(), C.c_uint64()
    check(call(lo3, hi3, n3, float(iso), float(tau), 0, C.byref(v), C.byref(nv), C.byref(t), C.byref(nt), C.byref(b) if info else None,
               vals.ctypes.data_as(C.c_void_p) if values else None))
    verts, tris, inf = np.zeros((0, 3)), np.zeros((0, 3), np.uint64), np.zeros(0, np.uint8)
    if nv.value:
        verts = np.ctypeslib.as_array(v, shape=(nv.value, 3)).copy()
        if info:
            inf = np.ctypeslib.as_array(b, shape=(nv.value,)).copy()
    if nt.value:
        tris = np.ctypeslib.as_array(t, shape=(nt.value, 3)).copy()
    for p in (v, t, b):
        lib()._libc.free(C.cast(p, C.c_void_p))
    return (verts, tris) + ((inf,) if info else ()) + ((vals,) if values else ())


def extract_surface_dual_block(block, lo, hi, n, iso=0.0, tau=0.1, values=False, info=False):
    """hpsdf_extract_surface_dual_block: DeviceTree.extract_surface_dual's arrays from a serialised block on the calling thread (no
    device; the process-wide reduction order)."""
    buf = bytes(block)
    return _dual_call(lambda *a: lib().hpsdf_extract_surface_dual_block(buf, len(buf), *a), lo, hi, n, iso, tau, values, info)


def surface_dual_last_timings():
    """Device milliseconds of the phases of this thread's last extract_surface_dual: lattice, ballots, scan, hermite, vertices, quads,
    d2h, total."""
    out = (C.c_double * 8)()
    check(lib().hpsdf_surface_dual_last_timings(out))
    return dict(zip(("lattice", "ballots", "scan", "hermite", "vertices", "quads", "d2h", "total"), list(out)))


def surface_block_count(n):
    """Blocks of the lattice of n[a] cubes per axis: the product of ceil(n[a] / 8)."""
    return int(np.prod([(int(x) + SURFACE_BLOCK - 1) // SURFACE_BLOCK for x in n], dtype=object))


def surface_classify_host(block, lo, hi, n, iso=0.0, first_block=0, count=None):
    """hpsdf_surface_classify_host: DeviceTree.classify_surface_blocks' bytes from a serialised block on the calling thread (no device)."""
    lo3, hi3, n3 = _lattice_args(lo, hi, n)
    count = surface_block_count(n) - int(first_block) if count is None else int(count)
    out = np.zeros(max(count, 0), np.uint8)
    buf = bytes(block)
    check(lib().hpsdf_surface_classify_host(buf, len(buf), lo3, hi3, n3, float(iso), int(first_block), count, out.ctypes.data_as(C.c_void_p)))
    return out


def surface_last_timings():
    """Device milliseconds of the phases of this thread's last extraction: lattice, count, scan, emit, d2h, total."""
    out = (C.c_double * 6)()
    check(lib().hpsdf_surface_last_timings(out))
    return dict(zip(("lattice", "count", "scan", "emit", "d2h", "total"), list(out)))


def save_obj(path, verts, tris, normals=None):
    """Writes `v` records (each vertex rounded to float32, printed with %.9g: hpsdf_obj_load reads back exactly
    verts.astype(float32)) and 1-based `f` records.  normals (one row a vertex): `vn` records (%.9g) behind the vertices and faces as
    `f a//a b//b c//c`, which hpsdf_obj_load reads as well."""
    v = np.asarray(verts, np.float64).reshape(-1, 3).astype(np.float32)
    t = np.asarray(tris, np.uint64).reshape(-1, 3)
    if normals is not None:
        vn = np.asarray(normals, np.float64).reshape(-1, 3)
        if len(vn) != len(v):
            raise ValueError("save_obj: one normal per vertex expected")
        with open(path, "w") as fh:
            fh.write("".join("v %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in v))
            fh.write("".join("vn %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in vn))
            fh.write("".join("f %d//%d %d//%d %d//%d\n" % (int(a) + 1, int(a) + 1, int(b) + 1, int(b) + 1, int(c) + 1, int(c) + 1) for a, b, c in t))
        return
    with open(path, "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in v))
        fh.write("".join("f %d %d %d\n" % (int(a) + 1, int(b) + 1, int(c) + 1) for a, b, c in t))


def load_obj(path):
    """Meshing::ObjParser::Load (Source/Meshing/ObjParser.cpp:11-164) through the native reader:
    (verts f32 [n,3], tris u64 [m,3]), zero-based."""
    v, t = C.POINTER(C.c_float)(), C.POINTER(C.c_uint64)()
    nv, nt = C.c_uint64(), C.c_uint64()
    check(lib().hpsdf_obj_load(os.fsencode(path), C.byref(v), C.byref(nv), C.byref(t), C.byref(nt)))
    verts = np.ctypeslib.as_array(v, shape=(nv.value, 3)).copy()
    tris = np.ctypeslib.as_array(t, shape=(nt.value, 3)).copy()
    lib()._libc.free(C.cast(v, C.c_void_p))
    lib()._libc.free(C.cast(t, C.c_void_p))
    return verts, tris
