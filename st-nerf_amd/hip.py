"""ctypes binding of the C ABI in ``include/stnerf.h`` (libstnerf_hip.so).

This is the only place Python touches the native library.  There is NO fallback: if the shared
library is missing, cannot be loaded, or a call returns an error code, a ``RuntimeError`` /
``ValueError`` is raised -- nothing in this package computes the hot path in PyTorch.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch  # imported first on purpose: the HIP runtime of the process must be torch's (same SONAME)

_PKG = os.path.dirname(os.path.abspath(__file__))
# STNERF_LIB (development): load a variant build (st-nerf_amd/build.py with STNERF_LIB_TAG) instead of the product library
LIB_PATH = os.environ.get("STNERF_LIB") or os.path.join(_PKG, "libstnerf_hip.so")

OK, EINVAL, ELAUNCH, EARCH = 0, -1, -2, -3
MAX_LAYERS = 16
NET_SPACE, NET_SPACE_TIME, NET_MOTION, NET_SPACE_DEEP, NET_SPACE_TIME_DEEP = 0, 1, 2, 3, 4

c_f32p = C.c_void_p  # device pointers travel as void*
c_i64 = C.c_int64


class LayerEdit(C.Structure):
    _fields_ = [("shift", C.c_float * 3), ("scale", C.c_float), ("has_shift", C.c_int32), ("has_scale", C.c_int32)]


class LayerRotation(C.Structure):
    """stnerf_layer_rotation (include/stnerf.h): m = R^T row-major, the centre, enabled."""
    _fields_ = [("m", C.c_float * 9), ("centre", C.c_float * 3), ("enabled", C.c_int32)]


class CompositeParams(C.Structure):
    _fields_ = [("border", C.c_float), ("near", C.c_float), ("fine", C.c_int32), ("cut_negative_t", C.c_int32),
                ("threshold", C.c_float * MAX_LAYERS), ("use_threshold", C.c_int32 * MAX_LAYERS),
                ("sigma_scale", C.c_float * MAX_LAYERS), ("rgb_activated", C.c_int32),
                ("evaluated", C.c_int32 * MAX_LAYERS)]


class Nets(C.Structure):
    _fields_ = [("bkgd", C.c_void_p), ("bkgd_fine", C.c_void_p), ("space", C.c_void_p * MAX_LAYERS),
                ("space_fine", C.c_void_p * MAX_LAYERS), ("motion", C.c_void_p * MAX_LAYERS)]


class StageLayer(C.Structure):
    _fields_ = [("space", C.c_void_p), ("motion", C.c_void_p), ("ray_list", C.c_void_p), ("ray_count", C.c_void_p),
                ("xyz", C.c_void_p), ("raw", C.c_void_p), ("times", C.c_void_p), ("use_time", C.c_int32),
                ("motion_flags", C.c_int32), ("rotation", C.POINTER(LayerRotation))]


class StageRows(C.Structure):
    """stnerf_stage_rows (include/stnerf.h): one stage layer's row list (device int32 words ray << 8 | k) and its count, or NULLs."""
    _fields_ = [("row_list", C.c_void_p), ("row_count", C.c_void_p)]


class RenderParams(C.Structure):
    _fields_ = [("l", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32), ("ray_stride", C.c_int32),
                ("retiming", C.c_int32), ("only_coarse", C.c_int32), ("use_deform_time", C.c_int32),
                ("use_space_time", C.c_int32), ("precision", C.c_int32), ("has_edits", C.c_int32),
                ("bkgd_use_deform_time", C.c_int32), ("bkgd_use_space_time", C.c_int32), ("deep_rgb", C.c_int32),
                ("shown", C.c_int32 * MAX_LAYERS), ("border", C.c_float), ("near", C.c_float), ("alpha", C.c_float),
                ("density_threshold", C.c_float), ("bkgd_density_threshold", C.c_float), ("seed", C.c_uint64),
                ("ray_index_base", C.c_int64), ("ray_index_stripe", C.c_int64), ("ray_index_period", C.c_int64),
                ("edits_coarse", LayerEdit * MAX_LAYERS),
                ("edits_fine", LayerEdit * MAX_LAYERS), ("pivot", C.c_float * 3)]


class BkgdCache(C.Structure):
    """stnerf_bkgd_cache (include/stnerf.h): layer 0's dense raw outputs of a launch piece and what to do with them."""
    _fields_ = [("raw_coarse", C.c_void_p), ("raw_fine", C.c_void_p), ("mode", C.c_int32)]


class LayerCache(C.Structure):
    """stnerf_layer_cache (include/stnerf.h): one performer's compact raw outputs (slot j = hit ray rays[j]), the list, its length
    (device) and capacity, and what to do with them."""
    _fields_ = [("raw_coarse", C.c_void_p), ("raw_fine", C.c_void_p), ("rays", C.c_void_p), ("count", C.c_void_p), ("capacity", C.c_int64),
                ("mode", C.c_int32)]


class Occupancy(C.Structure):
    """stnerf_occupancy (include/stnerf.h): one layer's bit table (device), its cell counts (Rx, Ry, Rz), lo and R / (hi - lo)."""
    _fields_ = [("bits", C.c_void_p), ("res", C.c_int32 * 3), ("lo", C.c_float * 3), ("inv_cell", C.c_float * 3)]


class RenderOptions(C.Structure):
    """stnerf_render_options (include/stnerf.h): every optional argument of the render call, in the order the named entries take them.
    ``RenderOptions()`` is "no feature": all zero, struct_size set."""
    _fields_ = [("struct_size", C.c_int32), ("cache", C.POINTER(BkgdCache)), ("rot", C.POINTER(LayerRotation)), ("scene_out", c_f32p),
                ("layer_alpha", C.POINTER(C.c_float)), ("occ", C.POINTER(Occupancy)), ("counts", C.c_void_p),
                ("samples", C.POINTER(C.c_int32)), ("sample_counts", C.c_void_p), ("tau", C.c_float),
                ("terminate", C.POINTER(C.c_int32)), ("visibility_counts", C.c_void_p), ("bkgd_grid", C.POINTER(Occupancy)),
                ("bkgd_counts", C.c_void_p), ("layers", C.POINTER(LayerCache)), ("mismatch", C.c_void_p), ("occluder", c_f32p),
                ("occluder_stops", C.c_int32), ("occluded_mixed", c_f32p), ("occluded_scene", c_f32p), ("occluder_share", c_f32p),
                ("bkgd_rays", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(struct_size=C.sizeof(RenderOptions), **fields)


class RenderOptionsDeep(C.Structure):
    """stnerf_render_options_deep (include/stnerf.h): ``RenderOptions`` followed by the deep fields; struct_size says which of the two
    a record is.  ``RenderOptionsDeep()`` is "no feature" too.  ``ref()`` is what the render entries take."""
    _fields_ = RenderOptions._fields_ + [("deep_w_min", C.c_float), ("deep_merge_dz", C.c_float), ("deep_offsets", C.c_void_p),
                                         ("deep_samples", c_f32p), ("deep_capacity", c_i64), ("deep_total", C.c_void_p),
                                         ("deep_workspace", C.c_void_p)]

    def __init__(self, **fields):
        super().__init__(struct_size=C.sizeof(RenderOptionsDeep), **fields)

    def ref(self):
        return C.cast(C.pointer(self), C.POINTER(RenderOptions))


class DensityGrid(C.Structure):
    """stnerf_density_grid (include/stnerf.h): one layer's vertex densities (device, (Rz+1, Ry+1, Rx+1) fp32), its cell counts
    (Rx, Ry, Rz), lo and R / (hi - lo).  sigma NULL: the layer has no proposal."""
    _fields_ = [("sigma", c_f32p), ("res", C.c_int32 * 3), ("lo", C.c_float * 3), ("inv_cell", C.c_float * 3)]


class RenderOptionsProposal(C.Structure):
    """stnerf_render_options_proposal (include/stnerf.h): ``RenderOptionsDeep`` followed by the table of density grids; struct_size
    says which of the three a record is.  ``RenderOptionsProposal()`` is "no feature" too.  ``ref()`` is what the render entries take."""
    _fields_ = RenderOptionsDeep._fields_ + [("proposal", C.POINTER(DensityGrid))]

    def __init__(self, **fields):
        super().__init__(struct_size=C.sizeof(RenderOptionsProposal), **fields)

    def ref(self):
        return C.cast(C.pointer(self), C.POINTER(RenderOptions))


DEEP_MAX_ELEMENTS = 8   # STNERF_DEEP_MAX_ELEMENTS


class LensRecord(C.Structure):
    """stnerf_lens (include/stnerf.h): the distortion coefficients, the plane in focus, the device table of lens points and the
    pass's place in it.  ``LensRecord()`` is "no lens": all zero, struct_size set."""
    _fields_ = [("struct_size", C.c_int32), ("distort", C.c_int32), ("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float),
                ("p1", C.c_float), ("p2", C.c_float), ("focus", C.c_float), ("points", c_f32p), ("n_points", C.c_int32),
                ("phase", C.c_int32), ("decorrelate", C.c_int32), ("key", C.c_uint32)]

    def __init__(self, **fields):
        super().__init__(struct_size=C.sizeof(LensRecord), **fields)


class ReprojectSource(C.Structure):
    """stnerf_reproject_source (include/stnerf.h): one source's rows on the device, the floats between rows, and how many."""
    _fields_ = [("values", c_f32p), ("row_stride", C.c_int64), ("n", C.c_int64)]


REPROJECT_MAX_SOURCES = 4   # STNERF_REPROJECT_MAX_SOURCES
BKGD_CACHE_OFF, BKGD_CACHE_CAPTURE, BKGD_CACHE_REUSE = 0, 1, 2   # STNERF_BKGD_CACHE_*
LAYER_CACHE_OFF, LAYER_CACHE_CAPTURE, LAYER_CACHE_REUSE = 0, 1, 2   # STNERF_LAYER_CACHE_*
MOTION_ADD_TO_XYZ, MOTION_PLAIN_TIME = 1, 2   # STNERF_MOTION_* bits of stnerf_motionnet_fwd's add_to_xyz argument


class DwProblem(C.Structure):
    """stnerf_dw_problem (include/stnerf.h): one layer of stnerf_train_dw_batch."""
    _fields_ = [("dy", C.c_void_p), ("lddy", C.c_int64), ("x", C.c_void_p), ("ldx", C.c_int64), ("dw", C.c_void_p), ("lddw", C.c_int64),
                ("db", C.c_void_p), ("n", C.c_int32), ("k", C.c_int32)]


class TransposeSection(C.Structure):
    """stnerf_transpose_section (include/stnerf.h)."""
    _fields_ = [("w", C.c_void_p), ("ldw", C.c_int64), ("dst_off", C.c_int64), ("n_out", C.c_int32), ("n_in", C.c_int32), ("n_pad", C.c_int32)]


class ProfileRecord(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("kind", C.c_int32), ("ns", C.c_int32), ("tag", C.c_int32),
                ("n_rays", C.c_int64), ("bytes_per_ray", C.c_int64), ("ms", C.c_float), ("pad_", C.c_int32)]


_PROTOS = {
    "stnerf_profile_begin": (C.c_int, []),
    "stnerf_profile_end": (C.c_int, [C.POINTER(ProfileRecord), C.c_int, C.POINTER(C.c_int)]),
    "stnerf_version": (C.c_char_p, []),
    "stnerf_last_error": (C.c_char_p, []),
    "stnerf_device_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "stnerf_generate_rays": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, c_i64, c_i64, c_i64,
                                       c_i64, C.POINTER(C.c_float), C.c_int, c_f32p, C.c_int, C.c_void_p]),
    "stnerf_intersect": (C.c_int, [c_f32p, c_i64, C.c_int, c_f32p, c_i64, C.c_int, c_f32p, C.c_void_p]),
    "stnerf_sample_coarse": (C.c_int, [c_f32p, c_i64, C.c_int, c_f32p, c_i64, C.c_int, C.c_int, c_f32p, C.c_uint64,
                                       c_i64, c_i64, c_i64, C.POINTER(LayerEdit), C.POINTER(C.c_float), c_f32p, c_f32p,
                                       C.c_void_p, C.c_void_p]),
    "stnerf_sample_coarse_rot": (C.c_int, [c_f32p, c_i64, C.c_int, c_f32p, c_i64, C.c_int, C.c_int, c_f32p, C.c_uint64,
                                           c_i64, c_i64, c_i64, C.POINTER(LayerEdit), C.POINTER(C.c_float), C.POINTER(LayerRotation),
                                           c_f32p, c_f32p, C.c_void_p, C.c_void_p]),
    "stnerf_compact_rays": (C.c_int, [C.c_void_p, c_i64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stnerf_packed_bytes": (c_i64, [C.c_int]),
    "stnerf_pack_net": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, c_i64]),
    "stnerf_pack_net_device": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_pack_net_bf16x3_device": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_spacenet_fwd": (C.c_int, [C.c_int, C.c_void_p, c_i64, C.c_int, C.c_void_p, C.c_void_p, c_f32p, c_i64,
                                      c_f32p, c_i64, c_f32p, c_i64, c_f32p, c_i64, c_f32p, C.c_void_p]),
    "stnerf_rgb_ray_bias": (C.c_int, [C.c_int, C.c_void_p, c_i64, C.c_void_p, C.c_void_p, c_f32p, c_i64, c_f32p, c_i64,
                                      c_f32p, C.c_void_p]),
    "stnerf_spacenet_fwd_rot": (C.c_int, [C.c_int, C.c_void_p, c_i64, C.c_int, C.c_void_p, C.c_void_p, c_f32p, c_i64,
                                          c_f32p, c_i64, c_f32p, c_i64, c_f32p, c_i64, c_f32p, C.POINTER(LayerRotation), C.c_void_p]),
    "stnerf_rgb_ray_bias_rot": (C.c_int, [C.c_int, C.c_void_p, c_i64, C.c_void_p, C.c_void_p, c_f32p, c_i64, c_f32p, c_i64,
                                          c_f32p, C.POINTER(LayerRotation), C.c_void_p]),
    "stnerf_packed_bytes_bf16x3": (c_i64, [C.c_int]),
    "stnerf_pack_net_bf16x3": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p,
                                         c_i64]),
    "stnerf_motionnet_fwd": (C.c_int, [C.c_void_p, c_i64, C.c_int, C.c_void_p, C.c_void_p, c_f32p, c_i64, c_f32p,
                                       c_i64, c_f32p, c_i64, C.c_int, C.c_void_p]),
    "stnerf_mlp_stage": (C.c_int, [C.POINTER(StageLayer), C.c_int, c_i64, C.c_int, c_f32p, c_i64, c_i64, c_i64, c_i64, C.c_int,
                                   C.c_void_p, c_f32p, C.c_void_p]),
    "stnerf_mlp_stage_rows": (C.c_int, [C.POINTER(StageLayer), C.POINTER(StageRows), C.c_int, c_i64, C.c_int, c_f32p, c_i64, c_i64, c_i64, c_i64,
                                        C.c_int, C.c_void_p, c_f32p, C.c_void_p]),
    "stnerf_train_linear_fwd": (C.c_int, [c_f32p, c_i64, c_f32p, c_i64, c_f32p, c_i64, C.c_int, C.c_int, C.c_int, c_f32p, c_i64, C.c_void_p]),
    "stnerf_train_linear_dx": (C.c_int, [c_f32p, c_i64, c_f32p, c_i64, c_i64, C.c_int, C.c_int, c_f32p, c_i64, C.c_int, c_f32p, c_i64,
                                         C.c_void_p]),
    "stnerf_train_dw_workspace_bytes": (c_i64, [c_i64, C.c_int, C.c_int]),
    "stnerf_train_linear_dw": (C.c_int, [c_f32p, c_i64, c_f32p, c_i64, c_i64, C.c_int, C.c_int, c_f32p, c_i64, c_f32p, C.c_int, C.c_void_p,
                                         c_i64, C.c_void_p]),
    "stnerf_train_dw_batch_workspace_bytes": (c_i64, [C.POINTER(DwProblem), C.c_int32, c_i64]),
    "stnerf_train_dw_batch_plan": (C.c_int, [C.POINTER(DwProblem), C.c_int32, c_i64, C.POINTER(C.c_int32)]),
    "stnerf_train_dw_batch": (C.c_int, [C.POINTER(DwProblem), C.c_int32, c_i64, C.c_int32, C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_train_encode": (C.c_int, [c_f32p, c_i64, C.c_int, C.c_int, C.c_int, c_i64, C.c_int, C.c_int, C.c_int, c_f32p, c_i64, C.c_int,
                                      C.c_void_p]),
    "stnerf_train_encode_bwd": (C.c_int, [c_f32p, c_i64, C.c_int, C.c_int, C.c_int, c_i64, c_f32p, c_i64, C.c_int, C.c_int, C.c_int, c_f32p,
                                          c_i64, C.c_void_p]),
    "stnerf_train_spacenet_fwd": (C.c_int, [C.c_int, C.c_void_p, c_i64, C.c_int, c_f32p, c_i64, c_f32p, c_i64, c_f32p, c_i64, c_f32p, c_i64,
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_int32), c_f32p, C.c_int32, C.c_void_p, c_i64, C.c_void_p, c_f32p, C.c_void_p]),
    "stnerf_train_spacenet_fwd_bf16x3": (C.c_int, [C.c_int, C.c_void_p, c_i64, C.c_int, c_f32p, c_i64, c_f32p, c_i64, c_f32p, c_i64, c_f32p, c_i64,
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_int32), c_f32p, C.c_int32, C.c_void_p, c_i64, C.c_void_p, c_f32p, C.c_void_p]),
    "stnerf_train_spacenet_dx": (C.c_int, [c_f32p, C.POINTER(C.c_uint32), c_f32p, c_i64, C.c_void_p, c_i64, C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                           c_f32p, C.c_int32, C.c_void_p]),
    "stnerf_packed_bytes_dx_bf16x3": (c_i64, [C.c_int, C.c_int]),
    "stnerf_pack_dx_bf16x3_device": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_train_spacenet_dx_bf16x3": (C.c_int, [C.c_void_p, C.c_int, c_f32p, c_i64, C.c_void_p, c_i64, C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                                  c_f32p, C.c_int32, c_f32p, C.c_int32, C.c_void_p]),
    "stnerf_pack_transposed": (C.c_int, [C.POINTER(TransposeSection), C.c_int, c_f32p, c_i64, C.c_void_p]),
    "stnerf_train_motionnet_fwd": (C.c_int, [C.c_void_p, c_f32p, c_i64, C.c_int, c_f32p, c_f32p, C.c_int32, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_int32), C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_train_motionnet_dx": (C.c_int, [c_f32p, C.POINTER(C.c_uint32), c_f32p, c_i64, C.c_void_p, c_i64, C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_int32), c_f32p, C.c_int32, C.c_void_p]),
    "stnerf_encode": (C.c_int, [c_f32p, c_i64, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p]),
    "stnerf_gen_weight": (C.c_int, [c_f32p, c_f32p, c_i64, C.c_int, c_f32p, C.c_void_p]),
    "stnerf_composite": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_i64, C.c_int, C.c_int, C.POINTER(CompositeParams),
                                   c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stnerf_composite_scene": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_i64, C.c_int, C.c_int, C.POINTER(CompositeParams),
                                         c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, C.c_void_p]),
    "stnerf_composite_bwd": (C.c_int, [c_f32p, c_f32p, C.c_void_p, C.c_void_p, c_i64, C.c_int, C.c_int, C.POINTER(CompositeParams),
                                       c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "stnerf_composite_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(c_i64)]),
    "stnerf_render_workspace_bytes": (c_i64, [c_i64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "stnerf_occupancy_build": (C.c_int, [c_f32p, c_f32p, C.POINTER(C.c_int32), C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "stnerf_occupancy_cull": (C.c_int, [c_f32p, c_i64, C.c_int, C.c_int, C.POINTER(Occupancy), C.c_void_p, C.c_void_p, C.c_void_p]),
    "stnerf_occupancy_rows": (C.c_int, [C.c_void_p, C.c_void_p, c_i64, C.c_int, c_f32p, c_i64, C.c_int, C.POINTER(Occupancy), c_f32p, c_i64,
                                        C.c_void_p, c_i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stnerf_render_workspace_bytes_samples": (c_i64, [c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "stnerf_ray_stop": (C.c_int, [c_f32p, c_f32p, c_i64, C.c_int, C.c_int, C.c_float, c_f32p, C.c_void_p]),
    "stnerf_visibility_rows": (C.c_int, [C.c_void_p, C.c_void_p, c_i64, C.c_int, c_f32p, c_i64, c_f32p, c_i64, c_f32p, C.c_int,
                                         C.POINTER(Occupancy), c_f32p, c_i64, C.c_void_p, c_i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stnerf_render_workspace_bytes_terminated": (c_i64, [c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "stnerf_background_rows": (C.c_int, [c_i64, c_f32p, c_i64, C.c_int, C.POINTER(Occupancy), c_f32p, c_i64, c_f32p, c_f32p, c_i64,
                                         C.c_void_p, c_i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stnerf_background_ray_rows": (C.c_int, [c_i64, c_f32p, c_i64, C.c_int, C.POINTER(Occupancy), c_f32p, c_i64, c_f32p, c_f32p, c_i64,
                                             C.c_void_p, c_i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stnerf_render_workspace_bytes_background": (c_i64, [c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                         C.c_int]),
    "stnerf_scene_occluder": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, c_i64, C.c_int, C.c_int, C.POINTER(CompositeParams), c_f32p, c_f32p,
                                        c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "stnerf_occluder_stop": (C.c_int, [c_f32p, c_i64, c_f32p, C.c_void_p]),
    "stnerf_deep_workspace_bytes": (c_i64, [c_i64]),
    "stnerf_deep_count": (C.c_int, [c_f32p, C.c_void_p, c_f32p, c_i64, C.c_int, C.c_int, C.POINTER(CompositeParams), C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p]),
    "stnerf_deep_offsets": (C.c_int, [C.c_void_p, c_i64, c_i64, C.c_void_p, C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_deep_fill": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, c_i64, C.c_int, C.c_int, C.POINTER(CompositeParams), C.c_float, C.c_float,
                                   C.c_void_p, c_f32p, c_i64, C.c_void_p, C.c_void_p]),
    "stnerf_deep_composite": (C.c_int, [C.c_void_p, c_f32p, c_i64, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "stnerf_proposal_density": (C.c_int, [C.c_void_p, C.c_void_p, c_i64, C.c_int, c_f32p, c_i64, C.c_int, C.POINTER(DensityGrid), c_f32p, c_i64,
                                          C.c_void_p]),
    "stnerf_generate_rays_list": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, c_i64, C.c_float,
                                            C.c_float, C.POINTER(C.c_float), C.c_int, c_f32p, C.c_int, C.c_void_p]),
    "stnerf_generate_rays_lens": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, c_i64, C.c_float,
                                            C.c_float, C.POINTER(LensRecord), C.POINTER(C.c_float), C.c_int, c_f32p, C.c_int, C.c_void_p]),
    "stnerf_accumulate": (C.c_int, [c_f32p, c_i64, C.c_int, c_i64, C.c_void_p, c_i64, C.c_int, c_f32p, c_f32p, C.c_void_p, C.c_void_p]),
    "stnerf_accumulate_select_workspace_bytes": (c_i64, [c_i64]),
    "stnerf_accumulate_select": (C.c_int, [c_f32p, C.c_void_p, c_i64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                           C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_reproject_splat": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, c_f32p, c_i64, c_i64,
                                         C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_float,
                                         C.c_void_p, C.c_void_p]),
    "stnerf_reproject_resolve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(ReprojectSource), C.c_int, C.c_int, c_f32p,
                                           c_f32p, C.c_void_p, C.c_void_p]),
    "stnerf_reproject_holes_workspace_bytes": (c_i64, [c_i64]),
    "stnerf_reproject_holes": (C.c_int, [C.c_void_p, c_i64, C.c_void_p, C.c_void_p, C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_lattice_begin": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stnerf_lattice_classify": (C.c_int, [c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p,
                                          c_i64, C.c_void_p]),
    "stnerf_lattice_select_workspace_bytes": (c_i64, [c_i64]),
    "stnerf_lattice_select": (C.c_int, [C.c_void_p, c_i64, C.c_void_p, C.c_void_p, C.c_void_p, c_i64, C.c_void_p]),
    "stnerf_lattice_scatter": (C.c_int, [c_f32p, c_i64, C.c_int, c_i64, C.c_void_p, c_i64, c_f32p, C.c_void_p, C.c_void_p]),
    "stnerf_copy_layer_raw_listed": (C.c_int, [c_f32p, c_i64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, c_f32p, C.c_void_p,
                                               C.c_void_p, c_i64, C.c_int, C.c_void_p, C.c_void_p]),
    "stnerf_copy_layer_raw": (C.c_int, [c_f32p, c_i64, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, C.c_void_p]),
    "stnerf_resample": (C.c_int, [c_f32p, c_f32p, c_i64, C.c_int, C.c_int, C.c_int, c_f32p, C.c_uint64, c_i64, c_i64, c_i64, c_f32p,
                                  C.c_int, C.POINTER(LayerEdit), C.POINTER(C.c_float), C.c_void_p, c_f32p, c_f32p, c_f32p,
                                  C.c_void_p, c_f32p, C.c_void_p]),
    "stnerf_resample_rot": (C.c_int, [c_f32p, c_f32p, c_i64, C.c_int, C.c_int, C.c_int, c_f32p, C.c_uint64, c_i64, c_i64, c_i64, c_f32p,
                                      C.c_int, C.POINTER(LayerEdit), C.POINTER(C.c_float), C.POINTER(LayerRotation), C.c_void_p, c_f32p,
                                      c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_void_p]),
}

# The render entries: the 15 arguments each of them starts with, then the options -- as one record (stnerf_render_rays_opts) or, in
# the named fixed-argument forms, the record's fields up to the one the entry introduced -- then the stream.
_RENDER_PREFIX = [c_f32p, c_i64, c_f32p, c_i64, C.POINTER(Nets), C.POINTER(RenderParams), c_f32p, c_f32p, C.c_void_p, c_i64,
                  c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p]
_OPTION_NAMES, _OPTION_TYPES = zip(*RenderOptions._fields_)
_LAST_OPTION = {"": "struct_size", "_cached": "cache", "_rot": "rot", "_scene": "scene_out", "_opacity": "layer_alpha",
                "_occupancy": "counts", "_samples": "sample_counts", "_terminated": "visibility_counts", "_background": "bkgd_counts",
                "_layers": "mismatch", "_occluded": "occluder_share"}
for _suffix, _last in _LAST_OPTION.items():   # (struct_size itself is no argument of a named entry)
    _PROTOS["stnerf_render_rays" + _suffix] = (C.c_int, _RENDER_PREFIX + list(_OPTION_TYPES[1:_OPTION_NAMES.index(_last) + 1]) + [C.c_void_p])
_PROTOS["stnerf_render_rays_opts"] = (C.c_int, _RENDER_PREFIX + [C.POINTER(RenderOptions), C.c_void_p])
_PROTOS["stnerf_render_workspace_bytes_opts"] = (c_i64, [c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RenderOptions)])

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """The loaded library (loads on first use; raises if it is not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python st-nerf_amd/build.py` "
                "(or __graft_entry__.build()).  There is no PyTorch fallback for the render path.")
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def exported_symbols():
    return sorted(_PROTOS)


def last_error() -> str:
    return lib().stnerf_last_error().decode()


def check(rc: int, what: str) -> None:
    if rc == OK:
        return
    msg = f"{what}: {last_error()} (code {rc})"
    if rc == EINVAL:
        raise ValueError(msg)
    raise RuntimeError(msg)


def stream_ptr() -> C.c_void_p:
    """The current torch stream as a hipStream_t."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t: Optional[torch.Tensor], dtype=torch.float32, name: str = "tensor") -> C.c_void_p:
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return C.c_void_p(t.data_ptr())


def fatbin_sha256(path: Optional[str] = None) -> Optional[str]:
    """sha256 of the library's ``.hip_fatbin`` section (the device code objects): what identifies the KERNELS of a build
    independently of where it was linked.  bench.py prints committed PMC counter bytes only when they were measured on
    exactly these kernels (tools/summarise.py records the digest beside them).  None when the file is not an ELF64 with
    that section."""
    import hashlib
    import struct
    try:
        with open(path or LIB_PATH, "rb") as f:
            ident = f.read(64)
            if ident[:4] != b"\x7fELF" or ident[4] != 2:
                return None
            shoff, = struct.unpack_from("<Q", ident, 0x28)
            shentsize, shnum, shstrndx = struct.unpack_from("<HHH", ident, 0x3A)
            f.seek(shoff)
            table = f.read(shentsize * shnum)
            sec = lambda i: struct.unpack_from("<IIQQQQ", table, i * shentsize)   # name, type, flags, addr, offset, size
            _, _, _, _, str_off, str_size = sec(shstrndx)
            f.seek(str_off)
            names = f.read(str_size)
            for i in range(shnum):
                name, _, _, _, off, size = sec(i)
                if names[name:names.index(b"\0", name)] == b".hip_fatbin":
                    f.seek(off)
                    return hashlib.sha256(f.read(size)).hexdigest()
    except (OSError, struct.error, ValueError):
        pass
    return None


def device_info() -> dict:
    cu, lds, clk = C.c_int(0), C.c_int(0), C.c_int(0)
    arch = C.create_string_buffer(64)
    rc = lib().stnerf_device_info(C.byref(cu), C.byref(lds), C.byref(clk), arch, 64)
    info = dict(cu_count=cu.value, lds_bytes_per_cu=lds.value, clock_khz=clk.value, arch=arch.value.decode())
    check(rc, "stnerf_device_info")
    return info
