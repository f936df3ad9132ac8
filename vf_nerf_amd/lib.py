"""ctypes binding of ``libvfn.so`` (the C ABI declared in ``include/vfn.h``).

There is no CPU fallback: if the shared library is missing, or a tensor is not a contiguous fp32
CUDA(HIP) tensor, the call raises.  ``import torch`` must come first so that the HIP runtime the
library binds to is the one PyTorch already loaded (same ``libamdhip64.so.7`` SONAME).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import List, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VFN_LIB") or os.path.join(_HERE, "csrc", "libvfn.so")     # VFN_LIB: an experimental build (tools/)

MAX_LAYERS = 16
HIDDEN = 256
NET_VF, NET_RENDER = 0, 1

EXPORTS = (
    "vfn_last_error", "vfn_abi_version", "vfn_abi_struct_bytes", "vfn_packed_size", "vfn_pack_weights", "vfn_raygen_uniform",
    "vfn_vf_mlp_fwd", "vfn_render_mlp_fwd", "vfn_vf_render_fused_fwd", "vfn_ray_density_weights",
    "vfn_range_fine_sample", "vfn_range_fine_sample_indexed", "vfn_fill_uniform", "vfn_sample_sphere_shell", "vfn_packed_bwd_size", "vfn_pack_weights_bwd",
    "vfn_vf_mlp_fwd_train", "vfn_vf_render_fused_fwd_train", "vfn_mlp_bwd_chain", "vfn_weight_grad_partials",
    "vfn_ray_density_weights_bwd", "vfn_pack16_size", "vfn_pack16_weights", "vfn_vf_mlp16_fwd",
    "vfn_vf_render_fused16_fwd", "vfn_vf_mlp16_fwd_train", "vfn_vf_render_fused16_fwd_train",
    "vfn_vf_feat16_fwd", "vfn_render16_from_blocks", "vfn_grid_divergence", "vfn_grid_smooth_axis",
    "vfn_grid_unify_direction", "vfn_grid_comb_format", "vfn_grid_unify_direction_sides", "vfn_grid_comb_format_sides", "vfn_weight_grad_partials_bf16", "vfn_unfold_weight_grads", "vfn_packed_bwd16_size", "vfn_pack_weights_bwd16", "vfn_pack_weights_bwd16_mode", "vfn_mlp_bwd_chain_bf16",
    "vfn_linear_rows", "vfn_linear_rows_stat_parts", "vfn_bstat_row_parts", "vfn_colsum_finish", "vfn_bstat_finalize",
    "vfn_bstat_relu_rows", "vfn_bstat_relu_bwd_sums", "vfn_bstat_relu_bwd_rows", "vfn_act_bwd_rows", "vfn_embed_rows",
    "vfn_embed_rows_bwd", "vfn_vf_render_fused16_scatter", "vfn_vf_render_fused16_products", "vfn_net_weight_grads_frag", "vfn_net_weight_grads_frag_part", "vfn_net_weight_grads_scratch_bytes", "vfn_vf_render_fused16_fwd_train_at",
    "vfn_vf_mlp16_fwd_train_at", "vfn_mlp_bwd_chain_bf16_ws_at",
    "vfn_weight_grad_groups", "vfn_scatter_rows3", "vfn_uniform_sample", "vfn_rows_argmax", "vfn_merge_sort_depths",
    "vfn_ray_density_sigma_bwd", "vfn_weight_grad_frag", "vfn_mlp_bwd_chain_bf16_ws", "vfn_f16x3_set_status", "vfn_f16x3_set_clock_probe", "vfn_flat_clip_workspace_bytes", "vfn_flat_clip_grad_norm", "vfn_flat_adam_step", "vfn_unfold_weight_grads_acc", "vfn_render_fwd", "vfn_render_fwd_workspace_bytes",
    "vfn_vf_loss_workspace_bytes", "vfn_vf_loss_fwd", "vfn_vf_loss_bwd", "vfn_train_step", "vfn_train_step_workspace_bytes",
    "vfn_train_step_workspace_layout", "vfn_train_step_supervision_points", "vfn_train_step_supervision_forward", "vfn_train_step_supervision_backward",
    "vfn_linear_rows_dx_sums", "vfn_weight_grad_partials_bf16_ld", "vfn_linear_rows_ws", "vfn_linear_rows_wplanes_bytes",
    "vfn_select_samples", "vfn_grid_lattice_points", "vfn_linear_rows_fold", "vfn_weight_grad_partials_bf16_fold",
    "vfn_mesh_tables", "vfn_mesh_scan_workspace_bytes", "vfn_mesh_count", "vfn_mesh_emit", "vfn_mesh_dedup", "vfn_mesh_number",
    "vfn_mesh_field_norms",
    "vfn_nn_sqdist", "vfn_tri_areas", "vfn_cumsum_workspace_bytes", "vfn_cumsum_f64", "vfn_sample_surface",
    "vfn_reduce_stats_workspace_bytes", "vfn_reduce_stats",
    "vfn_tsdf_integrate", "vfn_tsdf_count", "vfn_tsdf_emit", "vfn_tsdf_integrate_rgb", "vfn_tsdf_emit_colours", "vfn_tsdf_vertex_colours",
    "vfn_tsdf_sparse_mark", "vfn_tsdf_sparse_integrate", "vfn_tsdf_sparse_integrate_rgb", "vfn_tsdf_sparse_count", "vfn_tsdf_sparse_emit",
    "vfn_tsdf_sparse_emit_colours",
    "vfn_raster_depth", "vfn_smooth_laplacian_step",
    "vfn_transform_points", "vfn_nn_radius", "vfn_icp_accumulate_workspace_bytes", "vfn_icp_accumulate",
    "vfn_nn_nearest", "vfn_nn_nearest_list",
    "vfn_tri_cell_ranges", "vfn_tri_cell_pairs", "vfn_tri_nearest", "vfn_tri_nearest_list",
    "vfn_image_quantize8", "vfn_image_scores_workspace_bytes", "vfn_image_scores", "vfn_image_abs_err",
    "vfn_face_normals", "vfn_vertex_normals", "vfn_normal_dots",
    "vfn_voxel_keys", "vfn_voxel_means",
    "vfn_cc_union_runs", "vfn_cc_flatten", "vfn_cc_segment_sums",
    "vfn_orient_union_runs", "vfn_orient_flatten", "vfn_orient_votes",
    "vfn_face_planes", "vfn_cluster_quadrics",
    "vfn_boundary_planes", "vfn_vertex_quadrics", "vfn_edge_collapse_candidates", "vfn_collapse_select",
    "vfn_kmeans_assign", "vfn_kmeans_update_workspace_bytes", "vfn_kmeans_update", "vfn_kmeans_seed_workspace_bytes", "vfn_kmeans_seed",
)


class VfnError(RuntimeError):
    pass


class NetGeom(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("multires", C.c_int32), ("skip_layer", C.c_int32),
                ("feature_dims", C.c_int32), ("in_dims", C.c_int32 * MAX_LAYERS),
                ("out_dims", C.c_int32 * MAX_LAYERS), ("has_bn", C.c_int32 * MAX_LAYERS)]


class LayerParams(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("bn_weight", C.c_void_p),
                ("bn_bias", C.c_void_p), ("bn_mean", C.c_void_p), ("bn_var", C.c_void_p)]


class RaygenParams(C.Structure):
    _fields_ = [("n_rays", C.c_int32), ("n_samples", C.c_int32), ("pose_is_quat", C.c_int32),
                ("near", C.c_float), ("far", C.c_float)]


class DensityParams(C.Structure):
    _fields_ = [("n_rays", C.c_int32), ("n_samples", C.c_int32), ("n_window", C.c_int32),
                ("normalize", C.c_int32), ("dir_to_normal_th", C.c_float),
                ("beta_min", C.c_float), ("beta_max", C.c_float), ("mean_min", C.c_float),
                ("mean_max", C.c_float), ("scale_min", C.c_float), ("cutoff", C.c_float)]


class FineParams(C.Structure):
    _fields_ = [("n_rays", C.c_int32), ("n_coarse", C.c_int32), ("n_fine", C.c_int32),
                ("near", C.c_float), ("far", C.c_float), ("half_range", C.c_float),
                ("window_step", C.c_float), ("span", C.c_float)]


class RenderParams(C.Structure):
    """mirrors vfn_render_params"""
    _fields_ = [("n_rays", C.c_int32), ("n_coarse", C.c_int32), ("n_fine", C.c_int32), ("pose_is_quat", C.c_int32),
                ("perturb_coarse", C.c_int32), ("perturb_fine", C.c_int32), ("near_coarse", C.c_float), ("near_fine", C.c_float),
                ("far_coarse", C.c_float), ("far_fine", C.c_float), ("fine_range", C.c_float), ("window_step", C.c_float), ("span", C.c_float),
                ("density", DensityParams), ("seed", C.c_uint64), ("offset", C.c_uint64), ("colour_products", C.c_int32), ("separate_launches", C.c_int32), ("streams", C.c_int32), ("sparse_colours", C.c_int32),
                ("timing_events", C.c_void_p * 4), ("status_word", C.c_void_p), ("clock_stamps", C.c_void_p), ("clock_slots", C.c_int64)]


class LossParams(C.Structure):
    """mirrors vfn_loss_params"""
    _fields_ = [("n_rays", C.c_int64), ("n_normals", C.c_int64), ("n_sup", C.c_int64 * 3), ("has_depth", C.c_int32), ("smaller_on", C.c_int32),
                ("ray_center", C.c_int32), ("reserved", C.c_int32), ("w_rgb", C.c_float), ("w_depth", C.c_float), ("w_unit", C.c_float),
                ("w_sup", C.c_float), ("w_smaller", C.c_float), ("depth_clamp", C.c_float), ("radius", C.c_float), ("centroid", C.c_float * 3)]


class TrainStepParams(C.Structure):
    """mirrors vfn_train_step_params"""
    _fields_ = [("render", RenderParams), ("loss", LossParams), ("n_sup", C.c_int64), ("border", C.c_int32), ("center", C.c_int32),
                ("sup_centroid", C.c_float * 3), ("sup_radius", C.c_float), ("border_r_min", C.c_float), ("border_r_max", C.c_float), ("phases", C.c_int32),
                ("sup_seed", C.c_uint64), ("sup_offset", C.c_uint64), ("save_flags", C.c_int32), ("dy_flags", C.c_int32), ("dy_form", C.c_int32),
                ("x_form", C.c_int32), ("forward_products", C.c_int32), ("repack", C.c_int32), ("n_regions", C.c_int32), ("mults", C.c_int32 * 4),
                ("starts", C.c_int64 * 4), ("ends", C.c_int64 * 4), ("step_size", C.c_double * 8), ("bc2_sqrt", C.c_double * 8),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double), ("max_norm", C.c_float),
                ("sparse_colours", C.c_int32), ("sup_rows_reserved", C.c_int64), ("sup_rows_used", C.c_int64)]


class TrainStepIO(C.Structure):
    """mirrors vfn_train_step_io (every member a pointer except n_flat)"""
    _fields_ = [(n, C.c_void_p) for n in ("vf_geom", "rn_geom", "vf_packed16", "rn_packed16", "vf_packed_bwd16", "rn_packed_bwd16", "vf_layers", "rn_layers",
                                          "vf_wgrad", "rn_wgrad", "vf_head_w", "rn_head_w", "beta", "mean", "scale", "g_beta", "g_mean", "g_scale",
                                          "flat_param", "flat_grad", "exp_avg", "exp_avg_sq")] + [("n_flat", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("clip_workspace", "uv", "pose", "intrinsics", "t_vals", "far_coarse_per_ray", "far_fine_per_ray", "u_coarse", "u_fine",
                                          "u_add", "sup_u_border", "sup_u_center", "rgb_gt", "depth_gt", "workspace", "ray_dirs", "z_vals", "points", "normals",
                                          "colors", "weights", "rgb", "depth", "out_terms", "out_norm", "out_counts", "d_rgb_in", "d_depth_in", "d_normals_in")]


TRAIN_FORWARD_BACKWARD, TRAIN_OPTIMIZER, TRAIN_RENDER, TRAIN_BACKWARD, TRAIN_CLIP, TRAIN_ADAM = 1, 2, 4, 8, 16, 32
# indices of vfn_train_step_workspace_layout's output (VFN_TWS_* of include/vfn.h)
TWS_SUP_PTS, TWS_SUP_GT, TWS_SUP_PRED, TWS_D_SUP, TWS_DN, TWS_SUP_ROWS, TWS_TOTAL_ROWS, TWS_BYTES, TWS_COUNT = range(9)

_lib: Optional[C.CDLL] = None

def _find_header() -> str:
    """include/vfn.h of the repository, or the copy the build leaves inside the package (``vf_nerf_amd/vfn_abi.h``, written by
    csrc/build.sh) for a package that was copied / installed without the repository around it; ``VFN_HEADER`` overrides both."""
    for cand in (os.environ.get("VFN_HEADER"), os.path.join(os.path.dirname(_HERE), "include", "vfn.h"), os.path.join(_HERE, "vfn_abi.h")):
        if cand and os.path.exists(cand):
            return cand
    raise VfnError(f"include/vfn.h not found next to the package ({os.path.dirname(_HERE)}/include) nor as {_HERE}/vfn_abi.h: the binding's "
                   "signatures are generated from it; set VFN_HEADER or rebuild with vf_nerf_amd/csrc/build.sh")


_header_cache: dict = {}


def _header_raw() -> str:
    if "raw" not in _header_cache:
        path = _find_header()
        with open(path) as fh:
            _header_cache["raw"], _header_cache["path"] = fh.read(), path
    return _header_cache["raw"]


def _header_text() -> str:
    import re
    text = re.sub(r"/\*.*?\*/", "", _header_raw(), flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def header_abi_version() -> int:
    import re
    return int(re.search(r"#define\s+VFN_ABI_VERSION\s+(\d+)", _header_raw()).group(1))


@functools.lru_cache(maxsize=None)
def header_constant(name: str) -> int:
    """An integer ``#define`` of include/vfn.h (the header is the single source the kernels are compiled from)."""
    import re
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", _header_raw()).group(1))


def __getattr__(name: str):
    # read on first use, not at import: the CPU-only parts of the package (loss, optimizer, host logic) import this module too
    if name == "ABI_VERSION":            # include/vfn.h is the single source: the library must report the same number
        return header_abi_version()
    if name == "HEADER_PATH":
        _header_raw()
        return _header_cache["path"]
    if name == "REDUCE_TILE":            # values per first-level partial of the fixed tree
        return header_constant("VFN_TREE_LANES") * header_constant("VFN_TREE_PER")
    if name in ("REDUCE_TOP", "IMAGE_TOP"):          # lanes of its second level
        return header_constant("VFN_TREE_TOP")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def header_prototypes() -> dict:
    """{name: (return type, [parameter types])} of every ``vfn_*`` entry point declared in include/vfn.h, as C type strings
    without the parameter names (``"const float*"``, ``"int64_t"``, ...)."""
    import re
    out = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w\s\*]*?)\b(vfn_\w+)\s*\(([^;{}]*?)\)\s*;", _header_text(), flags=re.M | re.S):
        plist = []
        for prm in params.replace("\n", " ").split(","):
            prm = re.sub(r"\s+", " ", prm).strip()
            if prm in ("void", ""):
                continue
            if "[" in prm or "(" in prm:        # array parameters / function pointers: not a form this generator understands
                raise VfnError(f"{name}: parameter '{prm}' of include/vfn.h is an array or a function pointer; the binding generator "
                               "handles scalars and plain pointers only")
            plist.append(re.match(r"(.*?)\s*\w+$", prm).group(1).replace(" *", "*").strip())
        out[name] = (re.sub(r"\s+", " ", ret).strip(), plist)
    return out


_INT_TYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
_FLOAT_TYPES = {"float": C.c_float, "double": C.c_double}
_C_INTS = (C.c_int8, C.c_int16, C.c_int32, C.c_int64, C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64, C.c_bool)


class _IntArg:
    """argtypes entry of an integer parameter: Python ints and ctypes integers of any width pass (converted to the declared
    width); floats, pointers and None do not — a call whose arguments were reordered fails here instead of reaching the kernel."""

    def __init__(self, ctype, what):
        self.ctype, self.what = ctype, what

    def from_param(self, v):
        if isinstance(v, _C_INTS):
            v = v.value
        if isinstance(v, bool):
            v = int(v)
        if not isinstance(v, int):
            raise TypeError(f"{self.what}: expected an integer, got {type(v).__name__}")
        return self.ctype(v)


class _FloatArg:
    def __init__(self, ctype, what):
        self.ctype, self.what = ctype, what

    def from_param(self, v):
        if isinstance(v, (C.c_float, C.c_double)):
            v = v.value
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError(f"{self.what}: expected a real number, got {type(v).__name__}")
        return self.ctype(float(v))


class _PtrArg:
    """argtypes entry of a pointer parameter: None, c_void_p, byref()/pointer() results and ctypes arrays / structures pass."""

    def __init__(self, what):
        self.what = what

    def from_param(self, v):
        if v is None:
            return C.c_void_p(0)
        if isinstance(v, (C.c_void_p, C.c_char_p, C.Array, C._Pointer)) or type(v).__name__ == "CArgObject":
            return v
        if isinstance(v, C.Structure):
            return C.byref(v)
        raise TypeError(f"{self.what}: expected a pointer (None, c_void_p, byref(struct), ctypes array), got {type(v).__name__}")


def _declare(lib: C.CDLL) -> None:
    """restype / argtypes of EVERY export, generated from the prototypes of include/vfn.h (the header is the single source; a
    signature edited there reaches the binding without a second hand-written list)."""
    protos = header_prototypes()
    for name in EXPORTS:
        fn = getattr(lib, name)               # raises AttributeError if the ABI lost a symbol
        if name not in protos:
            raise VfnError(f"{name} is exported by the binding but not declared in {_header_cache['path']}")
        ret, params = protos[name]
        fn.restype = C.c_char_p if ret == "const char*" else _INT_TYPES[ret]
        args = []
        for i, t in enumerate(params):
            what = f"{name} argument {i} ({t})"
            args.append(_PtrArg(what) if t.endswith("*") else
                        _IntArg(_INT_TYPES[t], what) if t in _INT_TYPES else _FloatArg(_FLOAT_TYPES[t], what))
        fn.argtypes = args


def struct_mirrors():
    """The ctypes mirrors of the header's POD structs in the order of ``vfn_abi_struct_bytes``."""
    return (NetGeom, LayerParams, RaygenParams, DensityParams, FineParams, RenderParams, UnfoldEntry, WgradLayer, LossParams, TrainStepParams,
            TrainStepIO)


def load() -> C.CDLL:
    """Load libvfn.so once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VfnError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"or vf_nerf_amd/csrc/build.sh (there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    _declare(lib)
    if lib.vfn_abi_version() != header_abi_version():
        raise VfnError(f"libvfn.so reports ABI {lib.vfn_abi_version()}, include/vfn.h says {header_abi_version()}: rebuild the library")
    for i, mirror in enumerate(struct_mirrors()):
        if lib.vfn_abi_struct_bytes(i) != C.sizeof(mirror):
            raise VfnError(f"{mirror.__name__}: {C.sizeof(mirror)} bytes in the binding, {lib.vfn_abi_struct_bytes(i)} in libvfn.so")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise VfnError(f"{what} failed (status {rc}): {load().vfn_last_error().decode()}")


def _ptr(t: Optional[torch.Tensor], name: str, dtype=torch.float32) -> C.c_void_p:
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise VfnError(f"{name}: expected a CUDA/HIP tensor, got {t.device} (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise VfnError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise VfnError(f"{name}: tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _stream() -> C.c_void_p:
    # (the raw handle of the current stream of the current device: torch.cuda.current_stream() builds a Stream object around it, 13 us a call)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


# ------------------------------------------------------------------------------------------------
# geometry / packing
# ------------------------------------------------------------------------------------------------
def make_geom(n_layers: int, multires: int, skip_layer: int, feature_dims: int, in_dims: Sequence[int],
              out_dims: Sequence[int], has_bn: Sequence[bool]) -> NetGeom:
    if n_layers > MAX_LAYERS:
        raise VfnError(f"{n_layers} layers > {MAX_LAYERS}")
    g = NetGeom()
    g.n_layers, g.multires, g.skip_layer, g.feature_dims = n_layers, multires, skip_layer, feature_dims
    for i in range(n_layers):
        g.in_dims[i], g.out_dims[i], g.has_bn[i] = int(in_dims[i]), int(out_dims[i]), int(bool(has_bn[i]))
    return g


def packed_size(kind: int, geom: NetGeom) -> int:
    n = load().vfn_packed_size(kind, C.byref(geom))
    if n < 0:
        raise VfnError(f"unsupported network geometry: {load().vfn_last_error().decode()}")
    return int(n)


def _layer_array(geom: NetGeom, layers: Sequence[dict]):
    arr = (LayerParams * geom.n_layers)()
    for i, lp in enumerate(layers):
        arr[i].weight = _ptr(lp["weight"], f"layer{i}.weight")
        arr[i].bias = _ptr(lp["bias"], f"layer{i}.bias")
        for k in ("bn_weight", "bn_bias", "bn_mean", "bn_var"):
            setattr(arr[i], k, _ptr(lp.get(k), f"layer{i}.{k}"))
    return arr


def pack_weights(kind: int, geom: NetGeom, layers: Sequence[dict], packed: torch.Tensor) -> None:
    """layers[i] = dict(weight=, bias=, bn_weight=, bn_bias=, bn_mean=, bn_var=) of live tensors."""
    _check(load().vfn_pack_weights(kind, C.byref(geom), _layer_array(geom, layers), _ptr(packed, "packed"), _stream()),
           "vfn_pack_weights")


def packed_bwd_size(kind: int, geom: NetGeom) -> int:
    n = load().vfn_packed_bwd_size(kind, C.byref(geom))
    if n < 0:
        raise VfnError(f"unsupported network geometry: {load().vfn_last_error().decode()}")
    return int(n)


def pack_weights_bwd(kind: int, geom: NetGeom, layers: Sequence[dict], packed_bwd: torch.Tensor) -> None:
    _check(load().vfn_pack_weights_bwd(kind, C.byref(geom), _layer_array(geom, layers), _ptr(packed_bwd, "packed_bwd"),
                                       _stream()), "vfn_pack_weights_bwd")


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
def raygen_uniform(uv, pose, intrinsics, t_vals, n_samples, near, far, far_per_ray=None, u_coarse=None):
    n = uv.shape[0]
    dev = uv.device
    p = RaygenParams(n, n_samples, int(pose.dim() == 2 and pose.shape[1] == 7), float(near), float(far))
    directions = torch.empty(n, 3, device=dev)
    ray_dirs = torch.empty(n, 3, device=dev)
    cam_loc = torch.empty(n, 3, device=dev)
    z = torch.empty(n, n_samples, device=dev)
    pts = torch.empty(n, n_samples, 3, device=dev)
    _check(load().vfn_raygen_uniform(C.byref(p), _ptr(uv, "uv"), _ptr(pose, "pose"), _ptr(intrinsics, "intrinsics"),
                                     _ptr(t_vals, "t_vals"), _ptr(far_per_ray, "far_per_ray"),
                                     _ptr(u_coarse, "u_coarse"), _ptr(directions, "directions"),
                                     _ptr(ray_dirs, "ray_dirs"), _ptr(cam_loc, "cam_loc"), _ptr(z, "z"),
                                     _ptr(pts, "points"), _stream()), "vfn_raygen_uniform")
    return directions, ray_dirs, cam_loc, z, pts


def uniform_sample(directions, cam_loc, t_vals, n_samples: int, near: float, far: float, far_per_ray=None, u=None,
                   want_points: bool = True):
    """UniformSampler.get_z_vals / RaySampler.sample on given directions[N,3] / cam_loc[N,3] -> (z[N,S], points[N,S,3] | None)."""
    n = directions.shape[0]
    dev = directions.device
    z = torch.empty(n, n_samples, device=dev)
    pts = torch.empty(n, n_samples, 3, device=dev) if want_points else None
    _check(load().vfn_uniform_sample(C.c_int32(n), C.c_int32(n_samples), C.c_float(near), C.c_float(far),
                                     _ptr(directions, "directions"), _ptr(cam_loc, "cam_loc"), _ptr(t_vals, "t_vals"),
                                     _ptr(far_per_ray, "far_per_ray"), _ptr(u, "u"), _ptr(z, "z_vals"), _ptr(pts, "points"),
                                     _stream()), "vfn_uniform_sample")
    return z, pts


def _ptr3(tensors, name: str):
    arr = (C.c_void_p * 3)()
    for k in range(3):
        t = tensors[k] if k < len(tensors) else None
        arr[k] = _ptr(t, f"{name}[{k}]").value if t is not None else None
    return arr


def vf_loss_workspace(dev) -> torch.Tensor:
    return torch.empty(int(load().vfn_vf_loss_workspace_bytes()) // 4, device=dev)


def vf_loss_fwd(lp: LossParams, rgb, rgb_gt, depth, depth_gt, normals, points, sup_pred, sup_gt, workspace) -> torch.Tensor:
    """-> out[8] on the device: five terms, 0, weighted total, supervision rows (csrc/vfn_loss.hip)."""
    out = torch.empty(8, device=workspace.device)
    _check(load().vfn_vf_loss_fwd(C.byref(lp), _ptr(rgb, "rgb"), _ptr(rgb_gt, "rgb_gt"), _ptr(depth, "depth"), _ptr(depth_gt, "depth_gt"),
                                  _ptr(normals, "normals"), _ptr(points, "points"), _ptr3(sup_pred, "sup_pred"), _ptr3(sup_gt, "sup_gt"),
                                  _ptr(workspace, "workspace"), _ptr(out, "out_terms"), _stream()), "vfn_vf_loss_fwd")
    return out


def vf_loss_bwd(lp: LossParams, rgb, rgb_gt, depth, depth_gt, normals, points, sup_pred, sup_gt, workspace, grad_out, d_rgb, d_depth,
                d_normals, d_sup) -> None:
    _check(load().vfn_vf_loss_bwd(C.byref(lp), _ptr(rgb, "rgb"), _ptr(rgb_gt, "rgb_gt"), _ptr(depth, "depth"), _ptr(depth_gt, "depth_gt"),
                                  _ptr(normals, "normals"), _ptr(points, "points"), _ptr3(sup_pred, "sup_pred"), _ptr3(sup_gt, "sup_gt"),
                                  _ptr(workspace, "workspace"), _ptr(grad_out, "grad_out"), _ptr(d_rgb, "d_rgb"), _ptr(d_depth, "d_depth"),
                                  _ptr(d_normals, "d_normals"), _ptr3(d_sup, "d_sup"), _stream()), "vfn_vf_loss_bwd")


def merge_sort_depths(z: torch.Tensor, extra: torch.Tensor, directions=None, cam_loc=None):
    """sort(cat(z[N,S], extra[N,E]), dim=1) per ray on the device (+ the points along the rays when directions / cam_loc are given)
    -> (z_out[N,S+E], points[N,S+E,3] | None)."""
    n, s = z.shape
    e = extra.shape[1]
    out = torch.empty(n, s + e, device=z.device)
    pts = torch.empty(n, s + e, 3, device=z.device) if directions is not None else None
    _check(load().vfn_merge_sort_depths(_ptr(z, "z_vals"), _ptr(extra, "extra"), C.c_int32(n), C.c_int32(s), C.c_int32(e),
                                        _ptr(directions, "directions"), _ptr(cam_loc, "cam_loc"), _ptr(out, "z_out"), _ptr(pts, "points"),
                                        _stream()), "vfn_merge_sort_depths")
    return out, pts


def rows_argmax(w: torch.Tensor) -> torch.Tensor:
    """First-maximum index of every row (torch.argmax(w, dim=-1) semantics) -> int64 [rows]."""
    rows, cols = w.shape
    out = torch.empty(rows, dtype=torch.int64, device=w.device)
    _check(load().vfn_rows_argmax(_ptr(w, "w"), C.c_int32(rows), C.c_int32(cols), _ptr(out, "out", torch.int64), _stream()),
           "vfn_rows_argmax")
    return out


def ray_density_sigma_bwd(dp: DensityParams, normals, ray_dirs, z_vals, scalars, d_sigma, d_normals, d_scalars) -> None:
    n, s = z_vals.shape
    dp.n_rays, dp.n_samples = n, s
    _check(load().vfn_ray_density_sigma_bwd(C.byref(dp), _ptr(normals, "normals"), _ptr(ray_dirs, "ray_dirs"),
                                            _ptr(z_vals, "z_vals"), _ptr(scalars, "scalars"), _ptr(d_sigma, "d_sigma"),
                                            _ptr(d_normals, "d_normals"), _ptr(d_scalars, "d_scalars"), _stream()),
           "vfn_ray_density_sigma_bwd")


def render_workspace_bytes(rp: RenderParams) -> int:
    n = load().vfn_render_fwd_workspace_bytes(C.byref(rp))
    if n < 0:
        raise VfnError("vfn_render_fwd_workspace_bytes: bad sizes")
    return int(n)


def render_fwd(rp: RenderParams, vf_geom, vf_packed16, rn_geom, rn_packed16, uv, pose, intrinsics, t_vals, far_c, far_f, scalars,
               u_coarse, u_fine, u_add, workspace):
    """The whole gradient-free render() in one call (csrc/vfn_render.hip) -> dict of output tensors."""
    n, s_t = rp.n_rays, rp.n_coarse + rp.n_fine
    dev = uv.device
    out = dict(ray_dirs=torch.empty(n, 3, device=dev), z_vals=torch.empty(n, s_t, device=dev), points=torch.empty(n, s_t, 3, device=dev),
               normals=torch.empty(n * s_t, 3, device=dev), colors=torch.empty(n * s_t, 3, device=dev),
               weights=torch.empty(n, s_t, device=dev), rgb=torch.empty(n, 3, device=dev), depth=torch.empty(n, 1, device=dev))
    _check(load().vfn_render_fwd(C.byref(rp), C.byref(vf_geom), _ptr(vf_packed16, "vf_packed16", torch.uint8), C.byref(rn_geom),
                                 _ptr(rn_packed16, "rn_packed16", torch.uint8), _ptr(uv, "uv"), _ptr(pose, "pose"),
                                 _ptr(intrinsics, "intrinsics"), _ptr(t_vals, "t_vals"), _ptr(far_c, "far_coarse_per_ray"),
                                 _ptr(far_f, "far_fine_per_ray"), _ptr(scalars, "density_scalars"), _ptr(u_coarse, "u_coarse"),
                                 _ptr(u_fine, "u_fine"), _ptr(u_add, "u_add"), _ptr(workspace, "workspace", torch.uint8),
                                 _ptr(out["ray_dirs"], "ray_dirs"), _ptr(out["z_vals"], "z_vals"), _ptr(out["points"], "points"),
                                 _ptr(out["normals"], "normals"), _ptr(out["colors"], "colors"), _ptr(out["weights"], "weights"),
                                 _ptr(out["rgb"], "rgb"), _ptr(out["depth"], "depth"), _stream()), "vfn_render_fwd")
    return out


def vf_mlp_fwd(geom: NetGeom, packed, points, out_cols: int):
    m = points.shape[0]
    out = torch.empty(m, out_cols, device=points.device)
    _check(load().vfn_vf_mlp_fwd(C.byref(geom), _ptr(packed, "packed"), _ptr(points, "points"), C.c_int64(m),
                                 C.c_int32(out_cols), _ptr(out, "out"), _stream()), "vfn_vf_mlp_fwd")
    return out


def render_mlp_fwd(geom: NetGeom, packed, points, normals, view_dirs, feats):
    m = points.shape[0]
    colors = torch.empty(m, 3, device=points.device)
    _check(load().vfn_render_mlp_fwd(C.byref(geom), _ptr(packed, "packed"), _ptr(points, "points"),
                                     _ptr(normals, "normals"), _ptr(view_dirs, "view_dirs"), _ptr(feats, "feats"),
                                     C.c_int64(m), _ptr(colors, "colors"), _stream()), "vfn_render_mlp_fwd")
    return colors


def vf_render_fused_fwd(vf_geom, vf_packed, rn_geom, rn_packed, points, ray_dirs, samples_per_ray: int,
                        want_feats: bool = False):
    m = points.shape[0]
    dev = points.device
    normals = torch.empty(m, 3, device=dev)
    colors = torch.empty(m, 3, device=dev)
    feats = torch.empty(m, HIDDEN, device=dev) if want_feats else None
    _check(load().vfn_vf_render_fused_fwd(C.byref(vf_geom), _ptr(vf_packed, "vf_packed"), C.byref(rn_geom),
                                          _ptr(rn_packed, "rn_packed"), _ptr(points, "points"),
                                          _ptr(ray_dirs, "ray_dirs"), C.c_int64(m), C.c_int32(samples_per_ray),
                                          _ptr(normals, "normals"), _ptr(colors, "colors"), _ptr(feats, "feats"),
                                          _stream()), "vfn_vf_render_fused_fwd")
    return normals, colors, feats


def ray_density_weights(dp: DensityParams, normals, ray_dirs, z_vals, scalars, colors=None, want_sigma=True,
                        want_weights=True, want_argmax=False):
    n, s = z_vals.shape
    dev = z_vals.device
    dp.n_rays, dp.n_samples = n, s
    sigma = torch.empty(n, s, device=dev) if want_sigma else None
    weights = torch.empty(n, s, device=dev) if want_weights else None
    argmax = torch.empty(n, dtype=torch.int64, device=dev) if want_argmax else None
    rgb = torch.empty(n, 3, device=dev) if colors is not None else None
    depth = torch.empty(n, 1, device=dev) if colors is not None else None
    _check(load().vfn_ray_density_weights(C.byref(dp), _ptr(normals, "normals"), _ptr(ray_dirs, "ray_dirs"),
                                          _ptr(z_vals, "z_vals"), _ptr(scalars, "density_scalars"),
                                          _ptr(colors, "colors"), _ptr(sigma, "sigma"), _ptr(weights, "weights"),
                                          _ptr(argmax, "argmax", torch.int64), _ptr(rgb, "rgb"),
                                          _ptr(depth, "depth"), _stream()), "vfn_ray_density_weights")
    return sigma, weights, argmax, rgb, depth


def range_fine_sample(z_coarse, argmax, directions, cam_loc, n_fine, near, far, fine_range, u_add, u_fine=None,
                      far_per_ray=None):
    n, sc = z_coarse.shape
    dev = z_coarse.device
    step = 2 * fine_range / (n_fine - 1)            # Python double arithmetic, as ray_sampler.py:279
    span = (far - near) if far_per_ray is None else 0.0
    p = FineParams(n, sc, n_fine, float(near), float(far) if far_per_ray is None else 0.0, float(fine_range),
                   float(step), float(span))
    z = torch.empty(n, sc + n_fine, device=dev)
    pts = torch.empty(n, sc + n_fine, 3, device=dev)
    _check(load().vfn_range_fine_sample(C.byref(p), _ptr(z_coarse, "z_coarse"), _ptr(argmax, "argmax", torch.int64),
                                        _ptr(directions, "directions"), _ptr(cam_loc, "cam_loc"),
                                        _ptr(far_per_ray, "far_per_ray"), _ptr(u_fine, "u_fine"), _ptr(u_add, "u_add"),
                                        _ptr(z, "z_vals"), _ptr(pts, "points"), _stream()), "vfn_range_fine_sample")
    return z, pts


def block_rows(m: int) -> int:
    """Rows a block buffer needs for m stored rows: whole groups of 32 (vfn_vf_feat16_fwd)."""
    return (m + 31) & ~31


def range_fine_sample_indexed(z_coarse, argmax, directions, cam_loc, n_fine, near, far, fine_range, u_add, u_fine=None,
                              far_per_ray=None, new_row0: Optional[int] = None, want_dst: bool = False):
    """range_fine_sample plus src[N,S_t] (int32: the stored row every sorted sample comes from; the new samples' rows start
    at ``new_row0``, default N*S_c) and new_points[N,N_f,3]; with ``want_dst`` also the inverse map dst[new_row0 + N*N_f]
    (int32, -1 for rows no sample comes from)."""
    n, sc = z_coarse.shape
    dev = z_coarse.device
    step = 2 * fine_range / (n_fine - 1)
    span = (far - near) if far_per_ray is None else 0.0
    p = FineParams(n, sc, n_fine, float(near), float(far) if far_per_ray is None else 0.0, float(fine_range),
                   float(step), float(span))
    z = torch.empty(n, sc + n_fine, device=dev)
    pts = torch.empty(n, sc + n_fine, 3, device=dev)
    src = torch.empty(n, sc + n_fine, dtype=torch.int32, device=dev)
    new_pts = torch.empty(n, n_fine, 3, device=dev)
    row0 = n * sc if new_row0 is None else int(new_row0)
    dst = None
    if want_dst:
        rows = row0 + n * n_fine
        dst = torch.empty(rows, dtype=torch.int32, device=dev) if row0 == n * sc else \
            torch.full((rows,), -1, dtype=torch.int32, device=dev)
    _check(load().vfn_range_fine_sample_indexed(C.byref(p), _ptr(z_coarse, "z_coarse"), _ptr(argmax, "argmax", torch.int64),
                                                _ptr(directions, "directions"), _ptr(cam_loc, "cam_loc"),
                                                _ptr(far_per_ray, "far_per_ray"), _ptr(u_fine, "u_fine"),
                                                _ptr(u_add, "u_add"), _ptr(z, "z_vals"), _ptr(pts, "points"),
                                                _ptr(src, "src", torch.int32), _ptr(new_pts, "new_points"),
                                                _ptr(dst, "dst", torch.int32), C.c_int64(row0), _stream()),
           "vfn_range_fine_sample_indexed")
    return (z, pts, src, new_pts, dst) if want_dst else (z, pts, src, new_pts)


def fill_uniform(out: torch.Tensor, seed: int, offset: int) -> torch.Tensor:
    _check(load().vfn_fill_uniform(_ptr(out, "out"), C.c_int64(out.numel()), C.c_uint64(seed & (2 ** 64 - 1)),
                                   C.c_uint64(offset & (2 ** 64 - 1)), _stream()), "vfn_fill_uniform")
    return out


def sample_sphere_shell(n: int, r_min: float, r_max: float, centroid: torch.Tensor, inward: bool, seed: int = 0, offset: int = 0,
                        u: Optional[torch.Tensor] = None):
    dev = centroid.device
    pts = torch.empty(n, 3, device=dev)
    gt = torch.empty(n, 3, device=dev)
    _check(load().vfn_sample_sphere_shell(C.c_int64(n), C.c_float(r_min), C.c_float(r_max), _ptr(centroid, "centroid"),
                                          C.c_int32(1 if inward else 0), _ptr(u, "u"), C.c_uint64(seed & (2 ** 64 - 1)),
                                          C.c_uint64(offset & (2 ** 64 - 1)), _ptr(pts, "points"), _ptr(gt, "gt"), _stream()),
           "vfn_sample_sphere_shell")
    return pts, gt


# ------------------------------------------------------------------------------------------------
# training path
# ------------------------------------------------------------------------------------------------
AUX_K = 40


def vf_mlp_fwd_train(geom: NetGeom, packed, points, out_cols: int, saved, aux_vf):
    m = points.shape[0]
    out = torch.empty(m, out_cols, device=points.device)
    _check(load().vfn_vf_mlp_fwd_train(C.byref(geom), _ptr(packed, "packed"), _ptr(points, "points"), C.c_int64(m),
                                       C.c_int32(out_cols), _ptr(out, "out"), _ptr(saved, "saved"),
                                       _ptr(aux_vf, "aux_vf"), _stream()), "vfn_vf_mlp_fwd_train")
    return out


def vf_render_fused_fwd_train(vf_geom, vf_packed, rn_geom, rn_packed, points, ray_dirs, samples_per_ray, saved, aux_vf,
                              aux_rn):
    m = points.shape[0]
    dev = points.device
    normals = torch.empty(m, 3, device=dev)
    colors = torch.empty(m, 3, device=dev)
    _check(load().vfn_vf_render_fused_fwd_train(C.byref(vf_geom), _ptr(vf_packed, "vf_packed"), C.byref(rn_geom),
                                                _ptr(rn_packed, "rn_packed"), _ptr(points, "points"),
                                                _ptr(ray_dirs, "ray_dirs"), C.c_int64(m), C.c_int32(samples_per_ray),
                                                _ptr(normals, "normals"), _ptr(colors, "colors"), _ptr(saved, "saved"),
                                                _ptr(aux_vf, "aux_vf"), _ptr(aux_rn, "aux_rn"), _stream()),
           "vfn_vf_render_fused_fwd_train")
    return normals, colors


def mlp_bwd_chain(vf_geom, vf_packed, vf_packed_bwd, rn_geom, rn_packed, rn_packed_bwd, saved, dy, d_colors, colors,
                  d_vec, vec, d_feats, vec_stride: int, n_points: int, dz_rgb, dz_vec):
    rn = C.byref(rn_geom) if rn_geom is not None else None
    _check(load().vfn_mlp_bwd_chain(C.byref(vf_geom), _ptr(vf_packed, "vf_packed"), _ptr(vf_packed_bwd, "vf_packed_bwd"),
                                    rn, _ptr(rn_packed, "rn_packed"), _ptr(rn_packed_bwd, "rn_packed_bwd"),
                                    _ptr(saved, "saved"), _ptr(dy, "dy"), _ptr(d_colors, "d_colors"),
                                    _ptr(colors, "colors"), _ptr(d_vec, "d_vec"), _ptr(vec, "vec"),
                                    _ptr(d_feats, "d_feats"), C.c_int32(vec_stride), C.c_int64(n_points),
                                    _ptr(dz_rgb, "dz_rgb"), _ptr(dz_vec, "dz_vec"), _stream()), "vfn_mlp_bwd_chain")


def weight_grad_partials(shape: int, dy, ld_dy: int, n_valid: int, x, ld_x: int, k_valid: int, n_points: int,
                         groups: int, dw_part, db_part=None, x_f16: bool = False):
    _check(load().vfn_weight_grad_partials(C.c_int32(shape), _ptr(dy, "dy"), C.c_int32(ld_dy), C.c_int32(n_valid),
                                           _ptr(x, "x"), C.c_int32(ld_x), C.c_int32(k_valid), C.c_int64(n_points),
                                           C.c_int32(groups), _ptr(dw_part, "dw_part"), _ptr(db_part, "db_part"),
                                           C.c_int32(int(x_f16)), _stream()), "vfn_weight_grad_partials")


def packed_bwd16_size(kind: int, geom: NetGeom) -> int:
    n = load().vfn_packed_bwd16_size(kind, C.byref(geom))
    if n < 0:
        raise VfnError(f"vfn_packed_bwd16_size failed (status {n}): {load().vfn_last_error().decode()}")
    return int(n)


def pack_weights_bwd16(kind: int, geom: NetGeom, layers: Sequence[dict], packed: torch.Tensor, round_hi: bool = False) -> None:
    """``round_hi``: hi planes rounded to nearest instead of truncated — the pack of the single-product chain (DY_P1)."""
    _check(load().vfn_pack_weights_bwd16_mode(kind, C.byref(geom), _layer_array(geom, layers), C.c_int32(int(bool(round_hi))),
                                              _ptr(packed, "packed", torch.uint8), _stream()), "vfn_pack_weights_bwd16")


def relu_sign_words(saved: torch.Tensor) -> torch.Tensor:
    """saved[slots, M, 256] -> the sign-bit words the f16x3 training forwards write next to it: int32 [slots, M, 2, 4] (per slot,
    point and lane half g: tile t -> half t & 1 of dword t >> 1, bit r <-> column 32 t + (r & 3) + 8 (r >> 2) + 4 g).  A torch
    restatement for callers that build a workspace by hand (tests)."""
    dev = saved.device
    r = torch.arange(16, device=dev)
    col = (32 * torch.arange(8, device=dev)[None, :, None] + (r & 3)[None, None, :] + 8 * (r >> 2)[None, None, :]
           + 4 * torch.arange(2, device=dev)[:, None, None])                     # [g, t, r]
    bits = (saved[:, :, col.reshape(-1)] > 0).view(saved.shape[0], saved.shape[1], 2, 8, 16).to(torch.int64)
    half = (bits << r).sum(-1)                                                   # [slots, M, g, t] 16-bit fields
    words = half[..., 0::2] | (half[..., 1::2] << 16)                           # [slots, M, g, 4]
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


def unpack_sign_words(words: torch.Tensor) -> torch.Tensor:
    """The inverse view of relu_sign_words: int32 [slots, M, 2, 4] -> bool [slots, M, 256] (True where the saved ReLU output
    was positive) — exactly the masks the bf16 chain applies."""
    dev = words.device
    w = words.to(torch.int64) & 0xffffffff
    r = torch.arange(16, device=dev)
    half = torch.stack([w & 0xffff, w >> 16], dim=-1).reshape(*words.shape[:3], 8)       # [slots, M, g, t]
    bits = ((half[..., None] >> r) & 1).bool()                                            # [slots, M, g, t, r]
    col = (32 * torch.arange(8, device=dev)[None, :, None] + (r & 3)[None, None, :] + 8 * (r >> 2)[None, None, :]
           + 4 * torch.arange(2, device=dev)[:, None, None]).reshape(-1)                  # [g, t, r] -> column
    out = torch.zeros(words.shape[0], words.shape[1], 256, dtype=torch.bool, device=dev)
    out[:, :, col] = bits.reshape(words.shape[0], words.shape[1], -1)
    return out


def mlp_bwd_chain_bf16(vf_geom, vf_packed_bwd16, vf_head_w, rn_geom, rn_packed_bwd16, rn_head_w, saved, masks, dy, d_colors, colors,
                       d_vec, vec, d_feats, vec_stride: int, n_points: int, dz_rgb, dz_vec):
    rn = C.byref(rn_geom) if rn_geom is not None else None
    _check(load().vfn_mlp_bwd_chain_bf16(C.byref(vf_geom), _ptr(vf_packed_bwd16, "vf_packed_bwd16", torch.uint8),
                                         _ptr(vf_head_w, "vf_head_w"), rn,
                                         _ptr(rn_packed_bwd16, "rn_packed_bwd16", torch.uint8), _ptr(rn_head_w, "rn_head_w"),
                                         _ptr(saved, "saved"), _ptr(masks, "masks", torch.int32), _ptr(dy, "dy"),
                                         _ptr(d_colors, "d_colors"), _ptr(colors, "colors"), _ptr(d_vec, "d_vec"), _ptr(vec, "vec"),
                                         _ptr(d_feats, "d_feats"), C.c_int32(vec_stride), C.c_int64(n_points),
                                         _ptr(dz_rgb, "dz_rgb"), _ptr(dz_vec, "dz_vec"), _stream()), "vfn_mlp_bwd_chain_bf16")


# ------------------------------------------------------------------------------------------------
# fragment-ordered training workspace (include/vfn.h, "FRAGMENT-ORDERED training workspace")
# ------------------------------------------------------------------------------------------------
WS_F16, WS_FRAG, WS_P1 = 1, 2, 4             # flags of the f16x3 training forwards (save_f16 argument); WS_P1: single-product arithmetic
DY_FRAG, DY_BF16, DY_F16S, DY_P1 = 2, 4, 8, 16   # flags of the bf16 chain (dy_flags argument): fragment order, bf16, scaled f16, single product
DYF_FRAG32, DYF_FRAGBF16, DYF_DZ4, DYF_FRAGF16S = 0, 1, 2, 3  # operand forms of weight_grad_frag (3: tile-scaled f16)
XF_FRAG32, XF_FRAG16, XF_ROWS32, XF_AUX40 = 0, 1, 2, 3
GROUP_FLOATS = 8192                          # one group of 32 points = 32 KiB


def frag_groups(m: int) -> int:
    return (m + 31) // 32


def frag_to_rows(slot: torch.Tensor, m: int, dtype=torch.float32) -> torch.Tensor:
    """One fragment-ordered slot (flat fp32 buffer of frag_groups(m) * 8192 floats) -> the row-major [m, 256] matrix it
    holds.  ``dtype``: float32, float16 (activations stored as f16) or bfloat16 (gradients stored as bf16) — the 16-bit forms
    use the first half of every group.  Test / debugging helper: the kernels never need the row-major form."""
    g = frag_groups(m)
    flat = slot.reshape(-1)[: g * GROUP_FLOATS].view(g, GROUP_FLOATS)
    if dtype != torch.float32:
        flat = flat.view(dtype)[:, :GROUP_FLOATS]               # [g, 8192] 16-bit values = the first 16 KiB of each group
    # [group][tile t][quad q][lane half gg][point i][4 values]  ->  [group][point i][t][q][gg][4]
    rows = flat.reshape(g, 8, 4, 2, 32, 4).permute(0, 4, 1, 2, 3, 5).reshape(g * 32, 256)
    return rows[:m].float()


def rows_to_frag(rows: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """The inverse of frag_to_rows: [m, 256] -> one fragment-ordered slot (flat fp32 buffer, padded points zero)."""
    m = rows.shape[0]
    g = frag_groups(m)
    pad = torch.zeros(g * 32, 256, device=rows.device, dtype=torch.float32)
    pad[:m] = rows.float()
    frag = pad.reshape(g, 32, 8, 4, 2, 4).permute(0, 2, 3, 4, 1, 5).reshape(g, GROUP_FLOATS)
    out = torch.zeros(g, GROUP_FLOATS, device=rows.device, dtype=torch.float32)
    if dtype == torch.float32:
        out.copy_(frag)
    else:
        out.view(dtype)[:, :GROUP_FLOATS] = frag.to(dtype)
    return out.reshape(-1)


F16S_EXP_OFF = 16384     # byte offset of the 8 x 64 exponent bytes inside a group of a scaled f16 gradient slot (dy form 3)


def rows_to_frag_f16s(rows: torch.Tensor) -> torch.Tensor:
    """[m, 256] fp32 -> one fragment-ordered slot in the scaled f16 form the bf16 chain writes with DY_F16S (csrc/vfn_dwf.hip,
    "dY form 3"): per group, 32-column tile t and lane (point i, column half gg: the 16 columns 8 q + 4 gg + c of the tile),
    f16(v * 2^k) with max |v| * 2^k in [2^14, 2^15) and the byte k + 113 (255: all 16 values zero) at F16S_EXP_OFF + 64 t + lane.
    Test helper (the chain is the producer)."""
    m = rows.shape[0]
    g = frag_groups(m)
    pad = torch.zeros(g * 32, 256, device=rows.device, dtype=torch.float32)
    pad[:m] = rows.float()
    v = pad.reshape(g, 32, 8, 4, 2, 4)                                       # [group][point i][tile t][quad q][half gg][c]
    mx = v.abs().amax(dim=(3, 5))                                            # [g, i, t, gg]
    biased = (mx.view(torch.int32) >> 23) & 0xff
    b = torch.where(biased == 0, torch.full_like(biased, 255), (254 - biased).clamp(0, 239))
    scale = ((b.clamp(max=239) + 14) << 23).view(torch.float32)
    scale = torch.where(b == 255, torch.zeros_like(scale), scale)
    scaled = v * scale[:, :, :, None, :, None]
    frag = scaled.permute(0, 2, 3, 4, 1, 5).reshape(g, GROUP_FLOATS)          # [group][t][q][gg][i][c]
    out = torch.zeros(g, GROUP_FLOATS, device=rows.device, dtype=torch.float32)
    out.view(torch.float16)[:, :GROUP_FLOATS] = frag.to(torch.float16)
    out.view(torch.uint8)[:, F16S_EXP_OFF:F16S_EXP_OFF + 512] = b.permute(0, 2, 3, 1).reshape(g, 512).to(torch.uint8)   # [t][lane = 32 gg + i]
    return out.reshape(-1)


def frag_f16s_to_rows(slot: torch.Tensor, m: int) -> torch.Tensor:
    """The row-major [m, 256] fp32 values a scaled f16 gradient slot holds (test / debugging helper)."""
    g = frag_groups(m)
    flat = slot.reshape(-1)[: g * GROUP_FLOATS].view(g, GROUP_FLOATS)
    b = flat.view(torch.uint8)[:, F16S_EXP_OFF:F16S_EXP_OFF + 512].to(torch.int32).reshape(g, 8, 2, 32)     # [t][gg][i]
    inv = ((240 - b.clamp(max=239)) << 23).view(torch.float32)
    inv = torch.where(b == 255, torch.zeros_like(inv), inv)
    vals = flat.view(torch.float16)[:, :GROUP_FLOATS].float().reshape(g, 8, 4, 2, 32, 4) * inv[:, :, None, :, :, None]
    rows = vals.permute(0, 4, 1, 2, 3, 5).reshape(g * 32, 256)
    return rows[:m]


def weight_grad_frag(shape: int, dy, dy_form: int, x, x_form: int, n_points: int, groups: int, dw_part, db_part=None) -> None:
    _check(load().vfn_weight_grad_frag(C.c_int32(shape), _ptr(dy, "dy"), C.c_int32(dy_form), _ptr(x, "x"), C.c_int32(x_form),
                                       C.c_int64(n_points), C.c_int32(groups), _ptr(dw_part, "dw_part"), _ptr(db_part, "db_part"),
                                       _stream()), "vfn_weight_grad_frag")


class WgradLayer(C.Structure):
    """mirrors vfn_wgrad_layer"""
    _fields_ = [(n, C.c_void_p) for n in ("weight", "bias", "bn_weight", "bn_var", "bn_mean", "g_weight", "g_bias", "g_bn_weight", "g_bn_bias")]


def weight_grad_groups(n_points: int) -> int:
    return int(load().vfn_weight_grad_groups(C.c_int64(n_points)))


def net_weight_grads_scratch_bytes(kind: int, geom, n_points: int) -> int:
    n = int(load().vfn_net_weight_grads_scratch_bytes(C.c_int32(kind), C.byref(geom), C.c_int64(n_points)))
    if n < 0:
        _check(n, "vfn_net_weight_grads_scratch_bytes")
    return n


WGRAD_LAYERS, WGRAD_FEATURES, WGRAD_HEAD = 1, 2, 4


def net_weight_grads_frag(kind: int, geom, layer_table, saved, slot_index: int, dy, slot_floats: int, dy_form: int, x_form: int, feats,
                          aux, dz_head, n_points: int, with_features: bool, accumulate: bool, scratch, first_point: int = 0,
                          parts: Optional[int] = None) -> None:
    """All weight-gradient launches of one net + the un-fold, from C (csrc/vfn_wgrad.hip).  ``layer_table``: a WgradLayer array
    (parameter and gradient pointers per reference layer); ``saved`` / ``dy``: [slots, slot_floats] workspaces, ``slot_index`` the
    net's first slot in both."""
    for t, name in ((saved, "saved"), (dy, "dy")):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == slot_floats):
            raise VfnError(f"{name}: expected a contiguous CUDA float32 [slots, {slot_floats}] workspace")
    # ``first_point`` (a multiple of 32): the products run over points first_point .. first_point + n_points - 1 of the workspace;
    # ``parts``: WGRAD_* mask (default: everything, or everything but the feature block when ``with_features`` is False)
    if first_point % 32:
        raise VfnError(f"first_point = {first_point} is not a multiple of 32")
    off = slot_index * slot_floats * 4 + (first_point // 32) * GROUP_FLOATS * 4
    if parts is None:
        parts = (WGRAD_LAYERS | WGRAD_FEATURES | WGRAD_HEAD) if with_features else (WGRAD_LAYERS | WGRAD_HEAD)

    def at(t, row_floats):
        return None if t is None else C.c_void_p(t.data_ptr() + first_point * row_floats * 4)

    for t, name in ((feats, "feats"), (aux, "aux"), (dz_head, "dz_head")):
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise VfnError(f"{name}: expected a contiguous CUDA float32 tensor")
    _check(load().vfn_net_weight_grads_frag_part(C.c_int32(kind), C.byref(geom), layer_table, C.c_void_p(saved.data_ptr() + off),
                                                 C.c_void_p(dy.data_ptr() + off), C.c_int64(slot_floats * 4), C.c_int32(dy_form), C.c_int32(x_form),
                                                 at(feats, HIDDEN), at(aux, AUX_K), at(dz_head, 4), C.c_int64(n_points),
                                                 C.c_uint32(parts), C.c_int32(int(accumulate)), _ptr(scratch, "scratch", torch.uint8),
                                                 _stream()), "vfn_net_weight_grads_frag")


def mlp_bwd_chain_bf16_ws(vf_geom, vf_packed_bwd16, vf_head_w, rn_geom, rn_packed_bwd16, rn_head_w, feats, masks, dy, dy_flags: int,
                          d_colors, colors, d_vec, vec, d_feats, vec_stride: int, n_points: int, dz_rgb, dz_vec,
                          ws_first: int = 0, ws_points: Optional[int] = None):
    """``ws_first`` / ``ws_points``: the launch's points are points ws_first .. of a workspace (feats, masks, dy, dz_rgb, dz_vec)
    sized for ws_points; the per-sample inputs (d_colors, colors, d_vec, vec, d_feats) stay launch-local."""
    rn = C.byref(rn_geom) if rn_geom is not None else None
    _check(load().vfn_mlp_bwd_chain_bf16_ws_at(C.byref(vf_geom), _ptr(vf_packed_bwd16, "vf_packed_bwd16", torch.uint8),
                                               _ptr(vf_head_w, "vf_head_w"), rn,
                                               _ptr(rn_packed_bwd16, "rn_packed_bwd16", torch.uint8), _ptr(rn_head_w, "rn_head_w"),
                                               _ptr(feats, "feats"), _ptr(masks, "masks", torch.int32), _ptr(dy, "dy"), C.c_int32(dy_flags),
                                               _ptr(d_colors, "d_colors"), _ptr(colors, "colors"), _ptr(d_vec, "d_vec"), _ptr(vec, "vec"),
                                               _ptr(d_feats, "d_feats"), C.c_int32(vec_stride), C.c_int64(n_points),
                                               _ptr(dz_rgb, "dz_rgb"), _ptr(dz_vec, "dz_vec"), C.c_int64(ws_first),
                                               C.c_int64(n_points if ws_points is None else ws_points), _stream()), "vfn_mlp_bwd_chain_bf16_ws")


# ------------------------------------------------------------------------------------------------
# optimizer side over one flat buffer (csrc/vfn_adam.hip)
# ------------------------------------------------------------------------------------------------
def _regions(regions):
    n = len(regions)
    starts = (C.c_int64 * n)(*[int(r[0]) for r in regions])
    ends = (C.c_int64 * n)(*[int(r[1]) for r in regions])
    mults = (C.c_int32 * n)(*[int(r[2]) for r in regions])
    return n, starts, ends, mults


def flat_clip_workspace(device) -> torch.Tensor:
    return torch.zeros(int(load().vfn_flat_clip_workspace_bytes()), dtype=torch.uint8, device=device)


def flat_clip_grad_norm(flat_grad: torch.Tensor, regions, max_norm: float, workspace: torch.Tensor, out2: torch.Tensor) -> None:
    """regions: [(start, end, mult)]; out2[0] <- total norm, out2[1] <- clip coefficient; flat_grad scaled in place."""
    n, starts, ends, mults = _regions(regions)
    _check(load().vfn_flat_clip_grad_norm(_ptr(flat_grad, "flat_grad"), C.c_int64(flat_grad.numel()), C.c_int32(n), starts, ends, mults,
                                          C.c_float(max_norm), _ptr(workspace, "workspace", torch.uint8), _ptr(out2, "out2"), _stream()),
           "vfn_flat_clip_grad_norm")


def flat_adam_step(param, grad, exp_avg, exp_avg_sq, regions, step_size, bc2_sqrt, beta1, beta2, eps, weight_decay) -> None:
    n, starts, ends, mults = _regions(regions)
    ss = (C.c_double * (2 * n))(*[float(x) for x in step_size])
    bc = (C.c_double * (2 * n))(*[float(x) for x in bc2_sqrt])
    _check(load().vfn_flat_adam_step(_ptr(param, "param"), _ptr(grad, "grad"), _ptr(exp_avg, "exp_avg"), _ptr(exp_avg_sq, "exp_avg_sq"),
                                     C.c_int64(param.numel()), C.c_int32(n), starts, ends, mults, ss, bc, C.c_double(beta1), C.c_double(beta2),
                                     C.c_double(eps), C.c_double(weight_decay), _stream()), "vfn_flat_adam_step")


class UnfoldEntry(C.Structure):
    """mirrors vfn_unfold_entry"""
    _fields_ = [(n, C.c_void_p) for n in ("dw_act", "dw_aux", "db", "w", "b_lin", "bn_w", "bn_var", "bn_mean", "g_w", "g_b",
                                          "g_bn_w", "g_bn_b")] + \
               [(n, C.c_int32) for n in ("rows", "row_off", "in_dim", "slab_rows", "act_c0", "act_nc", "aux_c0", "aux_nc")] + \
               [("scale", C.c_float)] + [(n, C.c_int32) for n in ("groups_act", "groups_aux", "groups_db")]


def unfold_weight_grads(entries: Sequence[dict], groups: int, accumulate_mask: int = 0) -> None:
    """entries: dicts with the tensors / ints of vfn_unfold_entry (missing tensors = NULL); bit i of ``accumulate_mask``: entry i
    adds to its g_* tensors instead of overwriting them."""
    arr = (UnfoldEntry * len(entries))()
    for i, e in enumerate(entries):
        for name, _ in UnfoldEntry._fields_[:12]:
            setattr(arr[i], name, _ptr(e.get(name), name))
        for name, _ in UnfoldEntry._fields_[12:20]:
            setattr(arr[i], name, int(e.get(name, 0)))
        arr[i].scale = float(e.get("scale", 1.0))
    _check(load().vfn_unfold_weight_grads_acc(arr, C.c_int32(len(entries)), C.c_int32(groups), C.c_uint32(accumulate_mask), _stream()),
           "vfn_unfold_weight_grads")


def weight_grad_partials_bf16(dy, x, n_points: int, groups: int, dw_part, db_part=None, x_f16: bool = False):
    """shape-0 weight_grad_partials (256 x 256, every column valid) on the bf16 matrix cores (split operands)."""
    _check(load().vfn_weight_grad_partials_bf16(_ptr(dy, "dy"), _ptr(x, "x"), C.c_int64(n_points), C.c_int32(groups),
                                                _ptr(dw_part, "dw_part"), _ptr(db_part, "db_part"), C.c_int32(int(x_f16)), _stream()),
           "vfn_weight_grad_partials_bf16")


def weight_grad_partials_bf16_cols(dy, x, n_points: int, groups: int, dw_part, db_part=None):
    """The same over 256 columns of wider matrices (``Cols`` views: 16-byte aligned column offsets, leading dimensions >= 256)."""
    dy, x = _cols(dy), _cols(x)
    _check(load().vfn_weight_grad_partials_bf16_ld(dy.ptr, C.c_int32(dy.ld), x.ptr, C.c_int32(x.ld), C.c_int64(n_points), C.c_int32(groups),
                                                   _ptr(dw_part, "dw_part"), _ptr(db_part, "db_part"), C.c_int32(0), _stream()),
           "vfn_weight_grad_partials_bf16_ld")


def weight_grad_partials_bf16_fold(dy, z_prev, coef_prev: torch.Tensor, n_prev: int, post_prev: float, n_points: int, groups: int, dw_part, db_part=None):
    """dW = dY^T act(z_prev) over 256 columns with the activation formed in the operand read (vfn_weight_grad_partials_bf16_fold)."""
    dy, z_prev = _cols(dy), _cols(z_prev)
    if coef_prev.numel() < 2 * n_prev:
        raise VfnError(f"weight_grad_partials_bf16_fold: coefficients of {coef_prev.numel()} floats for n_prev = {n_prev} (needs scale | shift rows)")
    _check(load().vfn_weight_grad_partials_bf16_fold(dy.ptr, C.c_int32(dy.ld), z_prev.ptr, C.c_int32(z_prev.ld), _ptr(coef_prev, "coef_prev"),
                                                     C.c_int32(n_prev), C.c_float(post_prev), C.c_int64(n_points), C.c_int32(groups),
                                                     _ptr(dw_part, "dw_part"), _ptr(db_part, "db_part"), _stream()),
           "vfn_weight_grad_partials_bf16_fold")


def ray_density_weights_bwd(dp: DensityParams, normals, ray_dirs, z_vals, scalars, colors, d_rgb, d_depth, d_weights,
                            d_normals, d_colors, d_scalars):
    n, s = z_vals.shape
    dp.n_rays, dp.n_samples = n, s
    _check(load().vfn_ray_density_weights_bwd(C.byref(dp), _ptr(normals, "normals"), _ptr(ray_dirs, "ray_dirs"),
                                              _ptr(z_vals, "z_vals"), _ptr(scalars, "scalars"), _ptr(colors, "colors"),
                                              _ptr(d_rgb, "d_rgb"), _ptr(d_depth, "d_depth"),
                                              _ptr(d_weights, "d_weights"), _ptr(d_normals, "d_normals"),
                                              _ptr(d_colors, "d_colors"), _ptr(d_scalars, "d_scalars"), _stream()),
           "vfn_ray_density_weights_bwd")


# ------------------------------------------------------------------------------------------------
# f16x3 inference kernels
# ------------------------------------------------------------------------------------------------
PACK16_STATS_WORDS = 64          # tail of an f16x3 pack: max |folded weight| per pack entry (include/vfn.h, "Range guard")
STATUS_ACT_SATURATED, STATUS_INPUT_SATURATED = 1, 2


def f16x3_set_status(word: Optional[torch.Tensor]) -> None:
    """Route the range reports of this thread's f16x3 launches into ``word`` (int32 device tensor, >= 1 element); None: off."""
    _check(load().vfn_f16x3_set_status(_ptr(word, "status_word", torch.int32)), "vfn_f16x3_set_status")


def train_step_workspace_bytes(params: "TrainStepParams", vf_geom: NetGeom, rn_geom: NetGeom) -> int:
    n = int(load().vfn_train_step_workspace_bytes(C.byref(params), C.byref(vf_geom), C.byref(rn_geom)))
    if n < 0:
        raise VfnError(f"vfn_train_step_workspace_bytes failed (status {n}): {load().vfn_last_error().decode()}")
    return n


def train_step(params: "TrainStepParams", io: "TrainStepIO") -> None:
    """One training step (or some of its phases) from C: vf_nerf_amd/stepengine.py fills the structs."""
    _check(load().vfn_train_step(C.byref(params), C.byref(io), _stream()), "vfn_train_step")


def train_step_workspace_layout(params: "TrainStepParams", vf_geom: NetGeom, rn_geom: NetGeom) -> List[int]:
    """[TWS_*]: byte offsets of the session form's regions inside the step workspace, and its counts."""
    out = (C.c_int64 * TWS_COUNT)()
    _check(load().vfn_train_step_workspace_layout(C.byref(params), C.byref(vf_geom), C.byref(rn_geom), out, TWS_COUNT), "vfn_train_step_workspace_layout")
    return [int(v) for v in out]


def train_step_supervision_points(params: "TrainStepParams", io: "TrainStepIO", inward: bool, r_min: float, r_max: float, cx: float, cy: float,
                                  cz: float, centroid_dev: Optional[torch.Tensor], row0: int, count: int, u: Optional[torch.Tensor], seed: int,
                                  offset: int) -> bool:
    """Session form: one supervision batch sampled into rows [row0, row0 + count) of the open step.  -> True when it ran on the step's side
    stream (pass it on to ``train_step_supervision_forward``)."""
    rc = load().vfn_train_step_supervision_points(C.byref(params), C.byref(io), 1 if inward else 0, float(r_min), float(r_max), float(cx), float(cy),
                                                  float(cz), _ptr(centroid_dev, "centroid"), row0, count, _ptr(u, "u"), C.c_uint64(seed & (2 ** 64 - 1)),
                                                  C.c_uint64(offset & (2 ** 64 - 1)), _stream())
    if rc < 0:
        _check(rc, "vfn_train_step_supervision_points")
    return rc == 1


def train_step_supervision_forward(params: "TrainStepParams", io: "TrainStepIO", row0: int, count: int, on_side: bool) -> None:
    """Session form: the vector-only saving forward over supervision rows [row0, pad32(row0 + count)) of the open step."""
    _check(load().vfn_train_step_supervision_forward(C.byref(params), C.byref(io), row0, count, 1 if on_side else 0, _stream()),
           "vfn_train_step_supervision_forward")


def train_step_supervision_backward(params: "TrainStepParams", io: "TrainStepIO", row0: int, count: int) -> None:
    """Session form: chain + weight gradients of supervision rows [row0, pad32(row0 + count)) alone (a backward pass that never reaches the render)."""
    _check(load().vfn_train_step_supervision_backward(C.byref(params), C.byref(io), row0, count, _stream()), "vfn_train_step_supervision_backward")


def f16x3_set_clock_probe(stamps: Optional[torch.Tensor]) -> None:
    """Route the per-workgroup clock stamps of this thread's gradient-free fused launches into ``stamps`` (int64 device tensor
    [slots, 2]: shader-clock cycles, 100 MHz ticks of workgroup b; csrc/vfn_mlp16.hip); None: off."""
    slots = 0 if stamps is None else stamps.numel() // 2
    _check(load().vfn_f16x3_set_clock_probe(_ptr(stamps, "stamps", torch.int64), slots), "vfn_f16x3_set_clock_probe")


def clock_ghz_from_stamps(stamps: torch.Tensor) -> Optional[dict]:
    """{median, min, max} shader clock in GHz over the workgroups that left a stamp (cycles / 100-MHz-ticks x 0.1)."""
    st = stamps.reshape(-1, 2).cpu().double()
    st = st[(st[:, 1] > 0) & (st[:, 0] > 0)]
    if st.shape[0] == 0:
        return None
    ghz = st[:, 0] / st[:, 1] * 0.1
    return {"median": round(float(ghz.median()), 4), "min": round(float(ghz.min()), 4), "max": round(float(ghz.max()), 4),
            "workgroups": int(st.shape[0]), "median_workgroup_us": round(float(st[:, 1].median()) / 100.0, 2)}


def pack16_size(kind: int, geom: NetGeom) -> int:
    n = load().vfn_pack16_size(kind, C.byref(geom))
    if n < 0:
        raise VfnError(f"unsupported network geometry: {load().vfn_last_error().decode()}")
    return int(n)


def pack16_weights(kind: int, geom: NetGeom, layers: Sequence[dict], packed16: torch.Tensor) -> None:
    _check(load().vfn_pack16_weights(kind, C.byref(geom), _layer_array(geom, layers), _ptr(packed16, "packed16", torch.uint8),
                                     _stream()), "vfn_pack16_weights")


def vf_mlp16_fwd(geom: NetGeom, packed16, points):
    m = points.shape[0]
    out = torch.empty(m, 3, device=points.device)
    _check(load().vfn_vf_mlp16_fwd(C.byref(geom), _ptr(packed16, "packed16", torch.uint8), _ptr(points, "points"),
                                   C.c_int64(m), _ptr(out, "out"), _stream()), "vfn_vf_mlp16_fwd")
    return out


BLOCK_BYTES = 1024   # one point's 256 features as split-f16 operand blocks


def vf_feat16_fwd(geom: NetGeom, packed16, points, out_vec, out_blocks) -> None:
    """VF net on points[M,3]; writes out_vec[M,3] and the feature operand blocks: out_blocks[block_rows(M), 1024] (uint8),
    32-row groups in the rendering kernel's register order — slices of larger buffers are fine when they start on a
    multiple of 32 rows."""
    m = points.shape[0]
    if out_blocks.shape[0] < block_rows(m):
        raise VfnError(f"out_blocks holds {out_blocks.shape[0]} rows, {block_rows(m)} (whole groups of 32) are needed")
    _check(load().vfn_vf_feat16_fwd(C.byref(geom), _ptr(packed16, "packed16", torch.uint8), _ptr(points, "points"),
                                    C.c_int64(m), _ptr(out_vec, "out_vec"), _ptr(out_blocks, "out_blocks", torch.uint8),
                                    _stream()), "vfn_vf_feat16_fwd")


def _fused16_products(vf_geom, vf_packed16, rn_geom, rn_packed16, points, ray_dirs, samples_per_ray, out_index, colour_products,
                      normals, colors) -> None:
    _check(load().vfn_vf_render_fused16_products(C.byref(vf_geom), _ptr(vf_packed16, "vf_packed16", torch.uint8),
                                                 C.byref(rn_geom), _ptr(rn_packed16, "rn_packed16", torch.uint8),
                                                 _ptr(points, "points"), _ptr(ray_dirs, "ray_dirs"), C.c_int64(points.shape[0]),
                                                 C.c_int32(samples_per_ray),
                                                 _ptr(out_index, "out_index", torch.int32) if out_index is not None else None,
                                                 C.c_int32(colour_products), _ptr(normals, "normals"), _ptr(colors, "colors"),
                                                 _stream()), "vfn_vf_render_fused16_products")


def vf_render_fused16_scatter(vf_geom, vf_packed16, rn_geom, rn_packed16, points, ray_dirs, samples_per_ray: int, out_index,
                              normals, colors, colour_products: int = 3) -> None:
    """Fused VF + rendering launch over points[M,3] (view direction of point m: ray_dirs[m // samples_per_ray]); the outputs of
    point m are written to row out_index[m] of the caller's normals / colors (int32; negative: dropped).  colour_products: see
    vfn_vf_render_fused16_products."""
    m = points.shape[0]
    if out_index.shape[0] < m:
        raise VfnError(f"out_index holds {out_index.shape[0]} entries for {m} points")
    if colour_products != 3:
        return _fused16_products(vf_geom, vf_packed16, rn_geom, rn_packed16, points, ray_dirs, samples_per_ray, out_index,
                                 colour_products, normals, colors)
    _check(load().vfn_vf_render_fused16_scatter(C.byref(vf_geom), _ptr(vf_packed16, "vf_packed16", torch.uint8),
                                                C.byref(rn_geom), _ptr(rn_packed16, "rn_packed16", torch.uint8),
                                                _ptr(points, "points"), _ptr(ray_dirs, "ray_dirs"), C.c_int64(m),
                                                C.c_int32(samples_per_ray), _ptr(out_index, "out_index", torch.int32),
                                                _ptr(normals, "normals"), _ptr(colors, "colors"), _stream()),
           "vfn_vf_render_fused16_scatter")


def select_samples(weights, points, ray_dirs, sigma=None, z_vals=None, return_all: bool = False, index_fill: Optional[int] = None):
    """The sparse colour branch's sample selection on its own (vfn_select_samples) -> the selected indices ray * S + j as a Python list
    (synchronises: tests and diagnostics).  ``sigma`` / ``z_vals`` given: the training selection.  ``return_all``: (count, the whole
    index buffer [N S] — which held ``index_fill`` everywhere before the launch, if given —, points_sel[:count], dirs_sel[:count]) as
    device tensors instead, without the gather check below."""
    n, s = weights.shape
    dev = weights.device
    scratch = torch.empty(2 * n, dtype=torch.int32, device=dev)
    count = torch.zeros(4, dtype=torch.int32, device=dev)
    index = torch.empty(n * s, dtype=torch.int32, device=dev) if index_fill is None else torch.full((n * s,), int(index_fill), dtype=torch.int32, device=dev)
    pts_sel, dirs_sel = torch.empty(n * s, 3, device=dev), torch.empty(n * s, 3, device=dev)
    _check(load().vfn_select_samples(_ptr(weights, "weights"), _ptr(sigma, "sigma"), _ptr(z_vals, "z_vals"), C.c_int32(n), C.c_int32(s),
                                     _ptr(points, "points"), _ptr(ray_dirs, "ray_dirs"), _ptr(scratch, "scratch", torch.int32),
                                     _ptr(count, "count", torch.int32), _ptr(index, "index", torch.int32), _ptr(pts_sel, "points_sel"),
                                     _ptr(dirs_sel, "dirs_sel"), _stream()), "vfn_select_samples")
    k = int(count[0])
    if return_all:
        return k, index, pts_sel[:max(min(k, n * s), 0)], dirs_sel[:max(min(k, n * s), 0)]
    got = index[:k].tolist()
    flat = points.reshape(-1, 3)
    assert torch.equal(pts_sel[:k], flat[index[:k].long()]) and torch.equal(dirs_sel[:k], ray_dirs[(index[:k] // s).long()])
    return got


def scatter_rows3(a, b, index, out_a, out_b) -> None:
    """out_a[index[r]] = a[r], out_b[index[r]] = b[r] for [n,3] fp32 rows (int32 index, negative entries skipped)."""
    n = a.shape[0]
    if index.shape[0] < n:
        raise VfnError(f"index holds {index.shape[0]} entries for {n} rows")
    _check(load().vfn_scatter_rows3(_ptr(a, "a"), _ptr(b, "b"), _ptr(index, "index", torch.int32), C.c_int64(n), _ptr(out_a, "out_a"),
                                    _ptr(out_b, "out_b"), _stream()), "vfn_scatter_rows3")


def render16_from_blocks(rn_geom: NetGeom, rn_packed16, blocks, vecs, dst, points, ray_dirs, samples_per_ray: int,
                         normals=None, colors=None):
    """Rendering net over the stored rows: row r -> sorted position dst[r] (points[dst[r]], ray_dirs[dst[r] / S]); returns
    normals[M,3], colors[M,3] in sorted order (M = points.shape[0]; every sorted sample must be some row's dst)."""
    m = points.shape[0]
    n_rows = dst.shape[0]
    dev = points.device
    if blocks.shape[0] < block_rows(n_rows) or vecs.shape[0] < n_rows:
        raise VfnError(f"{n_rows} rows need blocks[{block_rows(n_rows)}] and vecs[{n_rows}]")
    if normals is None:
        normals = torch.empty(m, 3, device=dev)
        colors = torch.empty(m, 3, device=dev)
    _check(load().vfn_render16_from_blocks(C.byref(rn_geom), _ptr(rn_packed16, "rn_packed16", torch.uint8),
                                           _ptr(blocks, "blocks", torch.uint8), _ptr(vecs, "vecs"),
                                           _ptr(dst, "dst", torch.int32), _ptr(points, "points"), _ptr(ray_dirs, "ray_dirs"),
                                           C.c_int64(n_rows), C.c_int32(samples_per_ray), _ptr(normals, "normals"),
                                           _ptr(colors, "colors"), _stream()), "vfn_render16_from_blocks")
    return normals, colors


def vf_mlp16_fwd_train(geom: NetGeom, packed16, points, with_features: bool, saved, aux_vf, masks, save_f16: int = 0,
                       ws_first: int = 0, ws_points: Optional[int] = None):
    """f16x3 VF forward that fills the backward workspace; returns the vector columns [M,3] (the features, when
    evaluated, are in their ``saved`` slot).  ``ws_first`` / ``ws_points``: as in vf_render_fused16_fwd_train."""
    m = points.shape[0]
    out = torch.empty(m, 3, device=points.device)
    _check(load().vfn_vf_mlp16_fwd_train_at(C.byref(geom), _ptr(packed16, "packed16", torch.uint8), _ptr(points, "points"),
                                            C.c_int64(m), C.c_int32(1 if with_features else 0), _ptr(out, "out"),
                                            _ptr(saved, "saved"), _ptr(aux_vf, "aux_vf"), _ptr(masks, "masks", torch.int32),
                                            C.c_int32(int(save_f16)), C.c_int64(ws_first), C.c_int64(m if ws_points is None else ws_points),
                                            _stream()), "vfn_vf_mlp16_fwd_train")
    return out


def vf_render_fused16_fwd_train(vf_geom, vf_packed16, rn_geom, rn_packed16, points, ray_dirs, samples_per_ray, saved,
                                aux_vf, aux_rn, masks, save_f16: int = 0, ws_first: int = 0, ws_points: Optional[int] = None,
                                normals=None, colors=None, colour_products: int = 3):
    """``ws_first`` / ``ws_points``: the launch fills points ws_first .. of a workspace sized for ws_points points (default: the
    whole workspace = this launch's points).  ``normals`` / ``colors``: optional [m,3] outputs to write into."""
    m = points.shape[0]
    dev = points.device
    normals = torch.empty(m, 3, device=dev) if normals is None else normals
    colors = torch.empty(m, 3, device=dev) if colors is None else colors
    _check(load().vfn_vf_render_fused16_fwd_train_at(C.byref(vf_geom), _ptr(vf_packed16, "vf_packed16", torch.uint8),
                                                     C.byref(rn_geom), _ptr(rn_packed16, "rn_packed16", torch.uint8),
                                                     _ptr(points, "points"), _ptr(ray_dirs, "ray_dirs"), C.c_int64(m),
                                                     C.c_int32(samples_per_ray), _ptr(normals, "normals"),
                                                     _ptr(colors, "colors"), _ptr(saved, "saved"), _ptr(aux_vf, "aux_vf"),
                                                     _ptr(aux_rn, "aux_rn"), _ptr(masks, "masks", torch.int32),
                                                     C.c_int32(int(save_f16)), C.c_int64(ws_first), C.c_int64(m if ws_points is None else ws_points),
                                                     C.c_int32(colour_products), _stream()), "vfn_vf_render_fused16_fwd_train")
    return normals, colors


def vf_render_fused16_fwd(vf_geom, vf_packed16, rn_geom, rn_packed16, points, ray_dirs, samples_per_ray: int, colour_products: int = 3):
    m = points.shape[0]
    dev = points.device
    normals = torch.empty(m, 3, device=dev)
    colors = torch.empty(m, 3, device=dev)
    if colour_products != 3:
        _fused16_products(vf_geom, vf_packed16, rn_geom, rn_packed16, points, ray_dirs, samples_per_ray, None, colour_products,
                          normals, colors)
        return normals, colors
    _check(load().vfn_vf_render_fused16_fwd(C.byref(vf_geom), _ptr(vf_packed16, "vf_packed16", torch.uint8),
                                            C.byref(rn_geom), _ptr(rn_packed16, "rn_packed16", torch.uint8),
                                            _ptr(points, "points"), _ptr(ray_dirs, "ray_dirs"), C.c_int64(m),
                                            C.c_int32(samples_per_ray), _ptr(normals, "normals"),
                                            _ptr(colors, "colors"), _stream()), "vfn_vf_render_fused16_fwd")
    return normals, colors


# ------------------------------------------------------------------------------------------------
# dense-grid stages (mesh extraction)
# ------------------------------------------------------------------------------------------------
def grid_lattice_points(axes, n: int, row0: int, count: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rows [row0, row0 + count) of the separable n^3 lattice with axis tables ``axes`` = (a0[n], a1[n], a2[n]) -> points[count,3]."""
    a0, a1, a2 = axes
    if out is None:
        out = torch.empty(count, 3, device=a0.device)
    _check(load().vfn_grid_lattice_points(_ptr(a0, "axis0"), _ptr(a1, "axis1"), _ptr(a2, "axis2"), C.c_int32(n), C.c_int64(row0), C.c_int64(count),
                                          _ptr(out, "points"), _stream()), "vfn_grid_lattice_points")
    return out


def grid_divergence(vt: torch.Tensor, n: int, threshold: float = -0.5) -> torch.Tensor:
    out = torch.empty(n, n, n, device=vt.device)
    _check(load().vfn_grid_divergence(_ptr(vt, "vt"), C.c_int32(n), C.c_float(threshold), _ptr(out, "out"), _stream()),
           "vfn_grid_divergence")
    return out


def grid_smooth_axis(src: torch.Tensor, dst: torch.Tensor, n: int, axis: int, weights: Sequence[float]) -> None:
    w = (C.c_float * len(weights))(*[float(x) for x in weights])
    _check(load().vfn_grid_smooth_axis(_ptr(src, "in"), _ptr(dst, "out"), C.c_int32(n), C.c_int32(axis), w,
                                       C.c_int32(len(weights)), _stream()), "vfn_grid_smooth_axis")


def grid_unify_direction(divergence: torch.Tensor, vt: torch.Tensor, n: int) -> torch.Tensor:
    choice = torch.empty(n * n * n, 8, dtype=torch.int64, device=vt.device)
    _check(load().vfn_grid_unify_direction(_ptr(divergence, "divergence"), _ptr(vt, "vt"), C.c_int32(n),
                                           _ptr(choice, "choice", torch.int64), _stream()), "vfn_grid_unify_direction")
    return choice


def grid_unify_direction_sides(divergence: torch.Tensor, vt: torch.Tensor, n: int, want_table: bool = True):
    """-> (sides[n^3] uint8: bit q = corner q's side, choice[n^3,8] int64 | None)."""
    sides = torch.empty(n * n * n, dtype=torch.uint8, device=vt.device)
    choice = torch.empty(n * n * n, 8, dtype=torch.int64, device=vt.device) if want_table else None
    _check(load().vfn_grid_unify_direction_sides(_ptr(divergence, "divergence"), _ptr(vt, "vt"), C.c_int32(n), _ptr(sides, "sides", torch.uint8),
                                                 _ptr(choice, "choice", torch.int64), _stream()), "vfn_grid_unify_direction_sides")
    return sides, choice


def grid_comb_format_sides(sides: torch.Tensor, norms: torch.Tensor, n: int):
    dev = norms.device
    different = torch.empty(n * n * n, 28, device=dev)
    pair_norms = torch.empty(n * n * n, 28, 2, device=dev)
    _check(load().vfn_grid_comb_format_sides(_ptr(sides, "sides", torch.uint8), _ptr(norms, "norms"), C.c_int32(n),
                                             _ptr(different, "different_side"), _ptr(pair_norms, "pair_norms"), _stream()),
           "vfn_grid_comb_format_sides")
    return different, pair_norms


def grid_comb_format(choice: torch.Tensor, norms: torch.Tensor, n: int):
    dev = norms.device
    different = torch.empty(n * n * n, 28, device=dev)
    pair_norms = torch.empty(n * n * n, 28, 2, device=dev)
    _check(load().vfn_grid_comb_format(_ptr(choice, "choice", torch.int64), _ptr(norms, "norms"), C.c_int32(n),
                                       _ptr(different, "different_side"), _ptr(pair_norms, "pair_norms"), _stream()),
           "vfn_grid_comb_format")
    return different, pair_norms


# ------------------------------------------------------------------------------------------------
# mesh triangulation (csrc/vfn_mesh.hip; vf_nerf_amd/mesh.py is the public surface)
# ------------------------------------------------------------------------------------------------
MESH_GENERAL, MESH_FUSED = 0, 1
# the status word every geometry kernel reports bad input with (mesh, metrics, rasteriser): a non-finite value, an index out of range
GEOM_STATUS_NONFINITE, GEOM_STATUS_INDEX = 1, 2


def mesh_tables():
    """-> (edge_table[256] int32, edge_vertex[12,2] int32, tri_table[256,16] int8): host copies of the tables the kernels use."""
    import numpy as np
    et, ev, tt = (C.c_int32 * 256)(), (C.c_int32 * 24)(), (C.c_int8 * 4096)()
    _check(load().vfn_mesh_tables(et, ev, tt), "vfn_mesh_tables")
    return (np.frombuffer(et, dtype=np.int32).copy(), np.frombuffer(ev, dtype=np.int32).reshape(12, 2).copy(),
            np.frombuffer(tt, dtype=np.int8).reshape(256, 16).copy())


def mesh_field_norms(field: torch.Tensor, want_unit: bool = True):
    """field[n,3] -> (norms[n], unit[n,3] | None): torch.norm(field, dim=1) as torch's CPU kernel rounds it, F.normalize(field, dim=1)."""
    n = field.shape[0]
    norms = torch.empty(n, device=field.device)
    unit = torch.empty(n, 3, device=field.device) if want_unit else None
    _check(load().vfn_mesh_field_norms(_ptr(field, "field"), C.c_int64(n), _ptr(norms, "norms"), _ptr(unit, "unit"), _stream()),
           "vfn_mesh_field_norms")
    return norms, unit


def _bytes_ws(fn_name: str, n: int, dev) -> torch.Tensor:
    """The workspace the entry point ``fn_name`` asks for over n elements, as a uint8 tensor on ``dev``."""
    b = int(getattr(load(), fn_name)(C.c_int64(n)))
    if b < 0:
        raise VfnError(f"{fn_name} failed: {load().vfn_last_error().decode()}")
    return torch.empty(max(b, 1), dtype=torch.uint8, device=dev)


def _extract(count, emit, cells: int, dev, what: str, check_status=None):
    """The sequence both triangulating units run over their ``cells`` cell positions: count -> emit -> dedup -> number on the current
    stream of ``dev`` -> (vertices[V,3] float64, faces[F,3] int64, 0-based).  ``count`` and ``emit`` are the unit's entry points closed
    over the source's leading arguments; they receive the trailing ones.  Two values cross to the host, each to size the next outputs:
    the triangle count — with the input status, handed to ``check_status`` — and the vertex count."""
    return _extract_slots(count, emit, cells, dev, what, check_status)[:2]


def _extract_slots(count, emit, cells: int, dev, what: str, check_status=None, per_slot=None):
    """``_extract`` -> (vertices, faces, extra).  ``per_slot(scanned, ids, n_vertices)`` runs on a non-empty mesh after the numbering,
    with the counts / offsets pointers the entry points received and the slot -> vertex ids[3 F]; its result is ``extra`` (None otherwise)."""
    from .geomargs import empty_mesh          # (geomargs imports this module)
    with torch.cuda.device(dev):
        info = torch.zeros(4, dtype=torch.int64, device=dev)
        counts = torch.empty(max(cells, 1), dtype=torch.int32, device=dev)
        offsets = torch.empty_like(counts)
        ws = _bytes_ws("vfn_mesh_scan_workspace_bytes", cells, dev)
        scanned = (_ptr(counts, "counts", torch.int32), _ptr(offsets, "offsets", torch.int32))
        count(*scanned, _ptr(info, "info", torch.int64), _ptr(ws, "scan_ws", torch.uint8), C.c_int64(ws.numel()), _stream())
        n_tri, status = (int(x) for x in info[:2].cpu())
        if check_status is not None:
            check_status(status)
        n_slots = 3 * n_tri
        if n_tri < 0 or n_slots >= (1 << 31):
            raise VfnError(f"{what}: {n_tri} triangles exceed the 2^31 / 3 limit")
        if n_tri == 0:
            return empty_mesh(dev) + (None,)
        tri_verts = torch.empty(n_slots, 3, dtype=torch.float64, device=dev)
        emit(*scanned, _ptr(tri_verts, "tri_verts", torch.float64), _stream())
        vertices, ids = mesh_dedup(tri_verts, info=info)
        extra = per_slot(scanned, ids, vertices.shape[0]) if per_slot is not None else None
    return vertices, ids.view(n_tri, 3), extra


def mesh_triangulate(form: int, m: int, res: int, size: float, isovalue: float, comb: Optional[torch.Tensor] = None,
                     udf: Optional[torch.Tensor] = None, cells: Optional[torch.Tensor] = None, sides: Optional[torch.Tensor] = None,
                     norms: Optional[torch.Tensor] = None, device=None):
    """Contrastive marching cubes (csrc/vfn_mesh.hip) through ``_extract`` -> (vertices[V,3] float64, faces[F,3] int64, 0-based)."""
    dev = torch.device(device) if device is not None else (norms.device if norms is not None else comb.device)
    f64 = int(comb is not None and comb.dtype == torch.float64)
    dt = torch.float64 if f64 else torch.float32
    ptrs = (C.c_int32(form), _ptr(comb, "comb", dt), _ptr(udf, "udf", dt), C.c_int32(f64), _ptr(cells, "cells", torch.int64),
            _ptr(sides, "sides", torch.uint8), _ptr(norms, "norms"), C.c_int64(m), C.c_int32(res), C.c_double(size), C.c_double(isovalue))

    def check_status(status: int) -> None:
        if status & GEOM_STATUS_INDEX:
            raise VfnError(f"mesh triangulation: a cell index lies outside [0, {res})")
        if status & GEOM_STATUS_NONFINITE:
            raise VfnError("mesh triangulation: a non-finite norm / udf value in a triangulated cell (NaN vertices cannot be deduplicated "
                           "meaningfully; the reference's dict would keep every one of them)")

    return _extract(lambda *out: _check(load().vfn_mesh_count(*ptrs, *out), "vfn_mesh_count"),
                    lambda *out: _check(load().vfn_mesh_emit(*ptrs, *out), "vfn_mesh_emit"), m, dev, "mesh triangulation", check_status)


def mesh_dedup(tri_verts: torch.Tensor, info: Optional[torch.Tensor] = None):
    """tri_verts[S,3] float64 (finite) -> (vertices[V,3] float64, ids[S] int64): the distinct positions in order of first appearance (float
    equality: -0.0 and +0.0 are one key, the first occurrence's bits are kept) and every slot's vertex id; three consecutive slots are
    one face.  Table sizing, vfn_mesh_dedup and vfn_mesh_number on the current stream; the vertex count crosses to the host."""
    dev = tri_verts.device
    n_slots = tri_verts.shape[0]
    if n_slots >= (1 << 31):
        raise VfnError(f"mesh deduplication: {n_slots} slots exceed the 2^31 limit")
    if info is None:
        info = torch.zeros(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        if n_slots == 0:
            tri_verts = torch.empty(1, 3, dtype=torch.float64, device=dev)
        table_size = 1 << max(6, (2 * n_slots - 1).bit_length())
        table = torch.empty(table_size, dtype=torch.int32, device=dev)
        owner = torch.empty_like(table)
        bucket = torch.empty(max(n_slots, 1), dtype=torch.int32, device=dev)
        flags, vid = torch.empty_like(bucket), torch.empty_like(bucket)
        ws = _bytes_ws("vfn_mesh_scan_workspace_bytes", n_slots, dev)
        _check(load().vfn_mesh_dedup(_ptr(tri_verts, "tri_verts", torch.float64), C.c_int64(n_slots), _ptr(table, "table", torch.int32),
                                     _ptr(owner, "owner", torch.int32), C.c_int64(table_size), _ptr(bucket, "bucket", torch.int32),
                                     _ptr(flags, "flags", torch.int32), _ptr(vid, "vid", torch.int32), _ptr(info, "info", torch.int64),
                                     _ptr(ws, "scan_ws", torch.uint8), C.c_int64(ws.numel()), _stream()), "vfn_mesh_dedup")
        n_vert = int(info[2].cpu())
        vertices = torch.empty(n_vert, 3, dtype=torch.float64, device=dev)
        ids = torch.empty(n_slots, dtype=torch.int64, device=dev)
        _check(load().vfn_mesh_number(_ptr(tri_verts, "tri_verts", torch.float64), C.c_int64(n_slots), _ptr(owner, "owner", torch.int32),
                                      _ptr(bucket, "bucket", torch.int32), _ptr(vid, "vid", torch.int32),
                                      _ptr(vertices, "vertices", torch.float64) if n_vert else None,
                                      _ptr(ids, "faces", torch.int64) if n_slots else None, _stream()), "vfn_mesh_number")
    return vertices, ids


# ------------------------------------------------------------------------------------------------
# mesh scoring (csrc/vfn_metrics.hip; vf_nerf_amd/metrics3d.py is the public surface).  Everything float64, contiguous, on one device.
# ------------------------------------------------------------------------------------------------
CUMSUM_TILE = 1024                 # csrc/vfn_metrics.hip: SCAN_TILE


def nn_sqdist(queries: torch.Tensor, targets: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """queries[n,3], targets[m,3] -> best[n]: the squared distance of every query to its nearest target, all pairs in float64.  A
    non-finite coordinate in either set raises (one status word crosses to the host) — or, with the caller's zero-filled ``info``
    (int64 [1]), sets its bit GEOM_STATUS_NONFINITE for the caller to read with its results (``nn_check``)."""
    n, m = queries.shape[0], targets.shape[0]
    best = torch.empty(n, dtype=torch.float64, device=queries.device)
    own = info is None
    if own:
        info = torch.zeros(1, dtype=torch.int64, device=queries.device)
    _check(load().vfn_nn_sqdist(_ptr(queries, "queries", torch.float64), C.c_int64(n), _ptr(targets, "targets", torch.float64), C.c_int64(m),
                                _ptr(best, "best", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_nn_sqdist")
    if own:
        nn_check(int(info.cpu()))
    return best


def nn_check(status: int) -> None:
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError("nearest-neighbour search: a non-finite coordinate in the queries or the targets")


def tri_areas_check(status: int, nv: int) -> None:
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"triangle areas: a face index lies outside [0, {nv})")
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError("triangle areas: a non-finite area (non-finite or overflowing vertex coordinates)")


def tri_areas(vertices: torch.Tensor, faces: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vertices[V,3] float64, faces[F,3] int64 -> areas[F].  A face index outside [0, V) or a non-finite area raises — or, with the
    caller's zero-filled ``info`` (int64 [1]), sets its bits (``tri_areas_check``) and nothing is read here."""
    nv, nf = vertices.shape[0], faces.shape[0]
    areas = torch.empty(nf, dtype=torch.float64, device=faces.device)
    own = info is None
    if own:
        info = torch.zeros(1, dtype=torch.int64, device=faces.device)
    _check(load().vfn_tri_areas(_ptr(vertices, "vertices", torch.float64) if nv else None, C.c_int64(nv), _ptr(faces, "faces", torch.int64),
                                C.c_int64(nf), _ptr(areas, "areas", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_tri_areas")
    if not own:
        return areas
    tri_areas_check(int(info.cpu()), nv)
    return areas


def cumsum_levels(n: int) -> int:
    """Scan levels of vfn_cumsum_f64 over n values (a prefix is at most 12 additions deep per level)."""
    levels = 1
    while n > CUMSUM_TILE:
        n, levels = (n + CUMSUM_TILE - 1) // CUMSUM_TILE, levels + 1
    return levels


def cumsum_f64(x: torch.Tensor) -> torch.Tensor:
    """x[n] float64 -> the inclusive prefix sums as a fixed tree (the bits depend on n and the data alone)."""
    n = x.shape[0]
    out = torch.empty_like(x)
    ws = _bytes_ws("vfn_cumsum_workspace_bytes", n, x.device)
    _check(load().vfn_cumsum_f64(_ptr(x, "x", torch.float64), C.c_int64(n), _ptr(out, "out", torch.float64), _ptr(ws, "workspace", torch.uint8),
                                 C.c_int64(ws.numel()), _stream()), "vfn_cumsum_f64")
    return out


def sample_surface(vertices: torch.Tensor, faces: torch.Tensor, cum: torch.Tensor, uniforms: torch.Tensor):
    """-> (points[count,3] float64, face_index[count] int64) for uniforms[count,3]; see include/vfn.h for the expressions."""
    count = uniforms.shape[0]
    dev = uniforms.device
    points = torch.empty(count, 3, dtype=torch.float64, device=dev)
    face_index = torch.empty(count, dtype=torch.int64, device=dev)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    _check(load().vfn_sample_surface(_ptr(vertices, "vertices", torch.float64), C.c_int64(vertices.shape[0]), _ptr(faces, "faces", torch.int64),
                                     C.c_int64(faces.shape[0]), _ptr(cum, "cum", torch.float64), _ptr(uniforms, "uniforms", torch.float64),
                                     C.c_int64(count), _ptr(points, "points", torch.float64), _ptr(face_index, "face_index", torch.int64),
                                     _ptr(info, "info", torch.int64), _stream()), "vfn_sample_surface")
    return points, face_index, info


def reduce_stats(x: torch.Tensor, threshold: float) -> torch.Tensor:
    """x[n] float64 -> stats[4] on the device: sum, min, max, number of x[i] < threshold (as a double).  Nothing crosses to the host."""
    n = x.shape[0]
    stats = torch.empty(4, dtype=torch.float64, device=x.device)
    ws = _bytes_ws("vfn_reduce_stats_workspace_bytes", n, x.device)
    _check(load().vfn_reduce_stats(_ptr(x, "x", torch.float64), C.c_int64(n), C.c_double(threshold), _ptr(stats, "stats", torch.float64),
                                   _ptr(ws, "workspace", torch.uint8), C.c_int64(ws.numel()), _stream()), "vfn_reduce_stats")
    return stats


def tree_sum_levels(lane_levels: int, partials: int) -> int:
    """Addition levels of a sum along the fixed tree of include/vfn.h: what a lane adds before the block tree, the block tree over
    VFN_TREE_LANES lanes, the serial run of the second level (ceil(partials / VFN_TREE_TOP) - 1), its block tree."""
    lanes, top = header_constant("VFN_TREE_LANES"), header_constant("VFN_TREE_TOP")
    return lane_levels + (lanes.bit_length() - 1) + ((partials + top - 1) // top - 1) + (top.bit_length() - 1)


def _tree_tiles(n: int) -> int:
    tile = header_constant("VFN_TREE_LANES") * header_constant("VFN_TREE_PER")
    return (n + tile - 1) // tile


def reduce_sum_levels(n: int) -> int:
    """Addition levels of vfn_reduce_stats's sum over n values: a lane's 16 values (4), P = ceil(n / 4096) partials."""
    return tree_sum_levels(4, _tree_tiles(n))


# ------------------------------------------------------------------------------------------------
# point-set alignment (csrc/vfn_icp.hip; vf_nerf_amd/icp.py is the public surface).  Everything float64, contiguous, on one device.
# ------------------------------------------------------------------------------------------------
ICP_SUMS = 17                      # count, sum d2, sum p[3], sum s[3], sum p s^T [9] (include/vfn.h: vfn_icp_accumulate)


def icp_grid_limits():
    """-> (cells per axis at most, the least ratio of the cell edge to the radius): VFN_ICP_GRID_CAP, 1 + 2^-VFN_ICP_GRID_MARGIN_LOG2."""
    return header_constant("VFN_ICP_GRID_CAP"), 1.0 + 2.0 ** -header_constant("VFN_ICP_GRID_MARGIN_LOG2")


def _transform12(transform):
    """None, or 12 Python floats (r00 .. r22 row-major, t0 t1 t2) -> the HOST pointer the entry points take."""
    return None if transform is None else (C.c_double * 12)(*transform)


def transform_points(points: torch.Tensor, transform=None) -> torch.Tensor:
    """points[n,3] -> [n,3]: ((r00 x + r01 y) + r02 z) + t0, ... per point; ``transform`` None is the identity (a copy)."""
    n = points.shape[0]
    out = torch.empty(n, 3, dtype=torch.float64, device=points.device)
    _check(load().vfn_transform_points(_ptr(points, "points", torch.float64), C.c_int64(n), _transform12(transform),
                                       _ptr(out, "out", torch.float64), _stream()), "vfn_transform_points")
    return out


def nn_radius(queries: torch.Tensor, transform, grid, radius: float, order: Optional[torch.Tensor] = None,
              info: Optional[torch.Tensor] = None, check_finite: bool = True):
    """-> (index[n] int64, sqdist[n]) of every transformed query's nearest target within ``radius`` (-1 / +inf when there is none).
    ``grid`` = (sorted_targets[m,3], perm[m] int64, cell_start[cells+1] int32, box: 7 floats, dims: 3 ints) as include/vfn.h describes.
    ``info`` as in ``nn_sqdist``; ``check_finite=False`` skips the pass over the coordinates (a caller that has searched these two
    arrays before)."""
    sorted_targets, perm, cell_start, box, dims = grid
    n, m = queries.shape[0], sorted_targets.shape[0]
    if perm.shape[0] != m or cell_start.shape[0] != dims[0] * dims[1] * dims[2] + 1 or (order is not None and order.shape[0] != n):
        raise VfnError("nn_radius: perm / cell_start / order do not have the lengths the grid and the queries give")
    index = torch.empty(n, dtype=torch.int64, device=queries.device)
    sqdist = torch.empty(n, dtype=torch.float64, device=queries.device)
    own = info is None
    if own:
        info = torch.zeros(1, dtype=torch.int64, device=queries.device)
    _check(load().vfn_nn_radius(_ptr(queries, "queries", torch.float64), C.c_int64(n), _transform12(transform),
                                _ptr(sorted_targets, "sorted_targets", torch.float64), _ptr(perm, "perm", torch.int64), C.c_int64(m),
                                _ptr(cell_start, "cell_start", torch.int32), (C.c_double * 7)(*box), C.c_int32(dims[0]), C.c_int32(dims[1]),
                                C.c_int32(dims[2]), C.c_double(radius), _ptr(order, "order", torch.int64), C.c_int32(int(check_finite)),
                                _ptr(index, "index", torch.int64),
                                _ptr(sqdist, "sqdist", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_nn_radius")
    if own:
        nn_check(int(info.cpu()))
    return index, sqdist


def nn_nearest(queries: torch.Tensor, grid, max_rings: int, order: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None,
               check_finite: bool = True):
    """-> (index[n] int64, sqdist[n], leftover_count) of every query's nearest target over ALL targets, ties to the lowest original index
    (include/vfn.h: vfn_nn_nearest).  ``grid`` = (targets[m,3] in their original order, sorted_targets[m,3], perm[m] int64,
    cell_start[cells+1] int32, box: 7 floats, dims: 3 ints).  The ring search leaves the queries that have not stopped after ring
    ``max_rings`` on a list; ONE host read — the list's length and the status word — and, unless the list is empty, a second launch
    serves them by all pairs (vfn_nn_nearest_list).  ``leftover_count`` (a Python int) only tells how the work was split: no bit of
    the result depends on ``max_rings``, ``order`` or the grid.  That read brings the status word with it, so a non-finite coordinate
    raises here whether or not the caller gave its own zero-filled ``info`` (int64 [1])."""
    targets, sorted_targets, perm, cell_start, box, dims = grid
    n, m = queries.shape[0], sorted_targets.shape[0]
    if isinstance(max_rings, bool) or not isinstance(max_rings, int) or max_rings < 0:
        raise VfnError(f"nn_nearest: max_rings must be a non-negative integer, got {max_rings!r}")
    if (targets.shape[0] != m or perm.shape[0] != m or cell_start.shape[0] != dims[0] * dims[1] * dims[2] + 1
            or (order is not None and order.shape[0] != n)):
        raise VfnError("nn_nearest: targets / perm / cell_start / order do not have the lengths the grid and the queries give")
    dev = queries.device
    index = torch.empty(n, dtype=torch.int64, device=dev)
    sqdist = torch.empty(n, dtype=torch.float64, device=dev)
    leftover = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    if info is None:
        info = torch.zeros(1, dtype=torch.int64, device=dev)
    q = _ptr(queries, "queries", torch.float64)
    _check(load().vfn_nn_nearest(q, C.c_int64(n), _ptr(sorted_targets, "sorted_targets", torch.float64), _ptr(perm, "perm", torch.int64),
                                 C.c_int64(m), _ptr(cell_start, "cell_start", torch.int32), (C.c_double * 7)(*box), C.c_int32(dims[0]),
                                 C.c_int32(dims[1]), C.c_int32(dims[2]), C.c_int32(min(max_rings, 2 ** 31 - 1)), _ptr(order, "order", torch.int64),
                                 C.c_int32(int(check_finite)), _ptr(index, "index", torch.int64), _ptr(sqdist, "sqdist", torch.float64),
                                 _ptr(leftover, "leftover", torch.int64), _ptr(count, "leftover_count", torch.int64),
                                 _ptr(info, "info", torch.int64), _stream()), "vfn_nn_nearest")
    left, status = (int(x) for x in torch.cat((count, info)).cpu())          # the one read between the two launches
    nn_check(status)
    left = min(left, n)
    if left:
        _check(load().vfn_nn_nearest_list(q, C.c_int64(n), _ptr(targets, "targets", torch.float64), C.c_int64(m),
                                          _ptr(leftover, "leftover", torch.int64), C.c_int64(left), _ptr(index, "index", torch.int64),
                                          _ptr(sqdist, "sqdist", torch.float64), _stream()), "vfn_nn_nearest_list")
    return index, sqdist, left


# ------------------------------------------------------------------------------------------------
# the closest point on a triangle mesh (csrc/vfn_proximity.hip; vf_nerf_amd/metrics3d.py is the public surface)
# ------------------------------------------------------------------------------------------------
def proximity_check(status: int, nv: int) -> None:
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"closest point: a face index lies outside [0, {nv})")
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError("closest point: a non-finite coordinate in the queries or in a vertex that a face names")


def tri_cell_ranges(vertices: torch.Tensor, faces: torch.Tensor, box, dims, info: torch.Tensor):
    """vertices[V,3] float64, faces[F,3] int64, the grid's box (7 floats) and dims -> (tri[F,9], cell_lo[F,3] int32, cell_hi[F,3] int32,
    ncells[F] int32) of include/vfn.h: vfn_tri_cell_ranges.  ``info`` (int64 [1], zero-filled by the caller) collects the status bits."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise VfnError(f"tri_cell_ranges: vertices must be [V,3] and faces [F,3], got {tuple(vertices.shape)} / {tuple(faces.shape)}")
    nv, nf, dev = vertices.shape[0], faces.shape[0], faces.device
    tri = torch.empty(nf, 9, dtype=torch.float64, device=dev)
    cell_lo = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    cell_hi = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    ncells = torch.empty(nf, dtype=torch.int32, device=dev)
    _check(load().vfn_tri_cell_ranges(_ptr(vertices, "vertices", torch.float64), C.c_int64(nv), _ptr(faces, "faces", torch.int64), C.c_int64(nf),
                                      (C.c_double * 7)(*box), C.c_int32(dims[0]), C.c_int32(dims[1]), C.c_int32(dims[2]),
                                      _ptr(tri, "tri", torch.float64), _ptr(cell_lo, "cell_lo", torch.int32), _ptr(cell_hi, "cell_hi", torch.int32),
                                      _ptr(ncells, "ncells", torch.int32), _ptr(info, "info", torch.int64), _stream()), "vfn_tri_cell_ranges")
    return tri, cell_lo, cell_hi, ncells


def tri_cell_pairs(cell_lo: torch.Tensor, cell_hi: torch.Tensor, ncells: torch.Tensor, offset: torch.Tensor, big_face_cells: int, dims,
                   n_pairs: int, info: torch.Tensor):
    """-> (key[n_pairs] int32, face[n_pairs] int32), unsorted (include/vfn.h: vfn_tri_cell_pairs).  ``n_pairs`` >= 1."""
    nf = ncells.shape[0]
    if tuple(cell_lo.shape) != (nf, 3) or tuple(cell_hi.shape) != (nf, 3) or tuple(offset.shape) != (nf,):
        raise VfnError("tri_cell_pairs: cell_lo / cell_hi must be [F,3] and offset [F] for ncells [F]")
    key = torch.empty(n_pairs, dtype=torch.int32, device=ncells.device)
    face = torch.empty(n_pairs, dtype=torch.int32, device=ncells.device)
    _check(load().vfn_tri_cell_pairs(_ptr(cell_lo, "cell_lo", torch.int32), _ptr(cell_hi, "cell_hi", torch.int32), _ptr(ncells, "ncells", torch.int32),
                                     _ptr(offset, "offset", torch.int64), C.c_int64(nf), C.c_int64(big_face_cells), C.c_int32(dims[0]),
                                     C.c_int32(dims[1]), C.c_int32(dims[2]), C.c_int64(n_pairs), _ptr(key, "key", torch.int32),
                                     _ptr(face, "face", torch.int32), _ptr(info, "info", torch.int64), _stream()), "vfn_tri_cell_pairs")
    return key, face


def tri_nearest_list(queries: torch.Tensor, tri: torch.Tensor, ncells: torch.Tensor, listed: torch.Tensor, count: int, face: torch.Tensor,
                     closest: torch.Tensor, sqdist: torch.Tensor, info: torch.Tensor) -> None:
    """The all-pairs search for the first ``count`` queries of ``listed``, into the rows of face / closest / sqdist they name
    (include/vfn.h: vfn_tri_nearest_list)."""
    n, nf = queries.shape[0], tri.shape[0]
    if (tuple(tri.shape) != (nf, 9) or tuple(ncells.shape) != (nf,) or listed.shape[0] < count or tuple(face.shape) != (n,)
            or tuple(closest.shape) != (n, 3) or tuple(sqdist.shape) != (n,)):
        raise VfnError("tri_nearest_list: tri must be [F,9], ncells [F], the list at least count long, and face / closest / sqdist the queries' rows")
    _check(load().vfn_tri_nearest_list(_ptr(queries, "queries", torch.float64), C.c_int64(n), _ptr(tri, "tri", torch.float64),
                                       _ptr(ncells, "ncells", torch.int32), C.c_int64(nf), _ptr(listed, "list", torch.int64), C.c_int64(count),
                                       _ptr(face, "face", torch.int64), _ptr(closest, "closest", torch.float64),
                                       _ptr(sqdist, "sqdist", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_tri_nearest_list")


def tri_nearest(queries: torch.Tensor, grid, max_rings: Optional[int], n_vertices: int, order: Optional[torch.Tensor] = None,
                info: Optional[torch.Tensor] = None, serve_leftovers: bool = True):
    """-> (face[n] int64, closest[n,3], sqdist[n], leftover_count) of every query's closest point over ALL faces, ties to the lowest face
    (include/vfn.h: vfn_tri_nearest).  ``grid`` = (tri[F,9], ncells[F] int32, pair_face[n_pairs] int32, cell_start[cells+1] int32,
    large[n_large] int64, box: 7 floats, dims: 3 ints).  ``max_rings`` None: no ring search at all, every query goes through the
    all-pairs kernel (vfn_tri_nearest_list).  Otherwise the ring search leaves the queries that have not stopped after ring
    ``max_rings`` on a list; ONE host read — the list's length and the status word — and a second launch serves them by all pairs.
    No bit of the result depends on ``max_rings``, ``order`` or the grid.  With the caller's zero-filled ``info`` (int64 [1]) the status
    bits are left there for the caller; without it a set bit raises (``proximity_check``).  ``serve_leftovers=False`` stops after the
    ring launch: the rows of the ``leftover_count`` unsettled queries are then NOT written (tools/bench_proximity.py counts the queries
    each ring settles that way; nothing else should)."""
    tri, ncells, pair_face, cell_start, large, box, dims = grid
    n, nf, dev = queries.shape[0], tri.shape[0], queries.device
    if max_rings is not None and (isinstance(max_rings, bool) or not isinstance(max_rings, int) or max_rings < 0):
        raise VfnError(f"tri_nearest: max_rings must be None or a non-negative integer, got {max_rings!r}")
    if queries.dim() != 2 or queries.shape[1] != 3 or tuple(tri.shape) != (nf, 9) or tuple(ncells.shape) != (nf,):
        raise VfnError(f"tri_nearest: queries must be [n,3], tri [F,9] and ncells [F], got {tuple(queries.shape)} / {tuple(tri.shape)} / {tuple(ncells.shape)}")
    if cell_start.shape[0] != dims[0] * dims[1] * dims[2] + 1 or (order is not None and order.shape[0] != n):
        raise VfnError("tri_nearest: cell_start / order do not have the lengths the grid and the queries give")
    face = torch.empty(n, dtype=torch.int64, device=dev)
    closest = torch.empty(n, 3, dtype=torch.float64, device=dev)
    sqdist = torch.empty(n, dtype=torch.float64, device=dev)
    own = info is None
    if own:
        info = torch.zeros(1, dtype=torch.int64, device=dev)
    if max_rings is None:
        listed, left = torch.arange(n, dtype=torch.int64, device=dev), n
    else:
        listed = torch.empty(n, dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        n_pairs, n_large = pair_face.shape[0], large.shape[0]
        _check(load().vfn_tri_nearest(_ptr(queries, "queries", torch.float64), C.c_int64(n), _ptr(tri, "tri", torch.float64), C.c_int64(nf),
                                      _ptr(pair_face, "pair_face", torch.int32) if n_pairs else None, C.c_int64(n_pairs),
                                      _ptr(cell_start, "cell_start", torch.int32), _ptr(large, "large", torch.int64) if n_large else None,
                                      C.c_int64(n_large), (C.c_double * 7)(*box), C.c_int32(dims[0]), C.c_int32(dims[1]), C.c_int32(dims[2]),
                                      C.c_int32(min(max_rings, 2 ** 31 - 1)), _ptr(order, "order", torch.int64), _ptr(face, "face", torch.int64),
                                      _ptr(closest, "closest", torch.float64), _ptr(sqdist, "sqdist", torch.float64),
                                      _ptr(listed, "leftover", torch.int64), _ptr(count, "leftover_count", torch.int64),
                                      _ptr(info, "info", torch.int64), _stream()), "vfn_tri_nearest")
        left = min(int(count.cpu()), n)                                          # the one read between the two launches
    if left and serve_leftovers:
        tri_nearest_list(queries, tri, ncells, listed, left, face, closest, sqdist, info)
    if own:
        proximity_check(int(info.cpu()), n_vertices)
    return face, closest, sqdist, left


def icp_accumulate(queries: torch.Tensor, transform, targets: torch.Tensor, index: torch.Tensor, sqdist: torch.Tensor, anchor,
                   info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> sums[17] on the device over the rows with index >= 0 (include/vfn.h: vfn_icp_accumulate).  An index >= m raises — or, with
    the caller's ``info``, sets GEOM_STATUS_INDEX in it (``icp_check``)."""
    n, m = queries.shape[0], targets.shape[0]
    if index.shape[0] != n or sqdist.shape[0] != n:
        raise VfnError(f"icp_accumulate: index / sqdist must have the queries' {n} rows")
    dev = queries.device
    sums = torch.empty(ICP_SUMS, dtype=torch.float64, device=dev)
    ws = _bytes_ws("vfn_icp_accumulate_workspace_bytes", n, dev)
    own = info is None
    if own:
        info = torch.zeros(1, dtype=torch.int64, device=dev)
    _check(load().vfn_icp_accumulate(_ptr(queries, "queries", torch.float64), C.c_int64(n), _transform12(transform),
                                     _ptr(targets, "targets", torch.float64), C.c_int64(m), _ptr(index, "index", torch.int64),
                                     _ptr(sqdist, "sqdist", torch.float64), (C.c_double * 3)(*anchor), _ptr(sums, "sums", torch.float64),
                                     _ptr(info, "info", torch.int64), _ptr(ws, "workspace", torch.uint8), C.c_int64(ws.numel()), _stream()),
           "vfn_icp_accumulate")
    if own:
        icp_check(int(info.cpu()))
    return sums


def icp_check(status: int) -> None:
    nn_check(status)
    if status & GEOM_STATUS_INDEX:
        raise VfnError("point-set alignment: a neighbour index lies outside the targets")


def icp_sum_levels(n: int) -> int:
    """Addition levels of every sum of vfn_icp_accumulate over n rows: a lane's 16 rows (4), P = ceil(n / 4096) partials."""
    return tree_sum_levels(4, _tree_tiles(n))


# ------------------------------------------------------------------------------------------------
# image scores (csrc/vfn_image.hip; vf_nerf_amd/metrics2d.py is the public surface).  Contiguous tensors on one device.
# ------------------------------------------------------------------------------------------------
IMAGE_STATUS_RANGE = 4             # info bit of vfn_image_quantize8: a value outside the range of a byte
SSIM_C1, SSIM_C2 = 1e-4, 9e-4      # utils/utils.py:249 (get_ssim's defaults)


def image_tile() -> int:
    return header_constant("VFN_IMAGE_TILE")


def image_workspace_bytes(v: int, h: int, w: int, c: int) -> int:
    b = int(load().vfn_image_scores_workspace_bytes(C.c_int64(v), C.c_int64(h), C.c_int64(w), C.c_int64(c)))
    if b < 0:
        raise VfnError(f"vfn_image_scores_workspace_bytes failed: {load().vfn_last_error().decode()}")
    return b


def image_quantize8(x: torch.Tensor, info: torch.Tensor) -> torch.Tensor:
    """x float32 (any shape) -> uint8 of that shape: trunc(double(x) 255); ``info`` (int64 [1], zero-filled) collects the refusals."""
    u = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _check(load().vfn_image_quantize8(_ptr(x, "x"), C.c_int64(x.numel()), _ptr(u, "u", torch.uint8), _ptr(info, "info", torch.int64),
                                          _stream()), "vfn_image_quantize8")
    return u


def _image_operand(t: torch.Tensor, name: str):
    if t.dtype not in (torch.uint8, torch.float32):
        raise VfnError(f"{name}: expected uint8 or float32, got {t.dtype}")
    return _ptr(t, name, t.dtype), C.c_int32(int(t.dtype == torch.uint8))


def image_scores(pred: torch.Tensor, target: torch.Tensor, want_ssim: bool, info: torch.Tensor, c1: float = SSIM_C1,
                 c2: float = SSIM_C2) -> torch.Tensor:
    """pred, target [V,H,W,C] (uint8 or float32 each) -> sums[V,3] float64 on the device (include/vfn.h: vfn_image_scores)."""
    if pred.dim() != 4 or pred.shape != target.shape or pred.device != target.device:
        raise VfnError(f"image_scores: two [V,H,W,C] tensors of one shape on one device, got {tuple(pred.shape)} and {tuple(target.shape)}")
    v, h, w, c = pred.shape
    dev = pred.device
    ws = torch.empty(max(image_workspace_bytes(v, h, w, c), 1), dtype=torch.uint8, device=dev)
    sums = torch.empty(v, 3, dtype=torch.float64, device=dev)
    (pp, pu), (tp, tu) = _image_operand(pred, "pred"), _image_operand(target, "target")
    with torch.cuda.device(dev):
        _check(load().vfn_image_scores(pp, pu, tp, tu, C.c_int64(v), C.c_int64(h), C.c_int64(w), C.c_int64(c), C.c_int32(int(bool(want_ssim))),
                                       C.c_double(c1), C.c_double(c2), _ptr(sums, "sums", torch.float64), _ptr(info, "info", torch.int64),
                                       _ptr(ws, "workspace", torch.uint8), C.c_int64(ws.numel()), _stream()), "vfn_image_scores")
    return sums


def image_abs_err(a: torch.Tensor, b: torch.Tensor, scale: float, info: torch.Tensor) -> torch.Tensor:
    """a, b [V,H,W] float32 -> sums[V] float64 on the device: sum |a s - b s| (include/vfn.h: vfn_image_abs_err)."""
    if a.dim() != 3 or a.shape != b.shape or a.device != b.device:
        raise VfnError(f"image_abs_err: two [V,H,W] tensors of one shape on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    v, h, w = a.shape
    dev = a.device
    ws = torch.empty(max(image_workspace_bytes(v, h, w, 1), 1), dtype=torch.uint8, device=dev)
    sums = torch.empty(v, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _check(load().vfn_image_abs_err(_ptr(a, "a"), _ptr(b, "b"), C.c_int64(v), C.c_int64(h), C.c_int64(w), C.c_double(scale),
                                        _ptr(sums, "sums", torch.float64), _ptr(info, "info", torch.int64), _ptr(ws, "workspace", torch.uint8),
                                        C.c_int64(ws.numel()), _stream()), "vfn_image_abs_err")
    return sums


def image_sum_levels(h: int, w: int, c: int) -> int:
    """Addition levels of a per-view sum of vfn_image_scores: the lane's channels (c - 1), P = tiles per view."""
    t = image_tile()
    return tree_sum_levels(c - 1, ((h + t - 1) // t) * ((w + t - 1) // t))


# ------------------------------------------------------------------------------------------------
# TSDF fusion (csrc/vfn_tsdf.hip; vf_nerf_amd/tsdf.py is the public surface)
# ------------------------------------------------------------------------------------------------
def _tsdf_volume_args(tsdf: torch.Tensor, weight: torch.Tensor):
    if tsdf.dim() != 3 or weight.shape != tsdf.shape:
        raise VfnError(f"tsdf / weight must be two [nx,ny,nz] tensors of one shape, got {tuple(tsdf.shape)} and {tuple(weight.shape)}")
    if tsdf.numel() < 1 or tsdf.numel() >= (1 << 31):
        raise VfnError(f"a volume of {tsdf.numel()} voxels is outside [1, 2^31)")
    if weight.device != tsdf.device:
        raise VfnError("tsdf and weight live on different devices")
    nx, ny, nz = tsdf.shape
    return (_ptr(tsdf, "tsdf"), _ptr(weight, "weight"), C.c_int32(nx), C.c_int32(ny), C.c_int32(nz))


def _f32s(*values):
    """The values as the ``float`` arguments of an entry point."""
    return tuple(C.c_float(float(x)) for x in values)


def _tsdf_view_args(tsdf: torch.Tensor, depth: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor, rgb=None):
    if depth.dim() != 3:
        raise VfnError(f"depth must be [V,H,W], got {tuple(depth.shape)}")
    v, h, w = depth.shape
    if tuple(intrinsics.shape) != (v, 4) or tuple(extrinsics.shape) != (v, 12):
        raise VfnError(f"{v} views need intrinsics [{v},4] and extrinsics [{v},12], got {tuple(intrinsics.shape)} and {tuple(extrinsics.shape)}")
    if h < 1 or w < 1 or h * w >= (1 << 31) or v >= (1 << 31):
        raise VfnError(f"{v} depth maps of {h} x {w} are outside the limits of one call")
    if rgb is not None and tuple(rgb.shape) != (v, h, w, 3):
        raise VfnError(f"{v} depth maps of {h} x {w} need rgb [{v},{h},{w},3], got {tuple(rgb.shape)}")
    for t in (depth, intrinsics, extrinsics) + (() if rgb is None else (rgb,)):
        if t.device != tsdf.device:
            raise VfnError("the views and the volume live on different devices")
    return v, h, w


def _tsdf_colour_arg(tsdf: torch.Tensor, colour: torch.Tensor):
    if tuple(colour.shape) != tuple(tsdf.shape) + (3,) or colour.device != tsdf.device:
        raise VfnError(f"colour must be [nx,ny,nz,3] on the volume's device, got {tuple(colour.shape)} on {colour.device}")
    return _ptr(colour, "colour")


def _tsdf_integrate(tsdf, weight, colour, origin, voxel_length, sdf_trunc, depth, rgb, intrinsics, extrinsics) -> None:
    """Both dense integrations: ``colour`` / ``rgb`` are tensors for vfn_tsdf_integrate_rgb, both None for vfn_tsdf_integrate."""
    vol = _tsdf_volume_args(tsdf, weight)
    col = () if colour is None else (_tsdf_colour_arg(tsdf, colour),)
    v, h, w = _tsdf_view_args(tsdf, depth, intrinsics, extrinsics, rgb)
    name = "vfn_tsdf_integrate" if colour is None else "vfn_tsdf_integrate_rgb"
    with torch.cuda.device(tsdf.device):
        _check(getattr(load(), name)(*vol[:2], *col, *vol[2:], *_f32s(*origin, voxel_length, sdf_trunc), _ptr(depth, "depth"),
                                     *(() if rgb is None else (_ptr(rgb, "rgb", torch.uint8),)), C.c_int32(h), C.c_int32(w),
                                     _ptr(intrinsics, "intrinsics"), _ptr(extrinsics, "extrinsics"), C.c_int32(v), _stream()), name)


def tsdf_integrate(tsdf: torch.Tensor, weight: torch.Tensor, origin: Sequence[float], voxel_length: float, sdf_trunc: float,
                   depth: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor) -> None:
    """All views of depth[V,H,W] (intrinsics[V,4] = fx fy cx cy, extrinsics[V,12] = world -> camera rows) into the volume, in place, in one
    pass over it; origin / voxel_length / sdf_trunc are taken as float32.  See include/vfn.h for the arithmetic."""
    _tsdf_integrate(tsdf, weight, None, origin, voxel_length, sdf_trunc, depth, None, intrinsics, extrinsics)


def tsdf_integrate_rgb(tsdf: torch.Tensor, weight: torch.Tensor, colour: torch.Tensor, origin: Sequence[float], voxel_length: float,
                       sdf_trunc: float, depth: torch.Tensor, rgb: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor) -> None:
    """``tsdf_integrate`` with the views' images: rgb[V,H,W,3] uint8 into colour[nx,ny,nz,3] float32 (byte units), the running mean of the
    pixels whose depth updated the voxel.  tsdf / weight come out as ``tsdf_integrate`` leaves them.  See include/vfn.h."""
    _tsdf_integrate(tsdf, weight, colour, origin, voxel_length, sdf_trunc, depth, rgb, intrinsics, extrinsics)


def _tsdf_slot_colours(emit_colours, dev):
    """The ``per_slot`` of a coloured extraction: ``emit_colours`` launches the volume's ``*_emit_colours``, then every vertex takes its first slot's."""
    def colours_of(scanned, ids, n_vert):
        n_slots = ids.shape[0]
        tri_cols = torch.empty(n_slots, 3, dtype=torch.float64, device=dev)
        emit_colours(*scanned, _ptr(tri_cols, "tri_cols", torch.float64), _stream())
        first = torch.empty(max(n_vert, 1), dtype=torch.int32, device=dev)
        out = torch.empty(n_vert, 3, dtype=torch.float64, device=dev)
        _check(load().vfn_tsdf_vertex_colours(_ptr(ids, "ids", torch.int64), C.c_int64(n_slots), _ptr(tri_cols, "tri_cols", torch.float64),
                                              _ptr(first, "first", torch.int32), C.c_int64(n_vert),
                                              _ptr(out, "colours", torch.float64) if n_vert else None, _stream()), "vfn_tsdf_vertex_colours")
        return out

    return colours_of


def _tsdf_extract(count, emit, positions: int, dev, what: str, per_slot=None):
    """``_extract_slots`` for both volumes -> (vertices, faces) or, with ``per_slot``, (vertices, faces, colours [0,3] when empty)."""
    vertices, faces, colours = _extract_slots(count, emit, positions, dev, what, per_slot=per_slot)
    if per_slot is None:
        return vertices, faces
    return vertices, faces, colours if colours is not None else torch.empty(0, 3, dtype=torch.float64, device=dev)


def _tsdf_dense_extract(tsdf, weight, colour, origin, voxel_length):
    vol = _tsdf_volume_args(tsdf, weight)
    col = None if colour is None else _tsdf_colour_arg(tsdf, colour)
    per_slot = None if colour is None else _tsdf_slot_colours(
        lambda *out: _check(load().vfn_tsdf_emit_colours(*vol[:2], col, *vol[2:], *out), "vfn_tsdf_emit_colours"), tsdf.device)
    nx, ny, nz = tsdf.shape
    box = _f32s(*origin, voxel_length)
    return _tsdf_extract(lambda *out: _check(load().vfn_tsdf_count(*vol, *out), "vfn_tsdf_count"),
                         lambda *out: _check(load().vfn_tsdf_emit(*vol, *box, *out), "vfn_tsdf_emit"),
                         (nx - 1) * (ny - 1) * (nz - 1), tsdf.device, "TSDF extraction", per_slot)


def tsdf_extract(tsdf: torch.Tensor, weight: torch.Tensor, origin: Sequence[float], voxel_length: float):
    """The zero level set of the volume (csrc/vfn_tsdf.hip) through ``_tsdf_extract`` -> (vertices[n,3] float64, faces[m,3] int64, 0-based)."""
    return _tsdf_dense_extract(tsdf, weight, None, origin, voxel_length)


def tsdf_extract_coloured(tsdf: torch.Tensor, weight: torch.Tensor, colour: torch.Tensor, origin: Sequence[float], voxel_length: float):
    """``tsdf_extract`` with vertex colours -> (vertices, faces, colours[n,3] float64 in [0,1]): the vertices and faces are those of
    ``tsdf_extract``; a vertex takes the colour of the slot at which it first appears (include/vfn.h)."""
    return _tsdf_dense_extract(tsdf, weight, colour, origin, voxel_length)


# the block-sparse volume (include/vfn.h: "A block-sparse TSDF volume"; tsdf.SparseTSDFVolume owns the numbering and the tables)
TSDF_BLOCK = 8


def tsdf_block_lattice(dims: Sequence[int]):
    """ceil(dims / 8) per axis."""
    return tuple((int(n) + TSDF_BLOCK - 1) // TSDF_BLOCK for n in dims)


def tsdf_sparse_mark(marks: torch.Tensor, origin: Sequence[float], voxel_length: float, sdf_trunc: float, depth: torch.Tensor,
                     cameras: torch.Tensor) -> None:
    """marks[nbx,nby,nbz] uint8 (zeroed by the caller) gets a 1 in every block near a back-projected point of depth[V,H,W]; cameras[V,17]
    float64 = camera -> world rows, fx fy cx cy, q.  See include/vfn.h for the rule."""
    if marks.dim() != 3 or marks.numel() < 1 or marks.numel() >= (1 << 31):
        raise VfnError(f"marks must be [nbx,nby,nbz] with fewer than 2^31 blocks, got {tuple(marks.shape)}")
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1 or depth.shape[1] * depth.shape[2] >= (1 << 31):
        raise VfnError(f"depth must be [V,H,W] within the limits of one call, got {tuple(depth.shape)}")
    v, h, w = depth.shape
    if tuple(cameras.shape) != (v, 17):
        raise VfnError(f"{v} views need cameras [{v},17], got {tuple(cameras.shape)}")
    if depth.device != marks.device or cameras.device != marks.device:
        raise VfnError("the views and the marks live on different devices")
    with torch.cuda.device(marks.device):
        _check(load().vfn_tsdf_sparse_mark(_ptr(marks, "marks", torch.uint8), *(C.c_int32(n) for n in marks.shape),
                                           *_f32s(*origin, voxel_length, sdf_trunc), _ptr(depth, "depth"), C.c_int32(h), C.c_int32(w),
                                           _ptr(cameras, "cameras", torch.float64), C.c_int32(v), _stream()), "vfn_tsdf_sparse_mark")


def _tsdf_sparse_args(tsdf: torch.Tensor, weight: torch.Tensor, block_coords: torch.Tensor, dims: Sequence[int], block_of=None, colour=None):
    n = tsdf.shape[0] if tsdf.dim() == 4 else -1
    blk = (TSDF_BLOCK,) * 3
    if n < 0 or tuple(tsdf.shape[1:]) != blk or weight.shape != tsdf.shape or tuple(block_coords.shape) != (n, 3):
        raise VfnError(f"tsdf / weight must be [n,8,8,8] with block_coords [n,3], got {tuple(tsdf.shape)}, {tuple(weight.shape)} and "
                       f"{tuple(block_coords.shape)}")
    if n * TSDF_BLOCK ** 3 >= (1 << 31):
        raise VfnError(f"{n} blocks exceed the 2^31 voxel limit")
    if colour is not None and tuple(colour.shape) != tuple(tsdf.shape) + (3,):
        raise VfnError(f"colour must be [n,8,8,8,3], got {tuple(colour.shape)}")
    if block_of is not None and tuple(block_of.shape) != tsdf_block_lattice(dims):
        raise VfnError(f"block_of must be {tsdf_block_lattice(dims)} for dims {tuple(dims)}, got {tuple(block_of.shape)}")
    for t in (weight, block_coords, block_of, colour):
        if t is not None and t.device != tsdf.device:
            raise VfnError("the arrays of the sparse volume live on different devices")
    return n, tuple(C.c_int32(int(d)) for d in dims)


def tsdf_sparse_integrate(tsdf: torch.Tensor, weight: torch.Tensor, colour: Optional[torch.Tensor], block_coords: torch.Tensor,
                          dims: Sequence[int], origin: Sequence[float], voxel_length: float, sdf_trunc: float, depth: torch.Tensor,
                          rgb: Optional[torch.Tensor], intrinsics: torch.Tensor, extrinsics: torch.Tensor) -> None:
    """All views into every block of tsdf / weight [n,8,8,8] (colour [n,8,8,8,3] with rgb[V,H,W,3] uint8, or both None), in place: the
    dense volume's arithmetic at the global voxel index 8 block_coords + local.  See include/vfn.h."""
    if (colour is None) != (rgb is None):
        raise VfnError("colour and rgb go together")
    n, d3 = _tsdf_sparse_args(tsdf, weight, block_coords, dims, colour=colour)
    v, h, w = _tsdf_view_args(tsdf, depth, intrinsics, extrinsics, rgb)
    box = _f32s(*origin, voxel_length, sdf_trunc)
    views = (C.c_int32(h), C.c_int32(w), _ptr(intrinsics, "intrinsics"), _ptr(extrinsics, "extrinsics"), C.c_int32(v), _stream())
    name = "vfn_tsdf_sparse_integrate" if colour is None else "vfn_tsdf_sparse_integrate_rgb"
    with torch.cuda.device(tsdf.device):
        _check(getattr(load(), name)(_ptr(tsdf, "tsdf"), _ptr(weight, "weight"), *(() if colour is None else (_ptr(colour, "colour"),)),
                                     _ptr(block_coords, "block_coords", torch.int32), C.c_int32(n), *d3, *box, _ptr(depth, "depth"),
                                     *(() if rgb is None else (_ptr(rgb, "rgb", torch.uint8),)), *views), name)


def tsdf_sparse_extract(tsdf: torch.Tensor, weight: torch.Tensor, colour: Optional[torch.Tensor], block_of: torch.Tensor,
                        block_coords: torch.Tensor, dims: Sequence[int], origin: Sequence[float], voxel_length: float):
    """The zero level set of the blocks through ``_tsdf_extract`` -> (vertices, faces) or, with ``colour``, (vertices, faces, colours):
    the dense extraction's vertex bits, blocks in id order and cells in local C order."""
    n, d3 = _tsdf_sparse_args(tsdf, weight, block_coords, dims, block_of=block_of, colour=colour)
    dev = tsdf.device
    vol = (_ptr(tsdf, "tsdf"), _ptr(weight, "weight"))
    tables = (_ptr(block_of, "block_of", torch.int32), _ptr(block_coords, "block_coords", torch.int32), C.c_int32(n)) + d3
    box = _f32s(*origin, voxel_length)
    per_slot = None if colour is None else _tsdf_slot_colours(
        lambda *out: _check(load().vfn_tsdf_sparse_emit_colours(*vol, _ptr(colour, "colour"), *tables, *out), "vfn_tsdf_sparse_emit_colours"), dev)
    return _tsdf_extract(lambda *out: _check(load().vfn_tsdf_sparse_count(*vol, *tables, *out), "vfn_tsdf_sparse_count"),
                         lambda *out: _check(load().vfn_tsdf_sparse_emit(*vol, *tables, *box, *out), "vfn_tsdf_sparse_emit"),
                         n * TSDF_BLOCK ** 3, dev, "sparse TSDF extraction", per_slot)


# ------------------------------------------------------------------------------------------------
# depth rasteriser and Laplacian smoothing (csrc/vfn_raster.hip; vf_nerf_amd/raster.py and refuse.py are the public surface)
# ------------------------------------------------------------------------------------------------
def raster_depth(vertices: torch.Tensor, faces: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor, height: int, width: int,
                 near: float, far: float, pixel_centre: float):
    """vertices[n,3] float64, faces[m,3] int64, intrinsics[V,4] = fx fy cx cy, extrinsics[V,12] (float32) -> (depth[V,H,W] float32,
    counters) with counters = {"fragments", "atomics", "cooperative"} — see include/vfn.h for the arithmetic.  A face index outside
    [0, n) or a non-finite vertex raises (one status read), never faults."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise VfnError(f"vertices must be [n,3] and faces [m,3], got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    v = intrinsics.shape[0]
    if tuple(intrinsics.shape) != (v, 4) or tuple(extrinsics.shape) != (v, 12):
        raise VfnError(f"{v} views need intrinsics [{v},4] and extrinsics [{v},12], got {tuple(intrinsics.shape)} and {tuple(extrinsics.shape)}")
    h, w = int(height), int(width)
    if h < 1 or w < 1 or v * h * w >= (1 << 31):
        raise VfnError(f"{v} depth maps of {h} x {w} are outside the limits of one call")
    dev = intrinsics.device
    if not intrinsics.is_cuda:
        raise VfnError(f"intrinsics: expected a CUDA/HIP tensor, got {dev} (the HIP path has no CPU fallback)")
    for t in (vertices, faces, extrinsics):
        if t.device != dev:
            raise VfnError("the mesh and the views live on different devices")
    nv, nf = vertices.shape[0], faces.shape[0]
    with torch.cuda.device(dev):
        depth = torch.empty(v, h, w, dtype=torch.float32, device=dev)
        info = torch.zeros(4, dtype=torch.int64, device=dev)
        _check(load().vfn_raster_depth(_ptr(vertices, "vertices", torch.float64) if nv else None, C.c_int64(nv),
                                       _ptr(faces, "faces", torch.int64) if nf else None, C.c_int64(nf), _ptr(intrinsics, "intrinsics"),
                                       _ptr(extrinsics, "extrinsics"), C.c_int32(v), C.c_int32(h), C.c_int32(w), C.c_float(float(near)),
                                       C.c_float(float(far)), C.c_float(float(pixel_centre)), _ptr(depth, "depth"),
                                       _ptr(info, "info", torch.int64), _stream()), "vfn_raster_depth")
        status, fragments, atomics, cooperative = (int(x) for x in info.cpu()) if v else (0, 0, 0, 0)
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"depth rasteriser: a face index lies outside [0, {nv})")
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError("depth rasteriser: a non-finite vertex coordinate")
    return depth, {"fragments": fragments, "atomics": atomics, "cooperative": cooperative}


def smooth_laplacian(vertices: torch.Tensor, row_start: torch.Tensor, neighbours: torch.Tensor, iterations: int, lam: float) -> torch.Tensor:
    """``iterations`` Jacobi steps of vfn_smooth_laplacian_step over the CSR (row_start[n+1], neighbours, int64) between two buffers ->
    a new vertices[n,3] float64 tensor."""
    n = vertices.shape[0]
    if vertices.dim() != 2 or vertices.shape[1] != 3 or row_start.shape != (n + 1,):
        raise VfnError(f"vertices must be [n,3] with row_start [n+1], got {tuple(vertices.shape)} and {tuple(row_start.shape)}")
    if not vertices.is_cuda:
        raise VfnError(f"vertices: expected a CUDA/HIP tensor, got {vertices.device} (the HIP path has no CPU fallback)")
    a = vertices.clone()
    if n == 0 or iterations == 0:
        return a
    dev = vertices.device
    with torch.cuda.device(dev):
        b = torch.empty_like(a)
        info = torch.zeros(1, dtype=torch.int64, device=dev)
        nnz = neighbours.shape[0]
        for _ in range(iterations):
            _check(load().vfn_smooth_laplacian_step(_ptr(a, "src", torch.float64), _ptr(b, "dst", torch.float64), C.c_int64(n),
                                                    _ptr(row_start, "row_start", torch.int64),
                                                    _ptr(neighbours, "neighbours", torch.int64) if nnz else None, C.c_int64(nnz),
                                                    C.c_double(float(lam)), _ptr(info, "info", torch.int64), _stream()),
                   "vfn_smooth_laplacian_step")
            a, b = b, a
        if int(info.cpu()) != 0:
            raise VfnError("Laplacian smoothing: the adjacency names a vertex or a row outside its range")
    return a


# ------------------------------------------------------------------------------------------------
# mesh normals (csrc/vfn_normals.hip; vf_nerf_amd/meshops.py is the public surface).  Everything float64 / int64, contiguous, on one device.
# ------------------------------------------------------------------------------------------------
GEOM_STATUS_OVERFLOW = 4           # info bit of the normals unit: a length that overflowed


def normals_check(status: int, what: str) -> None:
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"{what}: an index lies outside its range")
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError(f"{what}: a non-finite coordinate or normal")
    if status & GEOM_STATUS_OVERFLOW:
        raise VfnError(f"{what}: a normal's length overflowed")


def _own_info(info: Optional[torch.Tensor], dev):
    return (info, False) if info is not None else (torch.zeros(1, dtype=torch.int64, device=dev), True)


def face_normals(vertices: torch.Tensor, faces: torch.Tensor, normalise: bool, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vertices[n,3] float64, faces[m,3] int64 -> [m,3]: the cross product of two edges, a unit vector with ``normalise`` (include/vfn.h:
    vfn_face_normals).  A bad input raises — or, with the caller's zero-filled ``info`` (int64 [1]), sets its bits (``normals_check``)."""
    n, m = vertices.shape[0], faces.shape[0]
    dev = faces.device
    out = torch.empty(m, 3, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_face_normals(_ptr(vertices, "vertices", torch.float64) if n else None, C.c_int64(n),
                                       _ptr(faces, "faces", torch.int64) if m else None, C.c_int64(m), C.c_int32(int(bool(normalise))),
                                       _ptr(out, "out", torch.float64) if m else None, _ptr(info, "info", torch.int64), _stream()),
               "vfn_face_normals")
    if own and m:
        normals_check(int(info.cpu()), "face normals")
    return out


def vertex_normals(face_normals_raw: torch.Tensor, row_start: torch.Tensor, incident: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The unnormalised face normals [m,3] and the incidence CSR (row_start[n+1], incident, int64) -> unit vertex normals [n,3]
    (include/vfn.h: vfn_vertex_normals).  ``info`` as in ``face_normals``."""
    m, n = face_normals_raw.shape[0], row_start.shape[0] - 1
    if n < 0:
        raise VfnError("vertex_normals: row_start must have n + 1 >= 1 entries")
    dev = row_start.device
    out = torch.empty(n, 3, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_vertex_normals(_ptr(face_normals_raw, "face_normals", torch.float64) if m else None, C.c_int64(m),
                                         _ptr(row_start, "row_start", torch.int64), _ptr(incident, "incident", torch.int64) if incident.shape[0] else None,
                                         C.c_int64(n), _ptr(out, "out", torch.float64) if n else None, _ptr(info, "info", torch.int64), _stream()),
               "vfn_vertex_normals")
    if own and n:
        normals_check(int(info.cpu()), "vertex normals")
    return out


def normal_dots(qn: torch.Tensor, tn: torch.Tensor, index: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qn[n,3], tn[m,3], index[n] int64 -> |qn[i] . tn[index[i]]| [n] (include/vfn.h: vfn_normal_dots).  ``info`` as in ``face_normals``."""
    n, m = qn.shape[0], tn.shape[0]
    if index.shape[0] != n:
        raise VfnError(f"normal_dots: index must have the queries' {n} rows")
    dev = qn.device
    out = torch.empty(n, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_normal_dots(_ptr(qn, "qn", torch.float64) if n else None, C.c_int64(n), _ptr(tn, "tn", torch.float64) if m else None,
                                      C.c_int64(m), _ptr(index, "index", torch.int64) if n else None,
                                      _ptr(out, "out", torch.float64) if n else None, _ptr(info, "info", torch.int64), _stream()),
               "vfn_normal_dots")
    if own and n:
        normals_check(int(info.cpu()), "normal dots")
    return out


# ------------------------------------------------------------------------------------------------
# voxel down-sampling (csrc/vfn_voxel.hip; vf_nerf_amd/voxel.py is the public surface).  Everything float64 / int64, contiguous, on one device.
# ------------------------------------------------------------------------------------------------
def voxel_limits():
    """-> (voxels per axis at most, channels of one means call at most): 2^VFN_VOXEL_AXIS_BITS, VFN_VOXEL_MAX_CHANNELS."""
    return 1 << header_constant("VFN_VOXEL_AXIS_BITS"), header_constant("VFN_VOXEL_MAX_CHANNELS")


def voxel_check(status: int, what: str = "voxel down-sampling") -> None:
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError(f"{what}: a non-finite coordinate")
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"{what}: a voxel index outside [0, 2^{header_constant('VFN_VOXEL_AXIS_BITS')}) or a segment outside its range")


def voxel_keys(points: torch.Tensor, origin, voxel_size: float, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """points[n,3], three host floats, the voxel edge -> keys[n] int64 (include/vfn.h: vfn_voxel_keys); -1 where a coordinate is not
    finite or a voxel index leaves [0, 2^21).  A bad input raises — or, with the caller's zero-filled ``info`` (int64 [1]), sets its
    bits (``voxel_check``)."""
    n = points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or len(origin) != 3:
        raise VfnError(f"voxel_keys: points must be [n,3] and origin three values, got {tuple(points.shape)} and {len(origin)}")
    dev = points.device
    ptr = _ptr(points, "points", torch.float64)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_voxel_keys(ptr, C.c_int64(n), (C.c_double * 3)(*(float(o) for o in origin)), C.c_double(voxel_size),
                                     _ptr(keys, "keys", torch.int64), _ptr(info, "info", torch.int64), _stream()), "vfn_voxel_keys")
    if own:
        voxel_check(int(info.cpu()))
    return keys


def voxel_means(sorted_values: torch.Tensor, start: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sorted_values[n,C] (1 <= C <= 9), start[V+1] int64 -> means[V,C]: every segment's serial sum in ascending position, started from
    its first row, over its count (include/vfn.h: vfn_voxel_means); NaN for a segment that is empty, decreasing or outside [0, n].
    ``info`` as in ``voxel_keys``."""
    if sorted_values.dim() != 2 or start.dim() != 1:
        raise VfnError(f"voxel_means: sorted_values must be [n,C] and start [V+1], got {tuple(sorted_values.shape)} and {tuple(start.shape)}")
    n, channels = sorted_values.shape
    n_voxels = start.shape[0] - 1
    if not 1 <= channels <= voxel_limits()[1]:
        raise VfnError(f"voxel_means: {channels} channels; one call takes 1 to {voxel_limits()[1]}")
    if not 1 <= n_voxels <= n:
        raise VfnError(f"voxel_means: start must have between 2 and n + 1 = {n + 1} entries, got {start.shape[0]}")
    dev = sorted_values.device
    ptr = _ptr(sorted_values, "sorted_values", torch.float64)
    means = torch.empty(n_voxels, channels, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_voxel_means(ptr, C.c_int64(n), C.c_int32(channels), _ptr(start, "start", torch.int64), C.c_int64(n_voxels),
                                      _ptr(means, "means", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_voxel_means")
    if own:
        voxel_check(int(info.cpu()))
    return means


# ------------------------------------------------------------------------------------------------
# connected components (csrc/vfn_cc.hip; vf_nerf_amd/meshops.py is the public surface).  Keys, nodes, tables int64, the forest int32,
# values float64; contiguous, on one device.
# ------------------------------------------------------------------------------------------------
def cc_check(status: int, what: str = "connected components") -> None:
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"{what}: a node, a parent or a segment lies outside its range")


def cc_union_runs(keys: torch.Tensor, nodes: torch.Tensor, parent: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sorted keys[k] with their nodes[k] (int64) and the forest parent[n] (int32, the caller's identity) -> parent, updated in place:
    where keys[i] == keys[i-1] >= 0 the trees of nodes[i-1] and nodes[i] are one (include/vfn.h: vfn_cc_union_runs).  A node outside
    [0, n) raises — or, with the caller's zero-filled ``info`` (int64 [1]), sets its bits (``cc_check``)."""
    if keys.dim() != 1 or nodes.dim() != 1 or parent.dim() != 1 or keys.shape[0] != nodes.shape[0]:
        raise VfnError(f"cc_union_runs: keys and nodes must be [k] and parent [n], got {tuple(keys.shape)}, {tuple(nodes.shape)} and "
                       f"{tuple(parent.shape)}")
    if keys.shape[0] < 1 or parent.shape[0] < 1:
        raise VfnError(f"cc_union_runs: {keys.shape[0]} items on {parent.shape[0]} nodes; both counts must be at least 1")
    dev = parent.device
    args = (_ptr(keys, "keys", torch.int64), _ptr(nodes, "nodes", torch.int64), C.c_int64(keys.shape[0]), _ptr(parent, "parent", torch.int32),
            C.c_int64(parent.shape[0]))
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_cc_union_runs(*args, _ptr(info, "info", torch.int64), _stream()), "vfn_cc_union_runs")
    if own:
        cc_check(int(info.cpu()))
    return parent


def cc_flatten(parent: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The forest parent[n] (int32) after the unions -> root[n] int64: where every node's chain ends (include/vfn.h: vfn_cc_flatten); -1
    where a parent leaves [0, its node].  ``info`` as in ``cc_union_runs``."""
    if parent.dim() != 1 or parent.shape[0] < 1:
        raise VfnError(f"cc_flatten: parent must be [n] with n >= 1, got {tuple(parent.shape)}")
    dev = parent.device
    ptr = _ptr(parent, "parent", torch.int32)
    root = torch.empty(parent.shape[0], dtype=torch.int64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_cc_flatten(ptr, C.c_int64(parent.shape[0]), _ptr(root, "root", torch.int64), _ptr(info, "info", torch.int64), _stream()),
               "vfn_cc_flatten")
    if own:
        cc_check(int(info.cpu()))
    return root


def cc_segment_sums(sorted_values: torch.Tensor, start: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sorted_values[n] float64, start[S+1] int64 -> sums[S]: every segment added by one wave in the fixed order of include/vfn.h
    (vfn_cc_segment_sums); NaN for a segment that is empty, decreasing or outside [0, n].  ``info`` as in ``cc_union_runs``."""
    if sorted_values.dim() != 1 or start.dim() != 1:
        raise VfnError(f"cc_segment_sums: sorted_values must be [n] and start [S+1], got {tuple(sorted_values.shape)} and {tuple(start.shape)}")
    n, segments = sorted_values.shape[0], start.shape[0] - 1
    if not 1 <= segments <= n:
        raise VfnError(f"cc_segment_sums: start must have between 2 and n + 1 = {n + 1} entries, got {start.shape[0]}")
    dev = sorted_values.device
    ptr = _ptr(sorted_values, "sorted_values", torch.float64)
    sums = torch.empty(segments, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_cc_segment_sums(ptr, C.c_int64(n), _ptr(start, "start", torch.int64), C.c_int64(segments),
                                          _ptr(sums, "sums", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_cc_segment_sums")
    if own:
        cc_check(int(info.cpu()))
    return sums


# ------------------------------------------------------------------------------------------------
# orientation (csrc/vfn_orient.hip; vf_nerf_amd/meshops.py is the public surface).  Keys, nodes, roots int64, the forest int32 holding
# (parent << 1) | parity, directions and parities uint8, votes float64; contiguous, on one device.
# ------------------------------------------------------------------------------------------------
ORIENT_VOLUME, ORIENT_VIEWPOINTS = 0, 1          # VFN_ORIENT_* of include/vfn.h
ORIENT_NODE_LIMIT = 1 << 30                      # a forest word holds the parent shifted by one bit


def orient_check(status: int, what: str = "orientation") -> None:
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"{what}: a node, a parent or a face index lies outside its range")
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError(f"{what}: a non-finite coordinate")


def orient_union_runs(keys: torch.Tensor, nodes: torch.Tensor, dirs: torch.Tensor, forest: torch.Tensor,
                      info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sorted keys[k] with their nodes[k] (int64) and direction bytes dirs[k] (uint8), and the forest[n] (int32, the caller's
    ``arange(n) << 1``) -> forest, updated in place: every run of exactly two equal keys >= 0 from two nodes unites them with the parity
    ``dirs[i-1] == dirs[i]`` (include/vfn.h: vfn_orient_union_runs).  A node outside [0, n) raises — or, with the caller's zero-filled
    ``info`` (int64 [1]), sets its bits (``orient_check``)."""
    if keys.dim() != 1 or nodes.dim() != 1 or dirs.dim() != 1 or forest.dim() != 1 or not keys.shape[0] == nodes.shape[0] == dirs.shape[0]:
        raise VfnError(f"orient_union_runs: keys, nodes and dirs must be [k] and forest [n], got {tuple(keys.shape)}, {tuple(nodes.shape)}, "
                       f"{tuple(dirs.shape)} and {tuple(forest.shape)}")
    if keys.shape[0] < 1 or not 1 <= forest.shape[0] < ORIENT_NODE_LIMIT:
        raise VfnError(f"orient_union_runs: {keys.shape[0]} items on {forest.shape[0]} nodes; at least 1 item, and nodes in [1, 2^30)")
    dev = forest.device
    args = (_ptr(keys, "keys", torch.int64), _ptr(nodes, "nodes", torch.int64), _ptr(dirs, "dirs", torch.uint8), C.c_int64(keys.shape[0]),
            _ptr(forest, "forest", torch.int32), C.c_int64(forest.shape[0]))
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_orient_union_runs(*args, _ptr(info, "info", torch.int64), _stream()), "vfn_orient_union_runs")
    if own:
        orient_check(int(info.cpu()))
    return forest


def orient_flatten(forest: torch.Tensor, info: Optional[torch.Tensor] = None):
    """The forest[n] (int32) after the unions -> (root[n] int64, parity[n] uint8): where every node's chain ends and the XOR of the
    parity bits along it (include/vfn.h: vfn_orient_flatten); (-1, 0) where a word is not ours.  ``info`` as in ``orient_union_runs``."""
    if forest.dim() != 1 or not 1 <= forest.shape[0] < ORIENT_NODE_LIMIT:
        raise VfnError(f"orient_flatten: forest must be [n] with n in [1, 2^30), got {tuple(forest.shape)}")
    dev = forest.device
    ptr = _ptr(forest, "forest", torch.int32)
    root = torch.empty(forest.shape[0], dtype=torch.int64, device=dev)
    parity = torch.empty(forest.shape[0], dtype=torch.uint8, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_orient_flatten(ptr, C.c_int64(forest.shape[0]), _ptr(root, "root", torch.int64), _ptr(parity, "parity", torch.uint8),
                                         _ptr(info, "info", torch.int64), _stream()), "vfn_orient_flatten")
    if own:
        orient_check(int(info.cpu()))
    return root, parity


def orient_votes(vertices: torch.Tensor, faces: torch.Tensor, parity: Optional[torch.Tensor], mode: int,
                 viewpoints: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vertices[n,3] float64, faces[m,3] int64 (m >= 1), parity[m] uint8 (None: all 0) -> votes[m] float64: every face's vote for the
    sign of its component, its corners 1 and 2 exchanged where ``parity`` is set (include/vfn.h: vfn_orient_votes).  ``mode`` is
    ``ORIENT_VOLUME`` (no viewpoints) or ``ORIENT_VIEWPOINTS`` (viewpoints[C,3] float64, C >= 1).  ``info`` as in ``orient_union_runs``."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise VfnError(f"orient_votes: vertices must be [n,3] and faces [m,3] with m >= 1, got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    if parity is not None and tuple(parity.shape) != (faces.shape[0],):
        raise VfnError(f"orient_votes: parity must be [{faces.shape[0]}], got {tuple(parity.shape)}")
    if mode not in (ORIENT_VOLUME, ORIENT_VIEWPOINTS):
        raise VfnError(f"orient_votes: mode must be ORIENT_VOLUME or ORIENT_VIEWPOINTS, got {mode!r}")
    if mode == ORIENT_VIEWPOINTS and (viewpoints is None or viewpoints.dim() != 2 or viewpoints.shape[1] != 3 or viewpoints.shape[0] < 1):
        raise VfnError(f"orient_votes: ORIENT_VIEWPOINTS takes viewpoints [C,3] with C >= 1, got "
                       f"{None if viewpoints is None else tuple(viewpoints.shape)}")
    if mode == ORIENT_VOLUME and viewpoints is not None:
        raise VfnError("orient_votes: ORIENT_VOLUME takes no viewpoints")
    n, m = vertices.shape[0], faces.shape[0]
    dev = faces.device
    args = (_ptr(vertices, "vertices", torch.float64) if n else None, C.c_int64(n), _ptr(faces, "faces", torch.int64), C.c_int64(m),
            _ptr(parity, "parity", torch.uint8), C.c_int32(mode), _ptr(viewpoints, "viewpoints", torch.float64),
            C.c_int64(0 if viewpoints is None else viewpoints.shape[0]))
    votes = torch.empty(m, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_orient_votes(*args, _ptr(votes, "votes", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_orient_votes")
    if own:
        orient_check(int(info.cpu()))
    return votes


# ------------------------------------------------------------------------------------------------
# vertex-clustering simplification (csrc/vfn_simplify.hip; vf_nerf_amd/meshops.py is the public surface).  Planes, centres, means and
# positions float64, indices and tables int64, the placed flags uint8; contiguous, on one device.
# ------------------------------------------------------------------------------------------------
def simplify_check(status: int, what: str = "mesh simplification") -> None:
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"{what}: a face index or a segment lies outside its range")
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError(f"{what}: a non-finite coordinate")
    if status & GEOM_STATUS_OVERFLOW:
        raise VfnError(f"{what}: a normal's length overflowed")


def face_planes(vertices: torch.Tensor, faces: torch.Tensor, origin, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vertices[n,3] float64, faces[m,3] int64 (m >= 1), three host floats -> planes[m,5]: every face's unit normal, its offset
    ``nrm . (v0 - origin)`` and its area; five +0.0 for a face without area (include/vfn.h: vfn_face_planes).  A bad input raises — or,
    with the caller's zero-filled ``info`` (int64 [1]), sets its bits (``simplify_check``)."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or len(origin) != 3:
        raise VfnError(f"face_planes: vertices must be [n,3], faces [m,3] with m >= 1 and origin three values, got {tuple(vertices.shape)}, "
                       f"{tuple(faces.shape)} and {len(origin)}")
    n, m = vertices.shape[0], faces.shape[0]
    dev = faces.device
    args = (_ptr(vertices, "vertices", torch.float64) if n else None, C.c_int64(n), _ptr(faces, "faces", torch.int64), C.c_int64(m),
            (C.c_double * 3)(*(float(o) for o in origin)))
    planes = torch.empty(m, 5, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_face_planes(*args, _ptr(planes, "planes", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_face_planes")
    if own:
        simplify_check(int(info.cpu()), "face planes")
    return planes


def cluster_quadrics(planes: torch.Tensor, item_face: torch.Tensor, start: torch.Tensor, centres: torch.Tensor, means: torch.Tensor, origin,
                     voxel_size: float, rcond: float, info: Optional[torch.Tensor] = None):
    """planes[m,5], item_face[k] and start[K+1] (int64), centres[K,3] and means[K,3], three host floats, the voxel edge and ``rcond`` ->
    (position[K,3] float64, placed[K] uint8, error[K] float64): every cluster's ten quadric sums added by one wave in the fixed order of
    include/vfn.h (vfn_cluster_quadrics), the minimiser by the adjugate, accepted inside its cell only; the mean otherwise.  NaN for a
    segment that is empty, decreasing or outside [0, k], or that names a face outside [0, m).  ``info`` as in ``face_planes``."""
    if planes.dim() != 2 or planes.shape[1] != 5 or planes.shape[0] < 1 or item_face.dim() != 1 or start.dim() != 1 or len(origin) != 3:
        raise VfnError(f"cluster_quadrics: planes must be [m,5] with m >= 1, item_face [k], start [K+1] and origin three values, got "
                       f"{tuple(planes.shape)}, {tuple(item_face.shape)}, {tuple(start.shape)} and {len(origin)}")
    m, items, clusters = planes.shape[0], item_face.shape[0], start.shape[0] - 1
    if not 1 <= clusters <= items:
        raise VfnError(f"cluster_quadrics: start must have between 2 and k + 1 = {items + 1} entries, got {start.shape[0]}")
    if tuple(centres.shape) != (clusters, 3) or tuple(means.shape) != (clusters, 3):
        raise VfnError(f"cluster_quadrics: centres and means must be [{clusters},3], got {tuple(centres.shape)} and {tuple(means.shape)}")
    dev = planes.device
    args = (_ptr(planes, "planes", torch.float64), C.c_int64(m), _ptr(item_face, "item_face", torch.int64), C.c_int64(items),
            _ptr(start, "start", torch.int64), C.c_int64(clusters), _ptr(centres, "centres", torch.float64), _ptr(means, "means", torch.float64),
            (C.c_double * 3)(*(float(o) for o in origin)), C.c_double(voxel_size), C.c_double(rcond))
    position = torch.empty(clusters, 3, dtype=torch.float64, device=dev)
    placed = torch.empty(clusters, dtype=torch.uint8, device=dev)
    error = torch.empty(clusters, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_cluster_quadrics(*args, _ptr(position, "position", torch.float64), _ptr(placed, "placed", torch.uint8),
                                           _ptr(error, "error", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_cluster_quadrics")
    if own:
        simplify_check(int(info.cpu()), "cluster quadrics")
    return position, placed, error


# ------------------------------------------------------------------------------------------------
# quadric edge-collapse decimation (csrc/vfn_collapse.hip; vf_nerf_amd/decimate.py is the public surface).  Planes, quadrics, points
# and costs float64, indices and tables int64, the flags uint8; contiguous, on one device.
# ------------------------------------------------------------------------------------------------
COLLAPSE_CANDIDATE, COLLAPSE_ACCEPTED, COLLAPSE_NONMANIFOLD, COLLAPSE_NONFINITE, COLLAPSE_OVER, COLLAPSE_FLIP = 1, 2, 4, 8, 16, 32
COLLAPSE_NO_EDGE = (1 << 63) - 1          # best_edge of a vertex without a candidate


def collapse_check(status: int, what: str = "edge collapse") -> None:
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"{what}: an index, a row or a segment lies outside its range")
    if status & GEOM_STATUS_NONFINITE:
        raise VfnError(f"{what}: a non-finite coordinate or quadric")
    if status & GEOM_STATUS_OVERFLOW:
        raise VfnError(f"{what}: a normal's length overflowed")


def boundary_planes(vertices: torch.Tensor, planes: torch.Tensor, face: torch.Tensor, start: torch.Tensor, end: torch.Tensor, origin,
                    boundary_weight: float, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vertices[n,3], the face planes[m,5], and per boundary edge its face and its two corners in the face's order (int64 [B], B >= 1)
    -> rows[B,5]: the plane through the edge perpendicular to its face, weighted ``boundary_weight`` times the face's area; five +0.0
    for an edge or a face without length (include/vfn.h: vfn_boundary_planes).  ``info`` as in ``face_planes``."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or planes.dim() != 2 or planes.shape[1] != 5 or face.dim() != 1 or face.shape[0] < 1 \
            or start.shape != face.shape or end.shape != face.shape or len(origin) != 3:
        raise VfnError(f"boundary_planes: vertices must be [n,3], planes [m,5], face / start / end [B] with B >= 1 and origin three values, got "
                       f"{tuple(vertices.shape)}, {tuple(planes.shape)}, {tuple(face.shape)}, {tuple(start.shape)}, {tuple(end.shape)} and {len(origin)}")
    count, dev = face.shape[0], planes.device
    args = (_ptr(vertices, "vertices", torch.float64), C.c_int64(vertices.shape[0]), _ptr(planes, "planes", torch.float64), C.c_int64(planes.shape[0]),
            _ptr(face, "face", torch.int64), _ptr(start, "start", torch.int64), _ptr(end, "end", torch.int64), C.c_int64(count),
            (C.c_double * 3)(*(float(o) for o in origin)), C.c_double(boundary_weight))
    out = torch.empty(count, 5, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_boundary_planes(*args, _ptr(out, "out", torch.float64), _ptr(info, "info", torch.int64), _stream()), "vfn_boundary_planes")
    if own:
        collapse_check(int(info.cpu()), "boundary planes")
    return out


def vertex_quadrics(planes: torch.Tensor, item_row: torch.Tensor, start: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """planes[R,5], item_row[k] and start[n+1] (int64) -> quadrics[n,10]: every vertex's ten sums over its rows, one lane a vertex, added
    serially from the first row (include/vfn.h: vfn_vertex_quadrics); ten +0.0 for a vertex without rows."""
    if planes.dim() != 2 or planes.shape[1] != 5 or planes.shape[0] < 1 or item_row.dim() != 1 or item_row.shape[0] < 1 or start.dim() != 1 \
            or start.shape[0] < 2:
        raise VfnError(f"vertex_quadrics: planes must be [R,5] with R >= 1, item_row [k] with k >= 1 and start [n+1] with n >= 1, got "
                       f"{tuple(planes.shape)}, {tuple(item_row.shape)} and {tuple(start.shape)}")
    n, dev = start.shape[0] - 1, planes.device
    args = (_ptr(planes, "planes", torch.float64), C.c_int64(planes.shape[0]), _ptr(item_row, "item_row", torch.int64), C.c_int64(item_row.shape[0]),
            _ptr(start, "start", torch.int64), C.c_int64(n))
    quadrics = torch.empty(n, 10, dtype=torch.float64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_vertex_quadrics(*args, _ptr(quadrics, "quadrics", torch.float64), _ptr(info, "info", torch.int64), _stream()),
               "vfn_vertex_quadrics")
    if own:
        collapse_check(int(info.cpu()), "vertex quadrics")
    return quadrics


def edge_collapse_candidates(vertices: torch.Tensor, faces: torch.Tensor, quadrics: torch.Tensor, item_row: torch.Tensor, start: torch.Tensor,
                             rows: int, edge_a: torch.Tensor, edge_b: torch.Tensor, run: torch.Tensor, origin, rcond: float, reach: float,
                             max_error: float, info: Optional[torch.Tensor] = None):
    """-> (point[E,3], cost[E], s[E] float64, flags[E] uint8): what the collapse of every edge would do, one lane an edge — the minimiser
    of the two ends' quadrics or the best of (midpoint, a, b), its cost, the attribute parameter, and whether the edge is a candidate
    (``COLLAPSE_*`` bits; include/vfn.h: vfn_edge_collapse_candidates).  ``max_error`` = inf: no bound."""
    n, m, count = vertices.shape[0], faces.shape[0], edge_a.shape[0]
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or tuple(quadrics.shape) != (n, 10) \
            or item_row.dim() != 1 or tuple(start.shape) != (n + 1,) or edge_a.dim() != 1 or edge_b.shape != edge_a.shape or run.shape != edge_a.shape \
            or len(origin) != 3:
        raise VfnError(f"edge_collapse_candidates: vertices must be [n,3], faces [m,3], quadrics [n,10], item_row [k], start [n+1], edge_a / edge_b / "
                       f"run [E] and origin three values, got {tuple(vertices.shape)}, {tuple(faces.shape)}, {tuple(quadrics.shape)}, "
                       f"{tuple(item_row.shape)}, {tuple(start.shape)}, {tuple(edge_a.shape)}, {tuple(edge_b.shape)}, {tuple(run.shape)} and {len(origin)}")
    if n < 1 or m < 1 or count < 1 or item_row.shape[0] < 1:
        raise VfnError("edge_collapse_candidates: at least one vertex, face, item and edge")
    dev = vertices.device
    args = (_ptr(vertices, "vertices", torch.float64), C.c_int64(n), _ptr(faces, "faces", torch.int64), C.c_int64(m),
            _ptr(quadrics, "quadrics", torch.float64), _ptr(item_row, "item_row", torch.int64), C.c_int64(item_row.shape[0]),
            _ptr(start, "start", torch.int64), C.c_int64(rows), _ptr(edge_a, "edge_a", torch.int64), _ptr(edge_b, "edge_b", torch.int64),
            _ptr(run, "run", torch.int64), C.c_int64(count), (C.c_double * 3)(*(float(o) for o in origin)), C.c_double(rcond), C.c_double(reach),
            C.c_double(max_error))
    point = torch.empty(count, 3, dtype=torch.float64, device=dev)
    cost = torch.empty(count, dtype=torch.float64, device=dev)
    s = torch.empty(count, dtype=torch.float64, device=dev)
    flags = torch.empty(count, dtype=torch.uint8, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_edge_collapse_candidates(*args, _ptr(point, "point", torch.float64), _ptr(cost, "cost", torch.float64),
                                                   _ptr(s, "s", torch.float64), _ptr(flags, "flags", torch.uint8), _ptr(info, "info", torch.int64),
                                                   _stream()), "vfn_edge_collapse_candidates")
    if own:
        collapse_check(int(info.cpu()), "edge collapse candidates")
    return point, cost, s, flags


def collapse_select(cost: torch.Tensor, flags: torch.Tensor, edge_a: torch.Tensor, edge_b: torch.Tensor, faces: torch.Tensor, n: int,
                    info: Optional[torch.Tensor] = None):
    """-> (best_edge[n] int64, proposed[E], withdrawn[E] uint8): every vertex's lowest (cost, edge) among its candidates
    (``COLLAPSE_NO_EDGE``: none), the edges both of whose ends chose them, and of those the ones some face withdrew in favour of a lower
    one (include/vfn.h: vfn_collapse_select).  A function of the costs alone."""
    count = cost.shape[0]
    if cost.dim() != 1 or count < 1 or flags.shape != cost.shape or edge_a.shape != cost.shape or edge_b.shape != cost.shape or faces.dim() != 2 \
            or faces.shape[1] != 3 or faces.shape[0] < 1 or n < 1:
        raise VfnError(f"collapse_select: cost / flags / edge_a / edge_b must be [E] with E >= 1, faces [m,3] with m >= 1 and n >= 1, got "
                       f"{tuple(cost.shape)}, {tuple(flags.shape)}, {tuple(edge_a.shape)}, {tuple(edge_b.shape)}, {tuple(faces.shape)} and {n}")
    dev = cost.device
    args = (_ptr(cost, "cost", torch.float64), _ptr(flags, "flags", torch.uint8), _ptr(edge_a, "edge_a", torch.int64), _ptr(edge_b, "edge_b", torch.int64),
            C.c_int64(count), _ptr(faces, "faces", torch.int64), C.c_int64(faces.shape[0]), C.c_int64(n))
    best_cost = torch.empty(n, dtype=torch.int64, device=dev)
    best_edge = torch.empty(n, dtype=torch.int64, device=dev)
    proposed = torch.empty(count, dtype=torch.uint8, device=dev)
    withdrawn = torch.empty(count, dtype=torch.uint8, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_collapse_select(*args, _ptr(best_cost, "best_cost", torch.int64), _ptr(best_edge, "best_edge", torch.int64), _ptr(proposed, "proposed", torch.uint8),
                                          _ptr(withdrawn, "withdrawn", torch.uint8), _ptr(info, "info", torch.int64), _stream()), "vfn_collapse_select")
    if own:
        collapse_check(int(info.cpu()), "collapse selection")
    return best_edge, proposed, withdrawn


# ------------------------------------------------------------------------------------------------
# k-means (csrc/vfn_kmeans.hip; vf_nerf_amd/cluster.py is the public surface).  Points, centres, sums and distances float64, labels
# int32, counts and indices int64; contiguous, on one device.
# ------------------------------------------------------------------------------------------------
def kmeans_max_k() -> int:
    return header_constant("VFN_KMEANS_MAX_K")


def kmeans_check(status: int, what: str = "k-means") -> None:
    if status & GEOM_STATUS_NONFINITE:          # (first: a NaN leaves the seeding without a farthest point, which then shows as a bad index)
        raise VfnError(f"{what}: a non-finite coordinate")
    if status & GEOM_STATUS_INDEX:
        raise VfnError(f"{what}: a label or an index lies outside its range")


def _kmeans_points(points: torch.Tensor, what: str) -> int:
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise VfnError(f"{what}: points must be [n,3] with n >= 1, got {tuple(points.shape)}")
    return points.shape[0]


def kmeans_assign(points: torch.Tensor, centres: torch.Tensor, previous: Optional[torch.Tensor], label: torch.Tensor, sqdist: torch.Tensor,
                  changed: torch.Tensor, info: Optional[torch.Tensor] = None) -> None:
    """points[n,3] and centres[k,3] float64 -> label[n] (int32) = every point's nearest centre, ties to the lowest, sqdist[n] its squared
    distance; changed (int64 [1]) is INCREASED by the number of labels that differ from ``previous`` (int32 [n]; None: every point; it
    may be ``label`` itself) — include/vfn.h: vfn_kmeans_assign.  A bad input raises — or, with the caller's zero-filled ``info`` (int64
    [1]), sets its bits (``kmeans_check``)."""
    n = _kmeans_points(points, "kmeans_assign")
    if centres.dim() != 2 or centres.shape[1] != 3 or not 1 <= centres.shape[0] <= kmeans_max_k():
        raise VfnError(f"kmeans_assign: centres must be [k,3] with 1 <= k <= {kmeans_max_k()}, got {tuple(centres.shape)}")
    if tuple(label.shape) != (n,) or tuple(sqdist.shape) != (n,) or (previous is not None and tuple(previous.shape) != (n,)) or changed.numel() != 1:
        raise VfnError(f"kmeans_assign: label, sqdist and previous must have the points' {n} rows and changed one word")
    dev, rows = points.device, _ptr(points, "points", torch.float64)          # (a host tensor is refused here, before a device is asked for)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        _check(load().vfn_kmeans_assign(rows, C.c_int64(n), _ptr(centres, "centres", torch.float64),
                                        C.c_int32(centres.shape[0]), _ptr(previous, "previous", torch.int32), _ptr(label, "label", torch.int32),
                                        _ptr(sqdist, "sqdist", torch.float64), _ptr(changed, "changed", torch.int64), _ptr(info, "info", torch.int64),
                                        _stream()), "vfn_kmeans_assign")
    if own:
        kmeans_check(int(info.cpu()), "k-means (assign)")


def _kmeans_ws(fn_name: str, dev, *sizes) -> torch.Tensor:
    need = getattr(load(), fn_name)(*sizes)
    if need < 0:
        raise VfnError(f"{fn_name}{sizes}: {load().vfn_last_error().decode()}")
    return torch.empty(max(int(need), 8), dtype=torch.uint8, device=dev)


def kmeans_update(points: torch.Tensor, label: torch.Tensor, centres: torch.Tensor, info: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None):
    """points[n,3] float64, label[n] int32 and centres[k,3] float64 (READ AND WRITTEN) -> (sums[k,3] float64, count[k] int64): every
    cluster's coordinate sums along the fixed tree, lane order "near", its exact count, and centres[j] = sums[j] / count[j] where the
    count is not 0 — an empty cluster's row keeps its bits (include/vfn.h: vfn_kmeans_update).  ``workspace``: ``kmeans_update_workspace``'s
    bytes, for a caller that loops.  ``info`` as in ``kmeans_assign``; a label outside [0, k) sets bit 2 and joins no cluster."""
    n = _kmeans_points(points, "kmeans_update")
    if centres.dim() != 2 or centres.shape[1] != 3 or not 1 <= centres.shape[0] <= kmeans_max_k():
        raise VfnError(f"kmeans_update: centres must be [k,3] with 1 <= k <= {kmeans_max_k()}, got {tuple(centres.shape)}")
    if tuple(label.shape) != (n,):
        raise VfnError(f"kmeans_update: label must have the points' {n} rows, got {tuple(label.shape)}")
    k, dev, rows = centres.shape[0], points.device, _ptr(points, "points", torch.float64)
    sums = torch.empty(k, 3, dtype=torch.float64, device=dev)
    count = torch.empty(k, dtype=torch.int64, device=dev)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        ws = workspace if workspace is not None else kmeans_update_workspace(n, k, dev)
        _check(load().vfn_kmeans_update(rows, C.c_int64(n), _ptr(label, "label", torch.int32), C.c_int32(k),
                                        _ptr(sums, "sums", torch.float64), _ptr(count, "count", torch.int64), _ptr(centres, "centres", torch.float64),
                                        _ptr(info, "info", torch.int64), _ptr(ws, "workspace", torch.uint8), C.c_int64(ws.numel()), _stream()),
               "vfn_kmeans_update")
    if own:
        kmeans_check(int(info.cpu()), "k-means (update)")
    return sums, count


def kmeans_update_workspace(n: int, k: int, dev) -> torch.Tensor:
    with torch.cuda.device(dev):
        return _kmeans_ws("vfn_kmeans_update_workspace_bytes", dev, C.c_int64(n), C.c_int32(k))


def kmeans_seed_workspace(n: int, dev) -> torch.Tensor:
    with torch.cuda.device(dev):
        return _kmeans_ws("vfn_kmeans_seed_workspace_bytes", dev, C.c_int64(n))


def kmeans_seed(points: torch.Tensor, newest: Optional[torch.Tensor], first: bool, mind2: torch.Tensor, farthest: Optional[torch.Tensor],
                info: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> None:
    """One seeding step on the device (include/vfn.h: vfn_kmeans_seed): ``newest`` (int64 [1], DEVICE) names the point that became a
    centre last; mind2[n] = its squared distance (``first``) or the minimum of that and what mind2 held; ``farthest`` (int64 [1]) gets
    the index of the greatest mind2, ties to the lowest index.  ``newest`` None: mind2 is only read.  ``farthest`` None: mind2 is only
    written.  An index outside [0, n) sets bit 2 of ``info`` (as in ``kmeans_assign``), writes -1 and reads nothing through it."""
    n = _kmeans_points(points, "kmeans_seed")
    if tuple(mind2.shape) != (n,) or (newest is not None and newest.numel() != 1) or (farthest is not None and farthest.numel() != 1) \
            or (newest is None and farthest is None):
        raise VfnError(f"kmeans_seed: mind2 must have the points' {n} rows, newest and farthest one word each (one of them may be None)")
    dev, rows = points.device, _ptr(points, "points", torch.float64)
    info, own = _own_info(info, dev)
    with torch.cuda.device(dev):
        ws = None if farthest is None else workspace if workspace is not None else kmeans_seed_workspace(n, dev)
        _check(load().vfn_kmeans_seed(rows, C.c_int64(n), _ptr(newest, "newest", torch.int64),
                                      C.c_int32(int(bool(first))), _ptr(mind2, "mind2", torch.float64), _ptr(farthest, "farthest", torch.int64),
                                      _ptr(info, "info", torch.int64), _ptr(ws, "workspace", torch.uint8), C.c_int64(0 if ws is None else ws.numel()),
                                      _stream()), "vfn_kmeans_seed")
    if own:
        kmeans_check(int(info.cpu()), "k-means (seed)")


# ------------------------------------------------------------------------------------------------
# networks in training mode: batch-statistics BatchNorm, one launch per layer (csrc/vfn_bstat.hip)
# ------------------------------------------------------------------------------------------------
class Cols:
    """Columns [col0, col0 + ...) of a contiguous row-major fp32 matrix: what the row-wise entry points take as
    (pointer, leading dimension)."""

    def __init__(self, base: torch.Tensor, col0: int = 0) -> None:
        if not (base.is_cuda and base.dtype == torch.float32 and base.is_contiguous() and base.dim() == 2):
            raise VfnError("Cols: expected a contiguous 2-D fp32 CUDA/HIP tensor (the HIP path has no CPU fallback)")
        self.base, self.col0, self.ld = base, col0, base.shape[1]

    @property
    def ptr(self) -> C.c_void_p:
        return C.c_void_p(self.base.data_ptr() + 4 * self.col0)

    # what _ptr() asks of a tensor, so that the (pointer, ld) entry points written for whole tensors take column views too
    is_cuda, dtype = True, torch.float32

    def is_contiguous(self) -> bool:
        return True

    def data_ptr(self) -> int:
        return self.base.data_ptr() + 4 * self.col0


def _cols(x) -> "Cols":
    return x if isinstance(x, Cols) else Cols(x)


ACT_NONE, ACT_TANH, ACT_SIGMOID = 0, 1, 2


def linear_rows_stat_parts(m: int) -> int:
    return int(load().vfn_linear_rows_stat_parts(m))


def bstat_row_parts(m: int) -> int:
    return int(load().vfn_bstat_row_parts(m))


GEMM_EXACT, GEMM_SPLIT_F16, GEMM_SPLIT_BF16, GEMM_BF16X6 = 0, 2, 4, 6      # arithmetic of vfn_linear_rows (bits 1-2 of its first argument)


_wplanes_cache: dict = {}


def wplanes(n_out: int, k_in: int, device) -> torch.Tensor:
    """The scratch the split layer products put W's 16-bit planes into (vfn_linear_rows_ws): one buffer per device AND stream, grown on
    demand — calls on one stream use it one after the other; calls on different streams must not share it."""
    need = int(load().vfn_linear_rows_wplanes_bytes(C.c_int32(n_out), C.c_int32(k_in)))
    key = (str(device), int(_stream().value or 0))
    buf = _wplanes_cache.get(key)
    if buf is None or buf.numel() < need:
        buf = _wplanes_cache[key] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=device)
    return buf


def linear_rows(a, w: torch.Tensor, bias, m: int, n_out: int, k_in: int, c, act: int = ACT_NONE, transpose_w: bool = False,
                stats_part=None, arith: int = GEMM_EXACT, planes=None) -> None:
    """``arith``: GEMM_EXACT (fp32 matrix instruction), GEMM_SPLIT_F16 (three f16 products per product, 22 bits: forward GEMMs on
    normalised activations), GEMM_SPLIT_BF16 (three bf16 products, 16 bits with fp32's exponent range) or GEMM_BF16X6 (operands in three
    bf16 parts, six products: 24 bits at fp32's exponent range, fp32-equivalent — backward GEMMs on gradients of any magnitude)."""
    a, c = _cols(a), _cols(c)
    _check(load().vfn_linear_rows_ws(C.c_int32(int(transpose_w) | int(arith)), a.ptr, C.c_int32(a.ld), _ptr(w, "w"), C.c_int32(w.shape[1]),
                                     _ptr(bias, "bias"), C.c_int64(m), C.c_int32(n_out), C.c_int32(k_in), C.c_int32(act), c.ptr,
                                     C.c_int32(c.ld), _ptr(stats_part, "stats_part"), _ptr(planes, "planes", torch.uint8), _stream()),
           "vfn_linear_rows")


def linear_rows_fold(z_prev, coef_prev: torch.Tensor, n_prev: int, post_prev: float, w: torch.Tensor, bias, m: int, n_out: int, k_in: int, c,
                     stats_part=None, arith: int = GEMM_SPLIT_F16, planes=None) -> None:
    """The forward product of a layer whose input is act(z_prev) — the previous layer's BatchNorm + ReLU (+ the skip layer's encoding
    columns behind the first ``n_prev``) — formed inside the product's operand read (include/vfn.h, vfn_linear_rows_fold)."""
    z_prev, c = _cols(z_prev), _cols(c)
    if coef_prev.numel() < 2 * n_prev or n_prev > k_in:
        raise VfnError(f"linear_rows_fold: coefficients of {coef_prev.numel()} floats for n_prev = {n_prev} (needs scale | shift rows), k_in = {k_in}")
    _check(load().vfn_linear_rows_fold(C.c_int32(int(arith)), z_prev.ptr, C.c_int32(z_prev.ld), _ptr(coef_prev, "coef_prev"), C.c_int32(n_prev),
                                       C.c_float(post_prev), _ptr(w, "w"), C.c_int32(w.shape[1]), _ptr(bias, "bias"), C.c_int64(m), C.c_int32(n_out),
                                       C.c_int32(k_in), c.ptr, C.c_int32(c.ld), _ptr(stats_part, "stats_part"), _ptr(planes, "planes", torch.uint8),
                                       _stream()), "vfn_linear_rows_fold")


def linear_rows_dx_sums(dz, w: torch.Tensor, m: int, n_out: int, k_in: int, c, z_prev, coef_prev: torch.Tensor, n_prev: int, post_prev: float,
                        part: torch.Tensor, arith: int = 4, planes=None) -> None:
    """C = dZ W (``arith``: GEMM_SPLIT_BF16 = three bf16 products, GEMM_BF16X6 = bf16 in three parts) + the per-workgroup partials of the previous layer's BatchNorm-backward column sums, taken from C
    in registers (include/vfn.h, vfn_linear_rows_dx_sums); ``part`` [linear_rows_stat_parts(m), 2, n_prev]."""
    dz, c, z_prev = _cols(dz), _cols(c), _cols(z_prev)
    _check(load().vfn_linear_rows_dx_sums(dz.ptr, C.c_int32(dz.ld), _ptr(w, "w"), C.c_int32(w.shape[1]), C.c_int64(m), C.c_int32(n_out),
                                          C.c_int32(k_in), c.ptr, C.c_int32(c.ld), z_prev.ptr, C.c_int32(z_prev.ld), _ptr(coef_prev, "coef_prev"),
                                          C.c_int32(n_prev), C.c_float(post_prev), _ptr(part, "part"), C.c_int32(int(arith)),
                                          _ptr(planes, "planes", torch.uint8), _stream()), "vfn_linear_rows_dx_sums")


def colsum_finish(part: torch.Tensor, n_parts: int, width: int, sums: torch.Tensor) -> None:
    _check(load().vfn_colsum_finish(_ptr(part, "part"), C.c_int64(n_parts), C.c_int32(width), _ptr(sums, "sums", torch.float64),
                                    _stream()), "vfn_colsum_finish")


def bstat_finalize(sums, m: int, n: int, gamma, beta, eps: float, momentum: float, running_mean, running_var, coef) -> None:
    _check(load().vfn_bstat_finalize(_ptr(sums, "sums", torch.float64), C.c_int64(m), C.c_int32(n), _ptr(gamma, "gamma"),
                                     _ptr(beta, "beta"), C.c_float(eps), C.c_float(momentum), _ptr(running_mean, "running_mean"),
                                     _ptr(running_var, "running_var"), _ptr(coef, "coef"), _stream()), "vfn_bstat_finalize")


def bstat_relu_rows(z, coef, m: int, n: int, post_scale: float, h) -> None:
    z, h = _cols(z), _cols(h)
    _check(load().vfn_bstat_relu_rows(z.ptr, C.c_int32(z.ld), _ptr(coef, "coef"), C.c_int64(m), C.c_int32(n),
                                      C.c_float(post_scale), h.ptr, C.c_int32(h.ld), _stream()), "vfn_bstat_relu_rows")


def bstat_relu_bwd_sums(g, z, coef, m: int, n: int, post_scale: float, part) -> None:
    g, z = _cols(g), _cols(z)
    _check(load().vfn_bstat_relu_bwd_sums(g.ptr, C.c_int32(g.ld), z.ptr, C.c_int32(z.ld),
                                          _ptr(coef, "coef"), C.c_int64(m), C.c_int32(n), C.c_float(post_scale),
                                          _ptr(part, "part"), _stream()), "vfn_bstat_relu_bwd_sums")


def bstat_relu_bwd_rows(g, z, coef, sums, m: int, n: int, post_scale: float, dz) -> None:
    g, z, dz = _cols(g), _cols(z), _cols(dz)
    _check(load().vfn_bstat_relu_bwd_rows(g.ptr, C.c_int32(g.ld), z.ptr, C.c_int32(z.ld),
                                          _ptr(coef, "coef"), _ptr(sums, "sums", torch.float64), C.c_int64(m), C.c_int32(n),
                                          C.c_float(post_scale), dz.ptr, C.c_int32(dz.ld), _stream()), "vfn_bstat_relu_bwd_rows")


def act_bwd_rows(act: int, dy, y, m: int, n: int, dz, onehot_col: int = -1) -> None:
    y, dz = _cols(y), _cols(dz)
    dy = None if dy is None else _cols(dy)
    _check(load().vfn_act_bwd_rows(C.c_int32(act), dy.ptr if dy is not None else C.c_void_p(0),
                                   C.c_int32(dy.ld if dy is not None else 0), y.ptr, C.c_int32(y.ld), C.c_int64(m), C.c_int32(n),
                                   C.c_int32(onehot_col), dz.ptr, C.c_int32(dz.ld), _stream()), "vfn_act_bwd_rows")


def embed_rows(src, m: int, multires: int, dst, scale: float = 1.0, rows_per_src: int = 1) -> None:
    src, dst = _cols(src), _cols(dst)
    _check(load().vfn_embed_rows(src.ptr, C.c_int32(src.ld), C.c_int32(rows_per_src), C.c_int64(m), C.c_int32(multires),
                                 C.c_float(scale), C.c_void_p(dst.base.data_ptr()), C.c_int32(dst.ld), C.c_int32(dst.col0),
                                 _stream()), "vfn_embed_rows")


def embed_rows_bwd(src3: torch.Tensor, m: int, multires: int, d_a, scale_a: float, d_b, scale_b: float, d_src3: torch.Tensor,
                   accumulate: bool = False) -> None:
    d_a = _cols(d_a)
    d_b = None if d_b is None else _cols(d_b)
    _check(load().vfn_embed_rows_bwd(_ptr(src3, "src3"), C.c_int64(m), C.c_int32(multires), d_a.ptr, C.c_int32(d_a.ld),
                                     C.c_int32(0), C.c_float(scale_a), d_b.ptr if d_b is not None else C.c_void_p(0),
                                     C.c_int32(d_b.ld if d_b is not None else 0), C.c_int32(0), C.c_float(scale_b),
                                     _ptr(d_src3, "d_src3"), C.c_int32(int(accumulate)), _stream()), "vfn_embed_rows_bwd")
