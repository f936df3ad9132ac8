"""``import vf_nerf_amd.dropin`` makes the reference's own import paths resolve to this implementation:

    import vf_nerf_amd.dropin                       # once, before the reference trainer/evaluator imports
    from models.nerf.vector_field_nerf import VectorFieldNerf      # -> vf_nerf_amd.nerf.VectorFieldNerf

so ``train/vector_field_nerf_train.py`` and ``evaluation/*`` run unchanged on the HIP path.  Only the modules
on the hot path are aliased; everything else (datasets, loss, config parser, mesh extraction)
keeps coming from the reference tree.  If the reference package is importable, its ``models`` / ``utils``
packages stay in place and only the leaf modules are replaced."""
from __future__ import annotations

import importlib
import sys
import types

from . import bases, density, evaluator, grid, loss, mesh, meshops, nerf, networks, render_output, samplers, supervision, voxel

_ALIASES = {
    "models.nerf.vector_field_nerf": nerf,
    "models.nerf.output": render_output,
    "models.vector_field.vector_field_network": networks,
    "models.vector_field.rendering_network": networks,
    "models.samplers.ray_sampler": samplers,
    "models.helpers.density_functions": density,
}


def _ensure_package(name: str) -> None:
    if name in sys.modules:
        return
    try:
        importlib.import_module(name)
    except Exception:
        pkg = types.ModuleType(name)
        pkg.__path__ = []  # namespace-like placeholder
        sys.modules[name] = pkg


def install(patch_evaluator: bool = True, patch_clip: bool = True, deferred_scalars=None, patch_mesh: bool = True,
            patch_metrics: bool = False, patch_tsdf_mesh: bool = False, tsdf_vertex_normals=None, tsdf_sparse=None,
            tsdf_min_component_faces=None, tsdf_simplify_voxel=None, dominant_bases_decimation=None, tsdf_simplify_faces=None,
            patch_dominant_bases: bool = False, mesh_orient=None) -> None:
    """``patch_clip=False`` leaves ``torch.nn.utils.clip_grad_norm_`` PyTorch's own function (no process-wide replacement): a step session then
    parks its gradient in the optimizer's flat buffer with every ``param.grad`` None, the trainer's clip call finds nothing to scale, and
    ``optimizer.step()`` all-reduces (more than one rank), clips with the model's ``scheduler_config.clip_norm`` — the value the trainer
    passes — and updates (optim.CLIP_INSIDE_STEP; SURVEY Q4's double clip of the aliased parameters is kept: same kernel).
    ``deferred_scalars`` (None: leave as is): False makes ``loss.item()`` / ``losses_dict[key]`` plain floats at once — a per-step logger
    that needs the exact type (``json.dumps`` without ``default=``, ``isinstance(x, float)``) pays a device synchronisation per step for it;
    ``vf_nerf_amd.deferred.resolve(payload)`` converts at the logger instead.
    ``patch_evaluator=False`` leaves ``evaluation.methods.render_images`` the reference's own loop (one upload, one ``model.render`` and
    six ``.cpu()`` read-backs per 512-ray chunk): every call of it still lands on the HIP ``render()``; what it gives up is the grouping
    into chip-filling chunks and the single download per image (profiles/r05/bench_view_as_evaluator.json: both loops timed).
    ``patch_mesh`` replaces ``evaluation.utils.marching_cubes_vt.contrastive_marching_cubes`` with ``mesh.contrastive_marching_cubes``
    (the device triangulation, same (vs, fs)); ``patch_mesh=False`` restores the reference's function.
    ``patch_metrics=True`` replaces ``evaluation.methods.metrics`` with ``evaluator.metrics`` (the image scores on the device, a float64
    specification: the PSNR values differ from the reference's float32 ones by its rounding) and keeps the reference's function as
    ``methods._reference_metrics``; the default leaves it alone, and ``False`` after ``True`` puts it back.
    ``patch_tsdf_mesh=True`` replaces ``evaluation.methods.tsdf_mesh`` with ``evaluator.tsdf_mesh`` (RGBD fusion on the device, a dense
    volume: the coloured ``tsdf-mesh/tsdf.ply``) and keeps the reference's function as
    ``methods._reference_tsdf_mesh``; off by default, and ``False`` after ``True`` puts it back.
    ``tsdf_vertex_normals`` (None: leave as is) sets ``evaluator.TSDF_VERTEX_NORMALS``: True makes ``evaluator.tsdf_mesh`` write the vertex
    normals (``meshops.vertex_normals``) into ``tsdf.ply``, as the reference's ``compute_vertex_normals()`` does; off by default.
    ``tsdf_sparse`` (None: leave as is) sets ``evaluator.TSDF_SPARSE``: True makes ``evaluator.tsdf_mesh`` fuse into the block-sparse
    volume (``tsdf.SparseTSDFVolume``), which has no 2^31 voxel limit; off by default.
    ``tsdf_min_component_faces`` (None: leave as is) sets ``evaluator.TSDF_MIN_COMPONENT_FACES``: an integer makes ``evaluator.tsdf_mesh``
    cull the components of the fused mesh with fewer faces (``meshops.filter_components``) before it writes ``tsdf.ply``; the module's
    default is None, the mesh as fused.
    ``tsdf_simplify_voxel`` (None: leave as is) sets ``evaluator.TSDF_SIMPLIFY_VOXEL``: a voxel edge makes ``evaluator.tsdf_mesh`` simplify
    the fused mesh by vertex clustering with quadric placement (``meshops.simplify_vertex_clustering``) after the culling and before
    it writes ``tsdf.ply``, the colours following as cluster means; the module's default is None, the mesh as fused.
    ``dominant_bases_decimation`` (None: leave as is) sets ``meshops.DECIMATION``: "collapse" makes ``meshops.dominant_bases(decimation=)``
    reach its face count by quadric edge collapse (``meshops.simplify_edge_collapse``) instead of the bisection over vertex clusterings;
    the module's default is "clustering".
    ``tsdf_simplify_faces`` (None: leave as is) sets ``evaluator.TSDF_SIMPLIFY_FACES``: an integer makes ``evaluator.tsdf_mesh`` decimate
    the fused mesh to at most about that many faces by edge collapse after the culling, the colours interpolated along the collapsed
    edges; it cannot be combined with ``tsdf_simplify_voxel`` (ValueError); the module's default is None.
    ``patch_dominant_bases=True`` replaces ``utils.utils.get_dominant_bases`` (trimesh's decimation, scikit-learn's KMeans) with
    ``bases.get_dominant_bases`` (same signature and return; vertex clustering, vertex normals and k-means on the device — this
    project's bases, not a recording of the reference's: see ``vf_nerf_amd.bases``) when that module can be imported, and keeps the
    reference's function as ``utils.utils._reference_get_dominant_bases``; off by default, and ``False`` after ``True`` puts it back.
    ``mesh_orient`` (None: leave as is) sets ``mesh.ORIENT``: "first", "majority" or "volume" makes ``mesh.contrastive_marching_cubes``
    rewind its faces consistently (``meshops.orient``) before it lists them; the module's default is None, every bit of (vs, fs) the
    reference's."""
    # every argument is checked before any switch is set: an install() that raises leaves everything as it was
    if mesh_orient is not None and mesh_orient not in mesh.ORIENT_REFERENCES:
        raise ValueError(f"mesh_orient must be None or one of {mesh.ORIENT_REFERENCES}, got {mesh_orient!r}")
    if tsdf_simplify_voxel is not None:
        tsdf_simplify_voxel = voxel.check_voxel_size(tsdf_simplify_voxel, "tsdf_simplify_voxel")
    if dominant_bases_decimation is not None and dominant_bases_decimation not in meshops.DECIMATIONS:
        raise ValueError(f"dominant_bases_decimation must be None or one of {meshops.DECIMATIONS}, got {dominant_bases_decimation!r}")
    if tsdf_simplify_faces is not None:
        if isinstance(tsdf_simplify_faces, bool) or not isinstance(tsdf_simplify_faces, int) or tsdf_simplify_faces < 1:
            raise ValueError(f"tsdf_simplify_faces must be None or an integer >= 1, got {tsdf_simplify_faces!r}")
        if (tsdf_simplify_voxel if tsdf_simplify_voxel is not None else evaluator.TSDF_SIMPLIFY_VOXEL) is not None:
            raise ValueError("tsdf_simplify_faces cannot be combined with tsdf_simplify_voxel")
    elif tsdf_simplify_voxel is not None and evaluator.TSDF_SIMPLIFY_FACES is not None:
        raise ValueError("tsdf_simplify_voxel cannot be combined with tsdf_simplify_faces")
    if tsdf_min_component_faces is not None:
        if isinstance(tsdf_min_component_faces, bool) or not isinstance(tsdf_min_component_faces, int) or tsdf_min_component_faces < 0:
            raise ValueError(f"tsdf_min_component_faces must be None or an integer >= 0, got {tsdf_min_component_faces!r}")
        evaluator.TSDF_MIN_COMPONENT_FACES = tsdf_min_component_faces
    if tsdf_simplify_voxel is not None:
        evaluator.TSDF_SIMPLIFY_VOXEL = tsdf_simplify_voxel
    if tsdf_simplify_faces is not None:
        evaluator.TSDF_SIMPLIFY_FACES = tsdf_simplify_faces
    if dominant_bases_decimation is not None:
        meshops.DECIMATION = dominant_bases_decimation
    if mesh_orient is not None:
        mesh.ORIENT = mesh_orient
    if tsdf_vertex_normals is not None:
        evaluator.TSDF_VERTEX_NORMALS = bool(tsdf_vertex_normals)
    if tsdf_sparse is not None:
        evaluator.TSDF_SPARSE = bool(tsdf_sparse)
    for dotted, module in _ALIASES.items():
        parts = dotted.split(".")
        for i in range(1, len(parts)):
            _ensure_package(".".join(parts[:i]))
        sys.modules[dotted] = module
        parent = sys.modules[".".join(parts[:-1])]
        setattr(parent, parts[-1], module)
    # evaluation/utils/mc_utils.get_set_predictions -> pinned, vector-only, rank-sharded version
    try:
        mc = importlib.import_module("evaluation.utils.mc_utils")
        mc.get_set_predictions = grid.get_set_predictions
        # the conv3d / gather stages after the queries, as device kernels (they expect the grid on the GPU)
        mc.extract_divergence = grid.extract_divergence
        mc.unify_direction = grid.unify_direction
        mc.make_comb_format = grid.make_comb_format
        importlib.import_module("evaluation.utils.guassian_smoothing").smooth_vf = grid.smooth_vf
    except Exception:
        pass
    # the evaluator's image loop (evaluation/methods.py:472-545: one upload, one render() and four .cpu() synchronisations per
    # chunk) -> chunks on alternating streams, one download per image; same dataset, same files
    try:
        methods = importlib.import_module("evaluation.methods")
        if patch_evaluator:
            if not hasattr(methods, "_reference_render_images"):
                methods._reference_render_images = methods.render_images
            methods.render_images = evaluator.render_images
        elif hasattr(methods, "_reference_render_images"):
            methods.render_images = methods._reference_render_images
        if patch_metrics:
            if not hasattr(methods, "_reference_metrics"):
                methods._reference_metrics = methods.metrics
            methods.metrics = evaluator.metrics
        elif hasattr(methods, "_reference_metrics"):
            methods.metrics = methods._reference_metrics
        if patch_tsdf_mesh:
            if not hasattr(methods, "_reference_tsdf_mesh"):
                methods._reference_tsdf_mesh = methods.tsdf_mesh
            methods.tsdf_mesh = evaluator.tsdf_mesh
        elif hasattr(methods, "_reference_tsdf_mesh"):
            methods.tsdf_mesh = methods._reference_tsdf_mesh
    except Exception:
        pass
    # evaluation/utils/marching_cubes_vt.contrastive_marching_cubes (a Python loop over every surface cell) -> the device triangulation;
    # same arguments and (vs, fs).  patch_mesh=False puts the reference's function back.
    try:
        mcv = importlib.import_module("evaluation.utils.marching_cubes_vt")
        if patch_mesh:
            if not hasattr(mcv, "_reference_contrastive_marching_cubes"):
                mcv._reference_contrastive_marching_cubes = mcv.contrastive_marching_cubes
            mcv.contrastive_marching_cubes = mesh.contrastive_marching_cubes
        elif hasattr(mcv, "_reference_contrastive_marching_cubes"):
            mcv.contrastive_marching_cubes = mcv._reference_contrastive_marching_cubes
    except Exception:
        pass
    # utils/utils.py:216-233 get_dominant_bases (trimesh + scikit-learn on the host) -> the device pipeline, only with the switch
    try:
        uu = importlib.import_module("utils.utils")
        if patch_dominant_bases:
            if not hasattr(uu, "_reference_get_dominant_bases"):
                uu._reference_get_dominant_bases = uu.get_dominant_bases
            uu.get_dominant_bases = bases.get_dominant_bases
        elif hasattr(uu, "_reference_get_dominant_bases"):
            uu.get_dominant_bases = uu._reference_get_dominant_bases
    except Exception:
        pass
    # models.helpers.functions stays the reference's module (the trainer uses more of it); only the two host-side numpy
    # samplers the trainer calls every step are replaced by the device-side ones
    try:
        fn = importlib.import_module("models.helpers.functions")
        fn.sample_border_points = supervision.sample_border_points
        fn.sample_center_points = supervision.sample_center_points
        # functions.py:137-157 compacts the centre-ball rows with boolean-mask indexing (a device synchronisation in the middle of every
        # step); inside an open training step the same rows are selected by the fused loss kernels instead (supervision.py)
        fn.get_center_indices_and_gt = supervision.get_center_indices_and_gt
    except Exception:
        pass
    # the datasets' get_centroid(device) uploads the same three floats five times per step (train/vector_field_nerf_train.py:186-214);
    # cached per device, and the cached tensor carries its host values so that the samplers above need no read-back
    for mod, cls in (("datasets.normal_datasets.base_dataset", "BaseDataset"), ("datasets.normal_datasets.replica_dataset", "ReplicaDataset"),
                     ("datasets.normal_datasets.scannet_dataset", "ScanNetDataset")):
        try:
            cache_centroid(getattr(importlib.import_module(mod), cls))
        except Exception:
            pass
    # the loss with one device read-back per step instead of six
    try:
        importlib.import_module("models.losses.vf_loss").VFLoss = loss.VFLoss
    except Exception:
        pass

    from . import optim
    if patch_clip:
        _patch_clip_grad_norm()
        optim.CLIP_INSIDE_STEP = False
    else:
        uninstall_clip_grad_norm()
        optim.CLIP_INSIDE_STEP = True
    if deferred_scalars is not None:
        loss.DEFERRED_SCALARS = bool(deferred_scalars)


def cache_centroid(cls) -> None:
    """Wrap ``cls.get_centroid(self, device)`` (datasets/normal_datasets/*_dataset.py: ``self.gt_mesh_centroid.to(device)``) so that it
    returns ONE tensor per device for as long as the source tensor is unchanged, with the three host values attached as ``_vfn_host``
    (read once, when the cache is filled).  The values are the dataset's; only the repeated uploads go away."""
    orig = cls.__dict__.get("get_centroid")
    if orig is None or getattr(orig, "_vfn_cached", False):
        return

    def get_centroid(self, device):
        cache = self.__dict__.setdefault("_vfn_centroid_cache", {})
        src = getattr(self, "gt_mesh_centroid", None)
        key = (str(device), id(src), getattr(src, "_version", 0))
        hit = cache.get(key)
        if hit is None:
            hit = orig(self, device)
            host = hit.detach().reshape(-1).tolist()
            if len(host) == 3:
                hit._vfn_host = tuple(float(v) for v in host)
            cache.clear()
            cache[key] = hit
        return hit

    get_centroid._vfn_cached = True
    get_centroid.__wrapped__ = orig
    cls.get_centroid = get_centroid


# One process per GPU (vf_nerf_amd.distributed replaces the reference's nn.DataParallel, models/nerf/vector_field_nerf.py:70-75): the
# unchanged trainer has no line for the gradient all-reduce, and the one place every replica passes between backward() and
# optimizer.step() is its clip_grad_norm_ call (train/vector_field_nerf_train.py:254-255).  With a process group of more than one rank
# the wrapped clip_grad_norm_ first averages the gradients of the list it was given over the ranks — ONE all-reduce of the flat gradient
# buffer when the list is the flat optimizer's — so that every replica clips and steps identically.  False: the caller does it.
data_parallel = True


def world_size() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def all_reduce_flat(f) -> bool:
    """Mean over the ranks of a FlatAdam's flat gradient buffer (ONE all-reduce of 805 780 fp32 on the shipped geometry)."""
    import torch.distributed as dist
    world = world_size()
    if world < 2:
        return False
    dist.all_reduce(f["grad"], op=dist.ReduceOp.SUM)
    f["grad"].div_(world)
    return True


def all_reduce_gradients(plist) -> bool:
    """Mean over the ranks of the gradients of ``plist`` (no-op without a process group of > 1 ranks).  -> whether a collective ran."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
        return False
    from . import optim
    world = dist.get_world_size()
    owner = optim.owner_of(plist[0])
    if owner is not None and owner.regions_for(plist):
        f = owner.flat()
        owner._rebind_grads(f)
        dist.all_reduce(f["grad"], op=dist.ReduceOp.SUM)
        f["grad"].div_(world)
        return True
    seen, grads = set(), []
    for p in plist:
        if id(p) not in seen and p.grad is not None:
            seen.add(id(p))
            grads.append(p.grad)
    if not grads:
        return False
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    flat.div_(world)
    off = 0
    for g in grads:
        g.copy_(flat[off:off + g.numel()].view_as(g))
        off += g.numel()
    return True


_torch_clip = None


def _patch_clip_grad_norm() -> None:
    """The trainer calls ``torch.nn.utils.clip_grad_norm_(self.model.parameters(), clip_norm)``
    (train/vector_field_nerf_train.py:254-255) on a list that names every VF parameter twice (Q4).  The sequential loop the
    reference was written against clips such a gradient twice; PyTorch's multi-tensor implementation, which newer versions
    pick on GPUs, scales duplicated tensors concurrently.  So that the trainer stays UNCHANGED, the function is wrapped: a
    list of device parameters with duplicates goes to ``optim.clip_grad_norm_`` (same semantics as the sequential loop,
    multi-tensor kernels over distinct tensors per pass); every other call reaches PyTorch's own function untouched."""
    global _torch_clip
    import torch
    from . import optim
    if _torch_clip is not None:
        return
    _torch_clip = torch.nn.utils.clip_grad_norm_

    def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
        plist = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
        if data_parallel and plist:
            all_reduce_gradients(plist)
        if float(norm_type) == 2.0 and not error_if_nonfinite and plist:
            owner = optim.owner_of(plist[0])
            if owner is not None and owner.regions_for(plist):     # the flat optimizer's own list (duplicates and all): two launches
                return optim.clip_grad_norm_(plist, max_norm, 2.0)
            ids = [id(p) for p in plist]
            if len(set(ids)) != len(ids) and all(p.is_cuda for p in plist if p.grad is not None):
                return optim.clip_grad_norm_(plist, max_norm, 2.0)
        return _torch_clip(plist, max_norm, norm_type, error_if_nonfinite, foreach)

    clip_grad_norm_.__wrapped__ = _torch_clip
    torch.nn.utils.clip_grad_norm_ = clip_grad_norm_


def uninstall_clip_grad_norm() -> None:
    """Put PyTorch's own clip_grad_norm_ back (tests)."""
    global _torch_clip
    import torch
    if _torch_clip is not None:
        torch.nn.utils.clip_grad_norm_ = _torch_clip
        _torch_clip = None


install()
