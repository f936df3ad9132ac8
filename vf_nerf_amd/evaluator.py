"""The evaluator's image loop on the HIP path (reference: ``evaluation/methods.py:472-545``, ``render_images``).

The reference renders a view ``split_size`` rays at a time and, per chunk, uploads three tensors, calls ``model.render`` and
pulls rgb and depth (and the pixel indices, four times) back with ``.cpu()`` — four device synchronisations per 512..1024-ray
chunk, with the device idle in between.  ``render_view`` does the same work with consecutive chunks on alternating HIP streams
(``VectorFieldNerf.render_chunked``: same per-chunk arithmetic, so the same values) and ONE download per image;
``render_images`` is the reference function's loop around it — same dataset, same files written — and is what
``vf_nerf_amd.dropin.install()`` puts in place of ``evaluation.methods.render_images``, so that ``evaluation/evaluate.py`` runs
unchanged.

``score_view`` renders a view the same way and scores it against its target on the device (``vf_nerf_amd.metrics2d``) without
downloading the image; ``metrics`` is the drop-in for ``evaluation.methods.metrics`` (methods.py:549-610: the PNGs written by
``render_images`` scored against the dataset's images, ``metrics.json``), installed by ``dropin.install(patch_metrics=True)``.

``tsdf_mesh`` is the drop-in for ``evaluation.methods.tsdf_mesh`` (methods.py:613-665: the rendered depth maps and PNGs fused into the
coloured ``tsdf-mesh/tsdf.ply``), installed by ``dropin.install(patch_tsdf_mesh=True)``; with ``TSDF_VERTEX_NORMALS`` set it writes the
vertex normals too, as the reference does (``compute_vertex_normals()``; ours are ``meshops.vertex_normals``)."""
from __future__ import annotations

import importlib
import json
import os
from typing import Optional, Tuple

import numpy as np
import torch


MIN_CHUNK = 8192        # rays per launch group of a whole view (see render_view)
# render_view keeps rgb and depth only (as the reference's loop does, evaluation/methods.py:528-540), so it asks render() for SPARSE
# colours: the rendering net is evaluated only for the samples whose weight is non-zero — a few percent — which leaves rgb and depth
# bit-identical (model.sparse_colours, include/vfn.h vfn_render_params.sparse_colours).  False: the dense plan.
SPARSE_COLOURS = True
# tsdf_mesh writes nx ny nz (meshops.vertex_normals of the fused mesh) into tsdf.ply; False: the file without normals.
# dropin.install(tsdf_vertex_normals=...) sets it.
TSDF_VERTEX_NORMALS = False
# tsdf_mesh fuses into the block-sparse volume (tsdf.SparseTSDFVolume: no 2^31 voxel limit on the box of the depths); False: the dense
# volume.  dropin.install(tsdf_sparse=...) sets it.
TSDF_SPARSE = False
# tsdf_mesh culls the components of the fused mesh with fewer faces (meshops.filter_components, edge connectivity) before it writes
# tsdf.ply; None: the mesh as fused.  dropin.install(tsdf_min_component_faces=...) sets it.
TSDF_MIN_COMPONENT_FACES = None
# tsdf_mesh simplifies the fused mesh by vertex clustering at this voxel edge (meshops.simplify_vertex_clustering, "quadric") after the
# component culling and before it writes tsdf.ply; None: the mesh as fused.  dropin.install(tsdf_simplify_voxel=...) sets it.
TSDF_SIMPLIFY_VOXEL = None
# tsdf_mesh decimates the fused mesh to at most this many faces by quadric edge collapse (meshops.simplify_edge_collapse) after the
# component culling; None: the mesh as fused.  Not together with TSDF_SIMPLIFY_VOXEL.  dropin.install(tsdf_simplify_faces=...) sets it.
TSDF_SIMPLIFY_FACES = None


@torch.no_grad()
def render_view(model, all_pose: torch.Tensor, all_pixels: torch.Tensor, all_intrinsics: torch.Tensor, epoch: int,
                split_size: int = 512, white: bool = False, n_streams: int = 2, min_chunk: int = MIN_CHUNK) -> Tuple[np.ndarray, np.ndarray]:
    """One view, as the dataset hands it over (host or device tensors, pose / intrinsics replicated per ray or shared) ->
    (rgb[N,3], depth[N,1]) numpy arrays.

    ``split_size`` is the reference loop's chunk (methods.py:513-545), there to bound ITS activation memory: its un-fused
    forward materialises [rays x samples, 256] per layer.  Here nothing of the kind exists (the fused kernels keep activations on
    chip; a chunk's outputs are 52 B per sample), and rays are independent end to end, so the view is rendered in chunks of
    max(split_size, ``min_chunk``) rays: at the shipped sampler sizes (100 + 35 samples) a 512-ray chunk is 1.6 + 0.5 rounds of
    workgroups per fused launch — 1.32 M rays/s against 2.06 M in 8 192-ray chunks on one MI355X.  Every ray's value is the one
    the 512-ray loop computes for the same random draws; which draws a ray gets (stratified jitter, the uniform fine samples of
    rays without a surface, Q9) depends on its position in the stream as it does in the reference.  ``min_chunk = 0``: exactly the
    reference's chunking."""
    chunk = max(int(split_size), int(min_chunk))
    keep = getattr(model, "sparse_colours", False)
    model.sparse_colours = bool(SPARSE_COLOURS) or keep
    try:
        rgb, depth = model.render_chunked(all_pose, all_pixels, all_intrinsics, epoch, chunk=chunk, n_streams=n_streams, white=white)
    finally:
        model.sparse_colours = keep
    host = torch.empty(rgb.shape[0], 4, pin_memory=True)
    host[:, :3].copy_(rgb, non_blocking=True)
    host[:, 3:].copy_(depth, non_blocking=True)
    torch.cuda.current_stream(rgb.device).synchronize()
    out = host.numpy()
    return out[:, :3].copy(), out[:, 3:].copy()


@torch.no_grad()
def render_images(model, eval_path: str, dataset_config, epoch: int, split_size: int = 512, device: torch.device = torch.device("cuda")) -> None:
    """Drop-in for ``evaluation.methods.render_images`` (methods.py:472-545): every image of the dataset rendered with all of its
    pixels and written as ``rendered_images/image-{i}.png`` / ``depth-{i}`` through the reference's own dataset and ``utils``
    helpers (they stay the reference's: datasets and image I/O are outside the hot path)."""
    dataset_dict = importlib.import_module("datasets.normal_datasets").dataset_dict
    utils = importlib.import_module("utils.utils")
    dataset = dataset_dict[dataset_config.dataset_name](dataset_config)
    dataset.all_pixels = True
    model.ray_sampler.near, model.ray_sampler.far = dataset.get_bounds()
    if model.config.ray_sampler_config.fine_sampling():
        model.fine_sampler.near, model.fine_sampler.far = dataset.get_bounds()
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False)
    path = os.path.join(eval_path, "rendered_images")
    utils.mkdir_ifnotexists(path)
    for i, batch in enumerate(dataloader):
        pixels = batch["uv"].squeeze(0)
        rgb_values, depth_values = render_view(model, batch["pose"].squeeze(0), pixels, batch["intrinsics"].squeeze(0), epoch, split_size,
                                               dataset.white_bkgd)
        rows, cols = pixels[:, 1].long().cpu().numpy(), pixels[:, 0].long().cpu().numpy()
        rgb = np.zeros((dataset.image_size[0], dataset.image_size[1], 3))
        depth_map = np.zeros((dataset.image_size[0], dataset.image_size[1], 1))
        rgb[rows, cols, :] = rgb_values
        depth_map[rows, cols, :] = depth_values
        utils.save_rgb(os.path.join(path, f"image-{i}.png"), rgb)
        utils.save_depth(os.path.join(path, f"depth-{i}"), depth_map)


METRICS_CHUNK = 8       # views scored per launch by metrics(): bounds the images held at once (a 680 x 1200 target is 9.8 MB)


@torch.no_grad()
def score_view(model, all_pose: torch.Tensor, all_pixels: torch.Tensor, all_intrinsics: torch.Tensor, epoch: int, target_rgb,
               target_depth=None, *, split_size: int = 512, white: bool = False, ssim: bool = True,
               image_size: Optional[Tuple[int, int]] = None) -> dict:
    """One view rendered as ``render_view`` renders it (same chunks, same streams, same sparse colours: the same values for the same
    random stream position) and scored against ``target_rgb`` ([H,W,3], or [H W,3] with ``image_size`` = (H, W)) on the device:
    rgb and depth are scattered into [H,W,3] / [H,W] images by ``all_pixels`` (a pixel no ray names stays 0, as in the reference's
    loop, methods.py:517-540), the rgb image goes through the byte quantisation of the PNG round trip, and
    ``metrics2d.image_scores`` returns {"psnr", "ssim" (``ssim=True``), "depth_l1_cm" (with ``target_depth``, H W values in metres)}.
    Nothing but the scores is downloaded."""
    from . import geomargs, metrics2d
    target = geomargs.as_tensor(target_rgb, "target_rgb")
    if image_size is None:
        if target.dim() != 3:
            raise ValueError(f"target_rgb must be [H,W,3] when image_size is not given, got {tuple(target.shape)}")
        image_size = (int(target.shape[0]), int(target.shape[1]))
    h, w = int(image_size[0]), int(image_size[1])
    if h < 1 or w < 1 or target.numel() != h * w * 3:
        raise ValueError(f"target_rgb {tuple(target.shape)} does not hold {h} x {w} x 3 values")
    target = target.reshape(h, w, 3)
    depth_target = None
    if target_depth is not None:
        depth_target = geomargs.as_tensor(target_depth, "target_depth")
        if depth_target.numel() != h * w:
            raise ValueError(f"target_depth {tuple(depth_target.shape)} does not hold {h} x {w} values")
        depth_target = depth_target.reshape(h, w)
    chunk = max(int(split_size), MIN_CHUNK)
    keep = getattr(model, "sparse_colours", False)
    model.sparse_colours = bool(SPARSE_COLOURS) or keep
    try:
        rgb, depth = model.render_chunked(all_pose, all_pixels, all_intrinsics, epoch, chunk=chunk, n_streams=2, white=white)
    finally:
        model.sparse_colours = keep
    dev = rgb.device
    uv = all_pixels.to(dev)
    rows, cols = uv[:, 1].long(), uv[:, 0].long()
    image = torch.zeros(h, w, 3, device=dev)
    image[rows, cols] = rgb
    pred_depth = None
    if depth_target is not None:
        pred_depth = torch.zeros(h, w, device=dev)
        pred_depth[rows, cols] = depth[:, 0]
    return metrics2d.image_scores(image, target, quantize=True, ssim=ssim, pred_depth=pred_depth, target_depth=depth_target, device=dev)


@torch.no_grad()
def metrics(model, eval_path: str, dataset_config, epoch: int, split_size: int = 200, device: torch.device = torch.device("cuda")) -> None:
    """Drop-in for ``evaluation.methods.metrics`` (methods.py:549-610): the same file checks, the same ``render_images`` call when an
    image or a depth map is missing, the same loop over the dataset and the same ``metrics.json`` ({"image-{i}": {"psnr"}, "mean_psnr"}),
    with the PSNR of every view computed on the device (``metrics2d.score_views``).  The PNGs are read through the reference's own
    ``utils.load_rgb`` (image I/O stays the reference's); it returns byte / 255 as float32, from which ``rint(p * 255)`` recovers the byte
    exactly whether skimage divides by 255 or multiplies by its reciprocal.  The values are the float64 specification's: they differ
    from the reference's float32 ``get_psnr`` by its rounding, and the mean is taken in float64."""
    from . import metrics2d
    dataset_dict = importlib.import_module("datasets.normal_datasets").dataset_dict
    utils = importlib.import_module("utils.utils")
    dataset = dataset_dict[dataset_config.dataset_name](dataset_config)
    dataset.all_pixels = True
    images_path = os.path.join(eval_path, "rendered_images")
    num_images = len(dataset)
    image_paths = [os.path.join(images_path, f"image-{i}.png") for i in range(num_images)]
    depth_paths = [os.path.join(images_path, f"depth-{i}.npy") for i in range(num_images)]
    if not all(os.path.exists(path) for path in image_paths) or not all(os.path.exists(path) for path in depth_paths):
        print("Not all images and depth maps exist. Rendering images and depth maps.")
        try:                                       # the function evaluate.py would reach: the reference's, or the one install() put there
            render = importlib.import_module("evaluation.methods").render_images
        except ImportError:
            render = render_images
        render(model, eval_path, dataset_config, epoch, split_size, device)
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False)
    rows, preds, targets = [], [], []

    def flush():
        if preds:
            scored = metrics2d.score_views(preds, targets, device=device)
            rows.extend(scored[f"image-{k}"] for k in range(len(preds)))
            preds.clear()
            targets.clear()

    for i, batch in enumerate(dataloader):
        if i >= num_images:
            break
        targets.append(batch["rgb"].squeeze(0).reshape(dataset.image_size[0], dataset.image_size[1], 3).float())
        loaded = utils.load_rgb(image_paths[i])                                    # [3,H,W] float32 = byte / 255
        preds.append(torch.from_numpy(np.rint(loaded.transpose(1, 2, 0).astype(np.float64) * 255.0).astype(np.uint8)))
        if len(preds) == METRICS_CHUNK:
            flush()
    flush()
    metrics_dict = metrics2d.views_dictionary(rows)
    with open(os.path.join(eval_path, "metrics.json"), "w") as f:
        json.dump(metrics_dict, f, indent=4)


@torch.no_grad()
def tsdf_mesh(eval_path: str, dataset_config) -> None:
    """Drop-in for ``evaluation.methods.tsdf_mesh`` (methods.py:613-665): every ``rendered_images/depth-{i}.npy`` with its
    ``image-{i}.png`` (read with PIL: the PNG's bytes) and the dataset's intrinsics / poses — per view for ``dtu`` / ``deepfashion``,
    shared otherwise — fused WITH colour on the device (``tsdf.fuse_rgbd_maps``: voxel length 4/512, ``sdf_trunc`` 0.04, the depth as
    ``tsdf.reference_depth`` states the reference's millimetre round trip, the box of the back-projected depths) and written to
    ``tsdf-mesh/tsdf.ply`` (``ply.write_ply``: binary, float vertices, uchar colours).  The reference calls ``compute_vertex_normals()``
    first: with the module switch ``TSDF_VERTEX_NORMALS`` set the file also holds ``meshops.vertex_normals`` of the fused mesh (the
    extraction already merges its vertices: no weld); by default it does not.  With ``TSDF_SPARSE`` set the fusion runs in the
    block-sparse volume, which a scene spanning more than 2^31 voxels does not stop.  With ``TSDF_MIN_COMPONENT_FACES`` set the components
    of the fused mesh with fewer faces are culled (``meshops.filter_components``) before the file is written; colours, and the normals
    of the fused mesh if asked for, follow the vertices that stay.  With ``TSDF_SIMPLIFY_VOXEL`` set the mesh — after that culling — is
    simplified by vertex clustering at that voxel edge (``meshops.simplify_vertex_clustering``, ``"quadric"``); the colours follow as
    cluster means and the normals, if asked for, are those of the simplified mesh.  With ``TSDF_SIMPLIFY_FACES`` set it is instead decimated
    to that face count by edge collapse (``meshops.simplify_edge_collapse``), the colours interpolated along the collapsed edges and the
    normals taken afterwards; both switches set raises ValueError.  Installed by ``dropin.install(patch_tsdf_mesh=True)``."""
    from PIL import Image
    from . import meshops, ply, tsdf
    if TSDF_SIMPLIFY_VOXEL is not None and TSDF_SIMPLIFY_FACES is not None:
        raise ValueError("evaluator.TSDF_SIMPLIFY_VOXEL and evaluator.TSDF_SIMPLIFY_FACES cannot both be set")
    dataset_dict = importlib.import_module("datasets.normal_datasets").dataset_dict
    dataset = dataset_dict[dataset_config.dataset_name](dataset_config)
    images_path = os.path.join(eval_path, "rendered_images")
    n = len([name for name in os.listdir(images_path) if name.endswith(".npy") and name.startswith("depth")])
    if n < 1:
        raise FileNotFoundError(f"no depth-*.npy under {images_path}")
    depths, images, intrinsics, poses = [], [], [], []
    for i in range(n):
        depth = np.load(os.path.join(images_path, f"depth-{i}.npy"))
        depth = depth[..., 0] if depth.ndim == 3 else depth
        with Image.open(os.path.join(images_path, f"image-{i}.png")) as png:
            images.append(np.asarray(png.convert("RGB"), dtype=np.uint8))
        depths.append(tsdf.reference_depth(np.ascontiguousarray(depth)))
        k = dataset.intrinsics[i] if dataset_config.dataset_name in ["dtu", "deepfashion"] else dataset.intrinsics
        intrinsics.append(torch.as_tensor(k).detach().cpu().to(torch.float64)[:3, :3])
        poses.append(torch.as_tensor(dataset.poses[i]).detach().cpu().to(torch.float64))
    vertices, faces, colours = tsdf.fuse_rgbd_maps(torch.stack(depths), np.stack(images), torch.stack(intrinsics), torch.stack(poses),
                                                   **({"sparse": True} if TSDF_SPARSE else {}))
    mesh_path = os.path.join(eval_path, "tsdf-mesh")
    os.makedirs(mesh_path, exist_ok=True)
    if TSDF_SIMPLIFY_VOXEL is not None or TSDF_SIMPLIFY_FACES is not None:
        if TSDF_MIN_COMPONENT_FACES is not None:
            vertices, faces, _, inverse = meshops.filter_components((vertices, faces), min_faces=TSDF_MIN_COMPONENT_FACES)
            colours = colours[(inverse >= 0).to(colours.device)]
        if TSDF_SIMPLIFY_FACES is not None:
            simple = meshops.simplify_edge_collapse((vertices, faces), target_faces=TSDF_SIMPLIFY_FACES, colours=colours)
        else:
            simple = meshops.simplify_vertex_clustering((vertices, faces), TSDF_SIMPLIFY_VOXEL, contraction="quadric", colours=colours)
        ply.write_ply(os.path.join(mesh_path, "tsdf.ply"), simple.vertices, simple.faces, simple.colours,
                      **({"normals": meshops.vertex_normals((simple.vertices, simple.faces))} if TSDF_VERTEX_NORMALS else {}))
    elif TSDF_MIN_COMPONENT_FACES is not None:
        normals = meshops.vertex_normals((vertices, faces)) if TSDF_VERTEX_NORMALS else None
        vertices, faces, _, inverse = meshops.filter_components((vertices, faces), min_faces=TSDF_MIN_COMPONENT_FACES)
        stays = (inverse >= 0).to(colours.device)
        colours = colours[stays]
        ply.write_ply(os.path.join(mesh_path, "tsdf.ply"), vertices, faces, colours,
                      **({} if normals is None else {"normals": normals[stays.to(normals.device)]}))
    elif TSDF_VERTEX_NORMALS:
        ply.write_ply(os.path.join(mesh_path, "tsdf.ply"), vertices, faces, colours, normals=meshops.vertex_normals((vertices, faces)))
    else:
        ply.write_ply(os.path.join(mesh_path, "tsdf.ply"), vertices, faces, colours)
