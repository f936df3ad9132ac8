"""Image scores on the MI355X (csrc/vfn_image.hip through vf_nerf_amd/metrics2d.py) against the NumPy restatement of the contract
(tests/metrics2d_restatement.py): the per-view sums bit for bit — borders, partial tiles, view strides and the order of the partials
included — and against math.fsum within the pairwise bound of the tree the kernel builds."""
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vf_nerf_amd  # noqa: E402
from vf_nerf_amd import evaluator, lib, metrics2d, synthetic  # noqa: E402
import metrics2d_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53          # unit roundoff of float64
T = R.TILE


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def images(shape, seed, pred_dtype=np.uint8, target_dtype=np.float32):
    g = np.random.default_rng(seed)

    def one(dtype):
        return g.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else g.random(shape, dtype=np.float32)
    return one(pred_dtype), one(target_dtype)


def device_sums(pred, target, want_ssim=True):
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    sums = lib.image_scores(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), want_ssim, info)
    assert int(info.cpu()) == 0
    return sums.cpu().numpy()


def assert_same_bits(pred, target, want_ssim=True):
    got, want = device_sums(pred, target, want_ssim), R.scores_sums(pred, target, want_ssim)
    assert got.shape == want.shape and (got[:, 2] == 0).all()
    assert np.array_equal(bits(got), bits(want)), f"device {got.tolist()} != restatement {want.tolist()}"
    return got


SHAPES = [(1, 1, 1, 3), (1, 7, 5, 3), (1, 5, 40, 3), (1, 40, 5, 3), (1, 11, 11, 3),
          (1, T - 1, 35, 3), (1, T, 35, 3), (1, T + 1, 35, 3), (1, 35, T - 1, 3), (1, 35, T, 3), (1, 35, T + 1, 3), (1, T, T, 3),
          (1, 70, 41, 1), (2, 19, 23, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_equal_the_restatement_bit_for_bit(shape):
    pred, target = images(shape, seed=sum(shape))
    assert_same_bits(pred, target)
    assert_same_bits(pred, target, want_ssim=False)


def test_three_views_with_distinct_content():
    """View 1 equals its target: its sums are exactly 0 and H W C.  A wrong view stride or partial order moves them."""
    pred, target = images((3, 37, 53, 3), seed=77, pred_dtype=np.float32)
    target[1] = pred[1]
    got = assert_same_bits(pred, target)
    assert got[1, 0] == 0.0 and got[1, 1] == 37 * 53 * 3
    assert got[0, 0] > 0 and got[2, 0] > 0 and got[0, 0] != got[2, 0] and got[0, 1] != got[2, 1]
    scores = metrics2d.image_scores(pred, target, quantize=False)
    assert scores[1] == {"psnr": math.inf, "ssim": 1.0}
    assert scores[0] == R.image_scores(pred[0], target[0]) and scores[2] == R.image_scores(pred[2], target[2])


def test_one_full_size_view():
    """680 x 1200 x 3 (the Replica views the evaluator scores): 43 x 75 tiles, so the second level takes four partials per lane."""
    pred, target = images((1, 680, 1200, 3), seed=5)
    assert_same_bits(pred, target)


@pytest.mark.parametrize("pred_dtype, target_dtype", [(np.uint8, np.float32), (np.float32, np.float32), (np.uint8, np.uint8), (np.float32, np.uint8)])
def test_byte_and_float_operands(pred_dtype, target_dtype):
    pred, target = images((2, 33, 47, 3), seed=12, pred_dtype=pred_dtype, target_dtype=target_dtype)
    assert_same_bits(pred, target)
    if pred_dtype == target_dtype:
        got = device_sums(pred, pred.copy())
        assert (got[:, 0] == 0).all() and (got[:, 1] == 33 * 47 * 3).all()          # p == t: every element exactly 1.0


def test_sums_are_within_the_pairwise_bound_of_fsum():
    shape = (1, 150, 210, 3)
    pred, target = images(shape, seed=21)
    got = device_sums(pred, target)[0]
    sq, ss = R.elements(pred[0], target[0])
    levels = lib.image_sum_levels(150, 210, 3)
    assert levels == 2 + 8 + 0 + 10
    for value, e in ((got[0], sq), (got[1], ss)):
        exact, scale = math.fsum(e.reshape(-1)), math.fsum(np.abs(e).reshape(-1))
        print(f"sum {value!r} fsum {exact!r} |difference| {abs(value - exact):.3e} bound {levels * U * scale:.3e}")
        assert abs(value - exact) <= levels * U * scale * 1.01
    got = device_sums(*images((1, 680, 300, 3), seed=22))[0]              # 43 x 19 = 817 tiles: one partial per lane
    assert np.isfinite(got).all()


def test_a_non_finite_element_is_reported():
    pred, target = images((2, 20, 20, 3), seed=3, pred_dtype=np.float32)
    for arr in (pred, target):
        bad = arr.copy()
        bad[-1, -1, -1, -1] = np.nan
        a, b = (bad, target) if arr is pred else (pred, bad)
        for want_ssim in (True, False):
            info = torch.zeros(1, dtype=torch.int64, device=DEV)
            lib.image_scores(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), want_ssim, info)
            assert int(info.cpu()) == 1
        with pytest.raises(lib.VfnError, match="non-finite"):
            metrics2d.image_scores(a, b, quantize=False)


def numpy_bytes(x):
    return (x.astype(np.float64) * 255).astype(np.uint8)


def test_quantize_rgb8_equals_numpy_and_refuses():
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    x = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), np.random.default_rng(11).random(100000, dtype=np.float32)])
    x = x[(x >= 0) & (x.astype(np.float64) * 255.0 < 256.0)]
    u = metrics2d.quantize_rgb8(x, device=DEV)
    assert u.is_cuda and u.dtype == torch.uint8 and np.array_equal(u.cpu().numpy(), numpy_bytes(x))
    image = np.random.default_rng(12).random((9, 13, 3), dtype=np.float32)
    assert tuple(metrics2d.quantize_rgb8(torch.from_numpy(image).to(DEV)).shape) == (9, 13, 3)
    for bad, word in ((256 / 255, "256/255"), (-1e-3, "256/255"), (np.nan, "non-finite")):
        y = np.full(1000, 0.25, dtype=np.float32)
        y[-1] = bad
        with pytest.raises(lib.VfnError, match=word):
            metrics2d.quantize_rgb8(y)
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        got = lib.image_quantize8(torch.from_numpy(y).to(DEV), info).cpu().numpy()
        assert int(info.cpu()) == R.quantize8(y)[1] and np.array_equal(got, R.quantize8(y)[0])


def test_abs_err_is_bit_equal():
    g = np.random.default_rng(31)
    a = (1.0 + 3.0 * g.random((3, 37, 53))).astype(np.float32)
    b = (a + 0.05 * g.standard_normal(a.shape)).astype(np.float32)
    for s in (100.0, 1.0, 0.3):
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        got = lib.image_abs_err(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), s, info).cpu().numpy()
        assert int(info.cpu()) == 0 and np.array_equal(bits(got), bits(R.abs_err_sums(a, b, s)))
    pred, target = images((37, 53, 3), seed=32)
    got = metrics2d.image_scores(pred, target, pred_depth=a[0], target_depth=b[0][:, :, None])
    assert got == R.image_scores(pred, target, True, a[0], b[0]) and list(got) == ["psnr", "ssim", "depth_l1_cm"]
    both = metrics2d.score_views([pred, pred], [target, pred], ssim=True, pred_depths=[a[0], a[1]], target_depths=[b[0], b[1]])
    assert both["image-0"] == got and both["image-1"]["psnr"] == math.inf and both["image-1"]["ssim"] == 1.0
    assert both["image-1"]["depth_l1_cm"] == R.abs_err_sums(a[1:2], b[1:2])[0] / (37 * 53)


def test_score_view_equals_render_view_then_image_scores():
    """The 64 x 64 synthetic pinhole view of smoke()'s model: score_view (render, scatter and score on the device) against
    metrics2d.image_scores applied to what render_view downloads for the same call, scattered on the host."""
    torch.manual_seed(0)
    cfg = vf_nerf_amd.shipped_config(DEV, n_samples=32, n_importance=32, perturb=True, dir_to_normal_th=-0.2)
    model = vf_nerf_amd.VectorFieldNerf(cfg)
    model.eval()
    synthetic.scale_hidden_weights(model.vector_field_network, model.rendering_network, 2.0)
    with torch.no_grad():
        pts = synthetic.frustum_points(20000, seed=1234).to(DEV)
        mean, std = synthetic.vector_head_stats_from_tanh(model.vector_field_network(pts, vector_only=True))
        synthetic.recentre_vector_head(model.vector_field_network, mean, std)
    w = h = 64
    uv, pose, K = synthetic.pinhole_image(w, h, 60.0)
    model.rng_seed, model._rng_offset = 5, 0
    rgb_values, depth_values = evaluator.render_view(model, pose, uv, K, 0)
    rows, cols = uv[:, 1].long().numpy(), uv[:, 0].long().numpy()
    rgb, depth = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.float32)
    rgb[rows, cols] = rgb_values
    depth[rows, cols] = depth_values[:, 0]
    g = np.random.default_rng(8)
    target = np.clip(rgb + 0.05 * g.standard_normal(rgb.shape), 0.0, 1.0).astype(np.float32)
    target_depth = (depth + 0.01 * g.standard_normal(depth.shape)).astype(np.float32)
    want = metrics2d.image_scores(rgb, target, pred_depth=depth, target_depth=target_depth)
    model.rng_seed, model._rng_offset = 5, 0
    got = evaluator.score_view(model, pose, uv, K, 0, target, target_depth)
    assert got == want and list(got) == ["psnr", "ssim", "depth_l1_cm"], (got, want)
    assert 15.0 < got["psnr"] < 40.0 and -1.0 < got["ssim"] < 1.0 and 0.0 < got["depth_l1_cm"] < 5.0
    # the flattened target the dataset hands over, with the image size beside it; PSNR only
    model.rng_seed, model._rng_offset = 5, 0
    flat = evaluator.score_view(model, pose, uv, K, 0, torch.from_numpy(target).reshape(-1, 3), ssim=False, image_size=(h, w))
    assert flat == {"psnr": want["psnr"]}
    assert want == R.image_scores(R.quantize8(rgb)[0], target, True, depth, target_depth)
