"""Image scores, host side: the NumPy restatement of the contract (tests/metrics2d_restatement.py) against recordings of the reference's
own get_psnr / get_ssim / get_l1_cm (tests/golden/image_metrics.npz, written by tests/golden/make_image_metrics_golden.py), the byte
quantisation against numpy's expression, the C-ABI surface, and the argument checks that run before any device call."""
import importlib
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, metrics2d  # noqa: E402
import metrics2d_restatement as R  # noqa: E402

NEW_EXPORTS = ("vfn_image_quantize8", "vfn_image_scores_workspace_bytes", "vfn_image_scores", "vfn_image_abs_err")
GOLDEN = os.path.join(REPO, "tests", "golden", "image_metrics.npz")
# Derived, not measured: a window sum carries at most ~150 roundings of 1.1e-16 on values <= 1 (2e-14 on the s terms, against C2 = 9e-4),
# the reference's window weights 1/121 differ from our division by one more rounding per term, and the mean is a pairwise tree.
BOUND = 1e-9


@pytest.fixture(scope="module")
def golden():
    """{case: dict(pred_u8, target, pred_depth, target_depth, ref32[3], ref64[3], ours[3])}: the restatement is evaluated once."""
    z = np.load(GOLDEN)
    out = {}
    for name in [str(n) for n in z["names"]]:
        pred = z[f"{name}/pred_u8"]
        target = z[f"{name}/target"] if f"{name}/target" in z.files else pred          # the 'equal' case: the target is the prediction
        case = dict(pred_u8=pred, target=target, pred_depth=z[f"{name}/pred_depth"], target_depth=z[f"{name}/target_depth"],
                    ref32=z[f"{name}/ref32"], ref64=z[f"{name}/ref64"])
        got = R.image_scores(pred, target, True, case["pred_depth"], case["target_depth"])
        case["ours"] = np.array([got["psnr"], got["ssim"], got["depth_l1_cm"]])
        out[name] = case
    return out


def test_fixture_has_the_cases_the_contract_names(golden):
    shapes = {name: c["pred_u8"].shape for name, c in golden.items()}
    for want in ((1, 1, 3), (7, 5, 3), (5, 40, 3), (11, 11, 3), (33, 47, 3), (120, 160, 3)):
        assert want in shapes.values(), want
    const = golden["const_target_120x160"]["target"]
    assert const.dtype == np.float32 and (const == 0.5).all()
    assert golden["equal_40x56"]["target"] is golden["equal_40x56"]["pred_u8"]
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_restatement_equals_the_reference_in_float64(golden):
    for name, c in golden.items():
        ours, ref = c["ours"], c["ref64"]
        print(f"{name:24s} psnr {ours[0]!r} vs {ref[0]!r}   ssim {ours[1]!r} vs {ref[1]!r}   l1_cm {ours[2]!r} vs {ref[2]!r}")
        if math.isinf(ref[0]):
            assert ours[0] == ref[0], name
        else:
            assert abs(ours[0] - ref[0]) <= BOUND, (name, ours[0], ref[0])
        assert abs(ours[1] - ref[1]) <= BOUND, (name, ours[1], ref[1])
        assert abs(ours[2] - ref[2]) <= BOUND, (name, ours[2], ref[2])


def test_restatement_is_within_the_references_own_float32_error(golden):
    """|ours - ref32| <= |ref32 - ref64| + 1e-9 case by case: the right-hand side is the reference's own float32 error, read from the
    fixture.  The per-case values are printed; DESIGN 6m quotes the largest per metric."""
    worst = np.zeros(3)
    for name, c in golden.items():
        ours, r32, r64 = c["ours"], c["ref32"], c["ref64"]
        for k, metric in enumerate(("psnr", "ssim", "l1_cm")):
            if math.isinf(r32[k]) or math.isinf(r64[k]):
                assert ours[k] == r32[k] == r64[k], (name, metric)
                continue
            own, dev = abs(r32[k] - r64[k]), abs(ours[k] - r32[k])
            worst[k] = max(worst[k], dev)
            print(f"{name:24s} {metric:6s} |ours - ref32| = {dev:.3e}   |ref32 - ref64| = {own:.3e}")
            assert dev <= own + BOUND, (name, metric, dev, own)
    print("largest |ours - ref32|: psnr %.3e dB, ssim %.3e, l1_cm %.3e" % tuple(worst))


def numpy_bytes(x):
    return (x.astype(np.float64) * 255).astype(np.uint8)


def test_quantisation_equals_numpys_expression():
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    x = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))])
    x = x[(x >= 0) & (x.astype(np.float64) * 255.0 < 256.0)]
    assert x.size >= 3 * 256 - 1                                  # only the lower neighbour of 0 is out of range
    u, info = R.quantize8(x)
    assert info == 0 and np.array_equal(u, numpy_bytes(x))
    assert np.array_equal(R.quantize8(k)[0], np.arange(256))      # float32(k / 255) 255 truncates back to k ...
    seeded = np.random.default_rng(11).random(100000, dtype=np.float32)
    u, info = R.quantize8(seeded)
    assert info == 0 and np.array_equal(u, numpy_bytes(seeded))
    # refusals: a non-finite value, a negative value, a product of 256 or more; -0.0 is 0
    assert R.quantize8(np.float32([0.5, np.nan]))[1] == 1 and R.quantize8(np.float32([np.inf]))[1] == 1
    assert R.quantize8(np.float32([-1e-3]))[1] == 4 and R.quantize8(np.float32([256 / 255]))[1] == 4
    assert R.quantize8(np.float32([-0.0, np.nextafter(np.float32(256 / 255), np.float32(0))]))[0].tolist() == [0, 255]


def test_identical_images_and_black_against_white():
    g = np.random.default_rng(5)
    for img in (g.integers(0, 256, (23, 37, 3), dtype=np.uint8), g.random((19, 18, 3), dtype=np.float32), np.zeros((12, 12, 1), dtype=np.float32)):
        sq, ss = R.elements(img, img)
        assert (ss == 1.0).all() and (sq == 0.0).all()
        got = R.image_scores(img, img)
        assert got["ssim"] == 1.0 and got["psnr"] == math.inf
    zeros, ones = np.zeros((9, 14, 3), dtype=np.float32), np.ones((9, 14, 3), dtype=np.float32)
    assert R.image_scores(zeros, ones)["psnr"] == 0.0 and R.image_scores(np.zeros((9, 14, 3), dtype=np.uint8), ones)["psnr"] == 0.0


def test_tree_sum_is_within_the_pairwise_bound_of_fsum():
    g = np.random.default_rng(9)
    e = g.random((70, 41, 3))
    s = R.view_sum(e)
    levels = (3 - 1) + 8 + 0 + 10
    assert abs(s - math.fsum(e.reshape(-1))) <= levels * 2.0 ** -53 * math.fsum(e.reshape(-1)) * 1.01
    assert lib.image_sum_levels(70, 41, 3) == levels and lib.image_sum_levels(680, 1200, 3) == 2 + 8 + 3 + 10
    assert R.view_sum(np.full((1, 1, 1), 0.25)) == 0.25


def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_image_quantize8"] == ("int", ["const float*", "int64_t", "uint8_t*", "int64_t*", "void*"])
    assert protos["vfn_image_scores_workspace_bytes"] == ("int64_t", ["int64_t"] * 4)
    assert lib.header_abi_version() == 5
    assert lib.image_tile() == R.TILE and lib.IMAGE_TOP == R.TOP and (lib.SSIM_C1, lib.SSIM_C2) == (R.C1, R.C2)
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None


def test_workspace_bytes_and_refusals_answer_on_the_host():
    handle = lib.load()
    ws = handle.vfn_image_scores_workspace_bytes
    assert ws(1, 1, 1, 3) == 16 and ws(1, 16, 16, 1) == 16 and ws(1, 17, 16, 3) == 32 and ws(3, 37, 53, 3) == 3 * 3 * 4 * 16
    assert ws(100, 680, 1200, 3) == 100 * 43 * 75 * 16
    for bad in ((0, 8, 8, 3), (-1, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 1 << 15, 8, 3), (1, 8, 1 << 15, 3), (1, 8, 8, 2), (1, 8, 8, 0),
                (1, 8, 8, 4), (1 << 31, 1, 1, 1), (1 << 29, 2, 2, 1), (3, 32767, 32767, 1), (1, 32767, 32767, 3), (1 << 62, 3, 3, 3)):
        assert ws(*bad) == -1, bad
        assert b"vfn_image_scores_workspace_bytes" in handle.vfn_last_error()
    assert ws(1, 32767, 32767, 1) == 2048 * 2048 * 16 and ws((1 << 31) - 1, 1, 1, 1) == ((1 << 31) - 1) * 16
    # refused before any launch (and before any pointer is read): the limits, then the NULL arguments
    assert handle.vfn_image_scores(None, 0, None, 0, 1, 8, 8, 2, 1, 1e-4, 9e-4, None, None, None, 0, None) != 0
    assert handle.vfn_image_scores(None, 0, None, 0, 1 << 29, 2, 2, 1, 1, 1e-4, 9e-4, None, None, None, 0, None) != 0
    assert handle.vfn_image_scores(None, 0, None, 0, 1, 8, 8, 3, 1, 1e-4, 9e-4, None, None, None, 0, None) != 0
    assert b"NULL argument" in handle.vfn_last_error()
    assert handle.vfn_image_abs_err(None, None, 1, 1 << 15, 8, 100.0, None, None, None, 0, None) != 0
    assert handle.vfn_image_abs_err(None, None, 1, 8, 8, 100.0, None, None, None, 0, None) != 0
    assert handle.vfn_image_quantize8(None, 0, None, None, None) != 0 and b"outside [1, 2^31)" in handle.vfn_last_error()
    assert handle.vfn_image_quantize8(None, 1 << 31, None, None, None) != 0
    assert handle.vfn_image_quantize8(None, 5, None, None, None) != 0


IMG = np.zeros((6, 5, 3), dtype=np.float32)
DEPTH = np.zeros((6, 5), dtype=np.float32)


@pytest.mark.parametrize("call", [
    lambda: metrics2d.image_scores(IMG, np.zeros((6, 4, 3), dtype=np.float32)),                    # shape mismatch
    lambda: metrics2d.image_scores(IMG, np.zeros((1, 6, 5, 3), dtype=np.float32)),
    lambda: metrics2d.image_scores(np.zeros((6, 5, 2), dtype=np.float32), np.zeros((6, 5, 2), dtype=np.float32)),     # C not in {1, 3}
    lambda: metrics2d.image_scores(np.zeros((6, 5, 4), dtype=np.uint8), np.zeros((6, 5, 4), dtype=np.uint8)),
    lambda: metrics2d.image_scores(np.zeros((6, 5), dtype=np.float32), np.zeros((6, 5), dtype=np.float32)),
    lambda: metrics2d.image_scores(np.zeros((0, 5, 3), dtype=np.float32), np.zeros((0, 5, 3), dtype=np.float32)),     # empty
    lambda: metrics2d.image_scores(np.zeros((0, 6, 5, 3), dtype=np.float32), np.zeros((0, 6, 5, 3), dtype=np.float32)),
    lambda: metrics2d.image_scores(IMG.astype(bool), IMG),                                          # bool / other dtypes
    lambda: metrics2d.image_scores(IMG, IMG.astype(bool)),
    lambda: metrics2d.image_scores(IMG.astype(np.float64), IMG),
    lambda: metrics2d.image_scores(IMG, IMG.astype(np.int32)),
    lambda: metrics2d.image_scores(torch.zeros(1).expand(2, 20000, 20000, 3), torch.zeros(1).expand(2, 20000, 20000, 3)),     # V H W C >= 2^31
    lambda: metrics2d.image_scores(torch.zeros(1).expand(1, 1 << 15, 3), torch.zeros(1).expand(1, 1 << 15, 3)),              # W >= 2^15
    lambda: metrics2d.image_scores(IMG, IMG, quantize=1),
    lambda: metrics2d.image_scores(IMG, IMG, ssim="yes"),
    lambda: metrics2d.image_scores(IMG, IMG, pred_depth=DEPTH),                                     # one depth without the other
    lambda: metrics2d.image_scores(IMG, IMG, pred_depth=DEPTH, target_depth=np.zeros((5, 6), dtype=np.float32)),
    lambda: metrics2d.image_scores(IMG, IMG, pred_depth=DEPTH.astype(np.float64), target_depth=DEPTH),
    lambda: metrics2d.quantize_rgb8(np.zeros((0, 3), dtype=np.float32)),
    lambda: metrics2d.quantize_rgb8(IMG.astype(np.float64)),
    lambda: metrics2d.quantize_rgb8(IMG.astype(bool)),
    lambda: metrics2d.score_views([], []),
    lambda: metrics2d.score_views([IMG], [IMG, IMG]),
    lambda: metrics2d.score_views([IMG, np.zeros((6, 5, 2), dtype=np.float32)], [IMG, np.zeros((6, 5, 2), dtype=np.float32)]),
    lambda: metrics2d.score_views([IMG], [IMG], pred_depths=[DEPTH]),
    lambda: metrics2d.score_views([IMG], [np.zeros((5, 6, 3), dtype=np.float32)]),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(metrics2d, "_device", no_device)
    with pytest.raises(ValueError):
        call()


def test_wrong_container_types_raise_type_error():
    with pytest.raises(TypeError):
        metrics2d.image_scores([[0.0]], IMG)
    with pytest.raises(TypeError):
        metrics2d.quantize_rgb8("image.png")


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the calls would run")
def test_no_cpu_fallback():
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics2d.image_scores(IMG, IMG)
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics2d.quantize_rgb8(IMG)
    with pytest.raises(lib.VfnError):
        lib.image_scores(torch.zeros(1, 6, 5, 3), torch.zeros(1, 6, 5, 3), True, torch.zeros(1, dtype=torch.int64))


@pytest.fixture
def host_kernels(monkeypatch):
    """The three entry points of vf_nerf_amd.lib replaced by the restatement on host tensors: what is under test is the Python around
    them (grouping, keys, means, refusals)."""
    launches = []

    def quantize8(x, info):
        u, bits = R.quantize8(x.numpy())
        info |= bits
        return torch.from_numpy(u)

    def scores(pred, target, want_ssim, info):
        launches.append(tuple(pred.shape))
        return torch.from_numpy(R.scores_sums(pred.numpy(), target.numpy(), want_ssim))

    def abs_err(a, b, scale, info):
        return torch.from_numpy(R.abs_err_sums(a.numpy(), b.numpy(), scale))

    monkeypatch.setattr(metrics2d, "_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(lib, "image_quantize8", quantize8)
    monkeypatch.setattr(lib, "image_scores", scores)
    monkeypatch.setattr(lib, "image_abs_err", abs_err)
    return launches


def test_score_views_returns_the_references_dictionary(host_kernels):
    g = np.random.default_rng(3)
    small = [g.random((9, 7, 3), dtype=np.float32) for _ in range(3)]
    large = [g.random((20, 18, 3), dtype=np.float32) for _ in range(2)]
    preds = [small[0], large[0], small[1], large[1], small[2]]
    targets = [g.random(p.shape, dtype=np.float32) for p in preds]
    out = metrics2d.score_views(preds, targets)
    assert list(out) == ["image-0", "image-1", "image-2", "image-3", "image-4", "mean_psnr"]                 # methods.py:604-607
    assert all(list(out[f"image-{i}"]) == ["psnr"] for i in range(5))
    assert sorted(host_kernels) == [(2, 20, 18, 3), (3, 9, 7, 3)]                                           # views of one size: one launch
    for i in range(5):
        assert out[f"image-{i}"]["psnr"] == R.image_scores(R.quantize8(preds[i])[0], targets[i], False)["psnr"]
    total = 0.0
    for i in range(5):
        total += out[f"image-{i}"]["psnr"]
    assert out["mean_psnr"] == total / 5
    depths = [g.random(p.shape[:2], dtype=np.float32) for p in preds]
    full = metrics2d.score_views(preds, targets, ssim=True, pred_depths=depths, target_depths=[d[:, :, None] + np.float32(0.5) for d in depths])
    assert list(full) == [f"image-{i}" for i in range(5)] + ["mean_psnr", "mean_ssim", "mean_depth_l1_cm"]
    assert list(full["image-3"]) == ["psnr", "ssim", "depth_l1_cm"] and full["image-3"]["psnr"] == out["image-3"]["psnr"]
    assert abs(full["mean_depth_l1_cm"] - 50.0) < 1e-4
    # a [V,H,W,3] array is V views
    stacked = metrics2d.score_views(np.stack(small), np.stack([targets[0], targets[2], targets[4]]))
    assert [stacked[f"image-{i}"] for i in range(3)] == [out["image-0"], out["image-2"], out["image-4"]]


def test_image_scores_keys_quantisation_and_refusals(host_kernels):
    g = np.random.default_rng(4)
    pred, target = g.random((13, 21, 3), dtype=np.float32), g.random((13, 21, 3), dtype=np.float32)
    got = metrics2d.image_scores(pred, target)
    assert list(got) == ["psnr", "ssim"] and got == R.image_scores(R.quantize8(pred)[0], target)
    assert metrics2d.image_scores(pred, target, quantize=False) == R.image_scores(pred, target)
    assert list(metrics2d.image_scores(pred, target, ssim=False)) == ["psnr"]
    both = metrics2d.image_scores(np.stack([pred, target]), np.stack([target, target]), quantize=False)
    assert isinstance(both, list) and both[0] == R.image_scores(pred, target) and both[1] == {"psnr": math.inf, "ssim": 1.0}
    assert metrics2d.image_scores(np.zeros((4, 4, 3), dtype=np.float32), np.ones((4, 4, 3), dtype=np.float32))["psnr"] == 0.0
    u = metrics2d.quantize_rgb8(pred)
    assert u.dtype == torch.uint8 and np.array_equal(u.numpy(), numpy_bytes(pred))
    for bad in (256 / 255, -1e-3, np.nan):
        x = np.zeros(1000, dtype=np.float32)
        x[-1] = bad
        with pytest.raises(lib.VfnError):
            metrics2d.quantize_rgb8(x)
        with pytest.raises(lib.VfnError):
            metrics2d.image_scores(x.reshape(10, 100, 1), np.zeros((10, 100, 1), dtype=np.float32))


def test_install_patches_metrics_only_when_asked():
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("models", "evaluation")}
    fake_pkg, fake = types.ModuleType("evaluation"), types.ModuleType("evaluation.methods")
    fake_pkg.__path__ = []
    reference_metrics = lambda *a, **k: "reference metrics"          # noqa: E731
    fake.render_images, fake.metrics = (lambda *a, **k: "reference"), reference_metrics
    try:
        sys.modules["evaluation"], sys.modules["evaluation.methods"] = fake_pkg, fake
        dropin = importlib.import_module("vf_nerf_amd.dropin")
        from vf_nerf_amd import evaluator
        dropin.install()
        assert fake.metrics is reference_metrics and not hasattr(fake, "_reference_metrics")       # the default leaves it alone
        dropin.install(patch_metrics=False)
        assert fake.metrics is reference_metrics
        dropin.install(patch_metrics=True)
        assert fake.metrics is evaluator.metrics and fake._reference_metrics is reference_metrics
        assert fake.render_images is evaluator.render_images
        dropin.install(patch_metrics=True)                                                         # twice: the reference's is kept
        assert fake._reference_metrics is reference_metrics
        dropin.install()
        assert fake.metrics is reference_metrics and fake.render_images is evaluator.render_images
    finally:
        import vf_nerf_amd.dropin as dropin
        dropin.uninstall_clip_grad_norm()
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "evaluation")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_evaluator_metrics_writes_the_references_json(host_kernels, tmp_path):
    """evaluator.metrics with the reference's modules stood in for: a ten-view dataset (more than one chunk of views), 'PNG' files that
    hold the bytes, a render_images that writes them when they are missing.  metrics.json has the reference's keys and the PSNR of the
    restatement for every view."""
    import json
    from vf_nerf_amd import evaluator
    h, w, n = 6, 9, 10
    g = np.random.default_rng(17)
    targets = [g.random((h, w, 3), dtype=np.float32) for _ in range(n)]
    renders = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    calls = []

    class Dataset(torch.utils.data.Dataset):
        image_size, white_bkgd = (h, w), False

        def __init__(self, config):
            self.config = config

        def __len__(self):
            return n

        def __getitem__(self, i):
            return {"rgb": torch.from_numpy(targets[i]).reshape(-1, 3), "depth": torch.zeros(h * w, 1)}

    def load_rgb(path):                                             # utils.load_rgb: [3,H,W] float32 = byte / 255
        with open(path, "rb") as fh:
            return (np.load(fh).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)

    def render_images(model, eval_path, dataset_config, epoch, split_size, device):
        calls.append((eval_path, epoch, split_size))
        os.makedirs(os.path.join(eval_path, "rendered_images"), exist_ok=True)
        for i in range(n):
            with open(os.path.join(eval_path, "rendered_images", f"image-{i}.png"), "wb") as fh:
                np.save(fh, renders[i])
            np.save(os.path.join(eval_path, "rendered_images", f"depth-{i}.npy"), np.zeros((h, w, 1)))

    names = ("datasets", "datasets.normal_datasets", "utils", "utils.utils", "evaluation", "evaluation.methods")
    saved = {k: sys.modules[k] for k in names if k in sys.modules}
    fakes = {k: types.ModuleType(k) for k in names}
    for k in ("datasets", "utils", "evaluation"):
        fakes[k].__path__ = []
    fakes["datasets.normal_datasets"].dataset_dict = {"fake": Dataset}
    fakes["utils.utils"].load_rgb = load_rgb
    fakes["evaluation.methods"].render_images = render_images
    config = types.SimpleNamespace(dataset_name="fake")
    try:
        sys.modules.update(fakes)
        evaluator.metrics(None, str(tmp_path), config, 7, split_size=200, device=torch.device("cpu"))
        evaluator.metrics(None, str(tmp_path), config, 7, split_size=200, device=torch.device("cpu"))      # the files exist now
    finally:
        for k in names:
            del sys.modules[k]
        sys.modules.update(saved)
    assert calls == [(str(tmp_path), 7, 200)]
    with open(os.path.join(str(tmp_path), "metrics.json")) as fh:
        text = fh.read()
    got = json.loads(text)
    assert list(got) == [f"image-{i}" for i in range(n)] + ["mean_psnr"] and text.startswith('{\n    "image-0": {\n        "psnr": ')
    want = [R.image_scores(renders[i], targets[i], False)["psnr"] for i in range(n)]
    assert [got[f"image-{i}"] for i in range(n)] == [{"psnr": x} for x in want]
    total = 0.0
    for x in want:
        total += x
    assert got["mean_psnr"] == total / n
    assert sorted(host_kernels) == [(2, h, w, 3), (2, h, w, 3), (8, h, w, 3), (8, h, w, 3)]
