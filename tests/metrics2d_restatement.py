"""The image-score contract of include/vfn.h (csrc/vfn_image.hip) restated in NumPy, operation for operation and in the same
association: the byte quantisation, the per-element squared difference and SSIM value, and the fixed tree that joins them per view.
Every operation is one IEEE float64 operation on whole arrays (NumPy does not contract or reassociate elementwise arithmetic), so the
bits are those of the device.  Vectorised: a 680 x 1200 x 3 view takes a few seconds."""
import math

import numpy as np

import tree_restatement as T

TILE, TOP = 16, T.TOP         # include/vfn.h: VFN_IMAGE_TILE, VFN_TREE_TOP
R, K = 5, 11                  # window radius, window edge
C1, C2 = 1e-4, 9e-4           # utils/utils.py:249


def quantize8(x):
    """float32 array -> (uint8 array, info): trunc(double(x) 255); info bit 1 = a non-finite value, bit 4 = x < 0 or the product >= 256
    (the byte is 0 in both cases)."""
    x = np.asarray(x, dtype=np.float32)
    v = x.astype(np.float64) * 255.0
    finite = np.isfinite(x)
    out_of_range = finite & ((x < 0) | (v >= 256.0))
    ok = finite & ~out_of_range
    u = np.zeros(x.shape, dtype=np.uint8)
    u[ok] = np.trunc(v[ok]).astype(np.uint8)
    return u, (0 if finite.all() else 1) | (4 if out_of_range.any() else 0)


def as_double(a):
    """uint8 -> double(u) / 255.0 (one rounded division); float32 -> double(x)."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.float64) / 255.0
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def _box(a):
    """a[H,W,C] -> m_a: zero padding, the 11 columns added serially from the left, then the 11 rows serially from the top, / 121."""
    h, w, c = a.shape
    pad = np.zeros((h + 2 * R, w + 2 * R, c))
    pad[R:R + h, R:R + w] = a
    r = pad[:, 0:w].copy()
    for d in range(1, K):
        r = r + pad[:, d:d + w]
    s = r[0:h].copy()
    for d in range(1, K):
        s = s + r[d:d + h]
    return s / 121.0


def ssim_map(p, t, c1=C1, c2=C2):
    """p, t float64 [H,W,C] -> the per-element SSIM values."""
    mu1, mu2 = _box(p), _box(t)
    m_pp, m_tt, m_pt = _box(p * p), _box(t * t), _box(p * t)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = m_pp - mu1_sq, m_tt - mu2_sq, m_pt - mu12
    return ((2.0 * mu12 + c1) * (2.0 * s12 + c2)) / (((mu1_sq + mu2_sq) + c1) * ((s1 + s2) + c2))


def squared_error_map(p, t):
    d = p - t
    return d * d


def view_sum(e):
    """e[H,W,C] per-element values of ONE view -> their sum along the fixed tree: a lane's channels serially, the 256 lanes of a
    16 x 16 tile as a balanced tree (l takes l + d, d = 128 .. 1; lanes outside the image hold +0.0), the tiles in (tile_y, tile_x) order
    joined by the second level of tests/tree_restatement.py."""
    h, w, c = e.shape
    lane = e[:, :, 0].copy()
    for k in range(1, c):
        lane = lane + e[:, :, k]
    ty, tx = -(-h // TILE), -(-w // TILE)
    pad = np.zeros((ty * TILE, tx * TILE))
    pad[:h, :w] = lane
    a = pad.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty * tx, TILE * TILE)     # [tile, l = 16 ly + lx]
    return float(T.top_join(T.block_tree(a)))


def elements(pred, target, want_ssim=True, c1=C1, c2=C2):
    """pred, target [H,W,C] (uint8 or float32) -> (squared-error map, ssim map or None), float64 [H,W,C]."""
    p, t = as_double(pred), as_double(target)
    return squared_error_map(p, t), (ssim_map(p, t, c1, c2) if want_ssim else None)


def scores_sums(pred, target, want_ssim=True, c1=C1, c2=C2):
    """pred, target [V,H,W,C] -> sums[V,3] as vfn_image_scores writes them."""
    pred, target = np.asarray(pred), np.asarray(target)
    assert pred.ndim == 4 and pred.shape == target.shape
    out = np.zeros((pred.shape[0], 3))
    for v in range(pred.shape[0]):
        sq, ss = elements(pred[v], target[v], want_ssim, c1, c2)
        out[v, 0] = view_sum(sq)
        if want_ssim:
            out[v, 1] = view_sum(ss)
    return out


def abs_err_sums(a, b, scale=100.0):
    """a, b [V,H,W] float32 -> sums[V] as vfn_image_abs_err writes them."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.ndim == 3 and a.shape == b.shape
    return np.array([view_sum(np.abs(a[v].astype(np.float64) * scale - b[v].astype(np.float64) * scale)[:, :, None]) for v in range(a.shape[0])])


def psnr_from(s0, n):
    return float("inf") if s0 == 0.0 else -10.0 * math.log10(float(s0) / n)


def image_scores(pred, target, want_ssim=True, pred_depth=None, target_depth=None):
    """One view [H,W,C] -> the dictionary metrics2d.image_scores returns for it (a float32 prediction is scored as it is)."""
    sums = scores_sums(np.asarray(pred)[None], np.asarray(target)[None], want_ssim)[0]
    n = np.asarray(pred).size
    out = {"psnr": psnr_from(sums[0], n)}
    if want_ssim:
        out["ssim"] = float(sums[1]) / n
    if pred_depth is not None:
        h, w = np.asarray(pred).shape[:2]
        out["depth_l1_cm"] = float(abs_err_sums(np.asarray(pred_depth).reshape(1, h, w), np.asarray(target_depth).reshape(1, h, w))[0]) / (h * w)
    return out
