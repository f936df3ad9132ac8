// vfn_image.hip — scoring rendered views on the device: the image half of evaluation/methods.py:549-610 (metrics) with
// utils/utils.py:235-289 (get_psnr, get_ssim), :312-325 (get_l1_cm) and the save_rgb -> PNG -> load_rgb round trip (:73-108).
//   quantize8   one lane per value: trunc(double(x) 255), refused (not wrapped) outside [0, 256).
//   scores      one 256-lane workgroup per IMG_TILE x IMG_TILE tile of pixels, the channels one after another.  For SSIM the tile and its
//               5-pixel halo are staged in LDS as doubles (26 x 26 per image), a horizontal pass forms the 11-term row sums of the five
//               windowed quantities for the tile's 26 rows, a vertical pass the 11-row sums of the lane's own pixel: 2 x 11 additions
//               per quantity instead of 121, in the association of include/vfn.h (direct sums, no running window).
//   abs_err     the same tiles over one-channel float images: |a s - b s|.
//   sums        the fixed tree of vfn_tree.h without a lane tree: the block tree over the 256 lanes of a tile into one partial per
//               tile, then the second level once per view over that view's partials.
// All arithmetic fp64 with -ffp-contract=off (build.sh): the expressions of include/vfn.h, operation for operation.
#include "vfn_common.h"
#include "vfn_tree.h"
#include <math.h>

namespace {

constexpr int IMG_TILE = VFN_IMAGE_TILE;            // pixels per tile edge: 16 x 16 = one lane per pixel
constexpr int IMG_BLOCK = IMG_TILE * IMG_TILE;      // 256 lanes
static_assert(IMG_BLOCK == TREE_LANES, "a tile is one first-level block of the fixed tree");
constexpr int IMG_R = 5, IMG_K = 2 * IMG_R + 1;     // window radius, window edge (11)
constexpr int IMG_HALO = IMG_TILE + 2 * IMG_R;      // 26 staged rows / columns
using Pair = TreeSum<2>;                            // a view's two sums travel together

__device__ __forceinline__ double img_value(const float* p, long long i) { return (double)p[i]; }
__device__ __forceinline__ double img_value(const unsigned char* p, long long i) { return (double)p[i] / 255.0; }
__device__ __forceinline__ bool img_bad(const float* p, long long i) { return !isfinite(p[i]); }
__device__ __forceinline__ bool img_bad(const unsigned char*, long long) { return false; }

// the block tree over the 256 lane values of a tile -> the tile's partial
__device__ __forceinline__ void img_tile_tree(double a, double b, Pair* red, double* __restrict__ partial) {
    const Pair r = tree_block<IMG_BLOCK>(Pair{{a, b}}, red, TreeAdd());
    if (threadIdx.x == 0) { partial[0] = r.v[0]; partial[1] = r.v[1]; }
}

// block (view v, tile_y, tile_x) = blockIdx.x in that order; lane l = 16 ly + lx owns pixel (16 tile_y + ly, 16 tile_x + lx)
template <typename PT, typename TT, bool SSIM>
__global__ __launch_bounds__(IMG_BLOCK) void vfn_image_scores_kernel(const PT* __restrict__ pred, const TT* __restrict__ target, int H, int W, int C,
                                                                     int tiles_y, int tiles_x, double c1, double c2,
                                                                     double* __restrict__ partials, unsigned long long* __restrict__ info) {
    __shared__ double sp[SSIM ? IMG_HALO : 1][IMG_HALO + 1], st[SSIM ? IMG_HALO : 1][IMG_HALO + 1];
    __shared__ double rs[SSIM ? 5 : 1][SSIM ? IMG_HALO : 1][IMG_TILE + 1];
    __shared__ Pair red[IMG_BLOCK];
    const int l = threadIdx.x, ly = l / IMG_TILE, lx = l % IMG_TILE;
    const long long b = blockIdx.x;
    const int tx = (int)(b % tiles_x), ty = (int)((b / tiles_x) % tiles_y);
    const long long v = b / ((long long)tiles_x * tiles_y);
    const int y0 = ty * IMG_TILE, x0 = tx * IMG_TILE;
    const int y = y0 + ly, x = x0 + lx;
    const bool inside = y < H && x < W;
    const long long view = v * H * W;                 // pixels before this view
    double acc_sq = 0.0, acc_ss = 0.0;
    bool bad = false;
    for (int c = 0; c < C; ++c) {
        double p = 0.0, t = 0.0, ss = 0.0;
        if (SSIM) {
            for (int i = l; i < IMG_HALO * IMG_HALO; i += IMG_BLOCK) {
                const int hy = i / IMG_HALO, hx = i % IMG_HALO;
                const int gy = y0 + hy - IMG_R, gx = x0 + hx - IMG_R;
                double pv = 0.0, tv = 0.0;                    // a term outside the image is +0.0
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    const long long e = (view + (long long)gy * W + gx) * C + c;
                    pv = img_value(pred, e);
                    tv = img_value(target, e);
                    bad = bad || img_bad(pred, e) || img_bad(target, e);
                }
                sp[hy][hx] = pv;
                st[hy][hx] = tv;
            }
            __syncthreads();
            // horizontal: row sums of p, t, p p, t t, p t for the 26 staged rows at the tile's 16 columns, ascending dx.  (A lane taking
            // two neighbouring columns — 12 staged values read and squared once for both windows — was measured slower, 4.88 against
            // 4.28 ms on 100 views: 136 VGPRs, three waves per SIMD instead of four.)
            for (int i = l; i < IMG_HALO * IMG_TILE; i += IMG_BLOCK) {
                const int hy = i / IMG_TILE, cx = i % IMG_TILE;
                double r0, r1, r2, r3, r4;
                {
                    const double pv = sp[hy][cx], tv = st[hy][cx];
                    r0 = pv; r1 = tv; r2 = pv * pv; r3 = tv * tv; r4 = pv * tv;
                }
#pragma unroll
                for (int d = 1; d < IMG_K; ++d) {
                    const double pv = sp[hy][cx + d], tv = st[hy][cx + d];
                    r0 = r0 + pv; r1 = r1 + tv; r2 = r2 + pv * pv; r3 = r3 + tv * tv; r4 = r4 + pv * tv;
                }
                rs[0][hy][cx] = r0; rs[1][hy][cx] = r1; rs[2][hy][cx] = r2; rs[3][hy][cx] = r3; rs[4][hy][cx] = r4;
            }
            __syncthreads();
            p = sp[ly + IMG_R][lx + IMG_R];
            t = st[ly + IMG_R][lx + IMG_R];
            // vertical: the lane's own pixel, ascending dy
            double s[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                double r = rs[a][ly][lx];
#pragma unroll
                for (int d = 1; d < IMG_K; ++d) r = r + rs[a][ly + d][lx];
                s[a] = r / 121.0;
            }
            const double mu1 = s[0], mu2 = s[1];
            const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const double s1 = s[2] - mu1_sq, s2 = s[3] - mu2_sq, s12 = s[4] - mu12;
            ss = ((2.0 * mu12 + c1) * (2.0 * s12 + c2)) / (((mu1_sq + mu2_sq) + c1) * ((s1 + s2) + c2));
        } else if (inside) {
            const long long e = (view + (long long)y * W + x) * C + c;
            p = img_value(pred, e);
            t = img_value(target, e);
            bad = bad || img_bad(pred, e) || img_bad(target, e);
        }
        const double diff = p - t;
        const double sq = diff * diff;
        if (inside) {                                  // a lane's channels serially, in ascending c
            acc_sq = c == 0 ? sq : acc_sq + sq;
            if (SSIM) acc_ss = c == 0 ? ss : acc_ss + ss;
        }
        if (SSIM) __syncthreads();                     // the next channel overwrites sp / st / rs
    }
    if (bad) atomicOr(info, 1ull);
    img_tile_tree(acc_sq, acc_ss, red, partials + 2 * b);
}

// the same tiles over a[V, H, W], b[V, H, W]: element = |a s - b s|
__global__ __launch_bounds__(IMG_BLOCK) void vfn_image_abs_err_kernel(const float* __restrict__ a, const float* __restrict__ bb, int H, int W,
                                                                      int tiles_y, int tiles_x, double scale, double* __restrict__ partials,
                                                                      unsigned long long* __restrict__ info) {
    __shared__ Pair red[IMG_BLOCK];
    const int l = threadIdx.x, ly = l / IMG_TILE, lx = l % IMG_TILE;
    const long long b = blockIdx.x;
    const int tx = (int)(b % tiles_x), ty = (int)((b / tiles_x) % tiles_y);
    const long long v = b / ((long long)tiles_x * tiles_y);
    const int y = ty * IMG_TILE + ly, x = tx * IMG_TILE + lx;
    double val = 0.0;
    if (y < H && x < W) {
        const long long e = (v * H + y) * W + x;
        if (!isfinite(a[e]) || !isfinite(bb[e])) atomicOr(info, 1ull);
        const double as = (double)a[e] * scale, bs = (double)bb[e] * scale;
        val = fabs(as - bs);
    }
    img_tile_tree(val, 0.0, red, partials + 2 * b);
}

// second level, one block per view over the view's per_view partials.  out[v n_out + k] = slot k for k < slots; the slots above are
// written 0.
__global__ __launch_bounds__(TREE_TOP) void vfn_image_top_kernel(const double* __restrict__ partials, long long per_view, double* __restrict__ out,
                                                                  int n_out, int slots) {
    __shared__ Pair sh[TREE_TOP];
    const double* __restrict__ part = partials + 2 * per_view * (long long)blockIdx.x;
    const Pair s = tree_top_lane(per_view, Pair{{0.0, 0.0}}, [&](long long i) { return Pair{{part[2 * i], part[2 * i + 1]}}; }, TreeAdd());
    const Pair r = tree_block<TREE_TOP>(s, sh, TreeAdd());
    if (threadIdx.x == 0) {
        double* o = out + (long long)blockIdx.x * n_out;
        o[0] = r.v[0];
        if (n_out > 1) o[1] = slots > 1 ? r.v[1] : 0.0;
        for (int k = 2; k < n_out; ++k) o[k] = 0.0;
    }
}

__global__ __launch_bounds__(256) void vfn_image_quantize8_kernel(const float* __restrict__ x, long long n, unsigned char* __restrict__ u,
                                                                  unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float f = x[i];
    const double val = (double)f * 255.0;             // exact: 24 bits x 8 bits
    unsigned char out = 0;
    if (!isfinite(f)) atomicOr(info, 1ull);
    else if (f < 0.0f || val >= 256.0) atomicOr(info, 4ull);
    else out = (unsigned char)(int)trunc(val);
    u[i] = out;
}

bool dims_ok(const char* who, int64_t V, int64_t H, int64_t W, int64_t C) {
    if (V < 1 || H < 1 || W < 1 || H >= (1ll << 15) || W >= (1ll << 15) || (C != 1 && C != 3)) {
        vfn_set_error("%s: V %lld, H %lld, W %lld, C %lld outside 1 <= V, 1 <= H, W < 2^15, C in {1, 3}", who, (long long)V, (long long)H,
                      (long long)W, (long long)C);
        return false;
    }
    // H W C < 3 x 2^30 cannot overflow; V is compared by division
    if (V > ((1ll << 31) - 1) / (H * W * C)) {
        vfn_set_error("%s: V H W C = %lld x %lld x %lld x %lld reaches 2^31", who, (long long)V, (long long)H, (long long)W, (long long)C);
        return false;
    }
    return true;
}

inline long long tiles_of(int64_t n) { return (n + IMG_TILE - 1) / IMG_TILE; }

template <typename PT, typename TT>
void launch_scores(const void* pred, const void* target, int64_t V, int64_t H, int64_t W, int64_t C, int want_ssim, double c1, double c2,
                   double* partials, int64_t* info, hipStream_t s) {
    const long long ty = tiles_of(H), tx = tiles_of(W);
    const dim3 grid((unsigned)(V * ty * tx)), block(IMG_BLOCK);
    if (want_ssim)
        hipLaunchKernelGGL((vfn_image_scores_kernel<PT, TT, true>), grid, block, 0, s, (const PT*)pred, (const TT*)target, (int)H, (int)W, (int)C,
                           (int)ty, (int)tx, c1, c2, partials, (unsigned long long*)info);
    else
        hipLaunchKernelGGL((vfn_image_scores_kernel<PT, TT, false>), grid, block, 0, s, (const PT*)pred, (const TT*)target, (int)H, (int)W, (int)C,
                           (int)ty, (int)tx, c1, c2, partials, (unsigned long long*)info);
}

}  // namespace

extern "C" int64_t vfn_image_scores_workspace_bytes(int64_t V, int64_t H, int64_t W, int64_t C) {
    if (!dims_ok("vfn_image_scores_workspace_bytes", V, H, W, C)) return -1;
    return (int64_t)(V * tiles_of(H) * tiles_of(W) * 2 * (long long)sizeof(double));
}

extern "C" int vfn_image_scores(const void* pred, int32_t pred_u8, const void* target, int32_t target_u8, int64_t V, int64_t H, int64_t W,
                                int64_t C, int32_t want_ssim, double c1, double c2, double* sums, int64_t* info, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    const int64_t need = vfn_image_scores_workspace_bytes(V, H, W, C);
    if (need < 0) return VFN_ERR_INVALID;
    VFN_REQUIRE(isfinite(c1) && isfinite(c2), "vfn_image_scores: C1 / C2 not finite");
    VFN_REQUIRE(pred && target && sums && info && workspace && workspace_bytes >= need,
                "vfn_image_scores: NULL argument or a workspace of %lld bytes < %lld", (long long)workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    double* partials = (double*)workspace;
    if (pred_u8 && target_u8) launch_scores<unsigned char, unsigned char>(pred, target, V, H, W, C, want_ssim, c1, c2, partials, info, s);
    else if (pred_u8) launch_scores<unsigned char, float>(pred, target, V, H, W, C, want_ssim, c1, c2, partials, info, s);
    else if (target_u8) launch_scores<float, unsigned char>(pred, target, V, H, W, C, want_ssim, c1, c2, partials, info, s);
    else launch_scores<float, float>(pred, target, V, H, W, C, want_ssim, c1, c2, partials, info, s);
    hipLaunchKernelGGL(vfn_image_top_kernel, dim3((unsigned)V), dim3(TREE_TOP), 0, s, (const double*)partials, tiles_of(H) * tiles_of(W), sums, 3,
                       want_ssim ? 2 : 1);
    return vfn_check_launch("vfn_image_scores");
}

extern "C" int vfn_image_abs_err(const float* a, const float* b, int64_t V, int64_t H, int64_t W, double scale, double* sums, int64_t* info,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    const int64_t need = vfn_image_scores_workspace_bytes(V, H, W, 1);
    if (need < 0) return VFN_ERR_INVALID;
    VFN_REQUIRE(isfinite(scale), "vfn_image_abs_err: scale not finite");
    VFN_REQUIRE(a && b && sums && info && workspace && workspace_bytes >= need,
                "vfn_image_abs_err: NULL argument or a workspace of %lld bytes < %lld", (long long)workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const long long ty = tiles_of(H), tx = tiles_of(W);
    hipLaunchKernelGGL(vfn_image_abs_err_kernel, dim3((unsigned)(V * ty * tx)), dim3(IMG_BLOCK), 0, s, a, b, (int)H, (int)W, (int)ty, (int)tx, scale,
                       (double*)workspace, (unsigned long long*)info);
    hipLaunchKernelGGL(vfn_image_top_kernel, dim3((unsigned)V), dim3(TREE_TOP), 0, s, (const double*)workspace, ty * tx, sums, 1, 1);
    return vfn_check_launch("vfn_image_abs_err");
}

extern "C" int vfn_image_quantize8(const float* x, int64_t n, uint8_t* u, int64_t* info, void* stream) {
    VFN_REQUIRE(n >= 1 && n < (1ll << 31), "vfn_image_quantize8: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(x && u && info, "vfn_image_quantize8: NULL argument");
    hipLaunchKernelGGL(vfn_image_quantize8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, u,
                       (unsigned long long*)info);
    return vfn_check_launch("vfn_image_quantize8");
}
