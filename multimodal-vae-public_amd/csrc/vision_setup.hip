// The edge step of the vision experiment's setup (the reference's vision/setup.py:55-75 calls scikit-image's
// feature.canny(image / 255., sigma) once per CelebA file): Canny edge detection for a batch of uint8 images resident in
// HBM, as two launches.  The algorithm is the documented one -- Gaussian blur with zeros outside the image, divided by the
// same blur of an all-ones image; unnormalised 3x3 Sobel on the border-duplicated result; non-maximum suppression with
// bilinear interpolation along the gradient; two thresholds; hysteresis over 8-connected components -- and is spelled
// out step by step in include/mvae_hip.h (K26) and restated with numpy / scipy.ndimage in tests/vision_setup_ref.py.
//
// THE SPLIT
//   float stage   grid (tiles * B), 256 threads, one 32 x 32 output tile per block.  A class needs the magnitude of the 3 x 3
//                 neighbourhood, a magnitude the blurred image of its 3 x 3 neighbourhood, a blurred sample the source r
//                 pixels around it: the block stages the tile plus a halo of r + 2 as fp32 luma in LDS ((36 + 2r)^2 samples,
//                 52 x 52 at sigma 2), blurs vertically then horizontally from LDS, divides by the product of the two
//                 one-dimensional blurs of ones (rebuilt per tile from the taps: at most 2r + 1 adds per entry, no table in
//                 HBM), takes the Sobel pair and the magnitude on 34 x 34 and classifies its 32 x 32 pixels.  One byte per
//                 pixel leaves the block (and the magnitude, when asked for).  The taps arrive by value in the kernel
//                 arguments (fp32, built on the host in double).
//                 The two blur passes accumulate in fp64 and round to fp32 once per pass, the 1-2-1 pass of the Sobel pair likewise:
//                 that is the rounding of a filter library which computes in double and stores the array's type, so the
//                 stage tracks an fp32 run of the restatement to the last place almost everywhere instead of adding the
//                 error of 17-term fp32 sums in front of a gradient that amplifies it eightfold.  17 + 17 fp64 FMAs per
//                 pixel are nothing next to the launch: the image is 38.8 K pixels.
//   hysteresis    grid B, 256 threads, one block per image with the whole class plane in LDS, padded by a zero frame so that
//                 no neighbour test checks a bound (218 x 178: 220 rows x 188 bytes = 41.4 KB).  "Strong" spreads to weak
//                 8-neighbours until a block-wide OR says a full round changed nothing.  A round is four sweeps: a thread
//                 owns a row and walks it left to right, then right to left; barrier; a thread owns a strip of four pixel
//                 columns over a segment of rows (45 strips x 5 segments of 44 rows at 218 x 178) and walks it down, then
//                 up.  A sweep reads dwords, eight per LDS round trip, and looks closer only at those that hold a weak
//                 pixel: the plane is ~95 % zeros and "no weak pixel here" stays true once it is.  A sweep carries a label
//                 along a whole straight run, so a round crosses a run per direction instead of a pixel; every sweep
//                 advances any chain by at least one pixel (a neighbour that was strong when the sweep began), which
//                 bounds the rounds by the longest chain / 4.  Threads read neighbours other threads are promoting: the
//                 plane only ever moves weak -> strong, a stale read delays a promotion to the next sweep, and the fixed
//                 point -- the union of the components that hold a strong pixel -- does not depend on the order.  The output
//                 is the same bits on every run; the number of rounds need not be.
// No atomics, no global scratch beyond the class plane between the two launches (the caller's cls, or ws).
#include "common.h"
#include <math.h>

namespace {

constexpr int CN_MAX_R = 16;
constexpr int CN_TH = 32, CN_TW = 32, CN_THREADS = 256;
constexpr int CN_BH = CN_TH + 4, CN_BW = CN_TW + 4;      // blurred samples a tile needs: its pixels and two around
constexpr int CN_MH = CN_TH + 2, CN_MW = CN_TW + 2;      // gradients and magnitudes: its pixels and one around
constexpr int HY_THREADS = 256;
constexpr size_t HY_MAX_LDS = 144 * 1024;

struct CannyArgs {
    const uint8_t *src;
    uint8_t *cls;
    float *mag;
    int channels, H, W, r, tiles_x, tiles_y;
    float low, high;
    float taps[2 * CN_MAX_R + 1];
};

__host__ __device__ inline size_t float_stage_lds_bytes(int r) {
    const int SH = CN_BH + 2 * r, SW = CN_BW + 2 * r;
    return sizeof(float) * (size_t)(SH * SW + CN_BH * SW + CN_BH * CN_BW + 3 * CN_MH * CN_MW + CN_BH + CN_BW);
}

// Both interpolated neighbours of a candidate, along (dy1, dx1) -> (dy2, dx2) with weight w and along the negated
// offsets, are <= its own magnitude.  mg points at the candidate in the [CN_MH][CN_MW] magnitude tile.
__device__ __forceinline__ bool is_local_max(const float *mg, int dy1, int dx1, int dy2, int dx2, float w, float m) {
    const int o1 = dy1 * CN_MW + dx1, o2 = dy2 * CN_MW + dx2;
    const bool plus = mg[o2] * w + mg[o1] * (1.0f - w) <= m;
    const bool minus = mg[-o2] * w + mg[-o1] * (1.0f - w) <= m;
    return plus && minus;
}

__global__ __launch_bounds__(CN_THREADS) void canny_float_kernel(CannyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cn_lds[];
    const int r = a.r, H = a.H, W = a.W, t = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int ty0 = (tile / a.tiles_x) * CN_TH, tx0 = (tile % a.tiles_x) * CN_TW;
    const int SH = CN_BH + 2 * r, SW = CN_BW + 2 * r, ntaps = 2 * r + 1;
    float *src = cn_lds;                      // [SH][SW]      luma / 255, zero outside the image
    float *vb = src + SH * SW;                // [CN_BH][SW]   after the vertical pass
    float *bl = vb + CN_BH * SW;              // [CN_BH][CN_BW] blurred and normalised; 0 outside the image (never read)
    float *gi = bl + CN_BH * CN_BW;           // [CN_MH][CN_MW] Sobel along rows
    float *gj = gi + CN_MH * CN_MW;           //               Sobel along columns
    float *mg = gj + CN_MH * CN_MW;           //               magnitude, 0 outside the image
    float *ny = mg + CN_MH * CN_MW;           // [CN_BH]       vertical blur of ones at the tile's rows
    float *nx = ny + CN_BH;                   // [CN_BW]       horizontal blur of ones at the tile's columns
    const size_t px = (size_t)H * W;
    const int by0 = ty0 - 2, bx0 = tx0 - 2;   // image coordinates of bl[0][0]
    const int sy0 = by0 - r, sx0 = bx0 - r;   // ... of src[0][0]

    const uint8_t *img = a.src + (size_t)b * px * a.channels;
    for (int idx = t; idx < SH * SW; idx += CN_THREADS) {
        const int ly = idx / SW, lx = idx - ly * SW;
        const int y = sy0 + ly, x = sx0 + lx;
        float v = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t p = (size_t)y * W + x;
            int u;
            if (a.channels == 3) {
                const uint8_t *q = img + 3 * p;
                u = (q[0] * 19595 + q[1] * 38470 + q[2] * 7471 + 0x8000) >> 16;
            } else {
                u = img[p];
            }
            v = (float)u / 255.0f;
        }
        src[idx] = v;
    }
    if (t < CN_BH + CN_BW) {                  // the blur of ones along one axis: the taps that fall inside the image
        const bool rows = t < CN_BH;
        const int c = rows ? by0 + t : bx0 + (t - CN_BH), n = rows ? H : W;
        double s = 0.0;
        for (int k = 0; k < ntaps; ++k) {
            const int q = c + k - r;
            if (q >= 0 && q < n) s += (double)a.taps[k];
        }
        (rows ? ny : nx)[rows ? t : t - CN_BH] = (float)s;
    }
    __syncthreads();
    for (int idx = t; idx < CN_BH * SW; idx += CN_THREADS) {
        const int ly = idx / SW, lx = idx - ly * SW;
        const float *col = src + ly * SW + lx;
        double acc = 0.0;
        for (int k = 0; k < ntaps; ++k) acc += (double)a.taps[k] * (double)col[k * SW];
        vb[idx] = (float)acc;
    }
    __syncthreads();
    for (int idx = t; idx < CN_BH * CN_BW; idx += CN_THREADS) {
        const int ly = idx / CN_BW, lx = idx - ly * CN_BW;
        const int y = by0 + ly, x = bx0 + lx;
        float v = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const float *row = vb + ly * SW + lx;
            double acc = 0.0;
            for (int k = 0; k < ntaps; ++k) acc += (double)a.taps[k] * (double)row[k];
            v = (float)acc / (ny[ly] * nx[lx]);
        }
        bl[idx] = v;
    }
    __syncthreads();
    for (int idx = t; idx < CN_MH * CN_MW; idx += CN_THREADS) {
        const int ly = idx / CN_MW, lx = idx - ly * CN_MW;
        const int y = ty0 - 1 + ly, x = tx0 - 1 + lx;
        float si = 0.0f, sj = 0.0f, m = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            // rows / columns of bl at y - 1, y, y + 1 and x - 1, x, x + 1 with the border sample duplicated
            const int r0 = max(y - 1, 0) - by0, r1 = y - by0, r2 = min(y + 1, H - 1) - by0;
            const int c0 = max(x - 1, 0) - bx0, c1 = x - bx0, c2 = min(x + 1, W - 1) - bx0;
            const float *R0 = bl + r0 * CN_BW, *R1 = bl + r1 * CN_BW, *R2 = bl + r2 * CN_BW;
            // the difference pass in fp32, the 1-2-1 pass summed in fp64 and rounded once
            const float d0 = R2[c0] - R0[c0], d1 = R2[c1] - R0[c1], d2 = R2[c2] - R0[c2];
            const float e0 = R0[c2] - R0[c0], e1 = R1[c2] - R1[c0], e2 = R2[c2] - R2[c0];
            si = (float)((double)d0 + 2.0 * (double)d1 + (double)d2);
            sj = (float)((double)e0 + 2.0 * (double)e1 + (double)e2);
            m = sqrtf(si * si + sj * sj);
        }
        gi[idx] = si; gj[idx] = sj; mg[idx] = m;
    }
    __syncthreads();
    for (int idx = t; idx < CN_TH * CN_TW; idx += CN_THREADS) {
        const int ly = idx / CN_TW, lx = idx - ly * CN_TW;
        const int y = ty0 + ly, x = tx0 + lx;
        if (y >= H || x >= W) continue;
        const int c = (ly + 1) * CN_MW + lx + 1;
        const float m = mg[c];
        int cl = 0;
        if (y > 0 && y < H - 1 && x > 0 && x < W - 1 && m > 0.0f) {
            const float si = gi[c], sj = gj[c], ai = fabsf(si), aj = fabsf(sj);
            const bool same = (si >= 0.0f && sj >= 0.0f) || (si <= 0.0f && sj <= 0.0f);
            const bool opposite = (si <= 0.0f && sj >= 0.0f) || (si >= 0.0f && sj <= 0.0f);
            bool lm = false;                  // the four cases in order: a later one overwrites an earlier one
            if (same && ai >= aj) lm = is_local_max(mg + c, 1, 0, 1, 1, aj / ai, m);
            if (same && ai <= aj) lm = is_local_max(mg + c, 0, 1, 1, 1, ai / aj, m);
            if (opposite && ai <= aj) lm = is_local_max(mg + c, 0, 1, -1, 1, ai / aj, m);
            if (opposite && ai >= aj) lm = is_local_max(mg + c, -1, 0, -1, 1, aj / ai, m);
            if (lm) cl = m >= a.high ? 2 : (m >= a.low ? 1 : 0);
        }
        const size_t o = (size_t)b * px + (size_t)y * W + x;
        a.cls[o] = (uint8_t)cl;
        if (a.mag) a.mag[o] = m;
    }
}

// The class plane in LDS: H + 2 rows of hy_stride(W) bytes, pixel (y, x) at (y + 1) * stride + 4 + x.  Four pad bytes on
// the left keep a row's pixels on dword boundaries, at least four on the right and a row above and below stay zero.
__host__ __device__ inline int hy_stride(int W) { return (W + 8 + 3) & ~3; }
__host__ __device__ inline size_t hy_lds_bytes(int H, int W) { return (size_t)(H + 2) * hy_stride(W); }

// The four pixels of the aligned dword at byte `o`, all at once: byte k of `(x << 8) | (prev >> 24)` is the left neighbour
// of pixel k, of `(x >> 8) | (next << 24)` the right one; strong is 2, so bit 1 of the OR of the eight neighbour words,
// moved to bit 0, marks the pixels with a strong neighbour, and adding it to a weak pixel (1) makes it strong.  The pixels of
// the dword feed each other, hence the loop (at most four passes).  The nine dwords are fetched in one LDS round trip.
__device__ __forceinline__ int hy_update(uint8_t *plane, int S, int o) {
    volatile uint32_t *p = reinterpret_cast<volatile uint32_t *>(plane + o);
    const int s = S >> 2;
    const uint32_t a0 = p[-s - 1], a1 = p[-s], a2 = p[-s + 1], c0 = p[-1], c1 = p[0], c2 = p[1], b0 = p[s - 1], b1 = p[s],
                   b2 = p[s + 1];
    const uint32_t rows = a1 | (a1 << 8) | (a0 >> 24) | (a1 >> 8) | (a2 << 24) | b1 | (b1 << 8) | (b0 >> 24) | (b1 >> 8) |
                          (b2 << 24) | (c0 >> 24) | (c2 << 24);
    uint32_t cur = c1;
    for (int pass = 0; pass < 4; ++pass) {
        const uint32_t promote = cur & ((rows | (cur << 8) | (cur >> 8)) >> 1) & 0x01010101u;
        if (!promote) break;
        cur += promote;
    }
    if (cur == c1) return 0;
    p[0] = cur;
    return 1;
}

// One sweep over n dwords of the plane, the first at byte `base`, consecutive ones `step` bytes apart; REVERSE walks them
// from the last to the first.  Eight dwords are fetched at a time with plain loads, so the common case -- no weak pixel in
// any of them -- costs one LDS round trip per eight instead of one per dword.  A fetched value may be stale by the time it
// is looked at, which is harmless: "no weak pixel here" never stops being true, and a dword that had one is re-read with
// its neighbours.  A thread stores only dwords it owns in the sweep (its row; its strip and segment).
template <bool REVERSE>
__device__ __forceinline__ int hy_sweep(uint8_t *plane, int S, int base, int step, int n) {
    int changed = 0;
    for (int i0 = 0; i0 < n; i0 += 8) {
        uint32_t d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = REVERSE ? n - 1 - (i0 + k) : i0 + k;
            d[k] = i0 + k < n ? *reinterpret_cast<const uint32_t *>(plane + base + i * step) : 0u;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (!(d[k] & 0x01010101u)) continue;                       // no weak pixel among these four
            changed |= hy_update(plane, S, base + (REVERSE ? n - 1 - (i0 + k) : i0 + k) * step);
        }
    }
    return changed;
}

__global__ __launch_bounds__(HY_THREADS) void canny_hysteresis_kernel(const uint8_t *cls, uint8_t *edges, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) uint8_t hy_lds[];
    const int S = hy_stride(W), t = threadIdx.x, n = H * W;
    const uint8_t *c = cls + (size_t)blockIdx.x * n;
    uint8_t *e = edges + (size_t)blockIdx.x * n;
    uint32_t *z = reinterpret_cast<uint32_t *>(hy_lds);
    for (int i = t; i < (H + 2) * (S >> 2); i += HY_THREADS) z[i] = 0;
    __syncthreads();
    for (int idx = t; idx < n; idx += HY_THREADS) {
        const int y = idx / W, x = idx - y * W;
        const uint8_t v = c[idx];
        hy_lds[(y + 1) * S + 4 + x] = v > 2 ? 2 : v;       // anything above weak counts as strong
    }
    __syncthreads();
    // rows: one thread per row.  Columns: one thread per strip of four pixel columns (a dword per row) and segment of
    // rows, as many segments as fill the block -- a vertical run crosses a segment per round.
    const int nd = (W + 3) >> 2;
    const int nseg = nd < HY_THREADS ? HY_THREADS / nd : 1, seg_rows = (H + nseg - 1) / nseg;
    int again;
    do {
        int changed = 0;
        for (int y = t; y < H; y += HY_THREADS) {
            changed |= hy_sweep<false>(hy_lds, S, (y + 1) * S + 4, 4, nd);
            changed |= hy_sweep<true>(hy_lds, S, (y + 1) * S + 4, 4, nd);
        }
        __syncthreads();
        for (int item = t; item < nd * nseg; item += HY_THREADS) {
            const int seg = item / nd, strip = item - seg * nd;
            const int y0 = seg * seg_rows, rows = min(H, y0 + seg_rows) - y0;
            if (rows <= 0) continue;
            changed |= hy_sweep<false>(hy_lds, S, (y0 + 1) * S + 4 + 4 * strip, S, rows);
            changed |= hy_sweep<true>(hy_lds, S, (y0 + 1) * S + 4 + 4 * strip, S, rows);
        }
        again = __syncthreads_or(changed);
    } while (again);
    for (int idx = t; idx < n; idx += HY_THREADS) {
        const int y = idx / W, x = idx - y * W;
        e[idx] = hy_lds[(y + 1) * S + 4 + x] == 2 ? 255 : 0;
    }
}

int canny_radius(float sigma) {
    if (!(sigma > 0.0f) || !(sigma <= 8.0f)) return -1;
    return (int)(4.0 * (double)sigma + 0.5);
}

bool plane_supported(int H, int W) {
    return H >= 3 && W >= 3 && H <= (1 << 20) && W <= (1 << 20) && (long long)(H + 2) * hy_stride(W) <= (long long)HY_MAX_LDS;
}

int launch_hysteresis(const uint8_t *cls, uint8_t *edges, int B, int H, int W, hipStream_t stream) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(canny_hysteresis_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)HY_MAX_LDS);
        attr_done = true;
    }
    hipLaunchKernelGGL(canny_hysteresis_kernel, dim3(B), dim3(HY_THREADS), hy_lds_bytes(H, W), stream, cls, edges, H, W);
    return mvae_launch_status();
}

}  // namespace

MVAE_EXPORT int mvae_canny_supported(int H, int W, float sigma) {
    const int r = canny_radius(sigma);
    return r >= 0 && r <= CN_MAX_R && plane_supported(H, W) ? 1 : 0;
}

MVAE_EXPORT size_t mvae_canny_ws_bytes(int B, int H, int W) {
    if (B <= 0 || !plane_supported(H, W)) return 0;
    return (size_t)B * H * W;
}

MVAE_EXPORT int mvae_canny(const uint8_t *src, int channels, int B, int H, int W, float sigma, float low, float high,
                           uint8_t *edges, uint8_t *cls, float *mag, void *ws, size_t ws_bytes, mvae_stream_t stream) {
    if (!src || !edges || (channels != 1 && channels != 3) || B <= 0 || !mvae_canny_supported(H, W, sigma) ||
        !(low >= 0.0f) || !(high >= low) || !(high < INFINITY))
        return MVAE_ERR_ARG;
    const int tiles_x = (W + CN_TW - 1) / CN_TW, tiles_y = (H + CN_TH - 1) / CN_TH;
    if ((long long)B * tiles_x * tiles_y >= (1ll << 31) || (long long)B * H * W * 3 >= (1ll << 40)) return MVAE_ERR_ARG;
    if (!cls) {
        if (!ws || ws_bytes < mvae_canny_ws_bytes(B, H, W)) return MVAE_ERR_WS;
        cls = static_cast<uint8_t *>(ws);
    }
    CannyArgs a;
    a.src = src; a.cls = cls; a.mag = mag;
    a.channels = channels; a.H = H; a.W = W; a.r = canny_radius(sigma); a.tiles_x = tiles_x; a.tiles_y = tiles_y;
    a.low = low; a.high = high;
    // w[k] = exp(-k^2 / 2 sigma^2) / sum, in double, handed over as fp32
    double w[2 * CN_MAX_R + 1], sum = 0.0;
    const double s = (double)sigma;
    for (int k = -a.r; k <= a.r; ++k) sum += (w[k + a.r] = exp(-0.5 * (double)(k * k) / (s * s)));
    for (int k = 0; k < 2 * CN_MAX_R + 1; ++k) a.taps[k] = k <= 2 * a.r ? (float)(w[k] / sum) : 0.0f;
    hipLaunchKernelGGL(canny_float_kernel, dim3(B * tiles_x * tiles_y), dim3(CN_THREADS), float_stage_lds_bytes(a.r),
                       (hipStream_t)stream, a);
    if (mvae_launch_status() != MVAE_OK) return MVAE_ERR_LAUNCH;
    return launch_hysteresis(cls, edges, B, H, W, (hipStream_t)stream);
}

MVAE_EXPORT int mvae_canny_hysteresis(const uint8_t *cls, uint8_t *edges, int B, int H, int W, mvae_stream_t stream) {
    if (!cls || !edges || B <= 0 || !plane_supported(H, W)) return MVAE_ERR_ARG;
    return launch_hysteresis(cls, edges, B, H, W, (hipStream_t)stream);
}
