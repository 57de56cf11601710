// MultiMNIST dataset builder on the GPU: the reference pastes 0-4 resized MNIST digits onto a 50 x 50 canvas and
// rejects canvases whose strokes overlap (multimnist/datasets.py:107-146: imresize -> np.pad -> canvas += ... ->
// np.max(canvas) > 255).  One launch composes M canvases from a digit bank already resident in HBM, following a
// plan the host drew: per canvas n in 0..4 and n records (bank index, w, top, left).
//
// Per digit: Pillow's 8-bit BILINEAR resize 28 x 28 -> w x w -- horizontal pass, uint8 intermediate, vertical pass,
// 22-bit fixed-point coefficients from the host tables of mvae_resample_coeffs(28, w), the arithmetic of
// resize_crop_kernel (preprocess.hip) -- added at rows top.., columns left.. of an integer canvas.  w = 28 is the
// identity (one tap of weight 1 << 22).  Per canvas: flag = any sum > 255, stored byte = min(sum, 255).
//
// One 256-thread block per canvas.  HBM-bound integer work: the <= 4 digits (784 bytes each) are read once as whole
// dwords into LDS, the filter taps read bytes from LDS, the uint8 intermediate and the 2500-entry integer canvas
// stay in LDS (14.5 KiB in all), and only the 2500 bytes go back, packed four to a dword store.  Within one digit
// every output pixel belongs to exactly one thread and digits are separated by barriers: no atomics.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int MM_THREADS = 256;
constexpr int DG = MVAE_MM_DIGIT, CV = MVAE_MM_CANVAS, KS = MVAE_MM_KSIZE;
constexpr int DG_BYTES = DG * DG;                    // 784 = 196 dwords
constexpr int CV_PIXELS = CV * CV;                   // 2500 = 625 dwords
static_assert(DG_BYTES % 4 == 0 && CV_PIXELS % 4 == 0, "whole-dword loads and stores");

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(MM_THREADS) void multimnist_compose_kernel(
        const uint8_t *__restrict__ bank, int n_bank, const int *__restrict__ plan, const int *__restrict__ kk,
        const int *__restrict__ bounds, uint8_t *__restrict__ canvas, int *__restrict__ flags) {
    __shared__ int acc[CV_PIXELS];
    __shared__ __attribute__((aligned(16))) uint8_t digit[MVAE_MM_MAX_DIGITS][DG_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t tmp[DG * CV];          // [28 source rows][w columns]
    const int m = blockIdx.x, t = threadIdx.x;
    const int *rec = plan + (size_t)m * MVAE_MM_PLAN_STRIDE;
    int n = rec[0];
    // the host wrapper validates every plan; a record that would index outside the bank, the tables or the canvas
    // is never followed here either: the canvas comes out empty with flag -1
    bool bad = n < 0 || n > MVAE_MM_MAX_DIGITS;
    if (bad) n = 0;
    for (int d = 0; d < n; ++d) {
        const int ix = rec[1 + 4 * d], w = rec[2 + 4 * d], top = rec[3 + 4 * d], left = rec[4 + 4 * d];
        bad = bad || ix < 0 || ix >= n_bank || w < MVAE_MM_WMIN || w > MVAE_MM_WMAX || top < 0 || left < 0 ||
              top + w > CV || left + w > CV;
    }
    if (bad) n = 0;
    for (int i = t; i < CV_PIXELS; i += MM_THREADS) acc[i] = 0;
    for (int i = t; i < n * (DG_BYTES / 4); i += MM_THREADS) {
        const int d = i / (DG_BYTES / 4), q = i % (DG_BYTES / 4);
        const uint32_t *g4 = reinterpret_cast<const uint32_t *>(bank + (size_t)rec[1 + 4 * d] * DG_BYTES);
        reinterpret_cast<uint32_t *>(digit[d])[q] = g4[q];
    }
    __syncthreads();
    for (int d = 0; d < n; ++d) {
        const int w = rec[2 + 4 * d], top = rec[3 + 4 * d], left = rec[4 + 4 * d];
        const int *kw = kk + (size_t)(w - MVAE_MM_WMIN) * CV * KS;
        const int *bw = bounds + (size_t)(w - MVAE_MM_WMIN) * CV * 2;
        // horizontal pass: tmp[r][j], r < 28, j < w
        for (int idx = t; idx < DG * w; idx += MM_THREADS) {
            const int r = idx / w, j = idx - r * w;
            const int xmin = bw[2 * j], xmax = bw[2 * j + 1];
            const int *k = kw + j * KS;
            const uint8_t *row = digit[d] + r * DG + xmin;
            int a = 1 << (PRECISION_BITS - 1);
            for (int x = 0; x < xmax; ++x) a += (int)row[x] * k[x];
            tmp[r * w + j] = (uint8_t)clip8(a >> PRECISION_BITS);
        }
        __syncthreads();
        // vertical pass, added to the canvas at (top + i, left + j)
        for (int idx = t; idx < w * w; idx += MM_THREADS) {
            const int i = idx / w, j = idx - i * w;
            const int ymin = bw[2 * i], ymax = bw[2 * i + 1];
            const int *k = kw + i * KS;
            const uint8_t *col = tmp + ymin * w + j;
            int a = 1 << (PRECISION_BITS - 1);
            for (int y = 0; y < ymax; ++y) a += (int)col[y * w] * k[y];
            acc[(top + i) * CV + left + j] += clip8(a >> PRECISION_BITS);
        }
        __syncthreads();
    }
    int over = 0;
    uint32_t *out4 = reinterpret_cast<uint32_t *>(canvas + (size_t)m * CV_PIXELS);
    for (int q = t; q < CV_PIXELS / 4; q += MM_THREADS) {
        uint32_t packed = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int v = acc[4 * q + b];
            over |= v > 255;
            packed |= (uint32_t)(v > 255 ? 255 : v) << (8 * b);
        }
        out4[q] = packed;
    }
    over = __syncthreads_or(over);
    if (t == 0) flags[m] = bad ? -1 : (over ? 1 : 0);
}

}  // namespace

MVAE_EXPORT int mvae_multimnist_compose(const uint8_t *bank, int n_bank, const int *plan_dev, int M, const int *kk_dev,
                                        const int *bounds_dev, uint8_t *canvas, int *flags, mvae_stream_t stream) {
    if (!bank || !plan_dev || !kk_dev || !bounds_dev || !canvas || !flags || M <= 0 || n_bank <= 0) return MVAE_ERR_ARG;
    // whole-dword loads of the digits and stores of the canvases: 784 and 2500 are multiples of 4, the bases must be too
    if ((reinterpret_cast<uintptr_t>(bank) & 3u) || (reinterpret_cast<uintptr_t>(canvas) & 3u)) return MVAE_ERR_ARG;
    hipLaunchKernelGGL(multimnist_compose_kernel, dim3(M), dim3(MM_THREADS), 0, (hipStream_t)stream, bank, n_bank,
                       plan_dev, kk_dev, bounds_dev, canvas, flags);
    return mvae_launch_status();
}
