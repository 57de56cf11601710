// loss_ragged.hip -- the reconstruction row sums of loss.hip for COMPACT logits rows that find their target through an
// index (weak supervision: a decoder only sees the rows whose modality is observed, the targets stay in batch order).
//
//   BCE-with-logits row sums   mnist/train.py:47-49,62-74    logits [R, P], target [B, P], rowmap int32 [R]
//   categorical cross-entropy  mnist/train.py:52,77-94       logits [R, K], label int64 [B], rowmap int32 [R]
//
//   row[r] = coef[r] * loss(logits[r, :], target[rowmap[r]])          (coef NULL: 1)
//   dlogits[r, :] = coef[r] * d loss / d logits                       (the forward can emit it in the same pass)
//
// No gathered copy of the targets is made, and a target row no logits row maps to is never read.  A rowmap entry
// outside 0..B-1 (or a label outside 0..K-1, as in loss.hip) makes its row NaN instead of indexing with it.
// Row-sum shape as in loss.hip: a block per row from MVAE_BCE_BLOCK_MIN_P logits on (float4 where P % 4 == 0 and the
// row's operands are 16-byte aligned), a wave per row below; one thread per row of the cross-entropy.
#include "common.h"

namespace {

struct BceIdxArgs {
    const float *logits, *target, *coef;
    const int *rowmap;
    float *rowsum, *dlogits;
    int R, P, B;
};

__global__ __launch_bounds__(256) void bce_idx_block_kernel(BceIdxArgs a) {
    __shared__ float red[16];
    const int r = blockIdx.x;
    const int tr = a.rowmap[r];
    const float *x = a.logits + (size_t)r * a.P;
    float *dx = a.dlogits ? a.dlogits + (size_t)r * a.P : nullptr;
    if (tr < 0 || tr >= a.B) {                         // block-uniform: the whole block leaves before the barriers
        for (int i = threadIdx.x; dx && i < a.P; i += 256) dx[i] = NAN;
        if (threadIdx.x == 0 && a.rowsum) a.rowsum[r] = NAN;
        return;
    }
    const float *t = a.target + (size_t)tr * a.P;
    const float c = a.coef ? a.coef[r] : 1.f;
    float s = 0.f;
    if (a.P % 4 == 0 && aligned16_dev(x) && aligned16_dev(t) && (!dx || aligned16_dev(dx))) {
        const int p4 = a.P / 4;
        for (int i = threadIdx.x; i < p4; i += 256) {
            const float4 xv = reinterpret_cast<const float4 *>(x)[i];
            const float4 tv = reinterpret_cast<const float4 *>(t)[i];
            s += bce_elem(xv.x, tv.x) + bce_elem(xv.y, tv.y) + bce_elem(xv.z, tv.z) + bce_elem(xv.w, tv.w);
            if (dx) {
                float4 gv;
                gv.x = c * bce_grad(xv.x, tv.x);
                gv.y = c * bce_grad(xv.y, tv.y);
                gv.z = c * bce_grad(xv.z, tv.z);
                gv.w = c * bce_grad(xv.w, tv.w);
                reinterpret_cast<float4 *>(dx)[i] = gv;
            }
        }
    } else {
        for (int i = threadIdx.x; i < a.P; i += 256) {
            s += bce_elem(x[i], t[i]);
            if (dx) dx[i] = c * bce_grad(x[i], t[i]);
        }
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0 && a.rowsum) a.rowsum[r] = c * s;
}

__global__ __launch_bounds__(256) void bce_idx_wave_kernel(BceIdxArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int tr = a.rowmap[r];
    const float *x = a.logits + (size_t)r * a.P;
    float *dx = a.dlogits ? a.dlogits + (size_t)r * a.P : nullptr;
    if (tr < 0 || tr >= a.B) {                         // wave-uniform
        for (int i = lane; dx && i < a.P; i += 64) dx[i] = NAN;
        if (lane == 0 && a.rowsum) a.rowsum[r] = NAN;
        return;
    }
    const float *t = a.target + (size_t)tr * a.P;
    const float c = a.coef ? a.coef[r] : 1.f;
    float s = 0.f;
    for (int i = lane; i < a.P; i += 64) {
        s += bce_elem(x[i], t[i]);
        if (dx) dx[i] = c * bce_grad(x[i], t[i]);
    }
    s = wave_sum(s);
    if (lane == 0 && a.rowsum) a.rowsum[r] = c * s;
}

// coef[r] * -log_softmax(x + 1e-6)[label]  and its gradient  coef[r] * (softmax(x + 1e-6) - onehot)
__global__ __launch_bounds__(256) void ce_idx_kernel(const float *logits, const int64_t *label, const int *rowmap,
                                                     const float *coef, float *row, float *dlogits, int R, int K,
                                                     int B) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float *x = logits + (size_t)r * K;
    const int lr = rowmap[r];
    const bool lost = lr < 0 || lr >= B;
    const int64_t yraw = lost ? -1 : label[lr];
    const bool bad = yraw < 0 || yraw >= K;            // must not index the logits row: the row becomes NaN
    const int y = bad ? 0 : (int)yraw;
    const float c = bad ? NAN : (coef ? coef[r] : 1.f);
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, x[k] + 1e-6f);
    float se = 0.f;
    for (int k = 0; k < K; ++k) se += expf(x[k] + 1e-6f - mx);
    const float lse = logf(se) + mx;
    if (row) row[r] = c * -((x[y] + 1e-6f) - lse);
    if (dlogits) {
        for (int k = 0; k < K; ++k) {
            const float p = expf(x[k] + 1e-6f - lse);
            dlogits[(size_t)r * K + k] = c * (p - (k == y ? 1.f : 0.f));
        }
    }
}

int bce_idx_launch(BceIdxArgs a, hipStream_t st) {
    if (!a.logits || !a.target || !a.rowmap || a.R <= 0 || a.P <= 0 || a.B <= 0) return MVAE_ERR_ARG;
    if (!a.rowsum && !a.dlogits) return MVAE_ERR_ARG;
    if (a.P >= MVAE_BCE_BLOCK_MIN_P)
        hipLaunchKernelGGL(bce_idx_block_kernel, dim3(a.R), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(bce_idx_wave_kernel, dim3((a.R + 3) / 4), dim3(256), 0, st, a);
    return mvae_launch_status();
}

}  // namespace

MVAE_EXPORT int mvae_bce_rows_indexed_fwd(const float *logits, const float *target, const int *rowmap_dev,
                                          const float *coef_dev, float *rowsum, float *dlogits, int R, int P, int B,
                                          mvae_stream_t stream) {
    if (!rowsum) return MVAE_ERR_ARG;
    BceIdxArgs a{logits, target, coef_dev, rowmap_dev, rowsum, dlogits, R, P, B};
    return bce_idx_launch(a, (hipStream_t)stream);
}

MVAE_EXPORT int mvae_bce_rows_indexed_bwd(const float *logits, const float *target, const int *rowmap_dev,
                                          const float *drow_dev, float *dlogits, int R, int P, int B,
                                          mvae_stream_t stream) {
    if (!dlogits) return MVAE_ERR_ARG;
    BceIdxArgs a{logits, target, drow_dev, rowmap_dev, nullptr, dlogits, R, P, B};
    return bce_idx_launch(a, (hipStream_t)stream);
}

MVAE_EXPORT int mvae_ce_rows_indexed_fwd(const float *logits, const int64_t *label, const int *rowmap_dev,
                                         const float *coef_dev, float *row, float *dlogits, int R, int K, int B,
                                         mvae_stream_t stream) {
    if (!logits || !label || !rowmap_dev || !row || R <= 0 || K <= 0 || K > 1024 || B <= 0) return MVAE_ERR_ARG;
    hipLaunchKernelGGL(ce_idx_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, logits, label,
                       rowmap_dev, coef_dev, row, dlogits, R, K, B);
    return mvae_launch_status();
}

MVAE_EXPORT int mvae_ce_rows_indexed_bwd(const float *logits, const int64_t *label, const int *rowmap_dev,
                                         const float *drow_dev, float *dlogits, int R, int K, int B,
                                         mvae_stream_t stream) {
    if (!logits || !label || !rowmap_dev || !dlogits || R <= 0 || K <= 0 || K > 1024 || B <= 0) return MVAE_ERR_ARG;
    hipLaunchKernelGGL(ce_idx_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, logits, label,
                       rowmap_dev, drow_dev, (float *)nullptr, dlogits, R, K, B);
    return mvae_launch_status();
}
