// loss_multi.hip -- K22: the BCE-with-logits row sums of SEVERAL image modalities in one launch (HBM-bound).
//
//   vision/train.py:20-58,61-73   BCE = sum over the six modalities of sum_p bce(recon, target); ELBO = mean(BCE / 6 + ...)
//   vision/train.py:183-288       seven ELBO terms per step: 7 x 6 = 42 such row sums at a batch of 50
//
// mvae_bce_rowsum_fwd (loss.hip) runs one block per row of ONE logits matrix: 42 launches of 50 blocks on 256 CUs, and
// the adds between them.  Here a row's elements -- all segments together, 49,152 for the vision step -- are cut into
// chunks of CHUNK elements and every (row, chunk) is a block of its own, so the grid follows the bytes, not R.  A block
// writes ONE weighted partial sum to scratch; a second small launch adds a row's partials in index order.  No atomics:
// the same inputs give the same bits.
#include "common.h"

namespace {

constexpr int CHUNK = 4096;             // elements per block: 256 threads x U float4 groups, U = 4 (loss.hip:39-67)
constexpr int U = 4;

struct MultiArgs {
    mvae_bce_seg seg[MVAE_BCE_MULTI_MAX];
    int first_chunk[MVAE_BCE_MULTI_MAX + 1];    // chunk index (within a row) at which segment s starts; [n] = chunks per row
    int n;
    const float *drow;
    float *partial;                             // [R, chunks per row] or NULL: gradient only
    int R, rows_per_group, target_rows;
};

__global__ __launch_bounds__(256) void bce_multi_kernel(MultiArgs a) {
    __shared__ float red[16];
    const int cpr = a.first_chunk[a.n];
    const int r = blockIdx.x / cpr, c = blockIdx.x - r * cpr;
    int s = 0;
    while (s + 1 < a.n && c >= a.first_chunk[s + 1]) ++s;
    const mvae_bce_seg &sg = a.seg[s];
    const int P = sg.P;
    const int lo = (c - a.first_chunk[s]) * CHUNK;             // first element of this block's chunk; lo < P
    const int len = min(CHUNK, P - lo);
    const float *x = sg.logits + (size_t)r * P;
    const float *t = sg.target + (size_t)(r % a.target_rows) * P;
    float *dx = (sg.dlogits && a.drow) ? sg.dlogits + (size_t)r * P : nullptr;
    if (!dx && !a.partial) return;                             // gradient-only launch, segment without a gradient
    const float dw = dx ? a.drow[r / a.rows_per_group] * sg.weight : 0.f;
    float acc = 0.f;
    // row bases are 16-byte aligned whenever the matrices are and P % 4 == 0; lo is a multiple of CHUNK
    const bool vec = (P % 4 == 0) && aligned16_dev(sg.logits) && aligned16_dev(sg.target) &&
                     (!sg.dlogits || aligned16_dev(sg.dlogits));
    if (vec) {
        const float4 *x4 = reinterpret_cast<const float4 *>(x + lo);
        const float4 *t4 = reinterpret_cast<const float4 *>(t + lo);
        float4 *d4 = reinterpret_cast<float4 *>(dx ? dx + lo : nullptr);
        const int n4 = len / 4;
        if (n4 == CHUNK / 4) {
            // a full chunk: the U groups of a thread are all requested before the first is used
            float4 xv[U], tv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                xv[u] = x4[threadIdx.x + 256 * u];
                tv[u] = t4[threadIdx.x + 256 * u];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                acc += bce_elem(xv[u].x, tv[u].x) + bce_elem(xv[u].y, tv[u].y) + bce_elem(xv[u].z, tv[u].z) +
                       bce_elem(xv[u].w, tv[u].w);
                if (dx) {
                    float4 gv;
                    gv.x = dw * bce_grad(xv[u].x, tv[u].x);
                    gv.y = dw * bce_grad(xv[u].y, tv[u].y);
                    gv.z = dw * bce_grad(xv[u].z, tv[u].z);
                    gv.w = dw * bce_grad(xv[u].w, tv[u].w);
                    d4[threadIdx.x + 256 * u] = gv;
                }
            }
        } else {
            for (int i = threadIdx.x; i < n4; i += 256) {      // the last chunk of a segment
                const float4 xv = x4[i], tv = t4[i];
                acc += bce_elem(xv.x, tv.x) + bce_elem(xv.y, tv.y) + bce_elem(xv.z, tv.z) + bce_elem(xv.w, tv.w);
                if (dx) {
                    float4 gv;
                    gv.x = dw * bce_grad(xv.x, tv.x);
                    gv.y = dw * bce_grad(xv.y, tv.y);
                    gv.z = dw * bce_grad(xv.z, tv.z);
                    gv.w = dw * bce_grad(xv.w, tv.w);
                    d4[i] = gv;
                }
            }
        }
    } else {
        for (int i = lo + threadIdx.x; i < lo + len; i += 256) {
            acc += bce_elem(x[i], t[i]);
            if (dx) dx[i] = dw * bce_grad(x[i], t[i]);
        }
    }
    if (!a.partial) return;                                    // block-uniform
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) a.partial[(size_t)r * cpr + c] = sg.weight * acc;
}

// rowsum[r] = the row's partials added lane-strided in index order, then across the wave: one wave per row
__global__ __launch_bounds__(256) void bce_multi_finish_kernel(const float *partial, float *rowsum, int R, int cpr) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    float s = 0.f;
    for (int i = lane; i < cpr; i += 64) s += partial[(size_t)r * cpr + i];
    s = wave_sum(s);
    if (lane == 0) rowsum[r] = s;
}

// argument checks and the chunk table; *cpr_out = chunks per row (0 on a bad table)
int multi_setup(const mvae_bce_seg *segs, int n_segs, int R, MultiArgs *a, long *cpr_out) {
    *cpr_out = 0;
    if (!segs || n_segs < 1 || n_segs > MVAE_BCE_MULTI_MAX || R <= 0) return MVAE_ERR_ARG;
    long cpr = 0;
    for (int s = 0; s < n_segs; ++s) {
        if (!segs[s].logits || !segs[s].target || segs[s].P <= 0) return MVAE_ERR_ARG;
        if (a) {
            a->seg[s] = segs[s];
            a->first_chunk[s] = (int)cpr;
        }
        cpr += ((long)segs[s].P + CHUNK - 1) / CHUNK;
    }
    if (cpr * (long)R > 0x7fffffffL) return MVAE_ERR_ARG;       // one block per (row, chunk)
    if (a) {
        a->first_chunk[n_segs] = (int)cpr;
        a->n = n_segs;
    }
    *cpr_out = cpr;
    return MVAE_OK;
}

int multi_launch(const mvae_bce_seg *segs, int n_segs, float *rowsum, const float *drow, int R, int rows_per_group,
                 int target_rows, void *ws, size_t ws_bytes, hipStream_t st) {
    MultiArgs a;
    long cpr;
    if (int rc = multi_setup(segs, n_segs, R, &a, &cpr)) return rc;
    if (rows_per_group <= 0 || R % rows_per_group != 0 || target_rows <= 0) return MVAE_ERR_ARG;
    bool any_grad = false;
    for (int s = 0; s < n_segs; ++s) any_grad |= (drow && segs[s].dlogits);
    if (!rowsum && !any_grad) return MVAE_ERR_ARG;
    if (rowsum) {
        if (ws_bytes < (size_t)R * cpr * sizeof(float)) return MVAE_ERR_WS;
        if (!ws) return MVAE_ERR_ARG;
    }
    a.drow = drow;
    a.partial = rowsum ? (float *)ws : nullptr;
    a.R = R;
    a.rows_per_group = rows_per_group;
    a.target_rows = target_rows;
    hipLaunchKernelGGL(bce_multi_kernel, dim3((unsigned)(cpr * R)), dim3(256), 0, st, a);
    if (rowsum)
        hipLaunchKernelGGL(bce_multi_finish_kernel, dim3((R + 3) / 4), dim3(256), 0, st, (const float *)ws, rowsum, R,
                           (int)cpr);
    return mvae_launch_status();
}

}  // namespace

MVAE_EXPORT size_t mvae_bce_multi_ws_bytes(const mvae_bce_seg *segs, int n_segs, int R) {
    long cpr;
    if (multi_setup(segs, n_segs, R, nullptr, &cpr)) return 0;
    return (size_t)R * cpr * sizeof(float);
}

MVAE_EXPORT int mvae_bce_multi_fwd(const mvae_bce_seg *segs, int n_segs, float *rowsum, const float *drow_dev, int R,
                                   int rows_per_group, int target_rows, void *ws, size_t ws_bytes, mvae_stream_t stream) {
    return multi_launch(segs, n_segs, rowsum, drow_dev, R, rows_per_group, target_rows, ws, ws_bytes, (hipStream_t)stream);
}

MVAE_EXPORT int mvae_bce_multi_bwd(const mvae_bce_seg *segs, int n_segs, const float *drow_dev, int R, int rows_per_group,
                                   int target_rows, mvae_stream_t stream) {
    if (!drow_dev) return MVAE_ERR_ARG;
    return multi_launch(segs, n_segs, nullptr, drow_dev, R, rows_per_group, target_rows, nullptr, 0, (hipStream_t)stream);
}
