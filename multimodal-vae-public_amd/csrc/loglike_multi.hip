// loglike_multi.hip -- K24: the importance-weighted estimates of SEVERAL image modalities from one decoder pass.
//
// The vision MVAE has six image decoders; its evaluation wants, for the same datum and the same K draws, the six marginals
// log p(x_m) and the joint log p(x_1..x_6).  With segment s = the logits [R, P_s] of decoder s on the R = Kc * B
// sample-major rows of mvae_iw_draw (row r = k * B + b reads target row r % B):
//     rec_s[k, b]  = sum_p bce(logits_s[k * B + b, p], target_s[b, p])                    (bce_elem of common.h, K11)
//     logw_s[k, b] = lw[k, b] - rec_s[k, b]                        s = 0 .. S-1           (the marginals)
//     logw_S[k, b] = lw[k, b] - (rec_0 + rec_1 + ... + rec_{S-1})  added in segment order (the joint)
//     state[j, b]  = online log-sum-exp merge of logw_j[:, b]      j = 0 .. S
// Two launches:
//   iw_score_multi_kernel   the plan of loss_multi.hip: a row's elements, all segments together, are cut into chunks of
//                           CHUNK and every (row, chunk) is a block, so the grid follows the bytes.  A block leaves ONE
//                           unweighted partial in scratch.  HBM-bound: it reads every logit once.
//   iw_fold_multi_kernel    one wave per (state, datum), lanes along k.  A lane adds its sample's partials per segment in
//                           index order -- the per-segment row sums live in registers only, there is no [S, R] array --
//                           forms its state's log-weight and the wave merges it into the state with iw_fold_wave
//                           (iw_fold.h), the fold of iw_accumulate_kernel (loglike.hip).  (One wave per datum carrying all S + 1 states in
//                           registers computes the same bits; at B = 8, S = 6 it measured 0.001 - 0.004 ms behind at
//                           Kc = 128 and 256 and level at 512, profiles/vision_loglike.txt, and was not kept.)
// No atomics, fixed reduction orders: the same inputs give the same bits.
#include "iw_fold.h"

namespace {

constexpr int CHUNK = 4096;             // elements per block: 256 threads x U float4 groups, as in loss_multi.hip
constexpr int U = 4;
constexpr int FOLD_THREADS = 256;       // 4 waves per block

struct ScoreArgs {
    mvae_bce_seg seg[MVAE_BCE_MULTI_MAX];
    int first_chunk[MVAE_BCE_MULTI_MAX + 1];    // chunk index (within a row) at which segment s starts; [n] = chunks per row
    int n;
    float *partial;                             // [R, chunks per row]
    int B;                                      // target rows: row r reads target row r % B
};

__global__ __launch_bounds__(256) void iw_score_multi_kernel(ScoreArgs a) {
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
    const float *t = sg.target + (size_t)(r % a.B) * P;
    float acc = 0.f;
    // row bases are 16-byte aligned whenever the matrices are and P % 4 == 0; lo is a multiple of CHUNK
    if ((P % 4 == 0) && aligned16_dev(sg.logits) && aligned16_dev(sg.target)) {
        const float4 *x4 = reinterpret_cast<const float4 *>(x + lo);
        const float4 *t4 = reinterpret_cast<const float4 *>(t + lo);
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
            for (int u = 0; u < U; ++u)
                acc += bce_elem(xv[u].x, tv[u].x) + bce_elem(xv[u].y, tv[u].y) + bce_elem(xv[u].z, tv[u].z) +
                       bce_elem(xv[u].w, tv[u].w);
        } else {
            for (int i = threadIdx.x; i < n4; i += 256) {      // the last chunk of a segment
                const float4 xv = x4[i], tv = t4[i];
                acc += bce_elem(xv.x, tv.x) + bce_elem(xv.y, tv.y) + bce_elem(xv.z, tv.z) + bce_elem(xv.w, tv.w);
            }
        }
    } else {
        for (int i = lo + threadIdx.x; i < lo + len; i += 256) acc += bce_elem(x[i], t[i]);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) a.partial[(size_t)r * cpr + c] = acc;
}

struct FoldArgs {
    int first_chunk[MVAE_BCE_MULTI_MAX + 1];
    int n;
    const float *partial, *lw;
    float *state, *out;                         // [n + 1, B, 2], [n + 1, B]
    int Kc, B, finish_k;
};

// reconstruction term of segment s for the sample whose partials start at p: its chunks added in index order
__device__ __forceinline__ float seg_rec(const FoldArgs &a, const float *p, int s) {
    float rec = 0.f;
    for (int i = a.first_chunk[s]; i < a.first_chunk[s + 1]; ++i) rec += p[i];
    return rec;
}

// The log-weight of sample (k, b) for state j: a marginal takes its own segment, the joint (j == n) all of them in segment
// order.  One segment's term passes through the same 0 + rec, so with n == 1 the two states hold the same bits.
__device__ __forceinline__ float fold_logw(const FoldArgs &a, int k, int b, int j) {
    const size_t r = (size_t)k * a.B + b;
    const float *p = a.partial + r * a.first_chunk[a.n];
    const int s0 = j < a.n ? j : 0, s1 = j < a.n ? j + 1 : a.n;
    float tot = 0.f;
    for (int s = s0; s < s1; ++s) tot += seg_rec(a, p, s);
    return a.lw[r] - tot;
}

__global__ __launch_bounds__(FOLD_THREADS) void iw_fold_multi_kernel(FoldArgs a) {
    // (n + 1) * B can pass 2^31 while Kc * B and R * chunks-per-row do not
    const long long w = (long long)blockIdx.x * (FOLD_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= (long long)(a.n + 1) * a.B) return;            // whole waves exit together; no block barrier below
    const int j = (int)(w / a.B), b = (int)(w - (long long)j * a.B);
    // state [n + 1, B, 2], out [n + 1, B]: w = j * B + b
    iw_fold_wave([&](int k) { return fold_logw(a, k, b, j); }, a.Kc, a.state + 2 * (size_t)w, a.out + w, a.finish_k);
}

// argument checks of the table and the chunk plan; *cpr_out = chunks per row (0 on a table the launch refuses)
int score_setup(const mvae_bce_seg *segs, int n_segs, long long R, ScoreArgs *sa, FoldArgs *fa, long long *cpr_out) {
    *cpr_out = 0;
    if (!segs || n_segs < 1 || n_segs > MVAE_BCE_MULTI_MAX || R <= 0 || R > 0x7fffffffLL) return MVAE_ERR_ARG;
    long long cpr = 0;
    for (int s = 0; s < n_segs; ++s) {
        if (!segs[s].logits || !segs[s].target || segs[s].P <= 0) return MVAE_ERR_ARG;
        if (sa) {
            sa->seg[s] = segs[s];
            sa->first_chunk[s] = fa->first_chunk[s] = (int)cpr;
        }
        cpr += ((long long)segs[s].P + CHUNK - 1) / CHUNK;
    }
    if (cpr * R > 0x7fffffffLL) return MVAE_ERR_ARG;            // one block per (row, chunk)
    if (sa) {
        for (int s = n_segs; s <= MVAE_BCE_MULTI_MAX; ++s) sa->first_chunk[s] = fa->first_chunk[s] = (int)cpr;
        sa->n = fa->n = n_segs;
    }
    *cpr_out = cpr;
    return MVAE_OK;
}

}  // namespace

MVAE_EXPORT size_t mvae_iw_score_multi_ws_bytes(const mvae_bce_seg *segs, int n_segs, int R) {
    long long cpr;
    if (score_setup(segs, n_segs, R, nullptr, nullptr, &cpr)) return 0;
    return (size_t)R * (size_t)cpr * sizeof(float);
}

MVAE_EXPORT int mvae_iw_score_multi(const mvae_bce_seg *segs, int n_segs, const float *lw, float *state, float *out,
                                    int Kc, int B, int finish_k, void *ws, size_t ws_bytes, mvae_stream_t stream) {
    if (Kc <= 0 || B <= 0 || finish_k < 0 || !lw || !state || (finish_k > 0 && !out)) return MVAE_ERR_ARG;
    const long long R = (long long)Kc * B;
    ScoreArgs sa;
    FoldArgs fa;
    long long cpr;
    if (int rc = score_setup(segs, n_segs, R, &sa, &fa, &cpr)) return rc;
    if (ws_bytes < (size_t)R * (size_t)cpr * sizeof(float)) return MVAE_ERR_WS;
    if (!ws) return MVAE_ERR_ARG;
    sa.partial = (float *)ws;
    sa.B = B;
    fa.partial = (const float *)ws;
    fa.lw = lw;
    fa.state = state;
    fa.out = out;
    fa.Kc = Kc;
    fa.B = B;
    fa.finish_k = finish_k;
    hipLaunchKernelGGL(iw_score_multi_kernel, dim3((unsigned)(cpr * R)), dim3(256), 0, (hipStream_t)stream, sa);
    const long long waves = (long long)(n_segs + 1) * B;       // one per (state, datum)
    const dim3 grid((unsigned)((waves + FOLD_THREADS / 64 - 1) / (FOLD_THREADS / 64)));
    hipLaunchKernelGGL(iw_fold_multi_kernel, grid, dim3(FOLD_THREADS), 0, (hipStream_t)stream, fa);
    return mvae_launch_status();
}
