// loglike_heads.hip -- K25: the importance-weighted estimates of MANY one-logit modalities from one decoder pass.
//
// The CelebA-19 MVAE has an image decoder and 18 attribute decoders that end in Linear(512, 1); its evaluation wants, for
// the same datum and the same K draws, the 19 marginals and the joint.  Two launches:
//   heads_bce_rows_kernel   the last layer of G one-logit heads fused with its Bernoulli term.  With h [G, R, H] the
//                           post-Swish output of the third grouped Linear on the R = Kc * B sample-major rows of
//                           mvae_iw_draw:
//                               logit[g, r] = sum_j h[g, r, j] * w[g, j] + bias[g]
//                               rec[g, r]   = bce(logit[g, r], target[r % target_rows, g])   (bce_elem of common.h, K11)
//                           Grid (row blocks, G): a block owns HB_ROWS consecutive rows of one group, a wave HB_RPW of
//                           them, one at a time with the lanes along H.  The group's weight row is loaded once per wave and
//                           its first HB_WREG elements stay in registers; every activation is read exactly once, so the
//                           launch is HBM-bound: the rows of a wave are all requested before the first is reduced.
//   iw_fold_rows_kernel     K24's fold for row sums that already exist: one wave per (state, datum), lanes along k.  State
//                           j < S takes lw - rec[sel[j]], state S takes lw - (rec[sel[0]] + ... + rec[sel[S-1]]) added in
//                           j order, merged with iw_fold_wave (iw_fold.h), the fold of iw_accumulate_kernel (loglike.hip).
// No atomics, no scratch, fixed reduction orders: the same inputs give the same bits, and a row's value depends neither on
// R nor on the grid.
#include <type_traits>
#include "iw_fold.h"

namespace {

constexpr int HB_THREADS = 256;         // 4 waves per block
constexpr int HB_RPW = 4;               // rows per wave, all in flight together
constexpr int HB_ROWS = HB_RPW * (HB_THREADS / 64);
constexpr int HB_WREG = 512;            // elements of the weight row a wave keeps in registers (the workload's H)

__device__ __forceinline__ float dot_acc(float x, float w, float s) { return fmaf(x, w, s); }
__device__ __forceinline__ float dot_acc(float4 x, float4 w, float s) {
    s = fmaf(x.x, w.x, s);
    s = fmaf(x.y, w.y, s);
    s = fmaf(x.z, w.z, s);
    return fmaf(x.w, w.w, s);
}

struct HeadsArgs {
    const float *h, *w, *bias, *target;
    float *rec, *logits_out;
    size_t h_gs, w_gs, b_gs, rec_gs, logits_gs;
    int ldh, ldt, target_rows, R, H;
};

// VEC: float4 loads (H % 4 == 0 and every row base 16-byte aligned), lane l of pass p holds elements 4 * (64 p + l) ..+3;
// otherwise lane l of pass p holds element 64 p + l.  Either way a lane adds its products in ascending order.
// A wave owns HB_RPW consecutive rows: their loads are all requested before the first is reduced.  (8 rows per wave, 8 or
// 16 in batches of 4 or 8: 0.025 - 0.026 ms against 0.024 at the workload's size, level below it; not kept.)
template <bool VEC>
__global__ __launch_bounds__(HB_THREADS) void heads_bce_rows_kernel(HeadsArgs a) {
    constexpr int NREG = VEC ? HB_WREG / 256 : HB_WREG / 64;      // passes whose weights are held in registers
    using T = typename std::conditional<VEC, float4, float>::type;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.y;
    const int row0 = (blockIdx.x * (HB_THREADS / 64) + (threadIdx.x >> 6)) * HB_RPW;
    if (row0 >= a.R) return;                                // whole waves exit together; no block barrier below
    const float *w = a.w + (size_t)g * a.w_gs;
    const float *hg = a.h + (size_t)g * a.h_gs;
    const int n = VEC ? a.H / 4 : a.H;                      // loads per row
    const T *wv = reinterpret_cast<const T *>(w);
    T wr[NREG];
#pragma unroll
    for (int u = 0; u < NREG; ++u) wr[u] = lane + 64 * u < n ? wv[lane + 64 * u] : T{};
    float mine = 0.f;
    T xv[HB_RPW][NREG];
#pragma unroll
    for (int i = 0; i < HB_RPW; ++i) {
        // rows past R repeat the last row: the loads stay in bounds and unconditional, the store below is guarded
        const T *x = reinterpret_cast<const T *>(hg + (size_t)min(row0 + i, a.R - 1) * a.ldh);
#pragma unroll
        for (int u = 0; u < NREG; ++u) xv[i][u] = lane + 64 * u < n ? x[lane + 64 * u] : T{};
    }
#pragma unroll
    for (int i = 0; i < HB_RPW; ++i) {
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < NREG; ++u) s = dot_acc(xv[i][u], wr[u], s);
        if (n > 64 * NREG) {                                // H past WREG: the weights come from the cache
            const T *x = reinterpret_cast<const T *>(hg + (size_t)min(row0 + i, a.R - 1) * a.ldh);
            for (int q = lane + 64 * NREG; q < n; q += 64) s = dot_acc(x[q], wv[q], s);
        }
        // the wave's sums in a fixed shuffle order; lane i keeps row i's
        s = wave_sum(s);
        if (lane == i) mine = s;
    }
    const int r = row0 + lane;
    if (lane < HB_RPW && r < a.R) {
        const float logit = mine + a.bias[(size_t)g * a.b_gs];
        const float t = a.target[(size_t)(r % a.target_rows) * a.ldt + g];
        a.rec[(size_t)g * a.rec_gs + r] = bce_elem(logit, t);
        if (a.logits_out) a.logits_out[(size_t)g * a.logits_gs + r] = logit;
    }
}

constexpr int FOLD_THREADS = 256;       // 4 waves per block

struct FoldRowsArgs {
    int sel[MVAE_IW_FOLD_MAX];
    int S;
    const float *rec, *lw;
    size_t rec_ss;
    float *state, *out;                         // [S + 1, B, 2], [S + 1, B]
    int Kc, B, finish_k;
};

// The log-weight of sample (k, b) for state j: a marginal takes its own row, the joint (j == S) all of them in j order.
// One row's term passes through the same 0 + rec, so with S == 1 the two states hold the same bits.
__device__ __forceinline__ float fold_rows_logw(const FoldRowsArgs &a, int k, int b, int j) {
    const size_t r = (size_t)k * a.B + b;
    const int s0 = j < a.S ? j : 0, s1 = j < a.S ? j + 1 : a.S;
    float tot = 0.f;
    for (int s = s0; s < s1; ++s) tot += a.rec[(size_t)a.sel[s] * a.rec_ss + r];
    return a.lw[r] - tot;
}

__global__ __launch_bounds__(FOLD_THREADS) void iw_fold_rows_kernel(FoldRowsArgs a) {
    const long long w = (long long)blockIdx.x * (FOLD_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= (long long)(a.S + 1) * a.B) return;            // whole waves exit together; no block barrier below
    const int j = (int)(w / a.B), b = (int)(w - (long long)j * a.B);
    // state [S + 1, B, 2], out [S + 1, B]: w = j * B + b
    iw_fold_wave([&](int k) { return fold_rows_logw(a, k, b, j); }, a.Kc, a.state + 2 * (size_t)w, a.out + w, a.finish_k);
}

}  // namespace

MVAE_EXPORT int mvae_heads_bce_rows(const float *h, int ldh, size_t h_gs, const float *w, size_t w_gs, const float *bias,
                                    size_t b_gs, const float *target, int target_rows, int ldt, float *rec, size_t rec_gs,
                                    float *logits_out, size_t logits_gs, int G, int R, int H, mvae_stream_t stream) {
    if (!h || !w || !bias || !target || !rec) return MVAE_ERR_ARG;
    if (G < 1 || G > 4096 || R <= 0 || H <= 0 || target_rows <= 0 || ldh < H || ldt < G) return MVAE_ERR_ARG;
    if ((long long)G * R > 0x7fffffffLL) return MVAE_ERR_ARG;
    HeadsArgs a{h, w, bias, target, rec, logits_out, h_gs, w_gs, b_gs, rec_gs, logits_gs, ldh, ldt, target_rows, R, H};
    // decided once per launch: every row base h + g * h_gs + r * ldh and w + g * w_gs is 16-byte aligned
    const bool vec = H % 4 == 0 && ldh % 4 == 0 && h_gs % 4 == 0 && w_gs % 4 == 0 && aligned16(h) && aligned16(w);
    const dim3 grid((unsigned)((R + HB_ROWS - 1) / HB_ROWS), (unsigned)G);
    if (vec)
        hipLaunchKernelGGL(heads_bce_rows_kernel<true>, grid, dim3(HB_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(heads_bce_rows_kernel<false>, grid, dim3(HB_THREADS), 0, (hipStream_t)stream, a);
    return mvae_launch_status();
}

MVAE_EXPORT int mvae_iw_fold_rows(const float *rec, size_t rec_ss, const int *sel, int S, const float *lw, float *state,
                                  float *out, int Kc, int B, int finish_k, mvae_stream_t stream) {
    if (!rec || !lw || !state || S < 1 || S > MVAE_IW_FOLD_MAX || Kc <= 0 || B <= 0) return MVAE_ERR_ARG;
    if (finish_k < 0 || (finish_k > 0 && !out)) return MVAE_ERR_ARG;
    const long long R = (long long)Kc * B;
    if (R > 0x7fffffffLL || rec_ss < (size_t)R) return MVAE_ERR_ARG;
    FoldRowsArgs a;
    for (int j = 0; j < MVAE_IW_FOLD_MAX; ++j) {
        a.sel[j] = j < S ? (sel ? sel[j] : j) : 0;
        if (a.sel[j] < 0) return MVAE_ERR_ARG;
    }
    a.S = S;
    a.rec = rec;
    a.lw = lw;
    a.rec_ss = rec_ss;
    a.state = state;
    a.out = out;
    a.Kc = Kc;
    a.B = B;
    a.finish_k = finish_k;
    const long long waves = (long long)(S + 1) * B;         // one per (state, datum)
    const dim3 grid((unsigned)((waves + FOLD_THREADS / 64 - 1) / (FOLD_THREADS / 64)));
    hipLaunchKernelGGL(iw_fold_rows_kernel, grid, dim3(FOLD_THREADS), 0, (hipStream_t)stream, a);
    return mvae_launch_status();
}
