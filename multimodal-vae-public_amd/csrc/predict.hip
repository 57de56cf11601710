// predict.hip -- the two element kernels of label prediction (predict.py): the Monte-Carlo posterior predictive
//     logp[b, c] = logsumexp_k log p(y = c | z_kb) - log K,   z_kb ~ q(z | x_b),
// of a categorical head (log_softmax of C logits per row) or of C Bernoulli heads (-softplus(-+l) per logit), and the
// scoring of it against labels.  The label decoders run on the K*B sample-major rows of mvae_iw_draw before these:
//   predict_fold_cat_kernel / predict_fold_bern_kernel   K20's streaming log-mean-exp with one (maximum, sum) state per
//                         (datum, class) instead of one per datum; a categorical row's log-normaliser is computed once.
//   predict_score_kernel  arg-max, -logp of the true class, correct flag and the confusion counts, in one block.
// Element / latency-bound work on a few thousand logits: lanes along k, wave reductions in a fixed order (deterministic,
// no global atomics, no scratch).
#include "iw_fold.h"          // wave_max; the float fold of that header is not this unit's merge (pf_merge below)

namespace {

constexpr int PF_THREADS = 256;                    // 4 waves
constexpr int PF_WAVES = PF_THREADS / 64;
constexpr int PF_TILE = PF_THREADS;                // rows of one datum whose log-normalisers sit in LDS at a time
constexpr int PF_PER_LANE = PF_TILE / 64;          // values of a tile a lane holds for one class
constexpr int PF_CLS_PER_WAVE = (MVAE_PREDICT_MAX_C + PF_WAVES - 1) / PF_WAVES;

struct FoldArgs {
    const float *logits;
    float *state, *out;
    long long rs, cs;                               // element (r, c) at r * rs + c * cs
    int Kc, B, C, finish_k;
};

__device__ __forceinline__ float pf_logit(const FoldArgs &a, int k, int b, int c) {
    return a.logits[((size_t)k * a.B + b) * (size_t)a.rs + (size_t)c * (size_t)a.cs];
}

// K20's merge of a chunk (its sum of exp(v - m_new)) into a running (maximum, sum).  The carry and the add are formed in
// double and rounded once: with chunks of a few samples a datum's sum passes through one merge per chunk, and three fp32
// roundings per merge showed as 1e-6 of a log-probability near -0.7 after 44 chunks.
__device__ __forceinline__ float pf_merge(float chunk_sum, float m_old, float s_old, float m_new) {
    // a maximum of -inf (an empty state) carries no mass: never form -inf - (-inf)
    const double carry = m_old != -INFINITY ? (double)s_old * exp((double)m_old - (double)m_new) : 0.0;
    return (float)((double)chunk_sum + carry);
}

// maximum + log(sum / K): the quotient lies in [1 / K, 1], so nothing of the size of log K is formed and cancelled
__device__ __forceinline__ float pf_finish(float m, float s, int finish_k) {
    return (float)((double)m + log((double)s / (double)finish_k));     // no mass at all: -inf + log 0 = -inf, not NaN
}

// One block per datum b.  Per tile of PF_TILE samples: thread t computes the log-normaliser of row (k0 + t, b) with the
// row's own maximum subtracted; then wave w folds the classes w, w + 4, ... with its lanes along k.
__global__ __launch_bounds__(PF_THREADS) void predict_fold_cat_kernel(FoldArgs a) {
    __shared__ float lse[PF_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    float m_run[PF_CLS_PER_WAVE], s_run[PF_CLS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < PF_CLS_PER_WAVE; ++j) {
        const int c = wave + PF_WAVES * j;
        m_run[j] = -INFINITY; s_run[j] = 0.f;
        if (c < a.C) {
            m_run[j] = a.state[((size_t)b * a.C + c) * 2];
            s_run[j] = a.state[((size_t)b * a.C + c) * 2 + 1];
        }
    }
    for (int k0 = 0; k0 < a.Kc; k0 += PF_TILE) {
        const int kt = k0 + (int)threadIdx.x;
        if (kt < a.Kc) {
            float mx = -INFINITY;
            for (int c = 0; c < a.C; ++c) mx = fmaxf(mx, pf_logit(a, kt, b, c));
            float sum = 0.f;
            if (mx != -INFINITY)
                for (int c = 0; c < a.C; ++c) sum += expf(pf_logit(a, kt, b, c) - mx);
            lse[threadIdx.x] = mx != -INFINITY ? mx + logf(sum) : -INFINITY;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PF_CLS_PER_WAVE; ++j) {
            const int c = wave + PF_WAVES * j;
            if (c < a.C) {                                             // the same for every lane of the wave
                float v[PF_PER_LANE], m = -INFINITY;
#pragma unroll
                for (int i = 0; i < PF_PER_LANE; ++i) {
                    const int t = lane + 64 * i;
                    v[i] = -INFINITY;
                    if (k0 + t < a.Kc) {
                        const float x = pf_logit(a, k0 + t, b, c);
                        if (x != -INFINITY) v[i] = x - lse[t];         // a -inf logit is log 0 whatever the row holds
                    }
                    m = fmaxf(m, v[i]);
                }
                m = wave_max(m);
                const float m_new = fmaxf(m_run[j], m);
                float s = 0.f;
                if (m_new != -INFINITY) {
#pragma unroll
                    for (int i = 0; i < PF_PER_LANE; ++i) s += expf(v[i] - m_new);
                }
                s = pf_merge(wave_sum(s), m_run[j], s_run[j], m_new);
                m_run[j] = m_new; s_run[j] = s;
            }
        }
        __syncthreads();                                               // the next tile overwrites lse
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < PF_CLS_PER_WAVE; ++j) {
            const int c = wave + PF_WAVES * j;
            if (c < a.C) {
                const size_t o = (size_t)b * a.C + c;
                a.state[2 * o] = m_run[j];
                a.state[2 * o + 1] = s_run[j];
                if (a.finish_k > 0) a.out[o] = pf_finish(m_run[j], s_run[j], a.finish_k);
            }
        }
    }
}

// log p(y = 1 | l) = -softplus(-l), log p(y = 0 | l) = -softplus(l); softplus(x) = max(x, 0) + log1p(exp(-|x|))
__device__ __forceinline__ float pf_neg_softplus(float x) { return -(fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)))); }

// One wave per (datum, head): lanes along k, the two classes' states side by side (class 1 first).
__global__ __launch_bounds__(PF_THREADS) void predict_fold_bern_kernel(FoldArgs a) {
    const int lane = threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * PF_WAVES + (threadIdx.x >> 6);
    if (idx >= (long long)a.B * a.C) return;                           // whole waves exit together; no barrier below
    const int b = (int)(idx / a.C), c = (int)(idx % a.C);
    float m1 = -INFINITY, m0 = -INFINITY;
    for (int k = lane; k < a.Kc; k += 64) {
        const float l = pf_logit(a, k, b, c);
        m1 = fmaxf(m1, pf_neg_softplus(-l));
        m0 = fmaxf(m0, pf_neg_softplus(l));
    }
    m1 = wave_max(m1); m0 = wave_max(m0);
    float *st = a.state + (size_t)idx * 4;
    const float m1_old = st[0], s1_old = st[1], m0_old = st[2], s0_old = st[3];
    const float m1_new = fmaxf(m1_old, m1), m0_new = fmaxf(m0_old, m0);
    float s1 = 0.f, s0 = 0.f;
    for (int k = lane; k < a.Kc; k += 64) {
        const float l = pf_logit(a, k, b, c);
        if (m1_new != -INFINITY) s1 += expf(pf_neg_softplus(-l) - m1_new);
        if (m0_new != -INFINITY) s0 += expf(pf_neg_softplus(l) - m0_new);
    }
    s1 = pf_merge(wave_sum(s1), m1_old, s1_old, m1_new);
    s0 = pf_merge(wave_sum(s0), m0_old, s0_old, m0_new);
    if (lane == 0) {
        st[0] = m1_new; st[1] = s1; st[2] = m0_new; st[3] = s0;
        if (a.finish_k > 0) {
            a.out[(size_t)idx * 2] = pf_finish(m1_new, s1, a.finish_k);
            a.out[(size_t)idx * 2 + 1] = pf_finish(m0_new, s0, a.finish_k);
        }
    }
}

struct ScoreArgs {
    const float *logp;
    const void *targets;                            // categorical: int64 [B]; Bernoulli: float [B, C], row stride ldt
    long long *pred;
    float *nll;
    unsigned char *correct;
    long long *confusion;
    int ldt, B, C;
};

constexpr int PS_THREADS = 256;
constexpr int PS_HIST = MVAE_PREDICT_MAX_C * MVAE_PREDICT_MAX_C;      // >= 4 * MVAE_PREDICT_MAX_C

// One block: threads loop over the rows, the counts go to an LDS histogram, the block adds it to the caller's table.
template <int MODE>
__global__ __launch_bounds__(PS_THREADS) void predict_score_kernel(ScoreArgs a) {
    __shared__ int hist[PS_HIST];
    const int cells = MODE == MVAE_PREDICT_CATEGORICAL ? a.C * a.C : a.C * 4;
    if (a.confusion) {
        for (int i = threadIdx.x; i < cells; i += PS_THREADS) hist[i] = 0;
        __syncthreads();
    }
    if (MODE == MVAE_PREDICT_CATEGORICAL) {
        const long long *y_all = (const long long *)a.targets;
        for (int b = threadIdx.x; b < a.B; b += PS_THREADS) {
            const float *row = a.logp + (size_t)b * a.C;
            int best = 0;
            float top = row[0];
            for (int c = 1; c < a.C; ++c)
                if (row[c] > top) { top = row[c]; best = c; }           // strict: the lowest index wins a tie
            a.pred[b] = best;
            if (y_all) {
                const long long y = y_all[b];
                const bool valid = y >= 0 && y < a.C;                   // anything else is counted nowhere
                a.nll[b] = valid ? -row[y] : INFINITY;
                a.correct[b] = valid && y == best;
                if (a.confusion && valid) atomicAdd(&hist[(int)y * a.C + best], 1);
            }
        }
    } else {
        const float *y_all = (const float *)a.targets;
        const long long n = (long long)a.B * a.C;
        for (long long i = threadIdx.x; i < n; i += PS_THREADS) {
            const int b = (int)(i / a.C), c = (int)(i % a.C);
            const float l1 = a.logp[2 * i], l0 = a.logp[2 * i + 1];
            const int best = l1 > l0 ? 1 : 0;
            a.pred[i] = best;
            if (y_all) {
                const float y = y_all[(size_t)b * a.ldt + c];
                const bool valid = y == 0.f || y == 1.f;
                const int yi = y == 1.f ? 1 : 0;
                a.nll[i] = valid ? -(yi ? l1 : l0) : INFINITY;
                a.correct[i] = valid && yi == best;
                if (a.confusion && valid) atomicAdd(&hist[c * 4 + yi * 2 + best], 1);
            }
        }
    }
    if (a.confusion) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += PS_THREADS) a.confusion[i] += hist[i];
    }
}

bool pf_mode_ok(int mode) { return mode == MVAE_PREDICT_CATEGORICAL || mode == MVAE_PREDICT_BERNOULLI; }

}  // namespace

MVAE_EXPORT int mvae_predict_fold(const float *logits, long long row_stride, long long col_stride, int R, int B, int C,
                                  int mode, float *state, float *out, int finish_k, mvae_stream_t stream) {
    if (!logits || !state || !pf_mode_ok(mode)) return MVAE_ERR_ARG;
    if (R <= 0 || B <= 0 || C <= 0 || C > MVAE_PREDICT_MAX_C || R % B != 0) return MVAE_ERR_ARG;
    if (finish_k < 0 || (finish_k > 0 && !out)) return MVAE_ERR_ARG;
    if ((long long)R * C >= 0x80000000LL) return MVAE_ERR_ARG;
    if (row_stride <= 0 || col_stride <= 0) return MVAE_ERR_ARG;
    // no two elements alias: the columns of a row lie inside one row stride, or the rows of a column inside one column
    // stride (an axis of extent 1 asks nothing of the other's stride)
    if (row_stride < (long long)(C - 1) * col_stride + 1 && col_stride < (long long)(R - 1) * row_stride + 1)
        return MVAE_ERR_ARG;
    FoldArgs a{logits, state, out, row_stride, col_stride, R / B, B, C, finish_k};
    if (mode == MVAE_PREDICT_CATEGORICAL) {
        hipLaunchKernelGGL(predict_fold_cat_kernel, dim3((unsigned)B), dim3(PF_THREADS), 0, (hipStream_t)stream, a);
    } else {
        const long long waves = (long long)B * C;
        hipLaunchKernelGGL(predict_fold_bern_kernel, dim3((unsigned)((waves + PF_WAVES - 1) / PF_WAVES)), dim3(PF_THREADS),
                           0, (hipStream_t)stream, a);
    }
    return mvae_launch_status();
}

MVAE_EXPORT int mvae_predict_score(const float *logp, int mode, const void *targets, int target_stride, int B, int C,
                                   int64_t *pred, float *nll, uint8_t *correct, int64_t *confusion,
                                   mvae_stream_t stream) {
    if (!logp || !pred || !pf_mode_ok(mode)) return MVAE_ERR_ARG;
    if (B <= 0 || C <= 0 || C > MVAE_PREDICT_MAX_C) return MVAE_ERR_ARG;
    if ((long long)B * C >= 0x80000000LL) return MVAE_ERR_ARG;
    if (targets ? (!nll || !correct) : (nll || correct || confusion)) return MVAE_ERR_ARG;
    if (targets && mode == MVAE_PREDICT_BERNOULLI && target_stride < C) return MVAE_ERR_ARG;
    ScoreArgs a{logp, targets, (long long *)pred, nll, correct, (long long *)confusion, target_stride, B, C};
    if (mode == MVAE_PREDICT_CATEGORICAL)
        hipLaunchKernelGGL(predict_score_kernel<MVAE_PREDICT_CATEGORICAL>, dim3(1), dim3(PS_THREADS), 0,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(predict_score_kernel<MVAE_PREDICT_BERNOULLI>, dim3(1), dim3(PS_THREADS), 0,
                           (hipStream_t)stream, a);
    return mvae_launch_status();
}
