// iw_fold.h -- the streaming log-mean-exp fold of the importance-weighted estimators, once: one wave merges the Kc
// log-weights of a chunk into a running (maximum, sum) state and, on the last chunk, writes logsumexp - log K.
// iw_accumulate_kernel (loglike.hip), iw_fold_multi_kernel (loglike_multi.hip) and iw_fold_rows_kernel (loglike_heads.hip)
// differ only in how a sample's log-weight is formed.  predict.hip shares wave_max alone: its merge carries in double.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// Called by every lane of a wave.  logw(k): the log-weight of the chunk's sample k, k = 0 .. Kc - 1, read twice; the lanes
// go along k.  st: the (maximum, sum) pair of the wave's state; out: where lane 0 stores the estimate when finish_k > 0
// (finish_k = K, the number of samples folded in with this chunk included).  Wave reductions in a fixed order.
template <typename LogW>
__device__ __forceinline__ void iw_fold_wave(LogW logw, int Kc, float *st, float *out, int finish_k) {
    const int lane = threadIdx.x & 63;
    float m = -INFINITY;
    for (int k = lane; k < Kc; k += 64) m = fmaxf(m, logw(k));
    m = wave_max(m);
    const float m_old = st[0], s_old = st[1];
    const float m_new = fmaxf(m_old, m);
    float s = 0.f;
    // a maximum of -inf (an empty state, or a chunk of -inf weights) carries no mass: never form -inf - (-inf)
    if (m_new != -INFINITY)
        for (int k = lane; k < Kc; k += 64) s += expf(logw(k) - m_new);
    s = wave_sum(s);
    if (m_old != -INFINITY) s += s_old * expf(m_old - m_new);
    if (lane == 0) {
        st[0] = m_new;
        st[1] = s;
        if (finish_k > 0) *out = m_new + logf(s) - logf((float)finish_k);
    }
}

}  // namespace
