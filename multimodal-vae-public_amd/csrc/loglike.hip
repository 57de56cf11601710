// loglike.hip -- the two element kernels of the importance-weighted marginal log-likelihood
//     L[b] = logsumexp_k( log p(x_b | z_kb) + log p(z_kb) - log q(z_kb | x_b) ) - log K,   z_kb ~ q(z | x_b),
// the number the reference's README promises from a `loglike.py` ("to compute the marginal log likelihood log p(x) using
// q(z|x,y) as the inference network") that was never published.  The decoders and the loss-row
// kernels (loss.hip) run on the K*B rows these two launches sit around:
//   iw_draw_kernel        z[k, b, :] = mu[b, :] + exp(0.5 logvar[b, :]) * eps[k, b, :]  and the density-ratio row
//                         lw[k, b] = sum_d 0.5 eps^2 - 0.5 z^2 + 0.5 logvar   (= log p(z) - log q(z | x); the 2 pi cancel)
//   iw_accumulate_kernel  the streaming log-mean-exp (iw_fold.h) over k of lw[k, b] - (reconstruction rows of sample (k, b)).
// Both are HBM- / latency-bound element work: one wave per row, lanes along the reduced index, wave reductions in a
// fixed order (deterministic, no atomics, no LDS).
#include "iw_fold.h"
#include "philox.h"

namespace {

constexpr int IW_THREADS = 256;    // 4 waves = 4 rows per block

struct IwDrawArgs {
    const float *mu, *logvar, *eps;
    float *eps_out, *z, *lw;
    int ld, R, B, D;                // R = Kc * B rows, row r belongs to datum r % B
    uint64_t seed; const uint64_t *counter; uint64_t counter_offset;
};

// Idx: uint32_t while Kc * B * D fits, size_t beyond
template <typename Idx>
__global__ __launch_bounds__(IW_THREADS) void iw_draw_kernel(IwDrawArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (IW_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= a.R) return;                              // whole waves exit together; no block barrier below
    const int b = r % a.B;
    const float *mu = a.mu + (size_t)b * a.ld, *lv = a.logvar + (size_t)b * a.ld;
    const Idx row = (Idx)r * (Idx)a.D;
    const uint64_t launch = a.eps ? 0 : *a.counter + a.counter_offset;
    float acc = 0.f;
    for (int d = lane; d < a.D; d += 64) {
        const Idx o = row + (Idx)d;
        const float e = a.eps ? a.eps[o] : philox_normal_at((size_t)o, launch, a.seed);
        const float l = lv[d];
        const float zv = e * expf(0.5f * l) + mu[d];
        if (a.eps_out) a.eps_out[o] = e;
        a.z[o] = zv;
        acc += 0.5f * (e * e - zv * zv + l);
    }
    acc = wave_sum(acc);
    if (lane == 0) a.lw[r] = acc;
}

struct IwAccArgs {
    const float *lw, *rec_a, *rec_b;
    float *state, *out;
    int rows_a, rows_b, Kc, B, finish_k;
};

// log-weight of sample (k, b): the density ratio minus the sample's reconstruction rows (loss rows are -log p)
__device__ __forceinline__ float iw_logw(const IwAccArgs &a, int k, int b) {
    const size_t s = (size_t)k * a.B + b;
    float v = a.lw[s];
    if (a.rec_a)
        for (int j = 0; j < a.rows_a; ++j) v -= a.rec_a[s * a.rows_a + j];
    if (a.rec_b)
        for (int j = 0; j < a.rows_b; ++j) v -= a.rec_b[s * a.rows_b + j];
    return v;
}

__global__ __launch_bounds__(IW_THREADS) void iw_accumulate_kernel(IwAccArgs a) {
    const int b = blockIdx.x * (IW_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;                              // whole waves exit together; no block barrier below
    iw_fold_wave([&](int k) { return iw_logw(a, k, b); }, a.Kc, a.state + 2 * b, a.out + b, a.finish_k);
}

}  // namespace

MVAE_EXPORT int mvae_iw_draw(const float *mu, const float *logvar, int ld, const float *eps, uint64_t seed,
                             const uint64_t *counter_dev, uint64_t counter_offset, float *eps_out, float *z, float *lw,
                             int Kc, int B, int D, mvae_stream_t stream) {
    if (Kc <= 0 || B <= 0 || D <= 0 || ld < D || !mu || !logvar || !z || !lw) return MVAE_ERR_ARG;
    if (!eps && !counter_dev) return MVAE_ERR_ARG;
    const long long rows = (long long)Kc * B;
    if (rows > 0x7fffffffLL - IW_THREADS) return MVAE_ERR_ARG;
    IwDrawArgs a{mu, logvar, eps, eps_out, z, lw, ld, (int)rows, B, D, seed, counter_dev, counter_offset};
    const dim3 grid((unsigned)((rows + IW_THREADS / 64 - 1) / (IW_THREADS / 64)));
    if (rows * D < 0x7fffffffLL)
        hipLaunchKernelGGL(iw_draw_kernel<uint32_t>, grid, dim3(IW_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(iw_draw_kernel<size_t>, grid, dim3(IW_THREADS), 0, (hipStream_t)stream, a);
    return mvae_launch_status();
}

MVAE_EXPORT int mvae_iw_accumulate(const float *lw, const float *rec_a, int rows_a, const float *rec_b, int rows_b,
                                   float *state, float *out, int Kc, int B, int finish_k, mvae_stream_t stream) {
    if (Kc <= 0 || B <= 0 || finish_k < 0 || !lw || !state) return MVAE_ERR_ARG;
    if ((rec_a && rows_a <= 0) || (rec_b && rows_b <= 0) || (finish_k > 0 && !out)) return MVAE_ERR_ARG;
    if ((long long)Kc * B > 0x7fffffffLL) return MVAE_ERR_ARG;
    IwAccArgs a{lw, rec_a, rec_b, state, out, rows_a, rows_b, Kc, B, finish_k};
    hipLaunchKernelGGL(iw_accumulate_kernel, dim3((B + IW_THREADS / 64 - 1) / (IW_THREADS / 64)), dim3(IW_THREADS), 0,
                       (hipStream_t)stream, a);
    return mvae_launch_status();
}
