// poe_table.hip -- the product of experts of C CONDITION ROWS that each pick their own subset of experts, and n
// reparameterised draws from every row, in one launch (K27).
//
// MVAE.infer (celeba19/model.py:63-89) takes None per modality for the WHOLE batch; a batch whose rows condition on
// different subsets -- a sweep over every attribute value, imputing the missing attributes of a data set -- has no launch
// there.  A celeba19 AttributeEncoder reads its {0, 1} input through Embedding(2, 512), so in eval mode expert a has only
// two possible heads: the 2 * A heads of a model are a fixed TABLE [A, 2, 2D], and the posterior of a row is the product
// over the prior, an optional image-encoder row and a per-row selection state[c, a] in {-1 absent, 0, 1} from that table.
// Arithmetic: PoE variant B exactly as poe.hip computes it for celeba19 (prior, image, attributes ascending).
//
// Tiny and latency-bound (C = 37, A = 18, D = 100: 37 x 19 rows of 800 B out of L2).  One wave per (condition, slice of
// PT_DRAWS draws), lanes along the latent dimension.  The wave reads its row of `state` with ONE vector load and turns it
// into two wave-uniform bit masks (present, value); per pass over d it then REQUESTS the image row and every selected
// table row -- up to 2 + 2 * 32 independent loads into registers, the loop is fully unrolled over MVAE_POE_TABLE_MAX_A and
// an absent expert is a uniform skip -- before the first is reduced, so a pass pays one L2 latency, not one per expert.
// Every slice of a condition recomputes the (cheap) posterior in the same fixed order, bit for bit; slice 0 stores it.
// No atomics, no LDS, no scratch.
#include "common.h"
#include "philox.h"

namespace {

constexpr int PT_MAX_A = MVAE_POE_TABLE_MAX_A;
constexpr int PT_DRAWS = 8;         // draws per wave: C = 37, n = 64 is 296 waves, about one per CU
constexpr float PT_EPS = 1e-8f;     // POE_EPS of poe.hip

struct PoeTableArgs {
    const float *table; const signed char *state; const float *img; const int *img_row; const float *eps;
    float *eps_out, *mu, *logvar, *z;
    int A, C, D, n, ld_img, img_rows;
    uint64_t seed; const uint64_t *counter; uint64_t counter_offset;
};

// variant B: 1 / (exp(lv) + eps)
__device__ __forceinline__ float pt_precision(float lv) { return 1.0f / (expf(lv) + PT_EPS); }

__global__ __launch_bounds__(64) void poe_table_draw_kernel(PoeTableArgs a) {
    const int lane = threadIdx.x;
    const int c = blockIdx.x;                         // grid.x == C
    // all 64 lanes are active here: lane i < A holds state[c, i], the others "absent"
    const int sv = lane < a.A ? (int)a.state[(size_t)c * a.A + lane] : -1;
    const uint32_t present = (uint32_t)__ballot(sv == 0 || sv == 1);     // anything else selects nothing
    const uint32_t ones = (uint32_t)__ballot(sv == 1);
    int ir = a.img_row ? a.img_row[c] : -1;
    if (!a.img || ir >= a.img_rows) ir = -1;          // the wrapper refuses these; never read past img_heads
    const float *irow = a.img + (size_t)(ir < 0 ? 0 : ir) * a.ld_img;
    const int k_lo = blockIdx.y * PT_DRAWS, k_hi = min(a.n, k_lo + PT_DRAWS);
    const uint64_t launch = (a.eps || a.n == 0) ? 0 : *a.counter + a.counter_offset;
    const float t0 = pt_precision(0.f);               // the N(0, 1) prior
    for (int d = lane; d < a.D; d += 64) {
        float em[PT_MAX_A], el[PT_MAX_A], im = 0.f, il = 0.f;
        const unsigned ud = (unsigned)d, uD = (unsigned)a.D;
#pragma unroll
        for (int e = 0; e < PT_MAX_A; ++e) {
            em[e] = 0.f; el[e] = 0.f;
            if ((present >> e) & 1u) {                // wave-uniform; 32-bit offsets: the host checks A * 4D < 2^31
                const unsigned ro = ((unsigned)e * 2u + ((ones >> e) & 1u)) * 2u * uD;
                em[e] = a.table[ro + ud]; el[e] = a.table[ro + uD + ud];
            }
        }
        if (ir >= 0) { im = irow[ud]; il = irow[uD + ud]; }
        // the order MVAE.infer stacks the experts in: prior, image, attributes ascending
        float sum_t = t0, sum_mt = 0.f * t0;
        if (ir >= 0) {
            const float te = pt_precision(il);
            sum_mt += im * te;
            sum_t += te;
        }
#pragma unroll
        for (int e = 0; e < PT_MAX_A; ++e) {
            if ((present >> e) & 1u) {
                const float te = pt_precision(el[e]);
                sum_mt += em[e] * te;
                sum_t += te;
            }
        }
        const float pmu = sum_mt / sum_t;
        const float plv = logf(1.0f / sum_t);
        if (blockIdx.y == 0) {
            a.mu[(size_t)c * a.D + d] = pmu;
            a.logvar[(size_t)c * a.D + d] = plv;
        }
        const float sd = expf(0.5f * plv);
        for (int k = k_lo; k < k_hi; ++k) {
            const size_t o = ((size_t)k * a.C + c) * a.D + d;
            const float e = a.eps ? a.eps[o] : philox_normal_at(o, launch, a.seed);
            if (a.eps_out) a.eps_out[o] = e;
            a.z[o] = e * sd + pmu;
        }
    }
}

}  // namespace

MVAE_EXPORT int mvae_poe_table_draw(const float *table, int A, const int8_t *state, const float *img_heads, int ld_img,
                                    int img_rows, const int32_t *img_row, const float *eps, uint64_t seed,
                                    const uint64_t *counter_dev, uint64_t counter_offset, float *eps_out, float *mu,
                                    float *logvar, float *z, int n, int C, int D, mvae_stream_t stream) {
    if (!table || !state || !mu || !logvar || A < 1 || A > PT_MAX_A || C <= 0 || D <= 0 || n < 0) return MVAE_ERR_ARG;
    if (img_heads && (!img_row || img_rows <= 0 || ld_img < 2 * D)) return MVAE_ERR_ARG;
    if (n > 0 && (!z || (!eps && !counter_dev))) return MVAE_ERR_ARG;
    const long long slices = n > 0 ? ((long long)n + PT_DRAWS - 1) / PT_DRAWS : 1;
    if (slices > 65535) return MVAE_ERR_ARG;          // grid.y
    if ((long long)A * 4 * D >= 0x7fffffffLL) return MVAE_ERR_ARG;      // the table is indexed with 32 bits
    PoeTableArgs a{table, (const signed char *)state, img_heads, img_heads ? (const int *)img_row : nullptr, eps,
                   n > 0 ? eps_out : nullptr, mu, logvar, z, A, C, D, n, ld_img, img_heads ? img_rows : 0,
                   seed, counter_dev, counter_offset};
    hipLaunchKernelGGL(poe_table_draw_kernel, dim3((unsigned)C, (unsigned)slices), dim3(64), 0, (hipStream_t)stream, a);
    return mvae_launch_status();
}
