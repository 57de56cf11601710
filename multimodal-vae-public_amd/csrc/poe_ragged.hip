// poe_ragged.hip -- the product of experts of poe.hip for a batch whose rows observe DIFFERENT modalities
// (weak supervision: some rows carry an image and a label, some an image alone, some a label alone).
//
// Term t is evaluated on batch row b iff slot[t][b] >= 0; slot[t][b] is then the row of the COMPACT outputs
// mu / logvar / z [R, D] and kl [R] that (t, b) owns.  Expert e's head is compact too -- [n_e, ld], one row per
// batch row that has the modality -- and erow[e][b] is batch row b's row in it (-1: the row does not have expert e).
// An inactive (t, b) is neither computed nor written; an absent expert row is never read.
//
// Same structure as poe.hip: one wave per batch row, lanes along the latent dim, every expert's precision computed
// once per element and reused by the terms that contain it, the KL row sum a wavefront reduction.  The backward writes
// EVERY element of every expert's compact gradient buffer (zero where no active term contains the expert on that row):
// batch row b's wave owns row erow[e][b] of expert e, and erow maps the rows that have e one-to-one onto 0..n_e-1.
// All sums run in a fixed order, nothing is accumulated atomically: two runs give the same bits.
#include "common.h"
#include "philox.h"

namespace {

// the launch shape, the limits and the precision of one expert: poe.hip's, restated (that unit is left untouched)
constexpr int POE_THREADS = 128;   // 2 waves = 2 batch rows per block
constexpr int POE_MAX_TERMS = 40;   // 3 * T * 128 floats of LDS in the backward <= 60 KiB
constexpr float POE_EPS = 1e-8f;

// precision of one expert: 1 / (exp(lv) + eps [+ eps])
__device__ __forceinline__ float poe_precision(float lv, int variant) {
    float var = expf(lv) + POE_EPS;
    if (variant == MVAE_POE_VARIANT_A) var = var + POE_EPS;
    return 1.0f / var;
}

struct RaggedArgs {
    mvae_experts_t ex;
    int n_rows[MVAE_MAX_EXPERTS];      // rows of each expert's compact buffer
    const int *erow;                   // [E, B]
    const int *slot;                   // [T, B]
    const uint32_t *masks;             // [T]
    int ld, E, T, B, D, R, variant, no_prior;
    // draw mode: eps of (t, b, d) is element (t * B + b) * D + d of the Philox stream (seed, *counter + counter_offset) --
    // the DENSE index, so a (term, row)'s draw does not depend on which other rows are present (and equals
    // mvae_poe_fwd_draw's at full presence); it is stored at that dense index for the backward
    uint64_t seed; const uint64_t *counter; uint64_t counter_offset; int draw;
};

// the compact output row of (t, b), or -1; a slot outside 0..R-1 counts as inactive (nothing is written out of bounds)
__device__ __forceinline__ int ragged_slot(const RaggedArgs &a, int t, int b) {
    const int s = a.slot[(size_t)t * a.B + b];
    return (s >= 0 && s < a.R) ? s : -1;
}

// batch row b's row in expert e's compact buffer, or -1; a row outside the buffer counts as absent
__device__ __forceinline__ int ragged_erow(const RaggedArgs &a, int e, int b) {
    const int r = a.erow[(size_t)e * a.B + b];
    return (r >= 0 && r < a.n_rows[e]) ? r : -1;
}

__global__ __launch_bounds__(POE_THREADS) void poe_ragged_fwd_kernel(RaggedArgs a, float *noise, float *mu,
                                                                     float *logvar, float *z, float *kl) {
    extern __shared__ float lds[];                     // [E][2][POE_THREADS] then [T][POE_THREADS]
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (POE_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;                              // whole waves exit together; no block barrier below
    float *mine = lds + threadIdx.x;
    float *klacc = lds + (size_t)a.E * 2 * POE_THREADS + threadIdx.x;
    uint32_t used = 0;                                 // experts an active term of this row contains (wave-uniform)
    bool any = false;
    for (int t = 0; t < a.T; ++t) {
        if (ragged_slot(a, t, b) < 0) continue;
        any = true;
        used |= a.masks[t];
        klacc[t * POE_THREADS] = 0.f;
    }
    if (!any) return;                                  // a row with no active term costs nothing
    const float t0 = a.no_prior ? 0.f : poe_precision(0.f, a.variant);
    const uint64_t launch = a.draw ? *a.counter + a.counter_offset : 0;
    for (int d = lane; d < a.D; d += 64) {
        for (int e = 0; e < a.E; ++e) {
            if (!((used >> e) & 1u)) continue;
            const int er = ragged_erow(a, e, b);       // (an expert the row lacks drops out of the product)
            float te = 0.f, mt = 0.f;
            if (er >= 0) {
                const size_t oe = (size_t)er * a.ld + d;
                te = poe_precision(a.ex.logvar[e][oe], a.variant);
                mt = a.ex.mu[e][oe] * te;
            }
            mine[(e * 2 + 0) * POE_THREADS] = te;
            mine[(e * 2 + 1) * POE_THREADS] = mt;
        }
        for (int t = 0; t < a.T; ++t) {
            const int s = ragged_slot(a, t, b);
            if (s < 0) continue;
            uint32_t mask = a.masks[t];
            float sum_t = t0, sum_mt = 0.f * t0;
            for (int e = 0; mask && e < a.E; ++e, mask >>= 1) {   // the experts of the term, in order
                if (!(mask & 1u)) continue;
                sum_mt += mine[(e * 2 + 1) * POE_THREADS];
                sum_t += mine[(e * 2 + 0) * POE_THREADS];
            }
            const float pmu = sum_mt / sum_t;
            const float pvar = 1.0f / sum_t;
            const float plv = (a.variant == MVAE_POE_VARIANT_A) ? logf(pvar + POE_EPS) : logf(pvar);
            const size_t o = (size_t)s * a.D + d;
            const size_t od = ((size_t)t * a.B + b) * a.D + d;
            mu[o] = pmu;
            logvar[o] = plv;
            if (a.draw) {
                const float eps = philox_normal_at(od, launch, a.seed);
                noise[od] = eps;
                z[o] = eps * expf(0.5f * plv) + pmu;
            } else if (z) {
                z[o] = noise ? noise[od] * expf(0.5f * plv) + pmu : pmu;
            }
            klacc[t * POE_THREADS] += 1.0f + plv - pmu * pmu - expf(plv);
        }
    }
    if (kl) {                                          // all 64 lanes are here again: wave sums per active term
        for (int t = 0; t < a.T; ++t) {
            const int s = ragged_slot(a, t, b);
            if (s < 0) continue;
            const float sum = wave_sum(klacc[t * POE_THREADS]);
            if (lane == 0) kl[s] = -0.5f * sum;
        }
    }
}

// Backward, as in poe.hip.  Phase 1 (per active term of the row): the gradient reaching (mu_t, logvar_t) from z, the KL
// row and direct consumers, folded into A_t = dmu_t / S_t, B_t = dlv_t * dlv/dS and the fused mean, kept in LDS.
// Phase 2 (per expert the row has): T_e and exp(lv_e) once, then a sweep over the active terms that contain the expert.
__global__ __launch_bounds__(POE_THREADS) void poe_ragged_bwd_kernel(RaggedArgs a, const float *noise, const float *mu,
                                                                     const float *logvar, const float *dz,
                                                                     const float *dmu, const float *dlogvar,
                                                                     const float *dkl, mvae_expert_grads_t gr, int ldg) {
    extern __shared__ float lds[];   // [T][3][POE_THREADS]
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (POE_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;            // whole waves exit together; no block barrier is used below
    float *mine = lds + threadIdx.x;
    uint32_t have = 0;               // experts this row owns a gradient row of (wave-uniform)
    for (int e = 0; e < a.E; ++e)
        if (ragged_erow(a, e, b) >= 0) have |= 1u << e;
    if (!have) return;
    for (int d = lane; d < a.D; d += 64) {
        for (int t = 0; t < a.T; ++t) {
            const int s = ragged_slot(a, t, b);
            if (s < 0 || !(a.masks[t] & have)) continue;
            const size_t o = (size_t)s * a.D + d;
            const float pmu = mu[o], plv = logvar[o];
            float gmu = dmu ? dmu[o] : 0.f;
            float glv = dlogvar ? dlogvar[o] : 0.f;
            if (dz) {
                const float g = dz[o];
                gmu += g;
                if (noise) glv += g * noise[((size_t)t * a.B + b) * a.D + d] * 0.5f * expf(0.5f * plv);
            }
            if (dkl) {
                const float ks = dkl[s];
                gmu += ks * pmu;
                glv += ks * (-0.5f) * (1.0f - expf(plv));
            }
            // recover S = sum of precisions from the fused log-variance
            float sp, dlv_ds;
            if (a.variant == MVAE_POE_VARIANT_A) {
                const float v = expf(plv) - POE_EPS;        // 1/S
                sp = 1.0f / v;
                dlv_ds = -(v * v) / (v + POE_EPS);          // d log(1/S + eps) / dS
            } else {
                sp = expf(-plv);
                dlv_ds = -1.0f / sp;
            }
            mine[(t * 3 + 0) * POE_THREADS] = gmu / sp;
            mine[(t * 3 + 1) * POE_THREADS] = glv * dlv_ds;
            mine[(t * 3 + 2) * POE_THREADS] = pmu;
        }
        for (int e = 0; e < a.E; ++e) {
            if (!((have >> e) & 1u)) continue;
            const int er = ragged_erow(a, e, b);
            const size_t oe = (size_t)er * a.ld + d;
            const float me = a.ex.mu[e][oe], lve = a.ex.logvar[e][oe];
            const float ex = expf(lve);
            const float te = poe_precision(lve, a.variant);
            float gm = 0.f, gt = 0.f;
            bool any = false;
            for (int t = 0; t < a.T; ++t) {
                if (!((a.masks[t] >> e) & 1u) || ragged_slot(a, t, b) < 0) continue;
                any = true;
                const float at = mine[(t * 3 + 0) * POE_THREADS];
                gm += at * te;
                gt += at * (me - mine[(t * 3 + 2) * POE_THREADS]) + mine[(t * 3 + 1) * POE_THREADS];
            }
            const size_t og = (size_t)er * ldg + d;
            gr.dmu[e][og] = any ? gm : 0.f;
            gr.dlogvar[e][og] = any ? gt * (-(te * te) * ex) : 0.f;
        }
    }
}

// fills the launch arguments; false where the shapes or pointers cannot be launched
bool ragged_args(RaggedArgs *a, const mvae_experts_t *ex, int ld, int E, const int *n_rows, const int *erow_dev,
                 const uint32_t *masks_dev, int T, const int *slot_dev, int R, int B, int D, int variant) {
    if (!ex || !n_rows || !erow_dev || !masks_dev || !slot_dev || E < 1 || E > MVAE_MAX_EXPERTS || T <= 0 ||
        T > POE_MAX_TERMS || B <= 0 || D <= 0 || ld < D || R < 0)
        return false;
    const int base = variant & ~MVAE_POE_NO_PRIOR;
    if (base != MVAE_POE_VARIANT_A && base != MVAE_POE_VARIANT_B) return false;
    for (int e = 0; e < MVAE_MAX_EXPERTS; ++e) {
        a->ex.mu[e] = nullptr; a->ex.logvar[e] = nullptr; a->n_rows[e] = 0;
    }
    for (int e = 0; e < E; ++e) {
        if (n_rows[e] < 0 || n_rows[e] > B) return false;
        if (n_rows[e] > 0 && (!ex->mu[e] || !ex->logvar[e])) return false;   // an expert no row has may be null
        a->ex.mu[e] = ex->mu[e]; a->ex.logvar[e] = ex->logvar[e]; a->n_rows[e] = n_rows[e];
    }
    a->erow = erow_dev; a->slot = slot_dev; a->masks = masks_dev;
    a->ld = ld; a->E = E; a->T = T; a->B = B; a->D = D; a->R = R;
    a->variant = base; a->no_prior = (variant & MVAE_POE_NO_PRIOR) ? 1 : 0;
    a->seed = 0; a->counter = nullptr; a->counter_offset = 0; a->draw = 0;
    return true;
}

}  // namespace

MVAE_EXPORT int mvae_poe_ragged_fwd(const mvae_experts_t *experts, int ld, int E, const int *n_rows,
                                    const int *erow_dev, const uint32_t *masks_dev, int T, const int *slot_dev, int R,
                                    float *noise, int draw, uint64_t seed, const uint64_t *counter_dev,
                                    uint64_t counter_offset, float *mu, float *logvar, float *z, float *kl, int B,
                                    int D, int variant, mvae_stream_t stream) {
    RaggedArgs a;
    if (!ragged_args(&a, experts, ld, E, n_rows, erow_dev, masks_dev, T, slot_dev, R, B, D, variant) || !mu || !logvar)
        return MVAE_ERR_ARG;
    if (draw && (!noise || !z || !counter_dev)) return MVAE_ERR_ARG;
    if (R == 0) return MVAE_OK;                        // no (term, row) is active: nothing to write
    a.draw = draw ? 1 : 0; a.seed = seed; a.counter = counter_dev; a.counter_offset = counter_offset;
    const int rows = POE_THREADS / 64;
    const size_t lds_bytes = ((size_t)E * 2 + T) * POE_THREADS * sizeof(float);
    hipLaunchKernelGGL(poe_ragged_fwd_kernel, dim3((B + rows - 1) / rows), dim3(POE_THREADS), lds_bytes,
                       (hipStream_t)stream, a, noise, mu, logvar, z, kl);
    return mvae_launch_status();
}

MVAE_EXPORT int mvae_poe_ragged_bwd(const mvae_experts_t *experts, int ld, int E, const int *n_rows,
                                    const int *erow_dev, const uint32_t *masks_dev, int T, const int *slot_dev, int R,
                                    const float *noise, const float *mu, const float *logvar, const float *dz,
                                    const float *dmu, const float *dlogvar, const float *dkl,
                                    const mvae_expert_grads_t *grads, int ldg, int B, int D, int variant,
                                    mvae_stream_t stream) {
    RaggedArgs a;
    if (!ragged_args(&a, experts, ld, E, n_rows, erow_dev, masks_dev, T, slot_dev, R, B, D, variant) || !grads ||
        ldg < D)
        return MVAE_ERR_ARG;
    if (R > 0 && (!mu || !logvar)) return MVAE_ERR_ARG;
    bool any_rows = false;
    for (int e = 0; e < E; ++e) {
        if (n_rows[e] > 0 && (!grads->dmu[e] || !grads->dlogvar[e])) return MVAE_ERR_ARG;
        any_rows |= n_rows[e] > 0;
    }
    if (!any_rows) return MVAE_OK;                     // no gradient row exists
    const int rows = POE_THREADS / 64;
    const size_t lds_bytes = (size_t)T * 3 * POE_THREADS * sizeof(float);
    hipLaunchKernelGGL(poe_ragged_bwd_kernel, dim3((B + rows - 1) / rows), dim3(POE_THREADS), lds_bytes,
                       (hipStream_t)stream, a, noise, mu, logvar, dz, dmu, dlogvar, dkl, *grads, ldg);
    return mvae_launch_status();
}
