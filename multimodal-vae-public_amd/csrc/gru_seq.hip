// gru_seq.hip -- the whole greedy TextDecoder of the MultiMNIST MVAE (multimnist/model.py:182-228) in one launch per
// direction, instead of ~12 (forward) / ~20 (backward) launches per character step (gru.hip + mvae_linear_*).
//
// Ownership.  The recurrence is independent per batch row: a workgroup owns RB = 16 consecutive rows for ALL L steps of
// both GRU layers, the h2o Linear and the arg-max feedback, and touches no other row of any activation buffer.  There is
// no grid barrier, no flag, no atomic and no cooperative launch: __syncthreads() is the only synchronisation.  Rows
// past B (the last tile) are computed on a clamped copy of row B-1 and never stored.
//
// Products.  Every matrix product is [16 rows] x [16-column tile] on v_mfma_f32_16x16x4_f32 (exact fp32): the A operand
// is the workgroup's activations in LDS (lane l: row l & 15, k = 4 (l >> 4) + q of a 16-wide k chunk, one ds_read_b128),
// the B operand is streamed from the weights in global memory / L2 (each weight element is used once per workgroup and
// step: no LDS staging).  A wave owns whole column tiles; the gate arithmetic is lane-local in the accumulator layout
// (lane l: column l & 15, rows 4 (l >> 4) + 0..3) and uses the sigmoidf_ / tanhf of gru.hip.  r and z accumulate
// x.W_i* + h.W_h* in one accumulator; the n gate keeps gi_n and gh_n apart.
//
// LDS (floats; ld(K) = roundup16(K) + 4 so that a k chunk past K reads zeros and rows are bank-skewed):
//   forward   xcat 16 ld(H+D) | h0 2 x 16 ld(H) (ping-pong) | d0 16 ld(H) | ocat 2 x 16 ld(H+D) (ping-pong) | logits 256
//             | c_in 16                                                    -> 98.6 KiB at (H, D) = (200, 100)
//   backward  dgi 16 ld(3H) | dgh 16 ld(3H) | dbuf 16 (H+D) | carry0, carry1 16 H each | dz 16 D | dlog 16 x 20
//                                                                          -> 127.8 KiB at (200, 100)
// mvae_gru_dec_seq_supported refuses what does not fit the CU's 160 KiB (and n_chars > 16: the logits are one tile).
#include "gru_seq_common.h"      // constants, seq_ld, seq_mma_nt / _nn, seq_cell_fwd, seq_vec

namespace {

struct SeqLdsFwd { int ldx, ldh, xcat, h0, d0, ocat, logits, cin, total; };
__host__ __device__ inline SeqLdsFwd seq_lds_fwd(int H, int D) {
    SeqLdsFwd p;
    p.ldx = seq_ld(H + D); p.ldh = seq_ld(H);
    p.xcat = 0;
    p.h0 = p.xcat + SEQ_RB * p.ldx;
    p.d0 = p.h0 + 2 * SEQ_RB * p.ldh;
    p.ocat = p.d0 + SEQ_RB * p.ldh;
    p.logits = p.ocat + 2 * SEQ_RB * p.ldx;
    p.cin = p.logits + SEQ_RB * 16;
    p.total = p.cin + SEQ_RB;
    return p;
}

struct SeqLdsBwd { int ldg, ldb, dgi, dgh, dbuf, c0, c1, dz, dlog, total; };
__host__ __device__ inline SeqLdsBwd seq_lds_bwd(int H, int D) {
    SeqLdsBwd p;
    p.ldg = seq_ld(3 * H); p.ldb = H + D;
    p.dgi = 0;
    p.dgh = p.dgi + SEQ_RB * p.ldg;
    p.dbuf = p.dgh + SEQ_RB * p.ldg;
    p.c0 = p.dbuf + ((SEQ_RB * p.ldb + 3) & ~3);
    p.c1 = p.c0 + ((SEQ_RB * H + 3) & ~3);
    p.dz = p.c1 + ((SEQ_RB * H + 3) & ~3);
    p.dlog = p.dz + ((SEQ_RB * D + 3) & ~3);
    p.total = p.dlog + SEQ_RB * 20;
    return p;
}

struct SeqFwdArgs {
    const float *z, *hz, *w_emb;
    const float *w_ih0, *w_hh0, *b_ih0, *b_hh0, *w_ih1, *w_hh1, *b_ih1, *b_hh1, *w_h2o, *b_h2o;
    const float *masks;
    float mask_scale;
    float *words, *xcat_all, *h0_all, *h1_all, *d0_all, *ocat_all, *gates0, *gates1;
    int64_t *fed;
    int B, H, D, n_chars, L, sos;
};

// VEC: every weight matrix is 16-byte aligned with a row length that is a multiple of 4 (float4 weight loads)
template <bool VEC>
__global__ __launch_bounds__(SEQ_NT) void gru_dec_seq_fwd_kernel(SeqFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float seq_lds[];
    const int B = a.B, H = a.H, D = a.D, L = a.L, HD = a.H + a.D, NC = a.n_chars;
    const SeqLdsFwd p = seq_lds_fwd(H, D);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * SEQ_RB;
    float *xcat = seq_lds + p.xcat, *h0b = seq_lds + p.h0, *d0 = seq_lds + p.d0, *ocb = seq_lds + p.ocat;
    float *logits = seq_lds + p.logits;
    int *cin = reinterpret_cast<int *>(seq_lds + p.cin);
    const bool tape = a.xcat_all != nullptr;

    for (int i = tid; i < p.total; i += SEQ_NT) seq_lds[i] = 0.f;
    __syncthreads();
    for (int i = tid; i < SEQ_RB * D; i += SEQ_NT) {
        const int row = i / D, d = i - row * D;
        const float v = a.z[(size_t)min(row0 + row, B - 1) * D + d];
        xcat[row * p.ldx + H + d] = v;
        ocb[row * p.ldx + H + d] = v;
        ocb[(SEQ_RB + row) * p.ldx + H + d] = v;
    }
    for (int i = tid; i < SEQ_RB * H; i += SEQ_NT) {
        const int row = i / H, j = i - row * H, grow = row0 + row;
        const float v = a.hz[(size_t)min(grow, B - 1) * H + j];
        h0b[row * p.ldh + j] = v;
        ocb[row * p.ldx + j] = v;
        if (tape && grow < B) {
            a.h0_all[(size_t)grow * H + j] = v;
            a.h1_all[(size_t)grow * H + j] = v;
        }
    }
    if (tid < SEQ_RB) {
        cin[tid] = a.sos;
        if (a.fed && row0 + tid < B) a.fed[row0 + tid] = a.sos;
    }
    __syncthreads();

    SeqCell c0, c1;
    c0.w_ih = a.w_ih0; c0.w_hh = a.w_hh0; c0.b_ih = a.b_ih0; c0.b_hh = a.b_hh0; c0.Kx = HD;
    c1.w_ih = a.w_ih1; c1.w_hh = a.w_hh1; c1.b_ih = a.b_ih1; c1.b_hh = a.b_hh1; c1.Kx = H;

    for (int s = 0; s < L; ++s) {
        const int cur = s & 1, nxt = cur ^ 1;
        const size_t sB = (size_t)s * B;
        // swish(embed(c_in)) | z
        for (int i = tid; i < SEQ_RB * H; i += SEQ_NT) {
            const int row = i / H, j = i - row * H, grow = row0 + row;
            const int ch = min(max(cin[row], 0), NC - 1);
            const float v = swishf_(a.w_emb[(size_t)ch * H + j]);
            xcat[row * p.ldx + j] = v;
            if (tape && grow < B) a.xcat_all[(sB + grow) * HD + j] = v;
        }
        if (tape)
            for (int i = tid; i < SEQ_RB * D; i += SEQ_NT) {
                const int row = i / D, d = i - row * D, grow = row0 + row;
                if (grow < B) {
                    const float v = xcat[row * p.ldx + H + d];
                    a.xcat_all[(sB + grow) * HD + H + d] = v;
                    a.ocat_all[(sB + grow) * HD + H + d] = v;
                }
            }
        __syncthreads();
        seq_cell_fwd<VEC>(c0, xcat, p.ldx, h0b + cur * SEQ_RB * p.ldh, p.ldh, h0b + nxt * SEQ_RB * p.ldh, p.ldh, d0, p.ldh,
                     a.masks ? a.masks + sB * H : nullptr, a.mask_scale, tape ? a.h0_all + (sB + B) * H : nullptr,
                     tape ? a.d0_all + sB * H : nullptr, H, tape ? a.gates0 + sB * 4 * H : nullptr, row0, B, H, wave,
                     lane);
        __syncthreads();
        seq_cell_fwd<VEC>(c1, d0, p.ldh, ocb + cur * SEQ_RB * p.ldx, p.ldx, ocb + nxt * SEQ_RB * p.ldx, p.ldx, nullptr, 0,
                     nullptr, 1.f, tape ? a.h1_all + (sB + B) * H : nullptr, tape ? a.ocat_all + sB * HD : nullptr, HD,
                     tape ? a.gates1 + sB * 4 * H : nullptr, row0, B, H, wave, lane);
        __syncthreads();
        // words[:, s, :] = (h1 | z) . W_h2o^T + b: one column tile
        if (wave == 0) {
            const int c = lane & 15, cc = min(c, NC - 1), kg = lane >> 4;
            const float bv = a.b_h2o[cc];
            seq_f32x4 acc = seq_f32x4{bv, bv, bv, bv};
            const int wrow[1] = {cc};
            seq_mma_nt<1, VEC>(&acc, ocb + nxt * SEQ_RB * p.ldx, p.ldx, a.w_h2o, HD, HD, wrow, lane);
            if (c < NC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 4 * kg + i, grow = row0 + row;
                    logits[row * 16 + c] = acc[i];
                    if (grow < B) a.words[((size_t)grow * L + s) * NC + c] = acc[i];
                }
            }
        }
        __syncthreads();
        // greedy feedback: the first maximum (strict >), as argmax_rows_kernel
        if (tid < SEQ_RB) {
            const float *rowp = logits + tid * 16;
            float best = rowp[0];
            int bi = 0;
            for (int k = 1; k < NC; ++k)
                if (rowp[k] > best) { best = rowp[k]; bi = k; }
            cin[tid] = bi;
            if (a.fed && s + 1 < L && row0 + tid < B) a.fed[(size_t)(s + 1) * B + row0 + tid] = bi;
        }
        __syncthreads();
    }
}

struct SeqBwdArgs {
    const float *dwords, *w_ih0, *w_hh0, *w_ih1, *w_hh1, *w_h2o, *masks;
    float mask_scale;
    const float *h0_all, *h1_all, *gates0, *gates1;
    float *dgi0_all, *dgh0_all, *dgi1_all, *dgh1_all, *demb_all, *dlog_all, *dhz, *dz;
    int B, H, D, n_chars, L;
};

// Backward of one cell's gate arithmetic for the workgroup's rows (gru_cell_bwd_kernel's expressions): dh' = din +
// carry -> dgi, dgh in LDS (A operands of the data-gradient products) and in the time-stacked tapes; carry = dh' * z.
__device__ __forceinline__ void seq_cell_bwd(const float *din, int ldd, float *carry, const float *gates,
                                             const float *h_prev, float *dgi, float *dgh, int ldg, float *dgi_all,
                                             float *dgh_all, int row0, int B, int H, int tid) {
    for (int i = tid; i < SEQ_RB * H; i += SEQ_NT) {
        const int row = i / H, j = i - row * H, grow = row0 + row, growc = min(grow, B - 1);
        const float *g = gates + (size_t)growc * 4 * H;
        const float r = g[j], z = g[H + j], n = g[2 * H + j], ghn = g[3 * H + j];
        const float d = din[row * ldd + j] + carry[row * H + j];
        const float hp = h_prev[(size_t)growc * H + j];
        const float dn_pre = d * (1.0f - z) * (1.0f - n * n);
        const float dz_pre = d * (hp - n) * z * (1.0f - z);
        const float dr_pre = dn_pre * ghn * r * (1.0f - r);
        float *x = dgi + row * ldg, *y = dgh + row * ldg;
        x[j] = dr_pre; x[H + j] = dz_pre; x[2 * H + j] = dn_pre;
        y[j] = dr_pre; y[H + j] = dz_pre; y[2 * H + j] = dn_pre * r;
        if (grow < B) {
            float *u = dgi_all + (size_t)grow * 3 * H, *v = dgh_all + (size_t)grow * 3 * H;
            u[j] = dr_pre; u[H + j] = dz_pre; u[2 * H + j] = dn_pre;
            v[j] = dr_pre; v[H + j] = dz_pre; v[2 * H + j] = dn_pre * r;
        }
        carry[row * H + j] = d * z;
    }
}

__global__ __launch_bounds__(SEQ_NT) void gru_dec_seq_bwd_kernel(SeqBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float seq_lds[];
    const int B = a.B, H = a.H, D = a.D, L = a.L, HD = a.H + a.D, NC = a.n_chars;
    const SeqLdsBwd p = seq_lds_bwd(H, D);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kg = lane >> 4;
    const int row0 = blockIdx.x * SEQ_RB;
    float *dgi = seq_lds + p.dgi, *dgh = seq_lds + p.dgh, *dbuf = seq_lds + p.dbuf;
    float *car0 = seq_lds + p.c0, *car1 = seq_lds + p.c1, *dzs = seq_lds + p.dz, *dlog = seq_lds + p.dlog;
    const int nH = (H + 15) >> 4, nX = (HD + 15) >> 4;

    for (int i = tid; i < p.total; i += SEQ_NT) seq_lds[i] = 0.f;
    __syncthreads();

    for (int s = L - 1; s >= 0; --s) {
        const size_t sB = (size_t)s * B;
        if (tid < SEQ_RB * 16) {
            const int row = tid >> 4, c = tid & 15, grow = row0 + row;
            float v = 0.f;
            if (c < NC) {
                v = a.dwords[((size_t)min(grow, B - 1) * L + s) * NC + c];
                if (grow < B) a.dlog_all[(sB + grow) * NC + c] = v;
            }
            dlog[row * 20 + c] = v;
        }
        __syncthreads();
        // d_ocat = dwords[:, s, :] . W_h2o
        for (int t = wave; t < nX; t += SEQ_NW) {
            seq_f32x4 acc = seq_f32x4{0.f, 0.f, 0.f, 0.f};
            seq_mma_nn(acc, dlog, 20, a.w_h2o, HD, NC, HD, t * 16, lane);
            const int col = t * 16 + (lane & 15);
            if (col < HD) {
#pragma unroll
                for (int i = 0; i < 4; ++i) dbuf[(4 * kg + i) * p.ldb + col] = acc[i];
            }
        }
        __syncthreads();
        for (int i = tid; i < SEQ_RB * D; i += SEQ_NT) {
            const int row = i / D, d = i - row * D;
            dzs[row * D + d] += dbuf[row * p.ldb + H + d];
        }
        seq_cell_bwd(dbuf, p.ldb, car1, a.gates1 + sB * 4 * H, a.h1_all + sB * H, dgi, dgh, p.ldg,
                     a.dgi1_all + sB * 3 * H, a.dgh1_all + sB * 3 * H, row0, B, H, tid);
        __syncthreads();
        // carry1 += dgh1 . W_hh1 ;  dd0 = (dgi1 . W_ih1) * mask / KEEP
        for (int job = wave; job < 2 * nH; job += SEQ_NW) {
            const bool is_carry = job < nH;
            const int t = is_carry ? job : job - nH;
            const int col = t * 16 + (lane & 15);
            seq_f32x4 acc = seq_f32x4{0.f, 0.f, 0.f, 0.f};
            if (is_carry) {
                if (col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = car1[(4 * kg + i) * H + col];
                }
                seq_mma_nn(acc, dgh, p.ldg, a.w_hh1, H, 3 * H, H, t * 16, lane);
                if (col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) car1[(4 * kg + i) * H + col] = acc[i];
                }
            } else {
                seq_mma_nn(acc, dgi, p.ldg, a.w_ih1, H, 3 * H, H, t * 16, lane);
                if (col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = 4 * kg + i;
                        float v = acc[i];
                        if (a.masks) v *= a.masks[(sB + min(row0 + row, B - 1)) * H + col] * a.mask_scale;
                        dbuf[row * p.ldb + col] = v;
                    }
                }
            }
        }
        __syncthreads();
        seq_cell_bwd(dbuf, p.ldb, car0, a.gates0 + sB * 4 * H, a.h0_all + sB * H, dgi, dgh, p.ldg,
                     a.dgi0_all + sB * 3 * H, a.dgh0_all + sB * 3 * H, row0, B, H, tid);
        __syncthreads();
        // carry0 += dgh0 . W_hh0 ;  dxcat = dgi0 . W_ih0 -> demb_all[s] | dz +=
        for (int job = wave; job < nH + nX; job += SEQ_NW) {
            const bool is_carry = job < nH;
            const int t = is_carry ? job : job - nH;
            const int col = t * 16 + (lane & 15);
            seq_f32x4 acc = seq_f32x4{0.f, 0.f, 0.f, 0.f};
            if (is_carry) {
                if (col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = car0[(4 * kg + i) * H + col];
                }
                seq_mma_nn(acc, dgh, p.ldg, a.w_hh0, H, 3 * H, H, t * 16, lane);
                if (col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) car0[(4 * kg + i) * H + col] = acc[i];
                }
            } else {
                seq_mma_nn(acc, dgi, p.ldg, a.w_ih0, HD, 3 * H, HD, t * 16, lane);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 4 * kg + i, grow = row0 + row;
                    if (col < H) {
                        if (grow < B) a.demb_all[(sB + grow) * H + col] = acc[i];
                    } else if (col < HD) {
                        dzs[row * D + col - H] += acc[i];
                    }
                }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < SEQ_RB * H; i += SEQ_NT) {
        const int row = i / H, j = i - row * H, grow = row0 + row;
        if (grow < B) a.dhz[(size_t)grow * H + j] = car0[row * H + j] + car1[row * H + j];
    }
    for (int i = tid; i < SEQ_RB * D; i += SEQ_NT) {
        const int row = i / D, d = i - row * D, grow = row0 + row;
        if (grow < B) a.dz[(size_t)grow * D + d] = dzs[row * D + d];
    }
}

}  // namespace

MVAE_EXPORT int mvae_gru_dec_seq_supported(int B, int H, int D, int n_chars, int L) {
    if (B < 1 || H < 1 || D < 1 || n_chars < 1 || n_chars > 16 || L < 1) return 0;
    if (H > 4096 || D > 4096 || L > 4096) return 0;        // keeps the plan arithmetic below far from int overflow
    // offsets inside one time slice of a tape are 32-bit in the kernels
    if ((size_t)B * 4 * H >= ((size_t)1 << 31) || (size_t)B * (H + D) >= ((size_t)1 << 31)) return 0;
    if ((size_t)seq_lds_fwd(H, D).total * sizeof(float) > SEQ_LDS_MAX) return 0;
    if ((size_t)seq_lds_bwd(H, D).total * sizeof(float) > SEQ_LDS_MAX) return 0;
    return 1;
}

MVAE_EXPORT int mvae_gru_dec_seq_fwd(const float *z, const float *hz, const float *w_emb, const float *w_ih0,
                                     const float *w_hh0, const float *b_ih0, const float *b_hh0, const float *w_ih1,
                                     const float *w_hh1, const float *b_ih1, const float *b_hh1, const float *w_h2o,
                                     const float *b_h2o, const float *masks, float mask_scale, float *words,
                                     float *xcat_all, float *h0_all, float *h1_all, float *d0_all, float *ocat_all,
                                     float *gates0, float *gates1, int64_t *fed, int B, int H, int D, int n_chars,
                                     int L, int sos, mvae_stream_t stream) {
    if (!z || !hz || !w_emb || !w_ih0 || !w_hh0 || !b_ih0 || !b_hh0 || !w_ih1 || !w_hh1 || !b_ih1 || !b_hh1 ||
        !w_h2o || !b_h2o || !words)
        return MVAE_ERR_ARG;
    if (!mvae_gru_dec_seq_supported(B, H, D, n_chars, L)) return MVAE_ERR_ARG;
    const int n_tape = !!xcat_all + !!h0_all + !!h1_all + !!d0_all + !!ocat_all + !!gates0 + !!gates1;
    if (n_tape != 0 && n_tape != 7) return MVAE_ERR_ARG;       // the tape is stored whole or not at all
    SeqFwdArgs a;
    a.z = z; a.hz = hz; a.w_emb = w_emb;
    a.w_ih0 = w_ih0; a.w_hh0 = w_hh0; a.b_ih0 = b_ih0; a.b_hh0 = b_hh0;
    a.w_ih1 = w_ih1; a.w_hh1 = w_hh1; a.b_ih1 = b_ih1; a.b_hh1 = b_hh1; a.w_h2o = w_h2o; a.b_h2o = b_h2o;
    a.masks = masks; a.mask_scale = mask_scale;
    a.words = words; a.xcat_all = xcat_all; a.h0_all = h0_all; a.h1_all = h1_all; a.d0_all = d0_all;
    a.ocat_all = ocat_all; a.gates0 = gates0; a.gates1 = gates1; a.fed = fed;
    a.B = B; a.H = H; a.D = D; a.n_chars = n_chars; a.L = L; a.sos = sos;
    const bool vec = seq_vec(w_ih0, H + D) && seq_vec(w_hh0, H) && seq_vec(w_ih1, H) && seq_vec(w_hh1, H) &&
                     seq_vec(w_h2o, H + D);
    const size_t lds = (size_t)seq_lds_fwd(H, D).total * sizeof(float);
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gru_dec_seq_fwd_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEQ_LDS_MAX);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gru_dec_seq_fwd_kernel<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEQ_LDS_MAX);
        attr_done = true;
    }
    const dim3 grid((B + SEQ_RB - 1) / SEQ_RB);
    if (vec) hipLaunchKernelGGL(gru_dec_seq_fwd_kernel<true>, grid, dim3(SEQ_NT), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gru_dec_seq_fwd_kernel<false>, grid, dim3(SEQ_NT), lds, (hipStream_t)stream, a);
    return mvae_launch_status();
}

MVAE_EXPORT int mvae_gru_dec_seq_bwd(const float *dwords, const float *w_ih0, const float *w_hh0, const float *w_ih1,
                                     const float *w_hh1, const float *w_h2o, const float *masks, float mask_scale,
                                     const float *h0_all, const float *h1_all, const float *gates0,
                                     const float *gates1, float *dgi0_all, float *dgh0_all, float *dgi1_all,
                                     float *dgh1_all, float *demb_all, float *dlog_all, float *dhz, float *dz, int B,
                                     int H, int D, int n_chars, int L, mvae_stream_t stream) {
    if (!dwords || !w_ih0 || !w_hh0 || !w_ih1 || !w_hh1 || !w_h2o || !h0_all || !h1_all || !gates0 || !gates1 ||
        !dgi0_all || !dgh0_all || !dgi1_all || !dgh1_all || !demb_all || !dlog_all || !dhz || !dz)
        return MVAE_ERR_ARG;
    if (!mvae_gru_dec_seq_supported(B, H, D, n_chars, L)) return MVAE_ERR_ARG;
    SeqBwdArgs a;
    a.dwords = dwords; a.w_ih0 = w_ih0; a.w_hh0 = w_hh0; a.w_ih1 = w_ih1; a.w_hh1 = w_hh1; a.w_h2o = w_h2o;
    a.masks = masks; a.mask_scale = mask_scale;
    a.h0_all = h0_all; a.h1_all = h1_all; a.gates0 = gates0; a.gates1 = gates1;
    a.dgi0_all = dgi0_all; a.dgh0_all = dgh0_all; a.dgi1_all = dgi1_all; a.dgh1_all = dgh1_all;
    a.demb_all = demb_all; a.dlog_all = dlog_all; a.dhz = dhz; a.dz = dz;
    a.B = B; a.H = H; a.D = D; a.n_chars = n_chars; a.L = L;
    const size_t lds = (size_t)seq_lds_bwd(H, D).total * sizeof(float);
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gru_dec_seq_bwd_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEQ_LDS_MAX);
        attr_done = true;
    }
    hipLaunchKernelGGL(gru_dec_seq_bwd_kernel, dim3((B + SEQ_RB - 1) / SEQ_RB), dim3(SEQ_NT), lds, (hipStream_t)stream,
                       a);
    return mvae_launch_status();
}
