// gru_enc_seq.hip -- the TextEncoder of the MultiMNIST MVAE (multimnist/model.py:145-181) in one launch per direction:
// the embedding gathers, the L cells of the forward-direction GRU, the ONE cell of the reverse direction that x[-1]
// uses (:177: its state at the last position), the direction sum and the h2p Linear; instead of ~22 (forward) / ~30
// (backward) launches of gru.hip + mvae_linear_*.
//
// Ownership, as gru_seq.hip: a workgroup owns RB = 16 consecutive batch rows for the whole sequence and touches no
// other row of any buffer.  No grid barrier, no flag, no atomic and no cooperative launch: __syncthreads() is the only
// synchronisation.  Rows past B (the last tile) are computed on a clamped copy of row B-1 and never stored.  Character
// indices are clamped to [0, n_chars) before any address is formed, as embedding_fwd_kernel does.
//
// Products: gru_seq_common.h (A from LDS, B streamed from the weights, v_mfma_f32_16x16x4_f32, lane-local gates).
//
// LDS (floats; ld(K) = roundup16(K) + 4):
//   forward   e 16 ld(H) | h 2 x 16 ld(H) (ping-pong) | hb 16 ld(H) (reverse state, then s = h_L + h_b)
//                                                                          -> 53.0 KiB at H = 200, any P
//   backward  dout 16 ld(P) | ds 16 H (then the reverse cell's part of de[L-1]) | carry 16 H | dgi 16 ld(3H)
//             | dgh 16 ld(3H)                  -> 109.8 KiB at (H, P) = (200, 128), 114.8 KiB at (200, 200)
// mvae_gru_enc_seq_supported refuses what does not fit the CU's 160 KiB.
#include "gru_seq_common.h"

namespace {

struct EncLdsFwd { int ldh, e, h, hb, total; };
__host__ __device__ inline EncLdsFwd enc_lds_fwd(int H) {
    EncLdsFwd p;
    p.ldh = seq_ld(H);
    p.e = 0;
    p.h = p.e + SEQ_RB * p.ldh;
    p.hb = p.h + 2 * SEQ_RB * p.ldh;
    p.total = p.hb + SEQ_RB * p.ldh;
    return p;
}

struct EncLdsBwd { int ldp, ldg, dout, ds, carry, dgi, dgh, total; };
__host__ __device__ inline EncLdsBwd enc_lds_bwd(int H, int P) {
    EncLdsBwd p;
    p.ldp = seq_ld(P); p.ldg = seq_ld(3 * H);
    p.dout = 0;
    p.ds = p.dout + SEQ_RB * p.ldp;
    p.carry = p.ds + ((SEQ_RB * H + 3) & ~3);
    p.dgi = p.carry + ((SEQ_RB * H + 3) & ~3);
    p.dgh = p.dgi + SEQ_RB * p.ldg;
    p.total = p.dgh + SEQ_RB * p.ldg;
    return p;
}

struct EncFwdArgs {
    const int64_t *x;
    const float *w_emb, *w_ih, *w_hh, *b_ih, *b_hh, *w_ih_r, *w_hh_r, *b_ih_r, *b_hh_r, *w_h2p, *b_h2p;
    float *out, *e_all, *h_all, *gates, *gates_r, *s;
    int64_t *idx_all;
    int B, H, P, n_chars, L;
};

// e[16, H] = w_emb[clamp(x[row, t])] -> LDS (and the tape)
__device__ __forceinline__ void enc_gather(const EncFwdArgs &a, int t, float *e, int ldh, bool tape, int row0, int tid) {
    const int B = a.B, H = a.H;
    for (int i = tid; i < SEQ_RB * H; i += SEQ_NT) {
        const int row = i / H, j = i - row * H, grow = row0 + row;
        int ch = (int)a.x[(size_t)min(grow, B - 1) * a.L + t];
        ch = min(max(ch, 0), a.n_chars - 1);
        const float v = a.w_emb[(size_t)ch * H + j];
        e[row * ldh + j] = v;
        if (tape && grow < B) {
            a.e_all[((size_t)t * B + grow) * H + j] = v;
            if (j == 0) a.idx_all[(size_t)t * B + grow] = ch;
        }
    }
}

// VEC: every weight matrix is 16-byte aligned with a row length that is a multiple of 4 (float4 weight loads)
template <bool VEC>
__global__ __launch_bounds__(SEQ_NT) void gru_enc_seq_fwd_kernel(EncFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float seq_lds[];
    const int B = a.B, H = a.H, P = a.P, L = a.L;
    const EncLdsFwd p = enc_lds_fwd(H);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * SEQ_RB;
    float *e = seq_lds + p.e, *hb = seq_lds + p.h, *sb = seq_lds + p.hb;
    const bool tape = a.e_all != nullptr;

    for (int i = tid; i < p.total; i += SEQ_NT) seq_lds[i] = 0.f;       // h = 0, the k tails of every A operand
    if (tape)
        for (int i = tid; i < SEQ_RB * H; i += SEQ_NT) {
            const int row = i / H, grow = row0 + row;
            if (grow < B) a.h_all[(size_t)grow * H + (i - row * H)] = 0.f;      // slot 0: h_prev of position 0
        }
    __syncthreads();

    // the reverse direction's single cell, on position L-1 from h = 0 (ping-pong slot 0 still holds the zeros).  Its
    // state goes to `sb` (and, taping, to the s buffer, which the sum below overwrites after the barriers between)
    if (a.w_ih_r) {
        SeqCell cr;
        cr.w_ih = a.w_ih_r; cr.w_hh = a.w_hh_r; cr.b_ih = a.b_ih_r; cr.b_hh = a.b_hh_r; cr.Kx = H;
        enc_gather(a, L - 1, e, p.ldh, false, row0, tid);
        __syncthreads();
        seq_cell_fwd<VEC>(cr, e, p.ldh, hb, p.ldh, sb, p.ldh, nullptr, 0, nullptr, 1.f, tape ? a.s : nullptr,
                          tape ? a.s : nullptr, H, tape ? a.gates_r : nullptr, row0, B, H, wave, lane);
        __syncthreads();
    }

    SeqCell cf;
    cf.w_ih = a.w_ih; cf.w_hh = a.w_hh; cf.b_ih = a.b_ih; cf.b_hh = a.b_hh; cf.Kx = H;
    for (int t = 0; t < L; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        const size_t tB = (size_t)t * B;
        enc_gather(a, t, e, p.ldh, tape, row0, tid);
        __syncthreads();
        float *t_h = tape ? a.h_all + (tB + B) * H : nullptr;          // slot t + 1
        seq_cell_fwd<VEC>(cf, e, p.ldh, hb + cur * SEQ_RB * p.ldh, p.ldh, hb + nxt * SEQ_RB * p.ldh, p.ldh, nullptr, 0,
                          nullptr, 1.f, t_h, t_h, H, tape ? a.gates + tB * 4 * H : nullptr, row0, B, H, wave, lane);
        __syncthreads();
    }

    // s = h_L + h_b
    const float *hl = hb + (L & 1) * SEQ_RB * p.ldh;
    for (int i = tid; i < SEQ_RB * H; i += SEQ_NT) {
        const int row = i / H, j = i - row * H, grow = row0 + row;
        const float v = hl[row * p.ldh + j] + sb[row * p.ldh + j];
        sb[row * p.ldh + j] = v;
        if (tape && grow < B) a.s[(size_t)grow * H + j] = v;
    }
    __syncthreads();
    // out = s . W_h2p^T + b_h2p by 16-column tiles
    const int kg = lane >> 4, nP = (P + 15) >> 4;
    for (int t = wave; t < nP; t += SEQ_NW) {
        const int c = t * 16 + (lane & 15), cc = min(c, P - 1);
        const float bv = a.b_h2p[cc];
        seq_f32x4 acc = seq_f32x4{bv, bv, bv, bv};
        const int wrow[1] = {cc};
        seq_mma_nt<1, VEC>(&acc, sb, p.ldh, a.w_h2p, H, H, wrow, lane);
        if (c < P) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int grow = row0 + 4 * kg + i;
                if (grow < B) a.out[(size_t)grow * P + c] = acc[i];
            }
        }
    }
}

struct EncBwdArgs {
    const float *dout, *w_h2p, *w_ih, *w_hh, *w_ih_r, *h_all, *gates, *gates_r;
    float *dgi_all, *dgh_all, *dgi_r, *dgh_r, *de_all;
    int B, H, P, L;
};

// Backward of one cell's gate arithmetic for the workgroup's rows (gru_cell_bwd_kernel's expressions) on dh' = d[16, H]
// in LDS: dgi (and dgh, where `dgh` is given) -> LDS, the A operands of the data-gradient products; both -> global
// memory; where `carry` is given, carry = dh' * z.  h_prev null: the cell started from h = 0.
__device__ __forceinline__ void enc_cell_bwd(const float *d_in, float *carry, const float *gates, const float *h_prev,
                                             float *dgi, float *dgh, int ldg, float *dgi_g, float *dgh_g, int row0, int B,
                                             int H, int tid) {
    for (int i = tid; i < SEQ_RB * H; i += SEQ_NT) {
        const int row = i / H, j = i - row * H, grow = row0 + row, growc = min(grow, B - 1);
        const float *g = gates + (size_t)growc * 4 * H;
        const float r = g[j], z = g[H + j], n = g[2 * H + j], ghn = g[3 * H + j];
        const float d = d_in[row * H + j];
        const float hp = h_prev ? h_prev[(size_t)growc * H + j] : 0.f;
        const float dn_pre = d * (1.0f - z) * (1.0f - n * n);
        const float dz_pre = d * (hp - n) * z * (1.0f - z);
        const float dr_pre = dn_pre * ghn * r * (1.0f - r);
        float *x = dgi + row * ldg;
        x[j] = dr_pre; x[H + j] = dz_pre; x[2 * H + j] = dn_pre;
        if (dgh) {
            float *y = dgh + row * ldg;
            y[j] = dr_pre; y[H + j] = dz_pre; y[2 * H + j] = dn_pre * r;
        }
        if (grow < B) {
            float *u = dgi_g + (size_t)grow * 3 * H, *v = dgh_g + (size_t)grow * 3 * H;
            u[j] = dr_pre; u[H + j] = dz_pre; u[2 * H + j] = dn_pre;
            v[j] = dr_pre; v[H + j] = dz_pre; v[2 * H + j] = dn_pre * r;
        }
        if (carry) carry[row * H + j] = d * z;
    }
}

__global__ __launch_bounds__(SEQ_NT) void gru_enc_seq_bwd_kernel(EncBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float seq_lds[];
    const int B = a.B, H = a.H, P = a.P, L = a.L;
    const EncLdsBwd p = enc_lds_bwd(H, P);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kg = lane >> 4;
    const int row0 = blockIdx.x * SEQ_RB;
    float *doutL = seq_lds + p.dout, *ds = seq_lds + p.ds, *carry = seq_lds + p.carry;
    float *dgi = seq_lds + p.dgi, *dgh = seq_lds + p.dgh;
    const int nH = (H + 15) >> 4;
    const bool bidir = a.w_ih_r != nullptr;

    for (int i = tid; i < p.total; i += SEQ_NT) seq_lds[i] = 0.f;
    __syncthreads();
    for (int i = tid; i < SEQ_RB * P; i += SEQ_NT) {
        const int row = i / P, c = i - row * P;
        doutL[row * p.ldp + c] = a.dout[(size_t)min(row0 + row, B - 1) * P + c];
    }
    __syncthreads();
    // ds = dout . W_h2p: the gradient of both directions' last state
    for (int t = wave; t < nH; t += SEQ_NW) {
        seq_f32x4 acc = seq_f32x4{0.f, 0.f, 0.f, 0.f};
        seq_mma_nn(acc, doutL, p.ldp, a.w_h2p, H, P, H, t * 16, lane);
        const int col = t * 16 + (lane & 15);
        if (col < H) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ds[(4 * kg + i) * H + col] = acc[i];
                carry[(4 * kg + i) * H + col] = acc[i];
            }
        }
    }
    __syncthreads();
    // the reverse direction's one cell, from ds; its part of de[L-1] = dgi_r . W_ih_r replaces ds in LDS
    if (bidir) {
        enc_cell_bwd(ds, nullptr, a.gates_r, nullptr, dgi, nullptr, p.ldg, a.dgi_r, a.dgh_r, row0, B, H, tid);
        __syncthreads();
        for (int t = wave; t < nH; t += SEQ_NW) {
            seq_f32x4 acc = seq_f32x4{0.f, 0.f, 0.f, 0.f};
            seq_mma_nn(acc, dgi, p.ldg, a.w_ih_r, H, 3 * H, H, t * 16, lane);
            const int col = t * 16 + (lane & 15);
            if (col < H) {
#pragma unroll
                for (int i = 0; i < 4; ++i) ds[(4 * kg + i) * H + col] = acc[i];
            }
        }
        __syncthreads();
    }
    // the forward direction, t = L-1 ... 0: carry holds dh'
    for (int t = L - 1; t >= 0; --t) {
        const size_t tB = (size_t)t * B;
        enc_cell_bwd(carry, carry, a.gates + tB * 4 * H, a.h_all + tB * H, dgi, dgh, p.ldg, a.dgi_all + tB * 3 * H,
                     a.dgh_all + tB * 3 * H, row0, B, H, tid);
        __syncthreads();
        // carry += dgh . W_hh (not at t = 0: nothing precedes h = 0) ;  de[t] = dgi . W_ih (+ the reverse cell's at L-1)
        const int njobs = t > 0 ? 2 * nH : nH;
        for (int job = wave; job < njobs; job += SEQ_NW) {
            const bool is_de = job < nH;
            const int tt = is_de ? job : job - nH;
            const int col = tt * 16 + (lane & 15);
            seq_f32x4 acc = seq_f32x4{0.f, 0.f, 0.f, 0.f};
            if (is_de) {
                if (bidir && t == L - 1 && col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = ds[(4 * kg + i) * H + col];
                }
                seq_mma_nn(acc, dgi, p.ldg, a.w_ih, H, 3 * H, H, tt * 16, lane);
                if (col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int grow = row0 + 4 * kg + i;
                        if (grow < B) a.de_all[(tB + grow) * H + col] = acc[i];
                    }
                }
            } else {
                if (col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = carry[(4 * kg + i) * H + col];
                }
                seq_mma_nn(acc, dgh, p.ldg, a.w_hh, H, 3 * H, H, tt * 16, lane);
                if (col < H) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) carry[(4 * kg + i) * H + col] = acc[i];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

MVAE_EXPORT int mvae_gru_enc_seq_supported(int B, int H, int P, int n_chars, int L, int bidirectional) {
    if (B < 1 || H < 1 || P < 1 || n_chars < 1 || L < 1) return 0;
    if (bidirectional != 0 && bidirectional != 1) return 0;
    if (H > 4096 || P > 4096 || L > 4096) return 0;        // keeps the plan arithmetic below far from int overflow
    // offsets inside one time slice of a tape are 32-bit in the kernels
    if ((size_t)B * 4 * H >= ((size_t)1 << 31)) return 0;
    if ((size_t)enc_lds_fwd(H).total * sizeof(float) > SEQ_LDS_MAX) return 0;
    if ((size_t)enc_lds_bwd(H, P).total * sizeof(float) > SEQ_LDS_MAX) return 0;
    return 1;
}

MVAE_EXPORT int mvae_gru_enc_seq_fwd(const int64_t *x, const float *w_emb, const float *w_ih, const float *w_hh,
                                     const float *b_ih, const float *b_hh, const float *w_ih_r, const float *w_hh_r,
                                     const float *b_ih_r, const float *b_hh_r, const float *w_h2p, const float *b_h2p,
                                     float *out, float *e_all, float *h_all, float *gates, float *gates_r, float *s,
                                     int64_t *idx_all, int B, int H, int P, int n_chars, int L, mvae_stream_t stream) {
    if (!x || !w_emb || !w_ih || !w_hh || !b_ih || !b_hh || !w_h2p || !b_h2p || !out) return MVAE_ERR_ARG;
    const int n_rev = !!w_ih_r + !!w_hh_r + !!b_ih_r + !!b_hh_r;
    if (n_rev != 0 && n_rev != 4) return MVAE_ERR_ARG;         // the reverse direction's parameters: all four or none
    const bool bidir = n_rev == 4;
    if (!mvae_gru_enc_seq_supported(B, H, P, n_chars, L, bidir ? 1 : 0)) return MVAE_ERR_ARG;
    const int n_tape = !!e_all + !!h_all + !!gates + !!s + !!idx_all;
    if (n_tape != 0 && n_tape != 5) return MVAE_ERR_ARG;       // the tape is stored whole or not at all
    if ((gates_r != nullptr) != (bidir && n_tape == 5)) return MVAE_ERR_ARG;
    EncFwdArgs a;
    a.x = x; a.w_emb = w_emb; a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh;
    a.w_ih_r = w_ih_r; a.w_hh_r = w_hh_r; a.b_ih_r = b_ih_r; a.b_hh_r = b_hh_r; a.w_h2p = w_h2p; a.b_h2p = b_h2p;
    a.out = out; a.e_all = e_all; a.h_all = h_all; a.gates = gates; a.gates_r = gates_r; a.s = s; a.idx_all = idx_all;
    a.B = B; a.H = H; a.P = P; a.n_chars = n_chars; a.L = L;
    const bool vec = seq_vec(w_ih, H) && seq_vec(w_hh, H) && seq_vec(w_h2p, H) &&
                     (!bidir || (seq_vec(w_ih_r, H) && seq_vec(w_hh_r, H)));
    const size_t lds = (size_t)enc_lds_fwd(H).total * sizeof(float);
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gru_enc_seq_fwd_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEQ_LDS_MAX);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gru_enc_seq_fwd_kernel<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEQ_LDS_MAX);
        attr_done = true;
    }
    const dim3 grid((B + SEQ_RB - 1) / SEQ_RB);
    if (vec) hipLaunchKernelGGL(gru_enc_seq_fwd_kernel<true>, grid, dim3(SEQ_NT), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gru_enc_seq_fwd_kernel<false>, grid, dim3(SEQ_NT), lds, (hipStream_t)stream, a);
    return mvae_launch_status();
}

MVAE_EXPORT int mvae_gru_enc_seq_bwd(const float *dout, const float *w_h2p, const float *w_ih, const float *w_hh,
                                     const float *w_ih_r, const float *h_all, const float *gates, const float *gates_r,
                                     float *dgi_all, float *dgh_all, float *dgi_r, float *dgh_r, float *de_all, int B,
                                     int H, int P, int n_chars, int L, mvae_stream_t stream) {
    if (!dout || !w_h2p || !w_ih || !w_hh || !h_all || !gates || !dgi_all || !dgh_all || !de_all) return MVAE_ERR_ARG;
    const int n_rev = !!w_ih_r + !!gates_r + !!dgi_r + !!dgh_r;
    if (n_rev != 0 && n_rev != 4) return MVAE_ERR_ARG;         // the reverse direction: all four or none
    if (!mvae_gru_enc_seq_supported(B, H, P, n_chars, L, n_rev == 4 ? 1 : 0)) return MVAE_ERR_ARG;
    EncBwdArgs a;
    a.dout = dout; a.w_h2p = w_h2p; a.w_ih = w_ih; a.w_hh = w_hh; a.w_ih_r = w_ih_r;
    a.h_all = h_all; a.gates = gates; a.gates_r = gates_r;
    a.dgi_all = dgi_all; a.dgh_all = dgh_all; a.dgi_r = dgi_r; a.dgh_r = dgh_r; a.de_all = de_all;
    a.B = B; a.H = H; a.P = P; a.L = L;
    const size_t lds = (size_t)enc_lds_bwd(H, P).total * sizeof(float);
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gru_enc_seq_bwd_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEQ_LDS_MAX);
        attr_done = true;
    }
    hipLaunchKernelGGL(gru_enc_seq_bwd_kernel, dim3((B + SEQ_RB - 1) / SEQ_RB), dim3(SEQ_NT), lds, (hipStream_t)stream,
                       a);
    return mvae_launch_status();
}
