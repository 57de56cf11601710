// gru_seq_common.h -- what the whole-sequence GRU units (gru_seq.hip: the TextDecoder, gru_enc_seq.hip: the TextEncoder)
// share: the row-tile constants, the LDS leading dimension, the two MFMA product helpers (A from LDS, B streamed from
// the weights in global memory) and the forward cell.  Everything is internal to the including unit (anonymous
// namespace, inlined): the units export only their mvae_* entry points.
//
// Products.  Every matrix product is [16 rows] x [16-column tile] on v_mfma_f32_16x16x4_f32 (exact fp32): the A operand
// is the workgroup's activations in LDS (lane l: row l & 15, k = 4 (l >> 4) + q of a 16-wide k chunk, one ds_read_b128),
// the B operand is streamed from the weights in global memory / L2 (each weight element is used once per workgroup and
// step: no LDS staging).  A wave owns whole column tiles; the gate arithmetic is lane-local in the accumulator layout
// (lane l: column l & 15, rows 4 (l >> 4) + 0..3) and uses the sigmoidf_ / tanhf of gru.hip.
#pragma once
#include "common.h"

namespace {

typedef float seq_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SEQ_RB = 16;              // rows of a workgroup = M of the matrix instruction
constexpr int SEQ_NW = 16;              // waves per workgroup: 13 column tiles at H = 200 -> one tile per wave
constexpr int SEQ_NT = SEQ_NW * 64;
constexpr size_t SEQ_LDS_MAX = 160 * 1024;

// LDS leading dimension of a [16, K] A operand: a k chunk past K reads zeros and rows are bank-skewed
__host__ __device__ inline int seq_ld(int k) { return ((k + 15) & ~15) + 4; }

// acc[g] += A[16, K] . W[wrow[g], 0:K]^T for NG weight rows per lane (one per gate).  A in LDS (zero past K up to the
// next multiple of 16), W row-major [., ldw] in global memory.  VEC: K % 4 == 0 and W 16-byte aligned.
template <int NG, bool VEC>
__device__ __forceinline__ void seq_mma_nt(seq_f32x4 *acc, const float *A, int lda, const float *W, int ldw, int K,
                                           const int *wrow, int lane) {
    const int kg = lane >> 4;
    const float *ap = A + (lane & 15) * lda + 4 * kg;
    const float *wp[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) wp[g] = W + (size_t)wrow[g] * ldw + 4 * kg;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int kk = k0 + 4 * kg;
        const seq_f32x4 a = *reinterpret_cast<const seq_f32x4 *>(ap + k0);
        seq_f32x4 b[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (VEC) {
                b[g] = seq_f32x4{0.f, 0.f, 0.f, 0.f};
                if (kk < K) b[g] = *reinterpret_cast<const seq_f32x4 *>(wp[g] + k0);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) b[g][q] = (kk + q < K) ? wp[g][k0 + q] : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[g][q], acc[g], 0, 0, 0);
    }
}

// acc += A[16, K] . W[0:K, c0 : c0 + 16] for W row-major [K, ldw] with N valid columns (the data-gradient form)
__device__ __forceinline__ void seq_mma_nn(seq_f32x4 &acc, const float *A, int lda, const float *W, int ldw, int K,
                                           int N, int c0, int lane) {
    const int kg = lane >> 4;
    const int col = min(c0 + (lane & 15), N - 1);
    const float *ap = A + (lane & 15) * lda + 4 * kg;
    const float *wp = W + col;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int kk = k0 + 4 * kg;
        const seq_f32x4 a = *reinterpret_cast<const seq_f32x4 *>(ap + k0);
        float b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = (kk + q < K) ? wp[(size_t)(kk + q) * ldw] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[q], acc, 0, 0, 0);
    }
}

// One GRU cell for the workgroup's 16 rows: x in LDS [16, Kx], h_prev in LDS; h' -> LDS `hnext`, (masked) -> LDS `dout`
// and, when taping, to global memory.
struct SeqCell {
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    int Kx;                 // width of x = leading dimension of w_ih
};

template <bool VEC>
__device__ __forceinline__ void seq_cell_fwd(const SeqCell &c, const float *X, int ldx, const float *hprev, int ldhp,
                                             float *hnext, int ldhn, float *dout, int lddo, const float *mask,
                                             float mask_scale, float *t_h, float *t_aux, int ld_aux, float *t_gates,
                                             int row0, int B, int H, int wave, int lane) {
    const int kg = lane >> 4;
    const int ntiles = (H + 15) >> 4;
    for (int t = wave; t < ntiles; t += SEQ_NW) {
        const int j = t * 16 + (lane & 15), jc = min(j, H - 1);
        seq_f32x4 acc[4];           // r | z | gi_n | gh_n
        const float br = c.b_ih[jc] + c.b_hh[jc], bz = c.b_ih[H + jc] + c.b_hh[H + jc];
        const float bn = c.b_ih[2 * H + jc], bh = c.b_hh[2 * H + jc];
        acc[0] = seq_f32x4{br, br, br, br}; acc[1] = seq_f32x4{bz, bz, bz, bz};
        acc[2] = seq_f32x4{bn, bn, bn, bn}; acc[3] = seq_f32x4{bh, bh, bh, bh};
        const int wrow[3] = {jc, H + jc, 2 * H + jc};
        seq_mma_nt<3, VEC>(acc, X, ldx, c.w_ih, c.Kx, c.Kx, wrow, lane);
        { seq_f32x4 s = acc[2]; acc[2] = acc[3]; acc[3] = s; }        // r | z | gh_n for the recurrent product
        seq_mma_nt<3, VEC>(acc, hprev, ldhp, c.w_hh, H, H, wrow, lane);
        { seq_f32x4 s = acc[2]; acc[2] = acc[3]; acc[3] = s; }
        if (j < H) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * kg + i, grow = row0 + row, growc = min(grow, B - 1);
                const float r = sigmoidf_(acc[0][i]);
                const float z = sigmoidf_(acc[1][i]);
                const float ghn = acc[3][i];
                const float n = tanhf(acc[2][i] + r * ghn);
                const float hp = hprev[row * ldhp + j];
                const float hn = (1.0f - z) * n + z * hp;
                float dv = hn;
                // offsets inside one time slice are 32-bit (the entry point checks B * 4H < 2^31): one register each
                if (mask) dv *= mask[(unsigned)(growc * H + j)] * mask_scale;
                hnext[row * ldhn + j] = hn;
                if (dout) dout[row * lddo + j] = dv;
                if (t_h && grow < B) {
                    t_h[(unsigned)(grow * H + j)] = hn;
                    t_aux[(unsigned)(grow * ld_aux + j)] = dv;
                    const unsigned g = (unsigned)(grow * 4 * H + j);
                    t_gates[g] = r; t_gates[g + H] = z; t_gates[g + 2 * H] = n; t_gates[g + 3 * H] = ghn;
                }
            }
        }
    }
}

inline bool seq_vec(const float *w, int K) { return (K % 4) == 0 && aligned16(w); }

}  // namespace
