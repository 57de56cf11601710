// conv_gen.hip -- the general stride-2 conv family (K17): Conv2d / ConvTranspose2d with a square 4x4 or 5x5 kernel,
// stride 2, pad 0 or 1, any map size (odd and non-square included), fp32 NCHW, bias=False.  These are the four
// geometries of MultiMNIST's 50 x 50 image stacks that the 4x4 family of conv.hip refuses (odd maps, pad 0, 5x5).
//
// All six launches are implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32).  Three kernels, each used twice:
//   gather, strided form   out[b,r,oh,ow] = sum_{c,kh,kw} W[r][c][kh][kw] * in[b,c,2oh-p+kh,2ow-p+kw]
//                          Conv2d forward (W = w) and ConvTranspose2d data gradient (in = dy, W = w[Cin][Cout]).
//   gather, parity form    out[b,r,oh,ow] = sum_{c, kh = q_h + 2 th, kw = q_w + 2 tw} W[c][r][kh][kw] * in[b,c,(oh+p-kh)/2,(ow+p-kw)/2]
//                          ConvTranspose2d forward and Conv2d data gradient.  The four output parity classes
//                          (q_h, q_w) = ((oh+p) & 1, (ow+p) & 1) are separate GEMMs (grid z) over their OWN taps only --
//                          2x2 for ks = 4; 3x3, 3x2, 2x3, 2x2 for ks = 5 -- on their own lattices, which differ in size
//                          when the map is odd (13x13, 13x12, ... for 25x25).  No structural zero is multiplied.
//                          The weights are read from a class-major copy wr[class][c][tap][r] that a small launch in
//                          front makes in the caller's scratch (in place, a lane would fetch one cache line per tap).
//   wgrad                  dw[r][c][kh][kw] = sum_{b,sh,sw} small[b,r,sh,sw] * big[b,c,2sh-p+kh,2sw-p+kw]
//                          Conv2d (small = dy, big = x) and ConvTranspose2d (small = x, big = dy); the reduction over
//                          the batch is split across grid z into the workspace and summed in a fixed order.
//
// The reduction axis of the gather forms is cut into k-steps of 32 slots = (whole channels) x (taps of the class):
// cpk = 32 / T channels of T taps each, the remaining slots zero on both operands.  A 5x5 strided gather thus spends
// 32 slots on 25 taps (MFMA work x 32/25), the 3x3 class 32 on 27, the 3x2 classes 32 on 30; 4x4 wastes nothing.
// Because a k-step is whole channels, every thread's (channel offset, tap) -- and with it the byte offset of each
// element it fetches -- is a per-thread CONSTANT computed once: the main loop issues raw buffer loads at those offsets
// from a scalar base that the k-step advances, LDS stores, and MFMAs.  An element that must read as zero (a tap outside
// the map, a padded slot, a row or column beyond the matrix) carries an out-of-range offset: the hardware returns 0 and
// touches no memory.  Only the last, partial k-step compares channel numbers.
// The weight gradient's reduction axis is (b, sh, sw); its threads each own one k-slot, decode their position once per
// k-step and derive the offsets of their 8 + 8 elements from it (vector-ALU work in that loop: see DESIGN.md).
#include "common.h"

typedef float gen_f32x16 __attribute__((ext_vector_type(16)));
typedef int gen_i32x4 __attribute__((ext_vector_type(4)));
__device__ float gen_raw_buffer_load_f32(gen_i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.f32");

namespace {

constexpr int GEN_OOB = (int)0x80000000u;       // beyond num_records: the load returns 0
constexpr int GEN_THREADS = 256;
constexpr long GEN_MAX_ELEMS = 1L << 28;        // byte offsets from the tensor's start stay far inside the 31-bit buffer range

// raw buffer (stride 0, 2 GiB - 1 records) at a block-uniform address
__device__ __forceinline__ gen_i32x4 gen_rsrc(const float *p) {
    const unsigned long long a = (unsigned long long)p;
    gen_i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));
    r.z = 0x7fffffff; r.w = 0x00020000;
    return r;
}

struct GenGeo {
    int B, C, R;            // batch, reduction channels (those of the gathered tensor), output rows
    int IH, IW, OH, OW;     // map of the gathered tensor, map of the output
    int ks, pad;
    int parity;             // 0 strided form (one class), 1 parity form (four classes)
    int dgrad;              // epilogue: 0 pre / act = swish(pre); 1 dx = v * swish'(pre_in)
};

// one class of the output lattice: positions oh = oh0 + os * u (u < LH), taps kh = qh + ts * th (th < nh)
struct GenClass { int oh0, ow0, LH, LW, nh, nw, qh, qw, bh, bw, tbase; };   // tbase: taps of the classes in front (repacked weights)

__host__ __device__ inline GenClass gen_class(const GenGeo &g, int cls) {
    GenClass c;
    if (!g.parity) {
        c.oh0 = c.ow0 = 0; c.LH = g.OH; c.LW = g.OW; c.nh = c.nw = g.ks; c.qh = c.qw = 0; c.bh = c.bw = -g.pad; c.tbase = 0;
    } else {
        c.qh = cls >> 1; c.qw = cls & 1;
        c.oh0 = (c.qh + g.pad) & 1; c.ow0 = (c.qw + g.pad) & 1;
        c.LH = g.OH > c.oh0 ? (g.OH - c.oh0 + 1) / 2 : 0;
        c.LW = g.OW > c.ow0 ? (g.OW - c.ow0 + 1) / 2 : 0;
        c.nh = (g.ks - c.qh + 1) / 2; c.nw = (g.ks - c.qw + 1) / 2;
        c.bh = (c.oh0 + g.pad - c.qh) / 2; c.bw = (c.ow0 + g.pad - c.qw) / 2;
        const int n0 = (g.ks + 1) / 2, n1 = g.ks / 2;              // taps per axis of parity 0 / 1
        c.tbase = cls == 0 ? 0 : cls == 1 ? n0 * n0 : cls == 2 ? n0 * g.ks : n0 * g.ks + n1 * n0;
    }
    return c;
}

// the 32 k-slots of wave group `kg` of the staged tile: 16 MFMAs of 32x32x2
template <int PA, int PB>
__device__ __forceinline__ void gen_mma(const float *As, const float *Bs, int kg, int arow, int bcol, int lane, gen_f32x16 &acc) {
    const int kh = lane >> 5, l = lane & 31;
    const float *ap = As + (kg * 32 + kh) * PA + arow + l;
    const float *bp = Bs + (kg * 32 + kh) * PB + bcol + l;
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk * PA], bp[kk * PB], acc, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ gather forms
// WGM x WGN waves of 32 x 32 outputs, KG wave groups along the reduction (each k-step feeds KG * 32 slots); the
// groups' accumulators are summed through LDS in a fixed order before the epilogue.
template <int WGM, int WGN, int KG>
__global__ __launch_bounds__(GEN_THREADS) void conv_gen_gather_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                                      float *__restrict__ o1, float *__restrict__ o2,
                                                                      const float *__restrict__ pre_in, GenGeo g) {
    static_assert(WGM * WGN * KG == 4, "four waves");
    constexpr int TM = 32 * WGM, TN = 32 * WGN, KS = 32 * KG;
    constexpr int PA = TM + 1, PB = TN + 1;
    constexpr int NA = KS * TM / GEN_THREADS, NB = KS * TN / GEN_THREADS;
    constexpr int RED = (KG - 1) * WGM * WGN * 16 * 64;
    // two staging buffers and one barrier per k-step; the four-group layout (128 slots per step) would need 66 KiB
    // that way and takes one buffer and two barriers
    constexpr int NBUF = KG == 4 ? 1 : 2;
    constexpr int LDSF = NBUF * KS * (PA + PB) > RED ? NBUF * KS * (PA + PB) : RED;
    __shared__ float lds[LDSF];
    float *const A0 = lds, *const B0 = lds + NBUF * KS * PA;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const GenClass c = gen_class(g, blockIdx.z);
    const int L = c.LH * c.LW, ncols = g.B * L;
    const int j0 = blockIdx.x * TN, r0 = blockIdx.y * TM;
    if (j0 >= ncols) return;                                   // a smaller class of an odd map: block-uniform
    const int T = c.nh * c.nw, cpk = 32 / T, CPS = KG * cpk;   // taps, channels per 32 slots, channels per k-step
    const int KK = g.ks * g.ks, IHW = g.IH * g.IW;

    int aoff[NA], boff[NB], ach[NA], bch[NB], asto[NA];
#pragma unroll
    for (int e = 0; e < NB; ++e) {
        const int id = t + GEN_THREADS * e, col = id % TN, kslot = id / TN;
        const int sub = kslot & 31, csub = sub / T, tap = sub - csub * T, th = tap / c.nw, tw = tap - th * c.nw;
        const int j = j0 + col, b = j / L, rem = j - b * L, u = rem / c.LW, v = rem - u * c.LW;
        const int ih = g.parity ? c.bh + u - th : 2 * u + c.bh + th;
        const int iw = g.parity ? c.bw + v - tw : 2 * v + c.bw + tw;
        bch[e] = (kslot >> 5) * cpk + csub;
        const bool ok = j < ncols && csub < cpk && (unsigned)ih < (unsigned)g.IH && (unsigned)iw < (unsigned)g.IW;
        boff[e] = ok ? 4 * (((b * g.C + bch[e]) * g.IH + ih) * g.IW + iw) : GEN_OOB;
    }
#pragma unroll
    for (int e = 0; e < NA; ++e) {
        // lanes run along the operand's contiguous axis: the taps of w[r][c][kh][kw] (strided form), the rows of the
        // repacked class-major copy wr[class][c][tap][r] (parity form: a dense [k][r] matrix per class)
        const int id = t + GEN_THREADS * e;
        const int kslot = g.parity ? id / TM : id % KS, row = g.parity ? id % TM : id / KS;
        const int sub = kslot & 31, csub = sub / T, tap = sub - csub * T;
        const int r = r0 + row;
        ach[e] = (kslot >> 5) * cpk + csub;
        asto[e] = kslot * PA + row;
        const bool ok = r < g.R && csub < cpk;
        const int off = g.parity ? (c.tbase * g.C + ach[e] * T + tap) * g.R + r : (r * g.C + ach[e]) * KK + tap;
        aoff[e] = ok ? 4 * off : GEN_OOB;
    }
    const int wstep = g.parity ? T * g.R : KK;                 // floats per channel on the weight's reduction axis

    float ra[NA], rb[NB];
    auto load = [&](int c0, bool tail) {
        const gen_i32x4 rsa = gen_rsrc(w + (size_t)c0 * wstep), rsb = gen_rsrc(in + (size_t)c0 * IHW);
        if (!tail) {
#pragma unroll
            for (int e = 0; e < NA; ++e) ra[e] = gen_raw_buffer_load_f32(rsa, aoff[e], 0, 0);
#pragma unroll
            for (int e = 0; e < NB; ++e) rb[e] = gen_raw_buffer_load_f32(rsb, boff[e], 0, 0);
        } else {                                               // the last, partial k-step: channels beyond C read as zero
#pragma unroll
            for (int e = 0; e < NA; ++e) ra[e] = gen_raw_buffer_load_f32(rsa, c0 + ach[e] < g.C ? aoff[e] : GEN_OOB, 0, 0);
#pragma unroll
            for (int e = 0; e < NB; ++e) rb[e] = gen_raw_buffer_load_f32(rsb, c0 + bch[e] < g.C ? boff[e] : GEN_OOB, 0, 0);
        }
    };
    auto store = [&](float *A, float *Bt) {
#pragma unroll
        for (int e = 0; e < NA; ++e) A[asto[e]] = ra[e];
#pragma unroll
        for (int e = 0; e < NB; ++e) { const int id = t + GEN_THREADS * e; Bt[(id / TN) * PB + id % TN] = rb[e]; }
    };

    const int kg = wave / (WGM * WGN), wm = (wave / WGN) % WGM, wn = wave % WGN;
    gen_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int nsteps = (g.C + CPS - 1) / CPS, nfull = g.C / CPS;
    load(0, nfull == 0);
    for (int s = 0; s < nsteps; ++s) {
        float *const A = A0 + (s & (NBUF - 1)) * KS * PA, *const Bt = B0 + (s & (NBUF - 1)) * KS * PB;
        store(A, Bt);
        __syncthreads();
        if (s + 1 < nsteps) load((s + 1) * CPS, s + 1 >= nfull);
        gen_mma<PA, PB>(A, Bt, kg, wm * 32, wn * 32, lane, acc);
        if (NBUF == 1) __syncthreads();
    }
    if (KG > 1) {                                              // sum the wave groups: group 0 adds 1, 2, ... in order
        __syncthreads();
        float *red = lds;
        if (kg > 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) red[(((kg - 1) * WGM * WGN + wm * WGN + wn) * 16 + i) * 64 + lane] = acc[i];
        }
        __syncthreads();
        if (kg > 0) return;
        for (int q = 1; q < KG; ++q)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += red[(((q - 1) * WGM * WGN + wm * WGN + wn) * 16 + i) * 64 + lane];
    }
    // epilogue: lane = output column (32 consecutive lattice positions), register = output channel
    const int j = j0 + wn * 32 + (lane & 31);
    if (j >= ncols) return;
    const int b = j / L, rem = j - b * L, u = rem / c.LW, v = rem - u * c.LW;
    const int os = g.parity ? 2 : 1, OHW = g.OH * g.OW;
    const size_t colbase = (size_t)b * g.R * OHW + (size_t)(c.oh0 + os * u) * g.OW + (c.ow0 + os * v);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = r0 + wm * 32 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
        if (r >= g.R) continue;
        const size_t a = colbase + (size_t)r * OHW;
        const float val = acc[i];
        if (g.dgrad) {
            o1[a] = pre_in ? val * swish_grad_(pre_in[a]) : val;
        } else {
            if (o1) o1[a] = val;
            if (o2) o2[a] = swishf_(val);
        }
    }
}

// the parity form's weights, class-major: wr[tbase(class) * C * R + (c * T + th * nw + tw) * R + r] = w[c][r][qh + 2 th][qw + 2 tw]
// (Cin * Cout * ks * ks floats, as the weights: every tap belongs to exactly one class)
__global__ __launch_bounds__(256) void conv_gen_repack_kernel(const float *__restrict__ w, float *__restrict__ wr, int C, int R, int ks,
                                                              int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int KK = ks * ks, kw = i % ks, kh = (i / ks) % ks, r = (i / KK) % R, c = i / (KK * R);
    const int n0 = (ks + 1) / 2, n1 = ks / 2, qh = kh & 1, qw = kw & 1, cls = qh * 2 + qw;
    const int nw = qw ? n1 : n0, T = (qh ? n1 : n0) * nw;
    const int tbase = cls == 0 ? 0 : cls == 1 ? n0 * n0 : cls == 2 ? n0 * ks : n0 * ks + n1 * n0;
    wr[(size_t)tbase * C * R + (size_t)(c * T + (kh >> 1) * nw + (kw >> 1)) * R + r] = w[i];
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct GenWg {
    int B, R, C;            // batch, rows (channels of `small`), column channels (those of `big`)
    int SH, SW, IH, IW;     // small map, big map
    int ks, pad;
    int splits, steps_per_split, accumulate;
};

// 64 x 64 tile of dw[R][C * ks * ks]; k-step = 32 positions (b, sh, sw); grid z = reduction split
__global__ __launch_bounds__(GEN_THREADS) void conv_gen_wgrad_kernel(const float *__restrict__ small, const float *__restrict__ big,
                                                                     float *__restrict__ dw, float *__restrict__ part, GenWg g) {
    constexpr int TM = 64, TN = 64, PA = TM + 1, PB = TN + 1, NE = 8;
    __shared__ float lds[2 * 32 * (PA + PB)];
    float *const A0 = lds, *const B0 = lds + 2 * 32 * PA;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int kslot = t & 31, sub = t >> 5;
    const int KK = g.ks * g.ks, CK = g.C * KK, S = g.SH * g.SW, IHW = g.IH * g.IW, N = g.B * S;
    const int j0 = blockIdx.x * TN, r0 = blockIdx.y * TM;

    int aconst[NE], bconst[NE], bkh[NE], bkw[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int r = r0 + sub + 8 * e;
        aconst[e] = r < g.R ? r * S : -1;
        const int j = j0 + sub + 8 * e, cc = j / KK, tap = j - cc * KK;
        bkh[e] = tap / g.ks; bkw[e] = tap - bkh[e] * g.ks;
        bconst[e] = j < CK ? cc * IHW + bkh[e] * g.IW + bkw[e] : -1;
    }
    const gen_i32x4 rsa = gen_rsrc(small), rsb = gen_rsrc(big);
    const int n_begin = blockIdx.z * g.steps_per_split * 32;
    const int n_end = min(N, n_begin + g.steps_per_split * 32);

    float ra[NE], rb[NE];
    auto load = [&](int n0) {
        const int n = n0 + kslot;
        const bool nok = n < n_end;
        const int b = n / S, s = n - b * S, sh = s / g.SW, sw = s - sh * g.SW;
        const int dh = 2 * sh - g.pad, dw_ = 2 * sw - g.pad;
        const int abase = b * g.R * S + s, bbase = b * g.C * IHW + dh * g.IW + dw_;
#pragma unroll
        for (int e = 0; e < NE; ++e)
            ra[e] = gen_raw_buffer_load_f32(rsa, (nok && aconst[e] >= 0) ? 4 * (abase + aconst[e]) : GEN_OOB, 0, 0);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const bool ok = nok && bconst[e] >= 0 && (unsigned)(dh + bkh[e]) < (unsigned)g.IH &&
                            (unsigned)(dw_ + bkw[e]) < (unsigned)g.IW;
            rb[e] = gen_raw_buffer_load_f32(rsb, ok ? 4 * (bbase + bconst[e]) : GEN_OOB, 0, 0);
        }
    };
    auto store = [&](float *A, float *Bt) {
#pragma unroll
        for (int e = 0; e < NE; ++e) { A[kslot * PA + sub + 8 * e] = ra[e]; Bt[kslot * PB + sub + 8 * e] = rb[e]; }
    };
    const int wm = wave >> 1, wn = wave & 1;
    gen_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int nsteps = n_end > n_begin ? (n_end - n_begin + 31) / 32 : 0;
    if (nsteps > 0) load(n_begin);
    for (int s = 0; s < nsteps; ++s) {
        float *const A = A0 + (s & 1) * 32 * PA, *const Bt = B0 + (s & 1) * 32 * PB;
        store(A, Bt);
        __syncthreads();
        if (s + 1 < nsteps) load(n_begin + (s + 1) * 32);
        gen_mma<PA, PB>(A, Bt, 0, wm * 32, wn * 32, lane, acc);
    }
    const int j = j0 + wn * 32 + (lane & 31);
    if (j >= CK) return;
    float *dst = g.splits > 1 ? part + (size_t)blockIdx.z * g.R * CK : dw;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = r0 + wm * 32 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
        if (r >= g.R) continue;
        const size_t a = (size_t)r * CK + j;
        dst[a] = (g.splits == 1 && g.accumulate) ? dst[a] + acc[i] : acc[i];
    }
}

// dw (+)= the partial slabs, in slab order
__global__ __launch_bounds__(256) void conv_gen_wgrad_finish_kernel(const float *__restrict__ part, float *__restrict__ dw,
                                                                    int total, int splits, int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float s = part[i];
    for (int z = 1; z < splits; ++z) s += part[(size_t)z * total + i];
    dw[i] = accumulate ? dw[i] + s : s;
}

// ------------------------------------------------------------------------------------------------ host side
inline bool gen_domain_ok(int transposed, int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return false;
    if (!(ks == 4 || ks == 5) || stride != 2 || !(pad == 0 || pad == 1)) return false;
    long OH, OW;
    if (!transposed) {
        if (H + 2 * pad < ks || W + 2 * pad < ks) return false;
        OH = (H + 2 * pad - ks) / 2 + 1; OW = (W + 2 * pad - ks) / 2 + 1;
    } else {
        OH = (long)(H - 1) * 2 - 2 * pad + ks; OW = (long)(W - 1) * 2 - 2 * pad + ks;
    }
    if (OH <= 0 || OW <= 0) return false;
    // 32-bit byte offsets from the start of each tensor
    if ((long)B * Cin * H * W >= GEN_MAX_ELEMS || (long)B * Cout * OH * OW >= GEN_MAX_ELEMS) return false;
    if ((long)Cin * Cout * ks * ks >= GEN_MAX_ELEMS) return false;
    return true;
}

inline int gen_launch_gather(const float *in, const float *w, float *o1, float *o2, const float *pre_in, const GenGeo &g,
                             hipStream_t st, void *ws = nullptr, size_t ws_bytes = 0) {
    const int ncls = g.parity ? 4 : 1;
    if (g.parity) {                             // the class-major weight copy, made in front of every launch
        const int total = g.C * g.R * g.ks * g.ks;
        if (!ws || ws_bytes < (size_t)total * sizeof(float)) return MVAE_ERR_WS;
        hipLaunchKernelGGL(conv_gen_repack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, w, (float *)ws, g.C, g.R, g.ks, total);
        w = (const float *)ws;
    }
    long maxcols = 0;
    for (int q = 0; q < ncls; ++q) {
        const GenClass c = gen_class(g, q);
        const long n = (long)g.B * c.LH * c.LW;
        if (n > maxcols) maxcols = n;
    }
    if (maxcols == 0) return MVAE_OK;
    const long tiles64 = ((maxcols + 63) / 64) * ((g.R + 63) / 64) * ncls;
    if (g.R <= 32) {                            // one row tile: all four waves along the columns
        dim3 grid((unsigned)((maxcols + 127) / 128), 1, ncls);
        hipLaunchKernelGGL((conv_gen_gather_kernel<1, 4, 1>), grid, dim3(GEN_THREADS), 0, st, in, w, o1, o2, pre_in, g);
    } else if (tiles64 < 128 && g.C >= 32) {    // few columns, long reduction (the 2 x 2 maps): 32 x 32 tiles, the block's
        dim3 grid((unsigned)((maxcols + 31) / 32), (g.R + 31) / 32, ncls);    // four waves split the reduction
        hipLaunchKernelGGL((conv_gen_gather_kernel<1, 1, 4>), grid, dim3(GEN_THREADS), 0, st, in, w, o1, o2, pre_in, g);
    } else {
        dim3 grid((unsigned)((maxcols + 63) / 64), (g.R + 63) / 64, ncls);
        hipLaunchKernelGGL((conv_gen_gather_kernel<2, 2, 1>), grid, dim3(GEN_THREADS), 0, st, in, w, o1, o2, pre_in, g);
    }
    return mvae_launch_status();
}

// reduction splits of a weight gradient: aim at two blocks per CU, at least four k-steps per split
inline void gen_wgrad_plan(int B, int R, int C, int SH, int SW, int ks, int *splits, int *steps_per_split) {
    const long CK = (long)C * ks * ks, tiles = ((CK + 63) / 64) * ((R + 63) / 64);
    const long nsteps = ((long)B * SH * SW + 31) / 32;
    long sp = 512 / tiles;
    if (sp > nsteps / 4) sp = nsteps / 4;
    if (sp < 1) sp = 1;
    const long per = (nsteps + sp - 1) / sp;
    *steps_per_split = (int)per;
    *splits = (int)((nsteps + per - 1) / per);
}

inline int gen_launch_wgrad(const float *small, const float *big, float *dw, int B, int R, int C, int SH, int SW, int IH, int IW,
                            int ks, int pad, int flags, void *ws, size_t ws_bytes, hipStream_t st) {
    GenWg g;
    g.B = B; g.R = R; g.C = C; g.SH = SH; g.SW = SW; g.IH = IH; g.IW = IW; g.ks = ks; g.pad = pad;
    g.accumulate = (flags & MVAE_ACCUMULATE) ? 1 : 0;
    gen_wgrad_plan(B, R, C, SH, SW, ks, &g.splits, &g.steps_per_split);
    const int CK = C * ks * ks, total = R * CK;
    if (g.splits > 1 && (!ws || ws_bytes < (size_t)g.splits * total * sizeof(float))) return MVAE_ERR_WS;
    dim3 grid((CK + 63) / 64, (R + 63) / 64, g.splits);
    hipLaunchKernelGGL(conv_gen_wgrad_kernel, grid, dim3(GEN_THREADS), 0, st, small, big, dw, (float *)ws, g);
    if (g.splits > 1)
        hipLaunchKernelGGL(conv_gen_wgrad_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (const float *)ws, dw, total,
                           g.splits, g.accumulate);
    return mvae_launch_status();
}

inline GenGeo gen_geo(int B, int C, int R, int IH, int IW, int OH, int OW, int ks, int pad, int parity, int dgrad) {
    GenGeo g;
    g.B = B; g.C = C; g.R = R; g.IH = IH; g.IW = IW; g.OH = OH; g.OW = OW; g.ks = ks; g.pad = pad; g.parity = parity; g.dgrad = dgrad;
    return g;
}

}  // namespace

// Conv2d: x[B,Cin,H,W], w[Cout,Cin,ks,ks], y[B,Cout,OH,OW], OH = (H + 2 pad - ks) / 2 + 1
MVAE_EXPORT int mvae_conv2d_gen_fwd(const float *x, const float *w, float *pre, float *act, int B, int Cin, int H, int W, int Cout,
                                    int ks, int stride, int pad, mvae_stream_t stream) {
    if (!x || !w || (!pre && !act) || !gen_domain_ok(0, B, Cin, H, W, Cout, ks, stride, pad)) return MVAE_ERR_ARG;
    const int OH = (H + 2 * pad - ks) / 2 + 1, OW = (W + 2 * pad - ks) / 2 + 1;
    return gen_launch_gather(x, w, pre, act, nullptr, gen_geo(B, Cin, Cout, H, W, OH, OW, ks, pad, 0, 0), (hipStream_t)stream);
}

MVAE_EXPORT int mvae_conv2d_gen_dgrad(const float *dy, const float *w, float *dx, const float *pre_in, int B, int Cin, int H, int W,
                                      int Cout, int ks, int stride, int pad, void *ws, size_t ws_bytes, mvae_stream_t stream) {
    if (!dy || !w || !dx || !gen_domain_ok(0, B, Cin, H, W, Cout, ks, stride, pad)) return MVAE_ERR_ARG;
    const int OH = (H + 2 * pad - ks) / 2 + 1, OW = (W + 2 * pad - ks) / 2 + 1;
    // rows of x that no output window reaches (odd maps) belong to no tap of any class and come out as exact zeros
    return gen_launch_gather(dy, w, dx, nullptr, pre_in, gen_geo(B, Cout, Cin, OH, OW, H, W, ks, pad, 1, 1), (hipStream_t)stream, ws,
                             ws_bytes);
}

MVAE_EXPORT int mvae_conv2d_gen_wgrad(const float *dy, const float *x, float *dw, int B, int Cin, int H, int W, int Cout, int ks,
                                      int stride, int pad, int flags, void *ws, size_t ws_bytes, mvae_stream_t stream) {
    if (!dy || !x || !dw || !gen_domain_ok(0, B, Cin, H, W, Cout, ks, stride, pad)) return MVAE_ERR_ARG;
    const int OH = (H + 2 * pad - ks) / 2 + 1, OW = (W + 2 * pad - ks) / 2 + 1;
    return gen_launch_wgrad(dy, x, dw, B, Cout, Cin, OH, OW, H, W, ks, pad, flags, ws, ws_bytes, (hipStream_t)stream);
}

// ConvTranspose2d: x[B,Cin,H,W], w[Cin,Cout,ks,ks], y[B,Cout,OH,OW], OH = (H - 1) * 2 - 2 pad + ks
MVAE_EXPORT int mvae_convT2d_gen_fwd(const float *x, const float *w, float *pre, float *act, int B, int Cin, int H, int W, int Cout,
                                     int ks, int stride, int pad, void *ws, size_t ws_bytes, mvae_stream_t stream) {
    if (!x || !w || (!pre && !act) || !gen_domain_ok(1, B, Cin, H, W, Cout, ks, stride, pad)) return MVAE_ERR_ARG;
    const int OH = (H - 1) * 2 - 2 * pad + ks, OW = (W - 1) * 2 - 2 * pad + ks;
    return gen_launch_gather(x, w, pre, act, nullptr, gen_geo(B, Cin, Cout, H, W, OH, OW, ks, pad, 1, 0), (hipStream_t)stream, ws,
                             ws_bytes);
}

MVAE_EXPORT int mvae_convT2d_gen_dgrad(const float *dy, const float *w, float *dx, const float *pre_in, int B, int Cin, int H, int W,
                                       int Cout, int ks, int stride, int pad, mvae_stream_t stream) {
    if (!dy || !w || !dx || !gen_domain_ok(1, B, Cin, H, W, Cout, ks, stride, pad)) return MVAE_ERR_ARG;
    const int OH = (H - 1) * 2 - 2 * pad + ks, OW = (W - 1) * 2 - 2 * pad + ks;
    return gen_launch_gather(dy, w, dx, nullptr, pre_in, gen_geo(B, Cout, Cin, OH, OW, H, W, ks, pad, 0, 1), (hipStream_t)stream);
}

MVAE_EXPORT int mvae_convT2d_gen_wgrad(const float *dy, const float *x, float *dw, int B, int Cin, int H, int W, int Cout, int ks,
                                       int stride, int pad, int flags, void *ws, size_t ws_bytes, mvae_stream_t stream) {
    if (!dy || !x || !dw || !gen_domain_ok(1, B, Cin, H, W, Cout, ks, stride, pad)) return MVAE_ERR_ARG;
    const int OH = (H - 1) * 2 - 2 * pad + ks, OW = (W - 1) * 2 - 2 * pad + ks;
    return gen_launch_wgrad(x, dy, dw, B, Cin, Cout, H, W, OH, OW, ks, pad, flags, ws, ws_bytes, (hipStream_t)stream);
}

MVAE_EXPORT size_t mvae_conv_gen_ws_bytes(int op, int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad) {
    const bool conv_w = op == MVAE_OP_CONV_WGRAD, convT_w = op == MVAE_OP_CONVT_WGRAD;
    if (op == MVAE_OP_CONV_DGRAD || op == MVAE_OP_CONVT_FWD)         // the parity-form launches: the class-major weight copy
        return gen_domain_ok(op == MVAE_OP_CONVT_FWD, B, Cin, H, W, Cout, ks, stride, pad) ? (size_t)Cin * Cout * ks * ks * sizeof(float) : 0;
    if (!(conv_w || convT_w) || !gen_domain_ok(convT_w, B, Cin, H, W, Cout, ks, stride, pad)) return 0;
    int splits, per;
    if (conv_w) gen_wgrad_plan(B, Cout, Cin, (H + 2 * pad - ks) / 2 + 1, (W + 2 * pad - ks) / 2 + 1, ks, &splits, &per);
    else gen_wgrad_plan(B, Cin, Cout, H, W, ks, &splits, &per);
    return splits > 1 ? (size_t)splits * Cin * Cout * ks * ks * sizeof(float) : 0;
}

MVAE_EXPORT int mvae_conv_gen_supported(int transposed, int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad) {
    return gen_domain_ok(transposed ? 1 : 0, B, Cin, H, W, Cout, ks, stride, pad) ? 1 : 0;
}
