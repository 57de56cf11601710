// The vision experiment's input pipeline on the GPU: what vision/datasets.py does per item on the CPU -- four decoded
// files, two derived modalities (right half blacked out :97-111, watermark pasted :114-129), Compose([Resize(64),
// CenterCrop(64), ToTensor()]) on all six (:43-45, :78-83) and 1 - mask (:87) -- as ONE launch over a batch of raw uint8
// sources already resident in HBM.
//
// Twelve planes per image: image R G B, gray, edge, mask, obscured R G B, watermark R G B.  Before the resample every
// plane is an exact integer function of the source pixels:
//     gray (when no gray source is given)   (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16        Pillow convert('L')
//     obscured                               the colour value where x <= W / 2, else 0
//     watermark                              t = dst * (255 - a) + src * a + 128; ((t >> 8) + t) >> 8  Pillow paste(mark, (0, 0), mark)
// then each plane takes the arithmetic of resize_crop_kernel (preprocess.hip): Pillow's 8-bit BILINEAR, horizontal pass
// into a uint8 intermediate, vertical pass, the crop window, u8 / 255.0f; the mask plane is stored as 1.0f - u8 / 255.0f.
// The coefficient tables are the host's (mvae_resample_coeffs), as for mvae_resize_crop_u8_to_f32.
//
// THE SPLIT: grid (B, 4), one 1024-thread block per (image, plane group), three planes per block:
//     group 0  image       stages rgb
//     group 1  obscured    stages rgb; the blacked-out columns are taps of value 0, so the tap loop stops at W / 2
//     group 2  watermark   stages rgb and the mark's rows, blends in LDS in place
//     group 3  gray, edge, mask   stages gray (or rgb, and writes the luma over R in LDS), edge and mask
// Why four: the horizontally resampled rows the crop needs are (y1 - y0) * S bytes per plane -- 11.8 KB for 218 x 178 -> 64,
// 142 KB for twelve planes, which leaves no room for the source rows beside it in one block's LDS.  Three planes per block
// is exactly the footprint of resize_crop_kernel (35.5 KB + 32 KiB of staged rows, two blocks per CU), every block does
// the work of one of its blocks, and a batch of 50 is 200 blocks -- one round on 256 CUs -- where one block per image
// would occupy 50.  The price is that rgb is read by up to four blocks (116 KB each time, served by L2 after the first);
// each BLOCK reads every source byte at most once, as whole dwords from the 4-byte boundary below the first byte (an image
// whose H * W is odd starts misaligned), 32 KiB of rows per round.  No atomics, no global scratch: a block owns its three
// output planes.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr size_t VD_MAX_LDS = 150 * 1024;
constexpr int VD_THREADS = 1024;
constexpr int VD_CHUNK_BYTES = 32 * 1024;      // source rows staged per round, all streams of a group together
constexpr int VD_GROUPS = 4;
enum { G_IMAGE = 0, G_OBSCURED = 1, G_WATERMARK = 2, G_GRAY_EDGE_MASK = 3 };

struct VisionArgs {
    const uint8_t *rgb, *edge, *mask, *gray, *mark;
    float *image, *gray_out, *edge_out, *mask_out, *obscured, *watermark;
    const int *kx, *bx, *ky, *by;     // coefficient tables [out, ksize] and (first tap, taps) [out, 2]
    int H, W, ksx, ksy, S, crop_top, crop_left, y0, y1;
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__host__ __device__ inline int align16(int n) { return (n + 15) & ~15; }

// bytes of source one image row takes in the staging area of a group, all its streams together
__host__ __device__ inline int group_row_bytes(int g, int W, bool has_gray) {
    return g == G_WATERMARK ? 7 * W : g == G_GRAY_EDGE_MASK ? (has_gray ? 3 * W : 5 * W) : 3 * W;
}

__host__ __device__ inline int group_rows_per_chunk(int g, int W, bool has_gray) {
    const int rc = VD_CHUNK_BYTES / group_row_bytes(g, W, has_gray);
    return rc > 0 ? rc : 1;
}

// the staging area of one stream: rc rows and the up to 3 bytes below a misaligned first byte, a multiple of 16
__host__ __device__ inline int stream_bytes(int rc, int row_bytes) { return align16(rc * row_bytes + 4); }

// Copy nbytes from g into dst as whole dwords from the 4-byte boundary below g (coalesced 256-byte wave loads), bytes for
// the tail; returns how far below g the copy starts, i.e. the offset of g's first byte in dst.
__device__ __forceinline__ int stage(const uint8_t *g, int nbytes, uint8_t *dst, int t) {
    const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 3);
    const int n = nbytes + mis, ndw = n >> 2;
    const uint32_t *g4 = reinterpret_cast<const uint32_t *>(g - mis);
    uint32_t *d4 = reinterpret_cast<uint32_t *>(dst);
    for (int i = t; i < ndw; i += VD_THREADS) d4[i] = g4[i];
    for (int i = (ndw << 2) + t; i < n; i += VD_THREADS) dst[i] = (g - mis)[i];
    return mis;
}

__global__ __launch_bounds__(VD_THREADS) void vision_compose_kernel(VisionArgs a) {
    // [y1 - y0][S][3] horizontally resampled rows of this group's three planes, then the staged source rows
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.x, grp = blockIdx.y, S = a.S, W = a.W, t = threadIdx.x;
    const bool has_gray = a.gray != nullptr;
    const size_t px = (size_t)a.H * W;
    const int rows = a.y1 - a.y0;
    uint8_t *tmp = lds;
    uint8_t *chunk = lds + align16(rows * S * 3);
    const int RC = group_rows_per_chunk(grp, W, has_gray);
    // the streams of this group: s0 is rgb (or the gray plane), s1 / s2 the further ones
    const bool planar = grp == G_GRAY_EDGE_MASK;
    const bool s0_rgb = !(planar && has_gray);
    const uint8_t *src0 = s0_rgb ? a.rgb + (size_t)b * px * 3 : a.gray + (size_t)b * px;
    const int rb0 = s0_rgb ? 3 * W : W;
    const uint8_t *src1 = grp == G_WATERMARK ? a.mark : a.edge + (size_t)b * px;
    const int rb1 = grp == G_WATERMARK ? 4 * W : W;
    const uint8_t *src2 = a.mask + (size_t)b * px;
    uint8_t *c0 = chunk, *c1 = c0 + stream_bytes(RC, rb0), *c2 = c1 + stream_bytes(RC, rb1);
    const int x_end = grp == G_OBSCURED ? W / 2 + 1 : W;      // taps at x >= x_end are zero

    for (int r0 = 0; r0 < rows; r0 += RC) {
        const int nr = min(RC, rows - r0);
        const size_t y = (size_t)(a.y0 + r0);
        const int m0 = stage(src0 + y * rb0, nr * rb0, c0, t);
        int m1 = 0, m2 = 0;
        if (grp == G_WATERMARK || planar) m1 = stage(src1 + y * rb1, nr * rb1, c1, t);
        if (planar) m2 = stage(src2 + y * W, nr * W, c2, t);
        __syncthreads();
        if (grp == G_WATERMARK) {                               // paste the mark over the staged rgb, in place
            for (int idx = t; idx < nr * W * 3; idx += VD_THREADS) {
                const int p = idx / 3, c = idx - 3 * p;
                const int al = c1[m1 + 4 * p + 3], s = c1[m1 + 4 * p + c], d = c0[m0 + idx];
                const int v = d * (255 - al) + s * al + 128;
                c0[m0 + idx] = (uint8_t)(((v >> 8) + v) >> 8);
            }
            __syncthreads();
        } else if (planar && !has_gray) {                       // the luma over R: a pixel is read and written by one thread
            for (int p = t; p < nr * W; p += VD_THREADS) {
                uint8_t *q = c0 + m0 + 3 * p;
                q[0] = (uint8_t)((q[0] * 19595 + q[1] * 38470 + q[2] * 7471 + 0x8000) >> 16);
            }
            __syncthreads();
        }
        // horizontal pass over these rows: plane c of pixel (r, x) is base_c[r * rs_c + x * ps_c]
        for (int idx = t; idx < nr * S * 3; idx += VD_THREADS) {
            const int c = idx % 3, j = (idx / 3) % S, r = idx / (3 * S);
            const int ox = a.crop_left + j;
            const int xmin = a.bx[2 * ox], xmax = min(a.bx[2 * ox + 1], x_end - xmin);
            const int *k = a.kx + (size_t)ox * a.ksx;
            const uint8_t *row;
            int ps;
            if (!planar) { row = c0 + m0 + (r * W + xmin) * 3 + c; ps = 3; }
            else if (c == 0) { row = c0 + m0 + (r * W + xmin) * (s0_rgb ? 3 : 1); ps = s0_rgb ? 3 : 1; }
            else if (c == 1) { row = c1 + m1 + r * W + xmin; ps = 1; }
            else { row = c2 + m2 + r * W + xmin; ps = 1; }
            int acc = 1 << (PRECISION_BITS - 1);
            for (int x = 0; x < xmax; ++x) acc += (int)row[ps * x] * k[x];
            tmp[(size_t)(r0 + r) * S * 3 + j * 3 + c] = (uint8_t)clip8(acc >> PRECISION_BITS);
        }
        __syncthreads();
    }
    // vertical pass + ToTensor: plane c of this group at [b][.][i][j]
    float *o0, *o1, *o2;
    if (planar) {
        o0 = a.gray_out + (size_t)b * S * S; o1 = a.edge_out + (size_t)b * S * S; o2 = a.mask_out + (size_t)b * S * S;
    } else {
        o0 = (grp == G_IMAGE ? a.image : grp == G_OBSCURED ? a.obscured : a.watermark) + (size_t)b * 3 * S * S;
        o1 = o0 + S * S; o2 = o1 + S * S;
    }
    for (int idx = t; idx < 3 * S * S; idx += VD_THREADS) {
        const int j = idx % S, i = (idx / S) % S, c = idx / (S * S);
        const int oy = a.crop_top + i;
        const int ymin = a.by[2 * oy], ymax = a.by[2 * oy + 1];
        const int *k = a.ky + (size_t)oy * a.ksy;
        const uint8_t *col = tmp + ((size_t)(ymin - a.y0) * S + j) * 3 + c;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int y = 0; y < ymax; ++y) acc += (int)col[(size_t)y * S * 3] * k[y];
        const float q = (float)clip8(acc >> PRECISION_BITS) / 255.0f;
        float *o = c == 0 ? o0 : c == 1 ? o1 : o2;
        o[i * S + j] = (planar && c == 2) ? 1.0f - q : q;
    }
}

}  // namespace

MVAE_EXPORT int mvae_vision_compose(const uint8_t *rgb, const uint8_t *edge, const uint8_t *mask, const uint8_t *gray,
                                    const uint8_t *mark, float *image_out, float *gray_out, float *edge_out,
                                    float *mask_out, float *obscured_out, float *watermark_out, int B, int H, int W,
                                    int out_h, int out_w, int S, int crop_top, int crop_left, const int *kx_dev,
                                    const int *bx_dev, int ksx, const int *ky_dev, const int *by_dev, int ksy, int y0,
                                    int y1, mvae_stream_t stream) {
    if (!rgb || !edge || !mask || !mark || !image_out || !gray_out || !edge_out || !mask_out || !obscured_out ||
        !watermark_out || !kx_dev || !bx_dev || !ky_dev || !by_dev || B <= 0 || H <= 0 || W <= 0 || S <= 0 || ksx <= 0 ||
        ksy <= 0 || crop_top < 0 || crop_left < 0 || crop_top + S > out_h || crop_left + S > out_w || y0 < 0 || y1 > H ||
        y1 <= y0)
        return MVAE_ERR_ARG;
    // the sizes below are formed in int: keep every product far inside it
    if ((long long)(y1 - y0) * S * 3 > (long long)VD_MAX_LDS || (long long)W * 7 > (long long)VD_MAX_LDS) return MVAE_ERR_ARG;
    const bool has_gray = gray != nullptr;
    size_t lds = 0;
    for (int g = 0; g < VD_GROUPS; ++g) {
        const int rc = group_rows_per_chunk(g, W, has_gray);
        size_t need = (size_t)align16((y1 - y0) * S * 3);
        if (g == G_WATERMARK) need += stream_bytes(rc, 3 * W) + stream_bytes(rc, 4 * W);
        else if (g == G_GRAY_EDGE_MASK) need += stream_bytes(rc, has_gray ? W : 3 * W) + 2 * (size_t)stream_bytes(rc, W);
        else need += stream_bytes(rc, 3 * W);
        if (need > lds) lds = need;
    }
    if (lds > VD_MAX_LDS) return MVAE_ERR_ARG;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(vision_compose_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)VD_MAX_LDS);
        attr_done = true;
    }
    VisionArgs a;
    a.rgb = rgb; a.edge = edge; a.mask = mask; a.gray = gray; a.mark = mark;
    a.image = image_out; a.gray_out = gray_out; a.edge_out = edge_out; a.mask_out = mask_out;
    a.obscured = obscured_out; a.watermark = watermark_out;
    a.kx = kx_dev; a.bx = bx_dev; a.ky = ky_dev; a.by = by_dev;
    a.H = H; a.W = W; a.ksx = ksx; a.ksy = ksy; a.S = S; a.crop_top = crop_top; a.crop_left = crop_left;
    a.y0 = y0; a.y1 = y1;
    hipLaunchKernelGGL(vision_compose_kernel, dim3(B, VD_GROUPS), dim3(VD_THREADS), lds, (hipStream_t)stream, a);
    return mvae_launch_status();
}
