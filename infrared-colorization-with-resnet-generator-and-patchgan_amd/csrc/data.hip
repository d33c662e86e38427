// KAIST data pipeline on the device: the per-sample work
// of KAISTPairDataset.__getitem__ (ir:1132-1177) for a whole batch at once.
//
// The reference, per sample and in CPU DataLoader workers: cv2.imread ->
// cv2.resize(..., INTER_AREA) to img_size^2 (uint8 in, uint8 out) -> float32
// / 255 (IR: only when the resized image's max exceeds 1, ir:1142-1146) ->
// random paired horizontal flip (ir:1166-1168) -> x * 2 - 1 (ir:1175-1176).
// Here the host only decodes; the uint8 images of a batch are uploaded once
// and these two launches do resize, flip and normalisation:
//
//  * area_resize_u8_kernel: INTER_AREA as OpenCV's general area path computes
//    it for scale factors >= 1 (resizeArea_: per destination pixel, each
//    source row of the vertical cell reduced horizontally with the x-table
//    weights -- buf = sum alpha * S in table order -- then sum = beta0 * buf0
//    (+ beta1 * buf1 ...), saturate_cast<uchar> = round half to even, clamp).
//    The tables (CSR: per destination index a run of (source index, weight))
//    come from the host (ops.area_table, computeResizeAreaTab's recurrence).
//    Every float op is a separately rounded mul / add (fp contract off: hipcc
//    would fuse them into FMAs), in OpenCV's order.  The flip writes column W-1-x; per-image max of the
//    resized bytes (IR rule) by one atomicMax per block.
//  * unit_kernel: uint8 -> float32 [-1, 1]: v / 255 (correctly rounded float32
//    division, as numpy), then * 2 - 1 (torch float32), the IR max rule applied.
//  * max_u8_kernel + native_unit_kernel: img_size=None (or a target equal to the
//    source size), where cv2.resize is skipped (ir:817-818) or copies: uint8 NHWC
//    -> float32 NCHW [-1, 1] in one pass with unit_kernel's arithmetic, 16-byte
//    loads and per-plane float4 stores; the IR max rule needs the max pass first.
// Config.load_size (the paired random-crop jitter): the *_crop entries take a device array
// crop [N][2] = {oy, ox} and compute only the Hout x Wout window at (oy, ox) of the load-size
// image -- the resizing kernels read their tables at (y + oy, x + ox), the native kernels read
// the window's rows out of the source with its row pitch; flip and the IR max see the window
// alone.  The same kernels with crop = null are the plain entries.
// Byte-sized HBM streams; no LDS, no MFMA.
#include "common.h"

namespace {

constexpr int TPB = 256;

// src: uint8 [N][Hin][Win][C] with image stride img_stride bytes; out: uint8
// [N][C][Hout][Wout] (NCHW, the dataset's tensor layout).  One thread = one
// destination pixel, all C (<= 4) channels.  crop (nullable, [N][2] = {oy, ox}): out is
// the Hout x Wout window at (oy, ox) of the image the tables describe.
__global__ __launch_bounds__(TPB) void area_resize_u8_kernel(const uint8_t* __restrict__ src, int Hin, int Win, int C,
                                                             long img_stride, const int* __restrict__ yptr,
                                                             const int* __restrict__ ysrc,
                                                             const float* __restrict__ yw, int Hout,
                                                             const int* __restrict__ xptr,
                                                             const int* __restrict__ xsrc,
                                                             const float* __restrict__ xw, int Wout,
                                                             const int* __restrict__ crop,
                                                             const uint8_t* __restrict__ flip,
                                                             uint8_t* __restrict__ out, int* __restrict__ img_max) {
#pragma clang fp contract(off)  // OpenCV's separate float mul / add: no FMA contraction (hipcc defaults to fast)
    const int n = blockIdx.y;
    const int e = blockIdx.x * TPB + threadIdx.x;
    __shared__ int bmax;
    if (threadIdx.x == 0) bmax = 0;
    __syncthreads();
    if (e < Hout * Wout) {
        const int y = e / Wout, x = e - y * Wout;
        const int yt = crop ? y + crop[2 * n] : y, xt = crop ? x + crop[2 * n + 1] : x;   // table rows
        const uint8_t* S = src + n * img_stride;
        float sum[4] = {0.f, 0.f, 0.f, 0.f};
        const int y0 = yptr[yt], y1 = yptr[yt + 1], x0 = xptr[xt], x1 = xptr[xt + 1];
        for (int ty = y0; ty < y1; ++ty) {
            const uint8_t* row = S + (long)ysrc[ty] * Win * C;
            const float beta = yw[ty];
            float buf[4] = {0.f, 0.f, 0.f, 0.f};
            for (int tx = x0; tx < x1; ++tx) {
                const uint8_t* p = row + xsrc[tx] * C;
                const float alpha = xw[tx];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < C) buf[c] = buf[c] + (float)p[c] * alpha;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) sum[c] = ty == y0 ? beta * buf[c] : sum[c] + beta * buf[c];
        }
        const int xo = (flip && flip[n]) ? Wout - 1 - x : x;
        int m = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= C) break;
            float r = rintf(sum[c]);                 // cvRound: nearest, ties to even
            r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
            const int v = (int)r;
            out[(((long)n * C + c) * Hout + y) * Wout + xo] = (uint8_t)v;
            m = v > m ? v : m;
        }
        if (img_max && m > 1) atomicMax(&bmax, m);
    }
    __syncthreads();
    if (img_max && threadIdx.x == 0 && bmax > 0) atomicMax(img_max + n, bmax);
}

// cv2.resize(INTER_AREA) when an axis UPscales: OpenCV's generic linear resampler with
// area-mode coefficients in 8-bit fixed point (resizeGeneric_, HResizeLinear<uchar, int,
// short, 2048>, VResizeLinear<uchar, int, short, FixedPtCast<..., 22>>): tables from the
// host (data.linear_area_table).  Per destination (y, x) and channel:
//   D(r) = S[r][x0] * a0 + S[r][min(x0 + 1, Win - 1)] * a1   (x >= xlim: S[r][x0] * 2048)
//   v = (((b0 * (D(y0) >> 4)) >> 16) + ((b1 * (D(min(y0 + 1, Hin - 1)) >> 4)) >> 16) + 2) >> 2
// all in int32, stored as uchar (no saturation, as OpenCV).  Flip, crop and the IR max as above.
__global__ __launch_bounds__(TPB) void linear_area_u8_kernel(const uint8_t* __restrict__ src, int Hin, int Win, int C,
                                                             long img_stride, const int* __restrict__ yofs,
                                                             const int* __restrict__ ycoef, int Hout,
                                                             const int* __restrict__ xofs,
                                                             const int* __restrict__ xcoef, int xlim, int Wout,
                                                             const int* __restrict__ crop,
                                                             const uint8_t* __restrict__ flip,
                                                             uint8_t* __restrict__ out, int* __restrict__ img_max) {
    const int n = blockIdx.y;
    const int e = blockIdx.x * TPB + threadIdx.x;
    __shared__ int bmax;
    if (threadIdx.x == 0) bmax = 0;
    __syncthreads();
    if (e < Hout * Wout) {
        const int y = e / Wout, x = e - y * Wout;
        const uint8_t* S = src + n * img_stride;
        const int yt = crop ? y + crop[2 * n] : y, xt = crop ? x + crop[2 * n + 1] : x;   // table rows
        const int y0 = yofs[yt], y1 = min(y0 + 1, Hin - 1);
        const int b0 = ycoef[2 * yt], b1 = ycoef[2 * yt + 1];
        const int x0 = xofs[xt], x1 = min(x0 + 1, Win - 1);
        const int a0 = xcoef[2 * xt], a1 = xcoef[2 * xt + 1];
        const bool one = xt >= xlim;
        const int xo = (flip && flip[n]) ? Wout - 1 - x : x;
        int m = 0;
        for (int c = 0; c < C; ++c) {
            const uint8_t* r0 = S + (long)y0 * Win * C + c;
            const uint8_t* r1 = S + (long)y1 * Win * C + c;
            const int d0 = one ? (int)r0[x0 * C] * 2048 : (int)r0[x0 * C] * a0 + (int)r0[x1 * C] * a1;
            const int d1 = one ? (int)r1[x0 * C] * 2048 : (int)r1[x0 * C] * a0 + (int)r1[x1 * C] * a1;
            const int v = ((((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2) & 0xFF;
            out[(((long)n * C + c) * Hout + y) * Wout + xo] = (uint8_t)v;
            m = v > m ? v : m;
        }
        if (img_max && m > 1) atomicMax(&bmax, m);
    }
    __syncthreads();
    if (img_max && threadIdx.x == 0 && bmax > 0) atomicMax(img_max + n, bmax);
}

// out[n][i] = f32(in[n][i]) / 255 * 2 - 1; with max_rule (IR) the division is
// skipped for images whose max byte is <= 1 (ir:1142).
__global__ __launch_bounds__(TPB) void unit_kernel(const uint8_t* __restrict__ in, long per_image,
                                                   const int* __restrict__ img_max, int max_rule,
                                                   float* __restrict__ out) {
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    const bool div = !max_rule || img_max[n] > 1;
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < per_image; i += (long)gridDim.x * TPB) {
        float v = (float)in[n * per_image + i];
        if (div) v = v / 255.0f;   // IEEE division (hipcc's default correctly rounded fp32 divide)
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);  // np.clip(img, 0, 1)
        out[n * per_image + i] = v * 2.0f - 1.0f;
    }
}

// The [-1, 1] value of one byte: unit_kernel's arithmetic, op for op.
IRGAN_HD float unit_value(uint32_t b, bool div) {
#pragma clang fp contract(off)
    float v = (float)b;
    if (div) v = v / 255.0f;
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return v * 2.0f - 1.0f;
}

constexpr int RUN = 16;  // pixels per lane of the native kernel: C 16-byte loads, 4 float4 stores per plane

// Where image n's window starts in src: the image itself, or with crop ([N][2] = {oy, ox})
// pixel (oy, ox) of its rows of pitch bytes, px bytes per pixel.
__device__ __forceinline__ const uint8_t* window_start(const uint8_t* src, int n, long img_stride,
                                                       const int* __restrict__ crop, long pitch, int px) {
    const uint8_t* S = src + n * img_stride;
    return crop ? S + crop[2 * n] * pitch + crop[2 * n + 1] * px : S;
}

// img_max[n] (zeroed) = max byte of image n's window: `spans` runs of len contiguous bytes,
// pitch bytes apart, from window_start on (a whole image: one span of H * W * C bytes; a crop:
// its h rows of w * C bytes).  Per span: 16-byte loads from the first aligned byte on, the
// < 16 bytes before and after it one per thread.  The gridDim.x blocks of a group share a
// span, the gridDim.z groups stride over the spans; one atomicMax per wave.
__global__ __launch_bounds__(TPB) void max_u8_kernel(const uint8_t* __restrict__ src, int spans, long len, long pitch,
                                                     long img_stride, const int* __restrict__ crop, int px,
                                                     int* __restrict__ img_max) {
    const int n = blockIdx.y;
    const uint8_t* S0 = window_start(src, n, img_stride, crop, pitch, px);
    const long t = blockIdx.x * (long)TPB + threadIdx.x, T = (long)gridDim.x * TPB;
    uint32_t m = 0;
    for (int r = blockIdx.z; r < spans; r += gridDim.z) {
        const uint8_t* S = S0 + r * pitch;
        const long head = min(len, (long)((16 - ((uintptr_t)S & 15)) & 15));
        const long nvec = (len - head) >> 4, tail0 = head + (nvec << 4);
        for (long i = t; i < nvec; i += T) {
            const uint4 v = *(const uint4*)(S + head + (i << 4));
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m = max(max(m, w[k] & 0xFF), (w[k] >> 8) & 0xFF);
                m = max(max(m, (w[k] >> 16) & 0xFF), w[k] >> 24);
            }
        }
        if (t < head) m = max(m, (uint32_t)S[t]);
        if (t < len - tail0) m = max(m, (uint32_t)S[tail0 + t]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(img_max + n, (int)m);
}

// src: uint8 [N][H][W][C] (image stride img_stride bytes); out: float32 [N][C][H][W] in [-1, 1]
// (unit_value), out8 (nullable): the same bytes as uint8 [N][C][H][W].  A row is cut into
// U = cdiv(W, RUN) + 1 units at the first pixel p whose byte address is 16-byte aligned:
// unit 0 = pixels [0, p), unit u = [p + RUN * (u - 1), p + RUN * u), clipped to the row.
// One lane = one unit: a whole unit takes C 16-byte loads and, per channel plane, 4 float4
// stores where the destination run is 16-byte aligned (dword stores otherwise); a clipped
// unit, or a row with no aligned pixel start (C = 2, 4 on an odd address), goes pixel by
// pixel.  The flip reverses the destination run: source pixel x lands on column W - 1 - x.
// With crop ([N][2] = {oy, ox}) the H x W image is the window at (oy, ox) of a wider source:
// its rows lie pitch bytes apart (pitch = W * C without one), each cut at its own address.
template <int C>
__global__ __launch_bounds__(TPB) void native_unit_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                          long img_stride, long pitch, const int* __restrict__ crop,
                                                          int U, const uint8_t* __restrict__ flip,
                                                          const int* __restrict__ img_max, int max_rule,
                                                          float* __restrict__ out, uint8_t* __restrict__ out8) {
    const int n = blockIdx.y;
    const long e = blockIdx.x * (long)TPB + threadIdx.x;
    if (e >= (long)H * U) return;
    const int y = (int)(e / U), u = (int)(e - (long)y * U);
    const uint8_t* row = window_start(src, n, img_stride, crop, pitch, C) + y * pitch;
    int p = -1;
#pragma unroll
    for (int k = RUN - 1; k >= 0; --k)
        if ((((uintptr_t)row + k * C) & 15) == 0) p = k;
    const bool aligned = p >= 0;
    if (!aligned) p = 0;
    const int x0 = p + (u - 1) * RUN, x1 = x0 + RUN;
    const bool fl = flip && flip[n];
    const bool div = !max_rule || img_max[n] > 1;
    const long HW = (long)H * W, o0 = (long)n * C * HW + (long)y * W;
    if (aligned && x0 >= 0 && x1 <= W) {
        uint32_t w[4 * C];
        const uint4* q = (const uint4*)(row + (long)x0 * C);
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const uint4 v = q[k];
            w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
        }
        const long od = o0 + (fl ? W - x1 : x0);   // destination run [od, od + RUN) of plane 0
#pragma unroll
        for (int c = 0; c < C; ++c) {
            uint32_t b[RUN];
#pragma unroll
            for (int j = 0; j < RUN; ++j) {
                const int i0 = j * C + c, i1 = (RUN - 1 - j) * C + c;   // byte of run pixel j, and flipped
                const uint32_t b0 = (w[i0 >> 2] >> (8 * (i0 & 3))) & 0xFF, b1 = (w[i1 >> 2] >> (8 * (i1 & 3))) & 0xFF;
                b[j] = fl ? b1 : b0;
            }
            float* d = out + od + c * HW;
            if (((uintptr_t)d & 15) == 0) {
#pragma unroll
                for (int j = 0; j < RUN; j += 4)
                    *(float4*)(d + j) = float4{unit_value(b[j], div), unit_value(b[j + 1], div),
                                               unit_value(b[j + 2], div), unit_value(b[j + 3], div)};
            } else {
#pragma unroll
                for (int j = 0; j < RUN; ++j) d[j] = unit_value(b[j], div);
            }
            if (out8) {
                uint8_t* d8 = out8 + od + c * HW;
                if (((uintptr_t)d8 & 15) == 0) {
                    uint32_t pk[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        pk[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
                    *(uint4*)d8 = uint4{pk[0], pk[1], pk[2], pk[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < RUN; ++j) d8[j] = (uint8_t)b[j];
                }
            }
        }
        return;
    }
    for (int x = max(x0, 0); x < min(x1, W); ++x) {
        const long od = o0 + (fl ? W - 1 - x : x);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint32_t b = row[(long)x * C + c];
            out[od + c * HW] = unit_value(b, div);
            if (out8) out8[od + c * HW] = (uint8_t)b;
        }
    }
}

// The entries' shared halves.  window = a *_crop entry: crop is required and the Hout x Wout
// output must fit the Hload x Wload image of the tables (the source itself for the native
// pass); the plain entries pass crop = null and the full extents.
bool bad_window(bool window, const int32_t* crop, int Hload, int Wload, int Hout, int Wout) {
    return window ? (!crop || Hout > Hload || Wout > Wload) : crop != nullptr;
}

int area_resize(bool window, const void* src, int N, int Hin, int Win, int C, long img_stride, const int32_t* yptr,
                const int32_t* ysrc, const float* yw, int Hload, const int32_t* xptr, const int32_t* xsrc,
                const float* xw, int Wload, const int32_t* crop, int Hout, int Wout, const void* flip, void* out_u8,
                int32_t* img_max, irgan_stream_t s) {
    if (N <= 0 || Hout <= 0 || Wout <= 0) return 0;
    if (!src || !yptr || !ysrc || !yw || !xptr || !xsrc || !xw || !out_u8 || C < 1 || C > 4 || Hin < 1 || Win < 1 ||
        img_stride < (long)Hin * Win * C || N > 65535 || bad_window(window, crop, Hload, Wload, Hout, Wout))
        return IRGAN_EINVAL;
    dim3 g(irgan_cdiv((long)Hout * Wout, TPB), N);
    area_resize_u8_kernel<<<g, TPB, 0, (hipStream_t)s>>>((const uint8_t*)src, Hin, Win, C, img_stride, yptr, ysrc, yw,
                                                         Hout, xptr, xsrc, xw, Wout, crop, (const uint8_t*)flip,
                                                         (uint8_t*)out_u8, img_max);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

int linear_area_resize(bool window, const void* src, int N, int Hin, int Win, int C, long img_stride,
                       const int32_t* yofs, const int32_t* ycoef, int Hload, const int32_t* xofs, const int32_t* xcoef,
                       int xlim, int Wload, const int32_t* crop, int Hout, int Wout, const void* flip, void* out_u8,
                       int32_t* img_max, irgan_stream_t s) {
    if (N <= 0 || Hout <= 0 || Wout <= 0) return 0;
    if (!src || !yofs || !ycoef || !xofs || !xcoef || !out_u8 || C < 1 || C > 4 || Hin < 1 || Win < 1 ||
        img_stride < (long)Hin * Win * C || N > 65535 || bad_window(window, crop, Hload, Wload, Hout, Wout))
        return IRGAN_EINVAL;
    dim3 g(irgan_cdiv((long)Hout * Wout, TPB), N);
    linear_area_u8_kernel<<<g, TPB, 0, (hipStream_t)s>>>((const uint8_t*)src, Hin, Win, C, img_stride, yofs, ycoef,
                                                         Hout, xofs, xcoef, xlim, Wout, crop, (const uint8_t*)flip,
                                                         (uint8_t*)out_u8, img_max);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

// src: [N][Hsrc][Wsrc][C]; the H x W output is the whole image (crop null) or its window.
int native_to_unit(bool window, const void* src, int N, int Hsrc, int Wsrc, int C, long img_stride,
                   const int32_t* crop, int H, int W, const void* flip, int max_rule, int32_t* img_max, float* out,
                   void* out_u8, irgan_stream_t s) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    if (!src || !out || (max_rule && !img_max) || C < 1 || C > 4 || img_stride < (long)Hsrc * Wsrc * C || N > 65535 ||
        bad_window(window, crop, Hsrc, Wsrc, H, W))
        return IRGAN_EINVAL;
    const long pitch = (long)Wsrc * C;
    if (max_rule) {   // the whole image's (window's) max decides every pixel (ir:1142): its own pass first
        // a whole image is one span shared by every block; a window's rows go one block each
        const int spans = window ? H : 1;
        const long len = window ? (long)W * C : (long)H * W * C;
        const dim3 g = window ? dim3(1, N, std::min(H, 128))
                              : dim3((int)std::min<long>(irgan_cdiv(len, TPB * 32), 128), N, 1);
        max_u8_kernel<<<g, TPB, 0, (hipStream_t)s>>>((const uint8_t*)src, spans, len, pitch, img_stride, crop, C,
                                                     img_max);
        IRGAN_LAUNCH_CHECK();
    }
    const int U = irgan_cdiv(W, RUN) + 1;
    const dim3 g(irgan_cdiv((long)H * U, TPB), N);
#define IRGAN_NATIVE(CC)                                                                                          \
    native_unit_kernel<CC><<<g, TPB, 0, (hipStream_t)s>>>((const uint8_t*)src, H, W, img_stride, pitch, crop, U,  \
                                                          (const uint8_t*)flip, img_max, max_rule, out,           \
                                                          (uint8_t*)out_u8)
    switch (C) {
        case 1: IRGAN_NATIVE(1); break;
        case 2: IRGAN_NATIVE(2); break;
        case 3: IRGAN_NATIVE(3); break;
        default: IRGAN_NATIVE(4); break;
    }
#undef IRGAN_NATIVE
    IRGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int irgan_area_resize_u8(const void* src, int32_t N, int32_t Hin, int32_t Win, int32_t C, int64_t img_stride,
                                    const int32_t* yptr, const int32_t* ysrc, const float* yw, int32_t Hout,
                                    const int32_t* xptr, const int32_t* xsrc, const float* xw, int32_t Wout,
                                    const void* flip, void* out_u8, int32_t* img_max, irgan_stream_t s) {
    return area_resize(false, src, N, Hin, Win, C, img_stride, yptr, ysrc, yw, Hout, xptr, xsrc, xw, Wout, nullptr,
                       Hout, Wout, flip, out_u8, img_max, s);
}

extern "C" int irgan_area_resize_crop_u8(const void* src, int32_t N, int32_t Hin, int32_t Win, int32_t C,
                                         int64_t img_stride, const int32_t* yptr, const int32_t* ysrc, const float* yw,
                                         int32_t Hload, const int32_t* xptr, const int32_t* xsrc, const float* xw,
                                         int32_t Wload, const int32_t* crop, int32_t Hout, int32_t Wout,
                                         const void* flip, void* out_u8, int32_t* img_max, irgan_stream_t s) {
    return area_resize(true, src, N, Hin, Win, C, img_stride, yptr, ysrc, yw, Hload, xptr, xsrc, xw, Wload, crop, Hout,
                       Wout, flip, out_u8, img_max, s);
}

extern "C" int irgan_u8_to_unit(const void* in, int32_t N, int64_t per_image, const int32_t* img_max, int32_t max_rule,
                                float* out, irgan_stream_t s) {
    if (N <= 0 || per_image <= 0) return 0;
    if (!in || !out || (max_rule && !img_max) || N > 65535) return IRGAN_EINVAL;
    const int bx = (int)std::min<long>(irgan_cdiv(per_image, TPB), 1024);
    unit_kernel<<<dim3(bx, N), TPB, 0, (hipStream_t)s>>>((const uint8_t*)in, per_image, img_max, max_rule, out);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_linear_area_resize_u8(const void* src, int32_t N, int32_t Hin, int32_t Win, int32_t C,
                                           int64_t img_stride, const int32_t* yofs, const int32_t* ycoef,
                                           int32_t Hout, const int32_t* xofs, const int32_t* xcoef, int32_t xlim,
                                           int32_t Wout, const void* flip, void* out_u8, int32_t* img_max,
                                           irgan_stream_t s) {
    return linear_area_resize(false, src, N, Hin, Win, C, img_stride, yofs, ycoef, Hout, xofs, xcoef, xlim, Wout,
                              nullptr, Hout, Wout, flip, out_u8, img_max, s);
}

extern "C" int irgan_linear_area_resize_crop_u8(const void* src, int32_t N, int32_t Hin, int32_t Win, int32_t C,
                                                int64_t img_stride, const int32_t* yofs, const int32_t* ycoef,
                                                int32_t Hload, const int32_t* xofs, const int32_t* xcoef, int32_t xlim,
                                                int32_t Wload, const int32_t* crop, int32_t Hout, int32_t Wout,
                                                const void* flip, void* out_u8, int32_t* img_max, irgan_stream_t s) {
    return linear_area_resize(true, src, N, Hin, Win, C, img_stride, yofs, ycoef, Hload, xofs, xcoef, xlim, Wload, crop,
                              Hout, Wout, flip, out_u8, img_max, s);
}

extern "C" int irgan_u8_native_to_unit(const void* src, int32_t N, int32_t H, int32_t W, int32_t C, int64_t img_stride,
                                       const void* flip, int32_t max_rule, int32_t* img_max, float* out, void* out_u8,
                                       irgan_stream_t s) {
    return native_to_unit(false, src, N, H, W, C, img_stride, nullptr, H, W, flip, max_rule, img_max, out, out_u8, s);
}

extern "C" int irgan_u8_native_crop_to_unit(const void* src, int32_t N, int32_t Hload, int32_t Wload, int32_t C,
                                            int64_t img_stride, const int32_t* crop, int32_t Hout, int32_t Wout,
                                            const void* flip, int32_t max_rule, int32_t* img_max, float* out,
                                            void* out_u8, irgan_stream_t s) {
    return native_to_unit(true, src, N, Hload, Wload, C, img_stride, crop, Hout, Wout, flip, max_rule, img_max, out,
                          out_u8, s);
}

