// Loss kernels of the G/D objectives (ir:1647-1679) and the fused Adam update
// (ir:1601-1604, 1651, 1681).  Images are NHWC fp32 (B, H, W, 3).  Every loss
// is reduced per block in fp32 and across blocks with one fp64 atomic, and
// writes its gradient in the same pass (no autograd tape).
#include "common.h"

namespace {

constexpr int TPB = 256;

IRGAN_HD void block_add(double* dst, float v) { block_sum_add<TPB>(dst, v); }

int nblocks(long total) { return (int)std::max<long>(1, std::min<long>((total + TPB - 1) / TPB, 8192)); }
// kernels that finish with block_add: every block adds into the SAME fp64 word,
// and same-address atomics serialise at the memory side (~10 ns each), so keep
// the grid small and let threads loop
int nblocks_red(long total) { return (int)std::max<long>(1, std::min<long>((total + TPB - 1) / TPB, 512)); }

// mode 0: pred = [real (n) ; fake (n)] -> 0.5*(mean relu(1-r) + mean relu(1+f))   (ir:1647-1649)
// mode 1: pred = fake (n) -> -mean(p) * scale                                    (ir:1662, x lambda_gan)
__global__ __launch_bounds__(TPB) void hinge_kernel(const float* __restrict__ pred, int n, int mode, float scale,
                                                    float* __restrict__ grad, double* __restrict__ loss) {
    const long total = mode == 0 ? 2L * n : n;
    float acc = 0.f;
    const float inv = 1.f / (float)n;
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const float p = pred[i];
        if (mode == 0) {  // [real; fake]
            if (i < n) {
                const float t = 1.f - p;
                acc += t > 0.f ? t : 0.f;
                grad[i] = t > 0.f ? -0.5f * inv * scale : 0.f;
            } else {
                const float t = 1.f + p;
                acc += t > 0.f ? t : 0.f;
                grad[i] = t > 0.f ? 0.5f * inv * scale : 0.f;
            }
        } else {
            acc += p;
            grad[i] = -scale * inv;
        }
    }
    block_add(loss, mode == 0 ? 0.5f * acc * inv * scale : -acc * inv * scale);
}

// The LSGAN and BCE ("vanilla") objectives on the same patch logits, with hinge_kernel's layout
// and sides.  Per element the target y and the weight c of its mean are
//   side 0, pred = [real (n) ; fake (n)]:  y = t (the smoothed real label) | 0,  c = 0.5
//   side 1, pred = fake (n):               y = 1,                            c = 1
// and   LSGAN: term (p - y)^2,                                   d term / d p = 2 (p - y)
//       BCE:   term max(p, 0) - p y + log1p(exp(-|p|)),          d term / d p = sigmoid(p) - y
// loss += scale * c * mean(term), grad = scale * c / n * d term / d p (written, not accumulated).
// exp(-|p|) <= 1 never overflows, so the BCE arm is finite for any finite logit.  The gradient's
// few operations after expf run in fp64 and round once: sigmoid(p) - 1 cancels, and the tensor is
// 2*B*30*30 logits, so the extra width costs nothing that shows in a step.
constexpr int GAN_LSGAN = 1, GAN_BCE = 2;

template <int OBJ>
__global__ __launch_bounds__(TPB) void gan_loss_kernel(const float* __restrict__ pred, int n, int side, float t,
                                                       float scale, float* __restrict__ grad,
                                                       double* __restrict__ loss) {
    const long total = side == 0 ? 2L * n : n;
    const float c = side == 0 ? 0.5f : 1.f;
    const double k = (double)c * (double)scale / (double)n;
    float acc = 0.f;
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const float p = pred[i];
        const float y = side == 0 ? (i < n ? t : 0.f) : 1.f;
        if constexpr (OBJ == GAN_LSGAN) {
            const float d = p - y;
            acc += d * d;
            grad[i] = (float)(2.0 * k * ((double)p - (double)y));
        } else {
            const float e = expf(-fabsf(p));
            acc += fmaxf(p, 0.f) - p * y + log1pf(e);
            const double ed = (double)e;
            const double sg = (p >= 0.f ? 1.0 : ed) / (1.0 + ed);
            grad[i] = (float)(k * (sg - (double)y));
        }
    }
    block_add(loss, c * acc * (1.f / (float)n) * scale);
}

template <typename T>
IRGAN_HD void ld8t(const T* p, long i, float* o) {
    if constexpr (sizeof(T) == 2) {
        const uint4 u = *(const uint4*)(p + i);
        const uint32_t q[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = __uint_as_float(q[k] << 16);
            o[2 * k + 1] = __uint_as_float(q[k] & 0xffff0000u);
        }
    } else {
        const float4 x0 = *(const float4*)(p + i), x1 = *(const float4*)(p + i + 4);
        o[0] = x0.x; o[1] = x0.y; o[2] = x0.z; o[3] = x0.w; o[4] = x1.x; o[5] = x1.y; o[6] = x1.z; o[7] = x1.w;
    }
}
template <typename T>
IRGAN_HD void st8t(T* p, long i, const float* v) {
    if constexpr (sizeof(T) == 2) {
        uint4 u;
        u.x = pk_bf16(v[0], v[1]);
        u.y = pk_bf16(v[2], v[3]);
        u.z = pk_bf16(v[4], v[5]);
        u.w = pk_bf16(v[6], v[7]);
        *(uint4*)(p + i) = u;
    } else {
        *(float4*)(p + i) = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
}

// loss += w * mean|a - b|, and the term's gradient written or added (accumulate) to ga, summed in
// fp32 and rounded once to ga's type.  Plain: d/da = sgn(a-b) * w/count, ga may be null (value
// only).  TAP, one perceptual tap (Config.perc_layers): a = relu(z) of the fake images, b the real
// images' map, and the gradient w.r.t. the PRE-activation z lands in ga (required):
//   dz = (accumulate ? dz : 0) + (a > 0 ? sgn(a-b) * w/count : 0)
// VEC: 8 elements per thread-iteration (16/32-byte accesses; count % 8 == 0)
template <typename T, typename G, bool VEC, bool TAP>
__global__ __launch_bounds__(TPB) void l1_kernel(const T* __restrict__ a, const T* __restrict__ b, long count, float w,
                                                 G* __restrict__ ga, int accumulate, double* __restrict__ loss) {
    float acc = 0.f;
    const float inv = w / (float)count;
    const bool wr = TAP || ga, rd = wr && accumulate;
    if constexpr (VEC) {
        for (long i = (blockIdx.x * (long)TPB + threadIdx.x) * 8; i < count; i += (long)gridDim.x * TPB * 8) {
            float av[8], bv[8], gv[8];
            ld8t<T>(a, i, av);
            ld8t<T>(b, i, bv);
            if (rd) ld8t<G>(ga, i, gv);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float d = av[k] - bv[k];
                acc += fabsf(d);
                gv[k] = (rd ? gv[k] : 0.f) + (TAP ? tap_grad(av[k], bv[k], inv) : sgn(d) * inv);
            }
            if (wr) st8t<G>(ga, i, gv);
        }
    } else {
        for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < count; i += (long)gridDim.x * TPB) {
            const float av = to_f<T>(a[i]), bv = to_f<T>(b[i]), d = av - bv;
            acc += fabsf(d);
            if constexpr (TAP) {
                ga[i] = from_f<G>((accumulate ? to_f<G>(ga[i]) : 0.f) + tap_grad(av, bv, inv));
            } else if (ga) {
                float gv = sgn(d) * inv;
                if (accumulate) gv += to_f<G>(ga[i]);
                ga[i] = from_f<G>(gv);
            }
        }
    }
    block_add(loss, acc * inv);
}


// TV (ir:686-694): mean|x[h+1]-x[h]| + mean|x[w+1]-x[w]| over N*C*(H-1)*W and N*C*H*(W-1).
// Grid-stride over image rows (n*H + y), threads over pixels x, channel loop.
__global__ __launch_bounds__(TPB) void tv_kernel(const float* __restrict__ x, int N, int H, int W, int C, float w,
                                                 float* __restrict__ g, double* __restrict__ loss, float inv_v,
                                                 float inv_h) {
    float acc = 0.f;
    const int WC = W * C;
    for (int row = blockIdx.x; row < N * H; row += gridDim.x) {
        const int yh = row % H;
        const float* xr = x + (long)row * WC;
        float* gr = g + (long)row * WC;
        for (int xw = threadIdx.x; xw < W; xw += TPB) {
            for (int c = 0; c < C; ++c) {
                const int e = xw * C + c;
                const float v = xr[e];
                float gv = 0.f;
                if (yh + 1 < H) {
                    const float d = xr[e + WC] - v;
                    acc += fabsf(d) * inv_v;
                    gv -= sgn(d) * inv_v;
                }
                if (yh > 0) gv += sgn(v - xr[e - WC]) * inv_v;
                if (xw + 1 < W) {
                    const float d = xr[e + C] - v;
                    acc += fabsf(d) * inv_h;
                    gv -= sgn(d) * inv_h;
                }
                if (xw > 0) gv += sgn(v - xr[e - C]) * inv_h;
                gr[e] += w * gv;
            }
        }
    }
    block_add(loss, w * acc);
}

// the separable Gaussian window of ssim_loss_torch (ir:699-712): K taps, K odd
template <int K>
struct WinK {
    float g[K];
};

// SSIM (ir:714-750) on a' = (a+1)/2, b' = (b+1)/2 with the separable 11-tap
// Gaussian (sigma 1.5) and zero padding 5.  Planar fp32 work maps of size S.
template <int K>
__global__ __launch_bounds__(TPB) void ssim_h5_kernel(const float* __restrict__ a, const float* __restrict__ b, int W,
                                                      int C, WinK<K> win, float* __restrict__ out, long S) {
    constexpr int HK = K / 2;
    const int xw = blockIdx.x * TPB + threadIdx.x;
    if (xw >= W) return;
    const long rowb = (long)blockIdx.y * W * C;
    for (int c = 0; c < C; ++c) {
        const long idx = rowb + (long)xw * C + c;
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int xx = xw + k - HK;
            if (xx < 0 || xx >= W) continue;
            const long j = idx + (long)(k - HK) * C;
            const float p = (a[j] + 1.f) * 0.5f, q = (b[j] + 1.f) * 0.5f, gk = win.g[k];
            m1 += gk * p;
            m2 += gk * q;
            e11 += gk * p * p;
            e22 += gk * q * q;
            e12 += gk * p * q;
        }
        out[idx] = m1;
        out[S + idx] = m2;
        out[2 * S + idx] = e11;
        out[3 * S + idx] = e22;
        out[4 * S + idx] = e12;
    }
}

// Horizontal 11-tap pass, one image row per block: the row's NI input maps are
// staged in LDS with coalesced loads (FIRST: a' = (a+1)/2 and b' = (b+1)/2, five
// outputs mu1, mu2, E[a'^2], E[b'^2], E[a'b']; else NI = NO planar maps), then every
// output element reads its 11 taps from LDS.  Same tap order as ssim_h5_kernel /
// ssim_h_kernel (bit-identical results) without their stride-C global re-reads.
template <int K, int NI, int NO, bool FIRST>
__global__ __launch_bounds__(TPB) void ssim_hrow_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ in, int W, int C, WinK<K> win,
                                                        float* __restrict__ out, long S) {
    constexpr int HK = K / 2;
    extern __shared__ float rowm[];  // NI x W*C
    const int WC = W * C;
    const long rb = (long)blockIdx.x * WC;
    for (int e = threadIdx.x; e < WC; e += TPB) {
        if (FIRST) {
            rowm[e] = (a[rb + e] + 1.f) * 0.5f;
            rowm[WC + e] = (b[rb + e] + 1.f) * 0.5f;
        } else {
#pragma unroll
            for (int m = 0; m < NI; ++m) rowm[m * WC + e] = in[m * S + rb + e];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < WC; e += TPB) {
        const int xw = e / C;
        float acc[NO];
#pragma unroll
        for (int m = 0; m < NO; ++m) acc[m] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int xx = xw + k - HK;
            if (xx < 0 || xx >= W) continue;
            const int j = e + (k - HK) * C;
            const float gk = win.g[k];
            if (FIRST) {
                const float p = rowm[j], q = rowm[WC + j];
                acc[0] += gk * p;
                acc[1] += gk * q;
                acc[2] += gk * p * p;
                acc[3] += gk * q * q;
                acc[4] += gk * p * q;
            } else {
#pragma unroll
                for (int m = 0; m < NO; ++m) acc[m] += gk * rowm[m * WC + j];
            }
        }
#pragma unroll
        for (int m = 0; m < NO; ++m) out[m * S + rb + e] = acc[m];
    }
}

// Round 6: the vertical pass fused with its elementwise consumer -- the five moment maps'
// vertical sums feed the SSIM map and dL/d{mu1, e11, e12} (ssim_map_kernel's arithmetic) in
// registers, and the three adjoint maps' sums feed the input gradient (ssim_grad_kernel's),
// so neither the 5 nor the 3 vertically filtered maps are written and re-read (5 + 3 fp32
// maps of N*H*W*C).  Per element the operations and their order are those of the unfused
// pair: d3 and g bit-identical; the loss is the same sum in another block grouping.
template <int K, int R, bool MAP>
__global__ __launch_bounds__(TPB) void ssim_vfused_kernel(const float* __restrict__ in, int H, int W, int C,
                                                          WinK<K> win, float w, float* __restrict__ d3,
                                                          double* __restrict__ loss, const float* __restrict__ a,
                                                          const float* __restrict__ b, float* __restrict__ g,
                                                          long S) {
    constexpr int HK = K / 2, NM = MAP ? 5 : 3;
    const int e = blockIdx.x * TPB + threadIdx.x;  // element within the row (x*C + c)
    float lacc = 0.f;
    if (e < W * C) {
        const int hb = (H + R - 1) / R;
        const int n = blockIdx.y / hb, y0 = (blockIdx.y - n * hb) * R;
        const long WC = (long)W * C;
        const long base = (long)n * H * WC + e;
        float v[NM][R + K - 1];
#pragma unroll
        for (int r = 0; r < R + K - 1; ++r) {
            const int yy = y0 + r - HK;
            const bool ok = yy >= 0 && yy < H;
#pragma unroll
            for (int m = 0; m < NM; ++m) v[m][r] = ok ? in[m * S + base + yy * WC] : 0.f;
        }
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float dLdS = -w / (float)S;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (y0 + r >= H) break;
            float mom[NM];
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) acc += win.g[k] * v[m][r + k];
                mom[m] = acc;
            }
            const long idx = base + (y0 + r) * WC;
            if constexpr (MAP) {
                const float mu1 = mom[0], mu2 = mom[1], e11 = mom[2], e22 = mom[3], e12 = mom[4];
                const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
                const float s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
                const float A1 = 2.f * m12 + C1, A2 = 2.f * s12 + C2;
                const float B1 = m11 + m22 + C1, B2 = s11 + s22 + C2;
                const float den = B1 * B2;
                const float Sv = (A1 * A2) / den;
                lacc += 1.f - Sv;
                const float dmu1 = (2.f * mu2 * (A2 - A1)) / den - Sv * 2.f * mu1 / B1 + Sv * 2.f * mu1 / B2;
                const float de11 = -Sv / B2;
                const float de12 = 2.f * A1 / den;
                d3[idx] = dLdS * dmu1;
                d3[S + idx] = dLdS * de11;
                d3[2 * S + idx] = dLdS * de12;
            } else {
                const float p = (a[idx] + 1.f) * 0.5f, q = (b[idx] + 1.f) * 0.5f;
                const float gp = mom[0] + 2.f * p * mom[1] + q * mom[2];
                g[idx] += 0.5f * gp;  // d a'/d a = 1/2
            }
        }
    }
    if constexpr (MAP) block_add(loss, w * lacc / (float)S);
}

// horizontal 11-tap pass over NM planar maps
template <int K, int NM>
__global__ __launch_bounds__(TPB) void ssim_h_kernel(const float* __restrict__ in, int W, int C, WinK<K> win,
                                                     float* __restrict__ out, long S) {
    constexpr int HK = K / 2;
    const int xw = blockIdx.x * TPB + threadIdx.x;
    if (xw >= W) return;
    const long rowb = (long)blockIdx.y * W * C;
    for (int c = 0; c < C; ++c) {
        const long idx = rowb + (long)xw * C + c;
        float acc[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int xx = xw + k - HK;
            if (xx < 0 || xx >= W) continue;
            const long j = idx + (long)(k - HK) * C;
#pragma unroll
            for (int m = 0; m < NM; ++m) acc[m] += win.g[k] * in[m * S + j];
        }
#pragma unroll
        for (int m = 0; m < NM; ++m) out[m * S + idx] = acc[m];
    }
}

// One element of torch.optim.Adam (ir:1601-1604): updates the moments in place and returns
// the new parameter.  Every Adam kernel below goes through this one body, so their p / m / v
// agree bit for bit -- which also needs every rounding pinned: left to the compiler, the
// one-element and the 16-byte kernels contract a*b + c differently.  Contraction is off in
// here and the fused operations are spelled out (m and p one fma each, v two products and a
// sum).
IRGAN_HD float adam_update(float pi, float gi, float& mi, float& vi, float step_size, float w1, float b2, float w2,
                           float bc2s, float eps) {
#pragma clang fp contract(off)
    // torch lerp: weight < 0.5 ? m + w*(g-m) : g - (g-m)*(1-w)
    const float d = gi - mi;
    mi = (w1 < 0.5f) ? __builtin_fmaf(w1, d, mi) : __builtin_fmaf(-(1.f - w1), d, gi);
    vi = vi * b2 + (w2 * gi) * gi;
    const float denom = sqrtf(vi) / bc2s + eps;
    return __builtin_fmaf(-step_size, mi / denom, pi);
}

// e + w * (p - e), one fma (pinned like adam_update: both EMA kernels round alike)
IRGAN_HD float ema_update(float ei, float pn, float we) {
#pragma clang fp contract(off)
    return __builtin_fmaf(we, pn - ei, ei);
}

// The clipped gradient g * coef: ONE fp32 product, rounded before adam_update sees it (torch's
// g.mul_(coef) followed by the optimizer step).  Pinned like adam_update: left to the compiler
// the product would fuse into the first moment's g - m.
template <bool CLIP>
IRGAN_HD float clip_grad(float gi, float coef) {
#pragma clang fp contract(off)
    if (!CLIP) return gi;
    return gi * coef;
}

// Adam (4 reads, 3 writes per element) and, with e (EMA), the exponential moving average of
// the new parameters, e += we * (p_new - e), in the same pass (5 reads, 4 writes).
// prm (device, nullable): {step_size, bc2s} and, EMA, {.., we}, written by adam_prep_kernel in
// the same stream (graph replay: the step count lives on the device, so a captured step stays
// valid).  Without EMA neither e nor prm[2] nor we is touched.
// CLIP (gradient-norm clipping): the update consumes g * coef, coef from prm[3]
// (adam_clip_prep_kernel) or from the host; g itself is only read.  Without CLIP neither
// prm[3] nor coef is touched.
struct AdamArgs {
    float *p, *m, *v, *e;
    const float* g;
    const float* prm;
    float step_size, b1, b2, bc2s, eps, we, coef;
};

template <bool EMA, bool CLIP>
IRGAN_HD void adam_coeffs(const AdamArgs& a, float& step_size, float& bc2s, float& we, float& coef) {
    step_size = a.step_size, bc2s = a.bc2s, we = a.we, coef = a.coef;
    if (a.prm) {
        step_size = a.prm[0];
        bc2s = a.prm[1];
        if (EMA) we = a.prm[2];
        if (CLIP) coef = a.prm[3];
    }
}

template <bool EMA, bool CLIP>
IRGAN_HD void adam_one(const AdamArgs& a, long i, float step_size, float w1, float w2, float bc2s, float we,
                       float coef) {
    float mi = a.m[i], vi = a.v[i];
    const float ei = EMA ? a.e[i] : 0.f;
    const float pn = adam_update(a.p[i], clip_grad<CLIP>(a.g[i], coef), mi, vi, step_size, w1, a.b2, w2, bc2s, a.eps);
    a.p[i] = pn;
    a.m[i] = mi;
    a.v[i] = vi;
    if (EMA) a.e[i] = ema_update(ei, pn, we);
}

// any 4-byte-aligned pointers: one element per thread and round
template <bool EMA, bool CLIP>
__global__ __launch_bounds__(TPB) void adam_kernel(AdamArgs a, long n) {
    float step_size, bc2s, we, coef;
    adam_coeffs<EMA, CLIP>(a, step_size, bc2s, we, coef);
    const float w1 = 1.f - a.b1, w2 = 1.f - a.b2;
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB)
        adam_one<EMA, CLIP>(a, i, step_size, w1, w2, bc2s, we, coef);
}

// The pointers share one offset from a 16-byte boundary: `head` (< 4) leading elements and
// the tail (< 4) one per thread (block 0), the nvec groups of four between them with
// 16-byte loads and stores, grid-stride.  n = head + 4 * nvec + tail.
template <bool EMA, bool CLIP>
__global__ __launch_bounds__(TPB) void adam_vec_kernel(AdamArgs a, int head, long nvec, int tail) {
    float step_size, bc2s, we, coef;
    adam_coeffs<EMA, CLIP>(a, step_size, bc2s, we, coef);
    const float w1 = 1.f - a.b1, w2 = 1.f - a.b2;
    float4* __restrict__ p4 = reinterpret_cast<float4*>(a.p + head);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(a.m + head);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(a.v + head);
    float4* __restrict__ e4 = EMA ? reinterpret_cast<float4*>(a.e + head) : nullptr;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(a.g + head);
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < nvec; i += (long)gridDim.x * TPB) {
        float4 P = p4[i], M = m4[i], V = v4[i], E;
        if (EMA) E = e4[i];
        float4 G = g4[i];
        if (CLIP) {
            G.x = clip_grad<CLIP>(G.x, coef);
            G.y = clip_grad<CLIP>(G.y, coef);
            G.z = clip_grad<CLIP>(G.z, coef);
            G.w = clip_grad<CLIP>(G.w, coef);
        }
        P.x = adam_update(P.x, G.x, M.x, V.x, step_size, w1, a.b2, w2, bc2s, a.eps);
        P.y = adam_update(P.y, G.y, M.y, V.y, step_size, w1, a.b2, w2, bc2s, a.eps);
        P.z = adam_update(P.z, G.z, M.z, V.z, step_size, w1, a.b2, w2, bc2s, a.eps);
        P.w = adam_update(P.w, G.w, M.w, V.w, step_size, w1, a.b2, w2, bc2s, a.eps);
        if (EMA) {
            E.x = ema_update(E.x, P.x, we);
            E.y = ema_update(E.y, P.y, we);
            E.z = ema_update(E.z, P.z, we);
            E.w = ema_update(E.w, P.w, we);
        }
        p4[i] = P;
        m4[i] = M;
        v4[i] = V;
        if (EMA) e4[i] = E;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < head + tail) {
        const int t = threadIdx.x;
        adam_one<EMA, CLIP>(a, t < head ? (long)t : (long)head + 4 * nvec + (t - head), step_size, w1, w2, bc2s, we,
                            coef);
    }
}

// One arm of the path below: the 16-byte kernel when the pointers allow (vec), else one element
// per lane.
template <bool EMA, bool CLIP>
void adam_arm(const AdamArgs& a, long n, bool vec, long head, long nvec, int tail, hipStream_t st) {
    if (vec)
        adam_vec_kernel<EMA, CLIP><<<nblocks(nvec), TPB, 0, st>>>(a, (int)head, nvec, tail);
    else
        adam_kernel<EMA, CLIP><<<nblocks(n), TPB, 0, st>>>(a, n);
}

// EMA iff a.e; clip: the gradient times prm[3] / a.coef.  16-byte accesses when the pointers
// that exist (four, with EMA five) share one
// offset from a 16-byte boundary and there is a whole group of four; one element per lane
// otherwise.  The vector kernel takes one group of four per thread under nblocks' cap: a full
// round of its grid is 8192 * TPB * 4 elements, the rest grid-strides.
int adam_launch(const AdamArgs& a, long n, hipStream_t st, bool clip = false) {
    const uintptr_t off = (uintptr_t)a.p % 16;
    auto at_off = [off](const float* q) { return (uintptr_t)q % 16 == off; };
    const bool same = at_off(a.g) && at_off(a.m) && at_off(a.v) && (!a.e || at_off(a.e)) && off % 4 == 0;
    const long head = std::min<long>(n, (16 - (long)off) % 16 / 4);
    const long nvec = (n - head) / 4;
    const int tail = (int)(n - head - 4 * nvec);
    const bool vec = same && nvec > 0;
    if (a.e && clip)
        adam_arm<true, true>(a, n, vec, head, nvec, tail, st);
    else if (a.e)
        adam_arm<true, false>(a, n, vec, head, nvec, tail, st);
    else if (clip)
        adam_arm<false, true>(a, n, vec, head, nvec, tail, st);
    else
        adam_arm<false, false>(a, n, vec, head, nvec, tail, st);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

// ---- gradient-norm clipping: the sum of squares of a flat fp32 buffer, deterministic ----
// The grid is a function of n alone (sumsq_parts), every thread accumulates g*g in fp64 (the
// square of an fp32 is exact there, and 1e25 does not overflow), a block combines its threads
// in a fixed tree and writes ONE fp64 partial; adam_clip_prep_kernel adds the partials in index
// order.  No atomics: the same buffer gives the same bits on every launch and every rank, so
// the data-parallel replicas clip by the same coefficient.
constexpr int SUMSQ_MAX_PARTS = 1024;   // partials of one buffer: the prep kernel holds them in LDS

int sumsq_parts(long n) {
    return (int)std::max<long>(1, std::min<long>((n + 4L * TPB - 1) / (4L * TPB), SUMSQ_MAX_PARTS));
}

// g: any 4-byte-aligned pointer.  `head` (< 4) elements up to the 16-byte boundary and the tail
// (< 4) one per thread (block 0), the nvec groups of four between them with 16-byte loads,
// grid-stride.  n = head + 4 * nvec + tail.
__global__ __launch_bounds__(TPB) void sumsq_kernel(const float* __restrict__ g, int head, long nvec, int tail,
                                                    double* __restrict__ partials) {
    __shared__ double red[TPB];
    auto sq = [](float x) { return (double)x * (double)x; };
    double acc = 0.0;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
#pragma unroll 4
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < nvec; i += (long)gridDim.x * TPB) {
        const float4 G = g4[i];
        acc += sq(G.x);
        acc += sq(G.y);
        acc += sq(G.z);
        acc += sq(G.w);
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < head + tail) {
        const int t = threadIdx.x;
        acc += sq(g[t < head ? (long)t : (long)head + 4 * nvec + (t - head)]);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = TPB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

template <int K>
WinK<K> gauss_win() {
    // ir:699-703 in fp32: coords = arange(K) - (K-1)/2, exp(-c^2 / (2*1.5^2)), normalised
    WinK<K> w;
    float s = 0.f;
    for (int k = 0; k < K; ++k) {
        float c = (float)k - (float)(K - 1) / 2.0f;
        w.g[k] = expf(-(c * c) / (2.f * 1.5f * 1.5f));
        s += w.g[k];
    }
    for (int k = 0; k < K; ++k) w.g[k] /= s;
    return w;
}

// the forward + gradient launches for one window size (S = N*H*W*C, maps in work)
template <int K>
int ssim_launch(const float* a, const float* b, int N, int H, int W, int C, float w, float* g, double* loss,
                float* work, hipStream_t st) {
    const long S = (long)N * H * W * C;
    const WinK<K> win = gauss_win<K>();
    float* w0 = work;          // 5 maps
    float* w1 = work + 5 * S;  // 5 maps
    constexpr int VR = 8;  // rows per thread in the vertical passes
    const dim3 gx(irgan_cdiv(W, TPB), N * H), ge(irgan_cdiv((long)W * C, TPB), N * irgan_cdiv(H, VR));
    const size_t row5 = (size_t)W * C * 2 * sizeof(float), row3 = (size_t)W * C * 3 * sizeof(float);
    if (row3 <= 64 * 1024) {  // row-staged horizontal passes (W*C <= 5461)
        ssim_hrow_kernel<K, 2, 5, true><<<N * H, TPB, row5, st>>>(a, b, nullptr, W, C, win, w0, S);
    } else {
        ssim_h5_kernel<K><<<gx, TPB, 0, st>>>(a, b, W, C, win, w0, S);
    }
    // vertical pass + SSIM map + its gradient maps (into w1's first 3 maps)
    ssim_vfused_kernel<K, VR, true><<<ge, TPB, 0, st>>>(w0, H, W, C, win, w, w1, loss, nullptr, nullptr, nullptr, S);
    if (row3 <= 64 * 1024) {
        ssim_hrow_kernel<K, 3, 3, false><<<N * H, TPB, row3, st>>>(nullptr, nullptr, w1, W, C, win, w0, S);
    } else {
        ssim_h_kernel<K, 3><<<gx, TPB, 0, st>>>(w1, W, C, win, w0, S);
    }
    // vertical pass of the adjoint + the input gradient
    ssim_vfused_kernel<K, VR, false><<<ge, TPB, 0, st>>>(w0, H, W, C, win, w, nullptr, nullptr, a, b, g, S);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int irgan_hinge(const float* pred, int32_t n_half, int32_t mode, float scale, float* grad, double* loss,
                           irgan_stream_t s) {
    if (mode != 0 && mode != 1) return IRGAN_EINVAL;
    long total = mode == 0 ? 2L * n_half : n_half;
    hinge_kernel<<<nblocks_red(total), TPB, 0, (hipStream_t)s>>>(pred, n_half, mode, scale, grad, loss);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

// objective 0 is irgan_hinge's launch itself (the default step's kernel and arguments are unchanged)
extern "C" int irgan_gan_loss(const float* pred, int32_t n_half, int32_t side, int32_t objective, float real_label,
                              float scale, float* grad, double* loss, irgan_stream_t s) {
    if (side != 0 && side != 1) return IRGAN_EINVAL;
    if (objective != 0 && objective != GAN_LSGAN && objective != GAN_BCE) return IRGAN_EINVAL;
    if (!(real_label > 0.f && real_label <= 1.f)) return IRGAN_EINVAL;   // NaN and inf fail it too
    if (objective == 0 && real_label != 1.f) return IRGAN_EINVAL;
    const long total = side == 0 ? 2L * n_half : n_half;
    const int nb = nblocks_red(total);
    hipStream_t st = (hipStream_t)s;
    if (objective == 0)
        hinge_kernel<<<nb, TPB, 0, st>>>(pred, n_half, side, scale, grad, loss);
    else if (objective == GAN_LSGAN)
        gan_loss_kernel<GAN_LSGAN><<<nb, TPB, 0, st>>>(pred, n_half, side, real_label, scale, grad, loss);
    else
        gan_loss_kernel<GAN_BCE><<<nb, TPB, 0, st>>>(pred, n_half, side, real_label, scale, grad, loss);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

// l1_kernel<.., TAP> for the dtypes of a / b and of ga: the 8-wide form where count and every
// pointer allow 16-byte accesses
template <bool TAP>
static int l1_launch(const void* a, const void* b, int32_t dtype, int64_t count, float w, void* ga, int32_t ga_dtype,
                     int32_t accumulate, double* loss, irgan_stream_t s) {
    if (count <= 0) return 0;
    const bool vec = count % 8 == 0 && ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0) &&
                     (!ga || (uintptr_t)ga % 16 == 0);
    const int nb = nblocks_red(vec ? count / 8 : count);
    auto go = [&](auto t, auto g) {
        using T = decltype(t);
        using G = decltype(g);
        auto k = vec ? l1_kernel<T, G, true, TAP> : l1_kernel<T, G, false, TAP>;
        k<<<nb, TPB, 0, (hipStream_t)s>>>((const T*)a, (const T*)b, count, w, (G*)ga, accumulate, loss);
    };
    if (dtype == IRGAN_F32) {
        if (ga_dtype == IRGAN_BF16) go(float(), bf16_t());
        else go(float(), float());
    } else {
        if (ga_dtype == IRGAN_BF16) go(bf16_t(), bf16_t());
        else go(bf16_t(), float());
    }
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_l1(const void* a, const void* b, int32_t dtype, int64_t count, float w, void* ga,
                        int32_t ga_dtype, int32_t accumulate, double* loss, irgan_stream_t s) {
    return l1_launch<false>(a, b, dtype, count, w, ga, ga_dtype, accumulate, loss, s);
}

extern "C" int irgan_l1_tap(const void* a, const void* b, int32_t dtype, int64_t count, float w, void* dz,
                            int32_t dz_dtype, int32_t accumulate, double* loss, irgan_stream_t s) {
    if ((dtype != IRGAN_F32 && dtype != IRGAN_BF16) || (dz_dtype != IRGAN_F32 && dz_dtype != IRGAN_BF16) || !dz)
        return IRGAN_EINVAL;
    return l1_launch<true>(a, b, dtype, count, w, dz, dz_dtype, accumulate, loss, s);
}


extern "C" int irgan_tv(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float w, float* g, double* loss,
                        irgan_stream_t s) {
    if ((long)N * H * W * C <= 0) return 0;
    float inv_v = H > 1 ? 1.f / (float)((long)N * C * (H - 1) * W) : 0.f;
    float inv_h = W > 1 ? 1.f / (float)((long)N * C * H * (W - 1)) : 0.f;
    tv_kernel<<<std::min(N * H, 512), TPB, 0, (hipStream_t)s>>>(x, N, H, W, C, w, g, loss, inv_v, inv_h);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_ssim_ws(const float* a, const float* b, int32_t N, int32_t H, int32_t W, int32_t C, float w,
                             float* g, double* loss, float* work, int32_t window, irgan_stream_t s) {
    hipStream_t st = (hipStream_t)s;
    if ((long)N * H * W * C <= 0) return 0;
    if ((long)N * H > 65535) return IRGAN_EUNSUPPORTED;
    switch (window) {
        case 1: return ssim_launch<1>(a, b, N, H, W, C, w, g, loss, work, st);
        case 3: return ssim_launch<3>(a, b, N, H, W, C, w, g, loss, work, st);
        case 5: return ssim_launch<5>(a, b, N, H, W, C, w, g, loss, work, st);
        case 7: return ssim_launch<7>(a, b, N, H, W, C, w, g, loss, work, st);
        case 9: return ssim_launch<9>(a, b, N, H, W, C, w, g, loss, work, st);
        case 11: return ssim_launch<11>(a, b, N, H, W, C, w, g, loss, work, st);
        case 13: return ssim_launch<13>(a, b, N, H, W, C, w, g, loss, work, st);
        case 15: return ssim_launch<15>(a, b, N, H, W, C, w, g, loss, work, st);
        default: return IRGAN_EUNSUPPORTED;
    }
}

extern "C" int irgan_ssim(const float* a, const float* b, int32_t N, int32_t H, int32_t W, int32_t C, float w,
                          float* g, double* loss, float* work, irgan_stream_t s) {
    return irgan_ssim_ws(a, b, N, H, W, C, w, g, loss, work, 11, s);
}

// t = ++*count; prm = {lr / (1 - b1^t), sqrt(1 - b2^t)}: the host formula of irgan_adam's
// arguments (ops.adam), in fp64 and then rounded to fp32, evaluated on the device.
// EMA (irgan_adam_ema_prep): also prm[2] = 1 - min(decay, (1 + t) / (10 + t)) (ops.ema_weight).
template <bool EMA>
IRGAN_HD void adam_prep_body(int32_t* count, double lr, double b1, double b2, double decay, float* prm) {
    const int t = *count + 1;
    *count = t;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    prm[0] = (float)(lr / bc1);
    prm[1] = (float)sqrt(bc2);
    if (EMA) {
        const double warm = (1.0 + (double)t) / (10.0 + (double)t);
        prm[2] = (float)(1.0 - (decay < warm ? decay : warm));
    }
}

template <bool EMA>
static __global__ void adam_prep_kernel(int32_t* count, double lr, double b1, double b2, double decay, float* prm) {
    if (threadIdx.x != 0) return;
    adam_prep_body<EMA>(count, lr, b1, b2, decay, prm);
}

// The clip form (irgan_adam_clip_prep): the same count and prm[0..2] (the EMA weight always: a
// decay of 0 where there is no average), and from sumsq_kernel's partials, added in index order
// in fp64: norm = sqrt(sum) -> *norm_out (fp64, nullable), prm[3] = min(1, max_norm / (norm + 1e-6))
// rounded to fp32 -- torch.nn.utils.clip_grad_norm_'s coefficient.  A non-finite norm gets what
// the formula gives (NaN stays NaN, inf gives 0), as with torch's error_if_nonfinite=False.
static __global__ void adam_clip_prep_kernel(int32_t* count, double lr, double b1, double b2, double decay,
                                             float* prm, const double* __restrict__ partials, int nparts,
                                             double max_norm, double* norm_out) {
    __shared__ double part[SUMSQ_MAX_PARTS];
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) part[i] = partials[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    adam_prep_body<true>(count, lr, b1, b2, decay, prm);
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += part[i];
    const double norm = sqrt(s);
    if (norm_out) *norm_out = norm;
    const double coef = max_norm / (norm + 1e-6);
    prm[3] = (float)(coef > 1.0 ? 1.0 : coef);
}

extern "C" int irgan_adam_prep(int32_t* count, double lr, double beta1, double beta2, float* prm, irgan_stream_t s) {
    if (!count || !prm) return IRGAN_EINVAL;
    adam_prep_kernel<false><<<1, 64, 0, (hipStream_t)s>>>(count, lr, beta1, beta2, 0.0, prm);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* prm, float beta1,
                              float beta2, float eps, irgan_stream_t s) {
    if (!prm) return IRGAN_EINVAL;
    if (n <= 0) return 0;
    return adam_launch(AdamArgs{p, m, v, nullptr, g, prm, 0.f, beta1, beta2, 1.f, eps, 0.f}, n, (hipStream_t)s);
}

extern "C" int irgan_adam(float* p, const float* g, float* m, float* v, int64_t n, float step_size, float beta1,
                          float beta2, float bc2_sqrt, float eps, irgan_stream_t s) {
    if (n <= 0) return 0;
    return adam_launch(AdamArgs{p, m, v, nullptr, g, nullptr, step_size, beta1, beta2, bc2_sqrt, eps, 0.f}, n,
                       (hipStream_t)s);
}

extern "C" int irgan_adam_ema_prep(int32_t* count, double lr, double beta1, double beta2, double ema_decay, float* prm,
                                   irgan_stream_t s) {
    if (!count || !prm || !(ema_decay >= 0.0 && ema_decay < 1.0)) return IRGAN_EINVAL;
    adam_prep_kernel<true><<<1, 64, 0, (hipStream_t)s>>>(count, lr, beta1, beta2, ema_decay, prm);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* prm,
                                  float beta1, float beta2, float eps, irgan_stream_t s) {
    if (!prm || !ema) return IRGAN_EINVAL;
    if (n <= 0) return 0;
    return adam_launch(AdamArgs{p, m, v, ema, g, prm, 0.f, beta1, beta2, 1.f, eps, 0.f}, n, (hipStream_t)s);
}

extern "C" int irgan_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float step_size,
                              float beta1, float beta2, float bc2_sqrt, float eps, float ema_weight, irgan_stream_t s) {
    if (!ema) return IRGAN_EINVAL;
    if (n <= 0) return 0;
    return adam_launch(AdamArgs{p, m, v, ema, g, nullptr, step_size, beta1, beta2, bc2_sqrt, eps, ema_weight},
                           n, (hipStream_t)s);
}

// ---- gradient-norm clipping (include/irgan.h) ----
extern "C" int irgan_grad_sumsq_parts(int64_t n) { return n > 0 ? sumsq_parts(n) : 0; }

extern "C" int irgan_grad_sumsq(const float* g, int64_t n, double* partials, int32_t nparts, irgan_stream_t s) {
    if (!g || !partials || n <= 0 || nparts != sumsq_parts(n)) return IRGAN_EINVAL;
    const long head = std::min<long>(n, (16 - (long)((uintptr_t)g % 16)) % 16 / 4);
    const long nvec = (n - head) / 4;
    sumsq_kernel<<<nparts, TPB, 0, (hipStream_t)s>>>(g, (int)head, nvec, (int)(n - head - 4 * nvec), partials);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_adam_clip_prep(int32_t* count, double lr, double beta1, double beta2, double ema_decay,
                                    const double* partials, int32_t nparts, int64_t n, double max_norm,
                                    double* norm_out, float* prm, irgan_stream_t s) {
    if (!count || !prm || !partials || !(ema_decay >= 0.0 && ema_decay < 1.0) || !(max_norm > 0.0)) return IRGAN_EINVAL;
    if (n <= 0 || nparts != sumsq_parts(n)) return IRGAN_EINVAL;
    adam_clip_prep_kernel<<<1, 256, 0, (hipStream_t)s>>>(count, lr, beta1, beta2, ema_decay, prm, partials, nparts,
                                                         max_norm, norm_out);
    IRGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int irgan_adam_clip_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                   const float* prm, float beta1, float beta2, float eps, irgan_stream_t s) {
    if (!prm) return IRGAN_EINVAL;
    if (n <= 0) return 0;
    return adam_launch(AdamArgs{p, m, v, ema, g, prm, 0.f, beta1, beta2, 1.f, eps, 0.f, 1.f}, n, (hipStream_t)s, true);
}

extern "C" int irgan_adam_clip(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float step_size,
                               float beta1, float beta2, float bc2_sqrt, float eps, float ema_weight, float coef,
                               irgan_stream_t s) {
    if (n <= 0) return 0;
    return adam_launch(AdamArgs{p, m, v, ema, g, nullptr, step_size, beta1, beta2, bc2_sqrt, eps, ema_weight, coef},
                       n, (hipStream_t)s, true);
}
